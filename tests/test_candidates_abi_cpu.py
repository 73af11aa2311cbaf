"""The candidate caller's C ABI without a GPU (dv_call_candidates_batch, include/dvhip.h): the symbols
exist, the struct layouts match the ctypes mirrors, argument errors are reported before any device
work, and DV_ABI_VERSION is still 8 (the entry points are additions).  Also the host half of the device
route, which needs no device: how calls are built from the sites a counter hands over."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import allelecounter as A
from deepvariant_amd import variant_calling as vc

HEADER = os.path.join(os.path.dirname(__file__), '..', 'include', 'dvhip.h')


def test_symbols_and_version():
  lib = _lib.lib()
  for name in ('dv_call_candidates_batch', 'dv_candidates_arrays', 'dv_candidates_free'):
    assert getattr(lib, name) is not None and name in _lib.ABI_SYMBOLS
  assert lib.dv_abi_version() == 8
  with open(HEADER) as f:
    header = f.read()
  assert re.search(r'#define DV_ABI_VERSION 8\b', header)
  for name in ('dv_candidate_options', 'dv_candidate_site', 'dv_candidate_allele', 'dv_candidates',
               'dv_call_candidates_batch'):
    assert name in header


def test_struct_layouts():
  # the static_asserts of csrc/candidates.hip hold the C side to the same sizes
  assert C.sizeof(_lib.DvCandidateOptions) == 24
  assert C.sizeof(_lib.DvCandidateSite) == 20 == A.CANDIDATE_SITE_DTYPE.itemsize
  assert C.sizeof(_lib.DvCandidateAllele) == 16 == A.CANDIDATE_ALLELE_DTYPE.itemsize
  assert [n for n, _ in _lib.DvCandidateSite._fields_] == list(A.CANDIDATE_SITE_DTYPE.names)        # pylint: disable=protected-access
  assert [n for n, _ in _lib.DvCandidateAllele._fields_] == list(A.CANDIDATE_ALLELE_DTYPE.names)    # pylint: disable=protected-access
  assert _lib.DvCandidateOptions.min_fraction_snps.size == 4            # a C float: the proto field's precision


def _status(options, n=1, counts=True, candidates=True, gvcf=None):
  lib = _lib.lib()
  slots = (C.c_void_p * 1)()
  out, cand = (C.c_void_p * 1)(), (C.c_void_p * 1)()
  rc = lib.dv_call_candidates_batch(n, slots, slots, None, C.byref(options) if options is not None else None, gvcf,
                                    out if counts else None, None, cand if candidates else None, None)
  assert not out[0] and not cand[0]                                      # nothing is left allocated
  return rc, lib.dv_last_error().decode()


@pytest.mark.parametrize('fields', [(-1, 2, 0.12, 0.06), (2, -1, 0.12, 0.06), (2, 2, -0.5, 0.06), (2, 2, 0.12, -1e-9),
                                    (2, 2, float('nan'), 0.06)])
def test_negative_thresholds_are_invalid_arguments(fields):
  rc, message = _status(_lib.DvCandidateOptions(*fields, 0, 0))
  assert rc == -1 and 'thresholds must be >= 0' in message             # DV_ERR_INVALID_ARGUMENT
  with pytest.raises(_lib.DvError):
    _lib.check(rc)


def test_null_arguments():
  good = _lib.DvCandidateOptions(2, 2, 0.12, 0.06, 0, 0)
  assert _status(None)[0] == -1
  assert _status(good, candidates=False)[0] == -1
  assert _status(good, counts=False)[0] == -1                            # counts_out may be NULL with positions_only alone
  rc, message = _status(good, n=-1)
  assert rc == -1 and 'dv_call_candidates_batch' in message
  # an empty batch is not an error, and needs no device
  assert _lib.lib().dv_call_candidates_batch(0, None, None, None, C.byref(good), None, None, None, None, None) == 0
  assert _lib.lib().dv_candidates_arrays(None, None, None, None, None, None) == -1
  _lib.lib().dv_candidates_free(None)


def test_candidate_options_mirror_the_callers_float32_thresholds():
  caller = vc.VariantCaller(vc.VariantCallerOptions(2, 3, 0.1, 0.06, track_ref_reads=True))
  opts = caller.candidate_options()
  assert (opts.min_count_snps, opts.min_count_indels, opts.track_ref_reads, opts.positions_only) == (2, 3, True, False)
  assert opts.min_fraction_snps == float(np.float32(0.1)) > 0.1
  assert C.c_float(opts.min_fraction_snps).value == opts.min_fraction_snps       # survives the C float exactly
  assert opts.positions_form().positions_only and opts.positions_form().key() == opts.key()
  assert opts.positions_form().calls_form().positions_only is False
  with pytest.raises(ValueError):
    vc.CandidateOptions(min_fraction_indels=-0.1)


class _Sites:
  """A counter that offers the device route and hands over prepared sites."""

  def __init__(self, sites):
    self._sites = sites

  def candidates(self, call):
    assert not call.positions_only
    return self._sites

  def candidate_positions(self, call):
    assert call.positions_only
    return [s.position.position for s in self._sites]


def _site(selected, read_alleles, ref_count=5):
  s = A.CandidateSite('c', 100, 'A')
  s.ref_supporting_read_count = ref_count
  s.selected = selected
  s.read_alleles = read_alleles
  s.total = ref_count + sum(1 for a in read_alleles.values() if not a.is_low_quality and a.type != A.REFERENCE)
  return s


def test_calls_are_built_from_the_sites_as_call_variant_builds_them():
  """The site's selected alleles, total and read_alleles (texts for the supporters of selected alleles
  only) give the call CallVariant gives on the full AlleleCount: the deletion's suffix on the keys, the
  map order of read_names, UNCALLED_ALLELE, low-quality support."""
  full = A.AlleleCount('c', 100, 'A')
  full.ref_supporting_read_count = 5
  full.read_alleles = {
      'r1': A.Allele('ACG', A.DELETION), 'r2': A.Allele('T', A.SUBSTITUTION), 'r3': A.Allele('ACG', A.DELETION),
      'r4': A.Allele('G', A.SUBSTITUTION), 'r5': A.Allele('T', A.SUBSTITUTION, 1, True), 'r6': A.Allele('T', A.SUBSTITUTION),
      'r7': A.Allele('ATT', A.SOFT_CLIP)}
  caller = vc.VariantCaller(vc.VariantCallerOptions(2, 2, 0.12, 0.06, sample_name='s'))
  want = caller.call_variant(full)
  narrowed = {k: A.Allele(a.bases if k not in ('r4', 'r7') else None, a.type, 1, a.is_low_quality)
              for k, a in full.read_alleles.items()}
  site = _site([A.Allele('ACG', A.DELETION, 2), A.Allele('T', A.SUBSTITUTION, 2)], narrowed)
  got = caller.calls_from_allele_counter(_Sites([site]))
  assert got == [want] and want.variant.reference_bases == 'ACG'
  assert list(want.allele_support['TCG'].read_names) == ['r2', 'r5', 'r6']
  assert list(want.allele_support[vc.K_SUPPORTING_UNCALLED_ALLELE].read_names) == ['r4', 'r7']
  assert caller.call_positions_from_allele_counter(_Sites([site])) == [100]


def test_non_unique_alternate_alleles_still_raise():
  """AddReadDepths' 'Non-unique alternative alleles!' is kept on the device route.  Alleles cut from
  real events cannot collide (a substitution's alternate has the reference bases' length, an insertion's
  is longer, a deletion's shorter, and within a type different texts give different alternates), so the
  site is hand-made: a one-base "insertion" whose alternate equals a substitution's."""
  caller = vc.VariantCaller(vc.VariantCallerOptions(1, 1, 0.0, 0.0))
  reads = {'r1': A.Allele('T', A.SUBSTITUTION), 'r2': A.Allele('T', A.INSERTION)}
  site = _site([A.Allele('T', A.SUBSTITUTION, 1), A.Allele('T', A.INSERTION, 1)], reads)
  with pytest.raises(ValueError, match='Non-unique alternative alleles!'):
    caller.calls_from_allele_counter(_Sites([site]))
  full = A.AlleleCount('c', 100, 'A')
  full.ref_supporting_read_count, full.read_alleles = 5, reads
  with pytest.raises(ValueError, match='Non-unique alternative alleles!'):
    caller.call_variant(full)
