"""The device form of the local aligner, as far as a machine without a GPU can check it
(include/dvhip.h: dv_local_align_pairs_device, dv_realign_regions_device):

  * the new symbols are declared, exported and mirrored, and the ABI version stays 8;
  * argument errors come back as DV_ERR_INVALID_ARGUMENT before any device work, an empty pair
    list is DV_OK, and without a device both entry points return DV_ERR_NO_DEVICE;
  * FastPassAligner::align_reads in phases (prepare -> one batch of pairs through the host
    aligner -> finish, the device route's order of work) gives align_reads() field for field on
    the windows of tests/golden/realigner_chr20.npz.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import dv_types as T
from deepvariant_amd import fast_pass_aligner as F
from tests import realigner_fixture as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dv_local_align_pairs_device', 'dv_local_align_device_last_stats', 'dv_realign_regions_device')
ALIGN_IN_PHASES = 6      # DV_ALIGNER_ALIGN_IN_PHASES


def test_symbols_are_declared_exported_and_mirrored():
  text = open(os.path.join(ROOT, 'include', 'dvhip.h')).read()
  l = _lib.lib()
  for name in NEW_SYMBOLS:
    assert re.search(r'\b%s\s*\(' % name, text), name
    assert name in _lib.ABI_SYMBOLS and hasattr(l, name), name
  assert re.search(r'#define DV_ABI_VERSION 8\b', text) and l.dv_abi_version() == 8
  assert 'DV_ALIGNER_ALIGN_IN_PHASES = %d' % ALIGN_IN_PHASES in text
  for name in ('DV_LOCAL_ALIGN_DEVICE_MAX_QUERY', 'DV_LOCAL_ALIGN_DEVICE_MAX_REFERENCE'):
    assert int(re.search(r'#define %s (\d+)' % name, text).group(1)) == getattr(_lib, name)


def test_device_stats_layout():
  assert C.sizeof(_lib.DvRealignDeviceStats) == 32
  assert [f[0] for f in _lib.DvRealignDeviceStats._fields_] == ['pairs', 'pairs_on_host', 'cells', 'launches']


def _pairs_call(n_seqs=2, bases=b'ACGTACGTTTGACGT', seq_off=(0, 10, 15), n_pairs=1, ref=(0,), query=(1,),
                scoring=(2, 2, 3, 1), out=True):
  off = None if seq_off is None else np.ascontiguousarray(seq_off, np.int64)
  r = None if ref is None else np.ascontiguousarray(ref, np.int32)
  q = None if query is None else np.ascontiguousarray(query, np.int32)
  res = (_lib.DvLocalAlignment * 4)() if out else None
  rc = _lib.lib().dv_local_align_pairs_device(
      n_seqs, bases, None if off is None else off.ctypes.data, n_pairs, None if r is None else r.ctypes.data,
      None if q is None else q.ctypes.data, *scoring, res, None)
  return rc


@pytest.mark.parametrize('what,kw', [
    ('negative sequence count', dict(n_seqs=-1)),
    ('negative pair count', dict(n_pairs=-1)),
    ('null offsets', dict(seq_off=None)),
    ('null bases', dict(bases=None)),
    ('null reference indices', dict(ref=None)),
    ('null query indices', dict(query=None)),
    ('null output', dict(out=False)),
    ('reference index past the table', dict(ref=(2,))),
    ('negative query index', dict(query=(-1,))),
    ('descending offsets', dict(seq_off=(0, 10, 5))),
    ('negative offset', dict(seq_off=(-1, 10, 15))),
    ('match 0', dict(scoring=(0, 2, 3, 1))),
    ('negative mismatch', dict(scoring=(2, -1, 3, 1))),
    ('negative gap_open', dict(scoring=(2, 2, -3, 1))),
    ('negative gap_extend', dict(scoring=(2, 2, 3, -1))),
    ('match past the int8 score matrix', dict(scoring=(128, 2, 3, 1))),
])
def test_argument_errors_come_before_any_device_work(what, kw):
  assert _pairs_call(**kw) == _lib.DV_ERR_INVALID_ARGUMENT, what
  assert 'dv_local_align_pairs_device' in _lib.last_error()


def test_empty_pair_list_is_ok_without_a_device():
  assert _pairs_call(n_pairs=0, ref=None, query=None, out=False) == _lib.DV_OK
  assert _pairs_call(n_seqs=0, bases=None, seq_off=None, n_pairs=0, ref=None, query=None, out=False) == _lib.DV_OK
  assert F.local_align_pairs_device(['ACGT'], []) == []
  stats = _lib.DvRealignDeviceStats(1, 1, 1, 1)
  assert _lib.lib().dv_local_align_device_last_stats(C.byref(stats)) == _lib.DV_OK
  assert (stats.pairs, stats.pairs_on_host, stats.cells, stats.launches) == (0, 0, 0, 0)
  assert _lib.lib().dv_local_align_device_last_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT


def _realign_options():
  from deepvariant_amd.realigner import realigner as R
  return R.Realigner(R.realigner_config(), None)._native_options()     # pylint: disable=protected-access


def test_realign_regions_device_checks_its_arguments_like_the_host_route():
  l = _lib.lib()
  handle, out, stats = C.c_void_p(), _lib.DvRealignOutput(), _lib.DvRealignDeviceStats()
  opt = _realign_options()
  call = lambda *a: l.dv_realign_regions_device(*a)     # noqa: E731
  assert call(None, 1, C.byref(opt), None, C.byref(handle), C.byref(out), C.byref(stats)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(None, 0, None, None, C.byref(handle), C.byref(out), None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(None, 0, C.byref(opt), None, None, C.byref(out), None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(None, -1, C.byref(opt), None, C.byref(handle), C.byref(out), None) == _lib.DV_ERR_INVALID_ARGUMENT
  bad = _realign_options()
  bad.dbg.step_k = 0
  assert call(None, 0, C.byref(bad), None, C.byref(handle), C.byref(out), None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert not handle.value


def test_no_device_no_fallback():
  if _lib.device_count() > 0:
    pytest.skip('GPU present')
  assert _pairs_call() == _lib.DV_ERR_NO_DEVICE
  with pytest.raises(_lib.DvError) as e:
    F.local_align_pairs_device(['ACGTACGT', 'ACGT'], [(0, 1)])
  assert e.value.status == _lib.DV_ERR_NO_DEVICE
  handle, out = C.c_void_p(), _lib.DvRealignOutput()
  opt = _realign_options()
  rc = _lib.lib().dv_realign_regions_device(None, 0, C.byref(opt), None, C.byref(handle), C.byref(out), None)
  assert rc == _lib.DV_ERR_NO_DEVICE and not handle.value
  # the host route is untouched by all this
  assert _lib.lib().dv_realign_regions(None, 0, C.byref(opt), C.byref(handle), C.byref(out)) == _lib.DV_OK
  _lib.lib().dv_realign_result_free(handle)


# ---------------------------------------------------------------- align_reads in phases
class _Recorder:
  """Stands in for Realigner._aligner: builds the real aligner and notes what it was given."""

  def __init__(self, realigner, log):
    self._make, self._log = realigner._aligner, log      # pylint: disable=protected-access

  def __call__(self, read_size, force_alignment, prefix_len, suffix_len):
    aligner = self._make(read_size, force_alignment, prefix_len, suffix_len)
    entry = dict(read_size=read_size, prefix_len=prefix_len, suffix_len=suffix_len)
    log = self._log
    set_reference, set_haplotypes, realign_reads = aligner.set_reference, aligner.set_haplotypes, aligner.realign_reads

    def note_reference(reference, ref_start=0):
      entry['reference'], entry['ref_start'] = reference, ref_start
      return set_reference(reference, ref_start)

    def note_haplotypes(haplotypes):
      entry['haplotypes'] = list(haplotypes)
      return set_haplotypes(haplotypes)

    def note_reads(reads):
      entry['sequences'] = [r.aligned_sequence for r in reads]
      log.append(entry)
      return realign_reads(reads)

    aligner.set_reference, aligner.set_haplotypes, aligner.realign_reads = note_reference, note_haplotypes, note_reads
    return aligner


_WINDOWS = []


def _windows():
  """The aligner inputs of every assembled window of the two known-answer regions and of the first
  3 kb of the golden slice (oracle counts pick the windows: no GPU in this file)."""
  if _WINDOWS:
    return _WINDOWS
  from deepvariant_amd.realigner import realigner as R
  from deepvariant_amd.realigner import utils as U
  ref, sets = RF.load()
  rl = R.Realigner(R.realigner_config(), ref)
  rl._aligner = _Recorder(rl, _WINDOWS)                   # pylint: disable=protected-access
  with RF.oracle_allele_counter():
    rl.realign_reads(sets['ex1'], T.Range('chr20', 10_095_378, 10_095_500))
    rl.realign_reads(sets['ex2'], T.Range('chr20', 10_046_079, 10_046_307))
    reads = sets['wgs']
    spans = [U.read_range(r) for r in reads]
    for start in range(9_999_999, 10_002_999, 1000):
      region = T.Range('chr20', start, start + 1000)
      rl.realign_reads([r for r, s in zip(reads, spans) if U.ranges_overlap(s, region)], region)
  return _WINDOWS


def _align(window, in_phases, **kw):
  a = F.FastPassAligner(read_size=window['read_size'], ref_prefix_len=window['prefix_len'],
                        ref_suffix_len=window['suffix_len'], **kw)
  a.set_reference(window['reference'], window['ref_start'])
  a.set_haplotypes(window['haplotypes'])
  a.stage(ALIGN_IN_PHASES, int(in_phases))
  result = a.align_reads(window['sequences'])
  per_haplotype = [(a.haplotype_alignment(k), [a.read_alignment(k, r) for r in range(len(window['sequences']))])
                   for k in range(len(window['haplotypes']))]
  return result, per_haplotype


@pytest.mark.parametrize('kw', [dict(), dict(force_alignment=True), dict(normalize_reads=True),
                                dict(match=2, mismatch=2, gap_open=3, gap_extend=1, force_alignment=True)])
def test_align_reads_in_phases_equals_align_reads(kw):
  windows = _windows()
  assert len(windows) >= 4
  moved = local = 0
  for w in windows:
    want, want_state = _align(w, False, **kw)
    got, got_state = _align(w, True, **kw)
    assert got == want
    assert got_state == want_state          # haplotype CIGARs, positions, scores, every read's alignment to each
    moved += sum(1 for status, _, _ in want if status == 1)
    local += sum(1 for _, reads in want_state for ra in reads if any(c in ra.cigar for c in 'XIDS'))
  assert moved > 20 and local > 0           # the windows do go through the local aligner


def test_unknown_stage_is_still_refused():
  a = F.FastPassAligner()
  assert _lib.lib().dv_aligner_stage(a._h, 7, 0) == _lib.DV_ERR_INVALID_ARGUMENT     # pylint: disable=protected-access
