"""dv_genotype_sites, the host code of the genotype merge, against the plain-Python restatement of
tests/genotype_cases.py: every array with ==.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import call_variants as cv
from deepvariant_amd import postprocess_variants as pp
from tests import genotype_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = G.cases()


def assert_equals_reference(result, want):
  assert result.rounded.tolist() == want['rounded']
  assert result.pred_off.tolist() == want['pred_off']
  assert result.predictions.tolist() == want['predictions']
  assert result.best.tolist() == want['best']
  assert result.removed.tolist() == want['removed']
  assert result.status.tolist() == want['status']


def host(name):
  probs, sites, t = CASES[name]
  return pp.genotype_sites(probs, *pp.site_tables(sites), t=t)


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_code_equals_the_restatement(name):
  probs, sites, t = CASES[name]
  assert_equals_reference(host(name), G.reference(probs, sites, t))


def test_default_threshold_is_the_recorded_one():
  assert pp.min_nonref_prob(1.0) == G.T1


# ---------------------------------------------------------------------------------------------- step 1
def test_hand_made_rows_round_as_round_gls_batch():
  rows = G.hand_made_rows()
  names = list(rows)
  result = host('hand_made_rows')
  good = [k for k, n in enumerate(names) if n != 'bad_sum']
  probs = np.stack([rows[n] for n in names])
  assert G.sums_to_one(probs).tolist() == [n != 'bad_sum' for n in names]
  assert (result.rounded[good] == cv.round_gls_batch(probs[good], 10)).all()
  assert result.status.tolist() == [pp.BAD_SUM if n == 'bad_sum' else pp.OK for n in names]
  with pytest.raises(ValueError, match='do not sum to one'):
    cv.round_gls_batch(probs, 10)
  by_name = dict(zip(names, result.rounded.tolist()))
  # the minimum's first index takes the residual
  assert by_name['tie_0_1'] == [0.25, 0.25, 0.5] and by_name['one_zero_zero'] == [1.0, 0.0, 0.0]
  tiny = float(rows['below_1e-3'][1])
  assert tiny < 1e-3 and by_name['below_1e-3'][1] != tiny            # rintf acted on it ...
  assert by_name['below_1e-3'][1] == float(np.round(rows['below_1e-3'][1], 10))
  assert by_name['clamps'][int(np.argmin(rows['clamps']))] == 0.0     # ... and this residual clamped


def test_seeded_rows_round_as_round_gls_batch():
  probs, sites, _ = CASES['dirichlet_4096']
  assert probs.shape == (4096, 3) and G.sums_to_one(probs).all()
  result = host('dirichlet_4096')
  want = cv.round_gls_batch(probs, 10)
  assert (result.rounded == want).all()
  # a site of one item keeps its rounded values as they are
  assert (result.predictions.reshape(-1, 3) == want).all() and (result.status == pp.OK).all()
  # the rows exercise what the rounding does: hundreds of each
  changed = (want != probs.astype(np.float64)).any(axis=1)
  lowest = np.argmin(probs, axis=1)
  clamped = (want[np.arange(4096), lowest] == 0.0) & (probs[np.arange(4096), lowest] > 0)
  ordered = np.sort(probs, axis=1)
  tied = ordered[:, 0] == ordered[:, 1]
  assert changed.sum() >= 3000 and clamped.sum() >= 300, (changed.sum(), clamped.sum())
  assert tied.sum() >= 10, tied.sum()      # 0.8 % of the rows tie at the minimum


# ---------------------------------------------------------------------------------------------- steps 2 and 3
def test_merge_known_answers():
  r = host('a2_complete')
  assert r.removed.tolist() == [0] and r.status.tolist() == [pp.OK] and r.n_kept_alts(0) == 2
  assert math.isclose(sum(r.site_predictions(0)), 1.0, rel_tol=1e-15)
  assert host('a2_alt0_removed').removed.tolist() == [1]
  assert host('a2_alt1_removed').removed.tolist() == [2]
  assert host('a2_both_below_best_stays').removed.tolist() == [1]      # alt 1 has the larger score
  assert host('a2_both_below_tie_first_stays').removed.tolist() == [2]
  assert host('a2_s_equals_t').removed.tolist() == [0]
  assert host('a2_s_just_below_t').removed.tolist() == [2]
  assert host('a2_qual_filter_0').removed.tolist() == [0]
  r = host('a2_alt0_removed')
  assert r.n_kept_alts(0) == 1 and len(r.site_predictions(0)) == 3
  assert r.predictions[3:].tolist() == [0.0, 0.0, 0.0]                  # slots by the unpruned alts, the rest 0
  incomplete = host('a2_singles_only_incomplete')
  assert incomplete.status.tolist() == [pp.INCOMPLETE] and incomplete.best.tolist() == [-1]
  assert incomplete.predictions[4] == math.inf                         # genotype (1, 2) got no contribution
  assert host('a2_no_items_incomplete').status.tolist() == [pp.INCOMPLETE, pp.OK]
  assert host('bad_sum_in_a2').status.tolist() == [pp.BAD_SUM]
  r7 = host('a7')
  assert r7.pred_off.tolist() == [0, 36] and r7.status.tolist() == [pp.OK]
  assert any(host(n).removed[0] for n in ('a3_low', 'a6_low'))         # the seeded sites prune too
  zero = host('zero_sites')
  assert zero.pred_off.tolist() == [0] and zero.predictions.size == 0 and zero.best.size == 0


def test_rows_of_call_variants_outputs_are_not_rounded_again():
  """The rounding is not idempotent in float32, so the records' values go through as they are."""
  probs, sites, t = CASES['dirichlet_4096']
  once = cv.round_gls_batch(probs, 10)
  stored = once.astype(np.float32)
  assert (stored.astype(np.float64) == once).all()
  again = cv.round_gls_batch(stored[G.sums_to_one(stored)], 10)
  assert (again != once[G.sums_to_one(stored)]).any()
  result = pp.genotype_sites(stored, *pp.site_tables(sites), t=t, already_rounded=True)
  assert (result.rounded == once).all()
  for name in ('a3', 'a6_low', 'a7', 'bad_sum_in_a2'):
    probs, sites, t = CASES[name]
    assert_equals_reference(pp.genotype_sites(probs, *pp.site_tables(sites), t=t, already_rounded=True),
                            G.reference(probs, sites, t, already_rounded=True))


def test_item_order_does_not_matter():
  a, b = host('a3'), host('a3_shuffled')
  assert a.predictions.tolist() == b.predictions.tolist() and a.best.tolist() == b.best.tolist()
  assert a.removed.tolist() == b.removed.tolist()


def test_python_errors():
  probs, sites, t = CASES['bad_sum_in_a2']
  tables = pp.site_tables(sites)
  with pytest.raises(ValueError, match='Invalid genotype likelihoods do not sum to one'):
    pp.check_status(pp.genotype_sites(probs, *tables, t=t), lambda i: probs[i], tables[1], lambda s: 'site')
  probs, sites, t = CASES['a2_singles_only_incomplete']
  tables = pp.site_tables(sites)
  with pytest.raises(ValueError, match='do not cover every genotype'):
    pp.check_status(pp.genotype_sites(probs, *tables, t=t), lambda i: probs[i], tables[1], lambda s: 'site')


def test_bad_input():
  p = G.f32([[.2, .5, .3], [.3, .4, .3]])

  def status(item_alts, site_off, n_alts):
    a, o, n = np.array(item_alts, np.int8), np.array(site_off, np.int32), np.array(n_alts, np.int32)
    h = C.c_void_p()
    rc = _lib.lib().dv_genotype_sites(p.ctypes.data, 2, a.ctypes.data, n.size, o.ctypes.data, n.ctypes.data, G.T1, 0, C.byref(h))
    assert (rc == _lib.DV_OK) == bool(h.value)
    if h.value:
      _lib.lib().dv_genotypes_free(h)
    return rc
  assert status([[0, -1], [1, -1]], [0, 2], [2]) == _lib.DV_OK
  assert status([[0, -1], [2, -1]], [0, 2], [2]) == _lib.DV_ERR_BAD_INPUT       # an index >= A
  assert status([[0, -1], [-1, -1]], [0, 2], [2]) == _lib.DV_ERR_BAD_INPUT      # an empty set
  assert status([[0, 0], [1, -1]], [0, 2], [2]) == _lib.DV_ERR_BAD_INPUT        # one alt twice
  assert status([[0, -2], [1, -1]], [0, 2], [2]) == _lib.DV_ERR_BAD_INPUT
  assert status([[0, -1], [0, -1]], [0, 2, 1, 2], [1, 1, 1]) == _lib.DV_ERR_BAD_INPUT    # site_off descends
  assert status([[0, -1], [0, -1]], [0, 1], [1]) == _lib.DV_ERR_BAD_INPUT       # ... does not reach n_items
  assert status([[0, -1], [0, -1]], [0, 2], [0]) == _lib.DV_ERR_BAD_INPUT
  assert status([[0, -1], [0, -1]], [0, 2], [33]) == _lib.DV_ERR_BAD_INPUT
  assert 'dv_genotype_sites' in _lib.last_error()
  with pytest.raises(ValueError):
    pp.site_tables([(3, [[0, 1, 2]])])                                          # a set of three


# ---------------------------------------------------------------------------------------------- the threshold
def _phred_reaches(p, qual_filter):
  return round(-10.0 * math.log10(1.0 - min(min(p, 1.0), 1.0 - 1e-15)), 7) >= qual_filter


def _bits(x):
  return int(np.float64(x).view(np.uint64))


def _double(bits):
  return float(np.uint64(bits).view(np.float64))


@pytest.mark.parametrize('qual_filter', [1.0, 3.0, 10.0, 20.0])
def test_min_nonref_prob(qual_filter):
  lo, hi = 0, _bits(1.0)
  assert not _phred_reaches(0.0, qual_filter) and _phred_reaches(1.0, qual_filter)
  while hi - lo > 1:
    mid = (lo + hi) // 2
    if _phred_reaches(_double(mid), qual_filter):
      hi = mid
    else:
      lo = mid
  t = pp.min_nonref_prob(qual_filter)
  assert t == _double(hi)
  # `s < t` decides what the phred comparison decides, on every double within 2,000 ulps of t
  for k in range(-2000, 2001):
    s = _double(hi + k)
    assert (s < t) == (not _phred_reaches(s, qual_filter)), k


def test_min_nonref_prob_edges():
  assert pp.min_nonref_prob(0.0) == 0.0 and pp.min_nonref_prob(-1.0) == 0.0
  assert pp.min_nonref_prob(1000.0) == math.inf       # the bounded phred never reaches it


# ---------------------------------------------------------------------------------------------- the ABI
def test_abi():
  header = open(os.path.join(ROOT, 'include', 'dvhip.h')).read()
  l = _lib.lib()
  for symbol in ('dv_genotype_sites', 'dv_genotype_sites_device', 'dv_genotypes_arrays', 'dv_genotypes_free',
                 'dv_genotype_min_nonref_prob', 'dv_genotype_device_last_stats'):
    assert re.search(r'\b%s\s*\(' % symbol, header), symbol
    assert hasattr(l, symbol) and symbol in _lib.ABI_SYMBOLS
  assert int(re.search(r'#define DV_GENOTYPE_DEVICE_MAX_ALTS (\d+)', header).group(1)) == \
      _lib.DV_GENOTYPE_DEVICE_MAX_ALTS == G.DEVICE_MAX_ALTS == 6
  assert re.search(r'DV_GENOTYPE_OK = 0, DV_GENOTYPE_BAD_SUM = 1, DV_GENOTYPE_INCOMPLETE = 2', header)
  assert (pp.OK, pp.BAD_SUM, pp.INCOMPLETE) == (0, 1, 2)
  stats = re.search(r'typedef struct dv_genotype_device_stats \{(.*?)\}', header, re.S).group(1)
  assert re.findall(r'int64_t (\w+);', stats) == [n for n, _ in _lib.DvGenotypeDeviceStats._fields_]
  assert C.sizeof(_lib.DvGenotypeDeviceStats) == 32 and C.sizeof(_lib.DvGenotypesView) == 72
  assert l.dv_abi_version() == 8
  assert l.dv_genotype_device_last_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT


def test_device_entry_point_without_a_device():
  """Zero sites need no device; with sites there is no quiet fall-back to the host code."""
  if _lib.device_count() > 0:
    pytest.skip('GPU present')
  zero = pp.genotype_sites_device(np.zeros((0, 3), np.float32), *pp.site_tables([]))
  assert zero.best.size == 0
  probs, sites, t = CASES['a1']
  with pytest.raises(_lib.DvError) as e:
    pp.genotype_sites_device(probs, *pp.site_tables(sites), t=t)
  assert e.value.status == _lib.DV_ERR_NO_DEVICE
