"""dv_fast_pass_batch_device (csrc/fast_pass.hip: the fast pass of every (window, haplotype) in one kernel launch)
against dv_fast_pass_batch, the host code, array for array, on the hand-made windows of tests/fast_pass_cases.py --
the smallest shapes at which the kernel can go wrong -- and on seeded ones.  The stats keep a run that never reached
the device from passing: one launch, nothing on the host unless the case is about the limits."""
import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import fast_pass_aligner as F
from tests import fast_pass_cases as K

pytestmark = pytest.mark.gpu
CAP = _lib.DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE


def _compare(windows, options, on_host=0):
  want = F.fast_pass_batch(windows, options)
  got, stats = F.fast_pass_batch_device(windows, options, with_stats=True)
  assert len(got) == len(want) == len(windows)
  for w, g, x in zip(windows, got, want):
    assert sorted(g) == sorted(x)
    for name in x:
      assert g[name].dtype == x[name].dtype and g[name].shape == x[name].shape, (w['name'], name)
      assert np.array_equal(g[name], x[name]), (w['name'], name, g[name].tolist(), x[name].tolist())
  n_haplotypes = sum(len(w['haplotypes']) for w in windows)
  assert stats.haplotypes == n_haplotypes and stats.haplotypes_on_host == on_host
  assert stats.launches == (1 if n_haplotypes > on_host else 0)
  return got, stats


@pytest.mark.parametrize('w', K.hand_made(), ids=lambda w: w['name'])
def test_hand_made_case(w):
  got, stats = _compare([w], w['options'])
  k = w['options']['kmer_size']
  pairs = sum(1 for h in w['haplotypes'] for r in w['reads'] if k < len(r) <= len(h))
  assert stats.pairs == pairs
  assert stats.cells == sum((len(h) - k + 1) * len(r) for h in w['haplotypes'] for r in w['reads'] if k < len(r) <= len(h))
  if w['expect_discarded'] is not None:
    assert got[0]['haplotype_discarded'].tolist() == w['expect_discarded']


def test_all_hand_made_cases_of_one_k_in_one_call():
  cases = K.hand_made()
  for k in sorted({w['options']['kmer_size'] for w in cases}):
    same = [w for w in cases if w['options'] == dict(kmer_size=k)]
    if len(same) > 1:
      _compare(same, same[0]['options'])


def test_one_byte_over_the_cap_goes_to_the_host_inside_the_call():
  w = K.over_the_cap(CAP)
  assert [len(h) for h in w['haplotypes']] == [CAP + 1, CAP]
  got, stats = _compare([w], w['options'], on_host=1)
  assert got[0]['read_position'][0].tolist() == [0, 8153, 8152, 4000, 100]
  assert got[0]['haplotype_discarded'].tolist() == [0, 1]
  assert stats.pairs == len(w['reads'])            # the pairs of the haplotype that stayed on the device


def test_scoring_past_the_kernels_limit_goes_to_the_host():
  w = dict(K.seeded(3, 1)[0])
  options = dict(w['options'], match=_lib.DV_FAST_PASS_DEVICE_MAX_SCORING + 1)
  _compare([w], options, on_host=len(w['haplotypes']))
  _compare([w], dict(options, match=_lib.DV_FAST_PASS_DEVICE_MAX_SCORING, mismatch=1))


@pytest.mark.parametrize('seed', [1, 2, 3, 4])
def test_seeded_windows(seed):
  windows = K.seeded(seed, 6)
  got, stats = _compare(windows, windows[0]['options'])
  assert sum(int((g['read_position'] >= 0).sum()) for g in got) > 50 and stats.pairs > 0 and stats.cells > 0


def test_two_hundred_small_windows_in_one_call():
  windows = K.seeded(9, 200, small=True)
  got, _ = _compare(windows, windows[0]['options'])
  flags = np.concatenate([g['haplotype_discarded'] for g in got])
  assert 0 < int(flags.sum()) < len(flags)


def test_a_second_call_on_the_same_thread_reuses_its_buffers():
  big, small = K.seeded(2, 6), K.seeded(9, 3, small=True)
  _compare(big, big[0]['options'])
  _compare(small, small[0]['options'])
  _compare(big, big[0]['options'])
