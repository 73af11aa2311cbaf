"""The five loops that carry a running total from one workgroup-wide step to the next -- alt_finish_scan_kernel,
pack_scan_kernel and trim_scan_kernel (1,024 elements a step), cand_pack_kernel and gvcf_pack_kernel (256 regions a
step) -- on batches of exactly 1,023, 1,024, 1,025, 2,048 and 2,049 pairs or candidates and of 257 and 300 regions
with reads (tests/batch_edge_cases.py; tests/test_batch_edges_cpu.py asserts what lies on each edge).  The checkers
are those of the kernels' own test modules: the host entry points, dv_pack_region region by region, the closed form
of csrc/trim_reads.hip, the Python restatements of the candidate caller and the gVCF blocks.  Every comparison is
== on integer arrays, bytes or dataclasses (GPU)."""
import numpy as np
import pytest

from deepvariant_amd import alt_aligned_pileup_lib as A
from deepvariant_amd import allelecounter as AL
from deepvariant_amd import variant_calling as vc
from tests import alt_align_cases as AC
from tests import batch_edge_cases as E
from tests import pack_cases as PC
from tests import test_hip_alt_align as HA
from tests import test_hip_candidates as HC
from tests import test_hip_gvcf as HG
from tests import test_hip_pack_regions as HP
from tests import trim_cases as TC

pytestmark = pytest.mark.gpu

_ALT_HOST = {}


# ---------------------------------------------------------------- alt-align
def _alt(n_pairs, normalize_reads, device):
  b = E.edge_alt_align(n_pairs)
  if not device and (n_pairs, normalize_reads) in _ALT_HOST:
    return _ALT_HOST[(n_pairs, normalize_reads)]
  d = A.alt_align_arrays(E.alt_align_table(n_pairs), b['items'], b['targets'],
                         dict(b['cfg'], normalize_reads=normalize_reads), device=device)
  if not device:
    _ALT_HOST[(n_pairs, normalize_reads)] = d
  return d


def _check_alt(n_pairs, normalize_reads, what):
  got = _alt(n_pairs, normalize_reads, device=True)
  HA._assert_same(got, _alt(n_pairs, normalize_reads, device=False), what)    # pylint: disable=protected-access
  HA._assert_stats_add_up(got)                                                  # pylint: disable=protected-access
  st = got['stats']
  # every pair went through the device's kernels: a fallback to the host cannot pass
  assert st['pairs'] == n_pairs and st['items_on_host'] == 0 and st['pairs_swept_on_host'] == 0
  assert st['launches'] == 5 and st['pairs_fast'] > 0 and st['pairs_swept'] > 0
  return got


@pytest.mark.parametrize('normalize_reads', [0, 1])
@pytest.mark.parametrize('n_pairs', E.SCAN_SIZES)
def test_alt_align_across_the_scan_step(n_pairs, normalize_reads, monkeypatch):
  monkeypatch.delenv('DV_REALIGN_DEVICE_TRACEBACK', raising=False)
  _check_alt(n_pairs, normalize_reads, ('alt-align', n_pairs, normalize_reads))


def test_alt_align_2049_pairs_with_the_device_traceback_then_a_small_batch(monkeypatch):
  """Three steps of the scan with the trace-back on the device, and then the 14-pair `kinds` batch on the same
  thread: the staging has grown and is reused smaller."""
  monkeypatch.setenv('DV_REALIGN_DEVICE_TRACEBACK', '1')
  for normalize_reads in (0, 1):
    _check_alt(2049, normalize_reads, ('alt-align with trace-back', normalize_reads))
  monkeypatch.delenv('DV_REALIGN_DEVICE_TRACEBACK')
  _check_alt(2049, 0, 'alt-align, 2,049 pairs')
  kinds = AC.kinds_batch()
  table = AC.table_of(kinds)
  for normalize_reads in (0, 1):
    cfg = dict(kinds['cfg'], normalize_reads=normalize_reads)
    got = A.alt_align_arrays(table, kinds['items'], kinds['targets'], cfg, device=True)
    want = A.alt_align_arrays(table, kinds['items'], kinds['targets'], cfg, device=False)
    HA._assert_same(got, want, ('kinds after 2,049 pairs', normalize_reads))   # pylint: disable=protected-access
    assert got['stats']['pairs'] == 14 and got['stats']['items_on_host'] == 0


# ---------------------------------------------------------------- pack
def _item_range(want, first_cand, n_cands):
  sel = np.nonzero((want['item_candidate'] >= first_cand) & (want['item_candidate'] < first_cand + n_cands))[0]
  return int(sel[0]), int(sel[-1]) + 1


@pytest.mark.parametrize('use_groups', [0, 1])
@pytest.mark.parametrize('n_cands', E.SCAN_SIZES)
def test_pack_across_the_scan_step(n_cands, use_groups):
  regions = list(E.edge_pack_regions(n_cands).regions)
  want = E.pack_expected(n_cands, use_groups)
  got, filled, stats = HP._device(regions, use_groups)                          # pylint: disable=protected-access
  HP._assert_same(got, want, use_groups, 'pack, %d candidates' % n_cands)       # pylint: disable=protected-access
  n_items, n_list = len(want['item_height']), len(want['list_read'])
  assert n_items > n_cands and n_list > 10 * n_cands
  assert stats == dict(regions=len(regions), candidates=n_cands, items=n_items, list_entries=n_list,
                       regions_unsorted=sum(not r.sorted and bool(r.candidates) for r in regions), launches=3)
  assert filled == dict(n_items=n_items, n_list=n_list, max_list_len=want['max_list_len'], has_groups=bool(use_groups),
                        blank=None, has_lists=True)
  # placement is a pure function of the input
  again, _, _ = HP._device(regions, use_groups)                                 # pylint: disable=protected-access
  for name in HP._NAMES + (('list_group',) if use_groups else ()):              # pylint: disable=protected-access
    assert got[name].tobytes() == again[name].tobytes(), name


def test_pack_candidates_with_257_and_513_masks_item_by_item():
  """pack_emit_kernel's item loop takes a second and a third step: every item's record and list, one by one."""
  case = E.edge_pack_regions(1025)
  regions = list(case.regions)
  k = [r.name for r in regions].index('wide')
  first_cand = sum(len(r.candidates) for r in regions[:k])
  want = E.pack_expected(1025, 1)
  got, _, _ = HP._device(regions, 1)                                            # pylint: disable=protected-access
  lo, hi = _item_range(want, first_cand, 2)
  assert hi - lo == sum(E.WIDE_COMBOS)
  masks = [m for c in regions[k].candidates for m in c.masks]
  for item in range(lo, hi):
    assert got['item_candidate'][item] == first_cand + (item - lo >= E.WIDE_COMBOS[0]), item
    assert got['item_combo'][item] == masks[item - lo] == want['item_combo'][item], item
    a, b = int(want['item_list_off'][item]), int(want['item_list_off'][item + 1])
    assert (int(got['item_list_off'][item]), int(got['item_list_off'][item + 1])) == (a, b) and b - a == 65, item
    for name in ('list_read', 'list_code', 'list_group'):
      assert got[name][a:b].tobytes() == want[name][a:b].tobytes(), (item, name)
  # alone, where the two candidates are elements 0 and 1 of the scan
  alone, _, _ = HP._device([regions[k]], 1)                                     # pylint: disable=protected-access
  HP._assert_same(alone, PC.expected([regions[k]], 1), 1, 'wide alone')         # pylint: disable=protected-access


def test_the_shared_batch_is_still_right_after_2049_candidates():
  for use_groups in (1, 0):
    got, _, _ = HP._device(list(E.edge_pack_regions(2049).regions), use_groups)     # pylint: disable=protected-access
    HP._assert_same(got, E.pack_expected(2049, use_groups), use_groups, 'pack, 2,049 candidates')   # pylint: disable=protected-access
    got, _, stats = HP._device(PC.batch(), use_groups)                          # pylint: disable=protected-access
    HP._assert_same(got, HP._want(use_groups), use_groups, 'the 136-candidate batch afterwards')    # pylint: disable=protected-access
    assert stats['candidates'] == 136 and stats['launches'] == 3


# ---------------------------------------------------------------- trim
@pytest.mark.parametrize('n_pairs', E.SCAN_SIZES)
def test_trim_across_the_scan_step(n_pairs):
  case, table = E.edge_trim(n_pairs), E.trim_table(n_pairs)
  want, kept, _ = E.trim_expected(n_pairs)
  host = A.trim_arrays(table, case.windows, device=False)
  got = A.trim_arrays(table, case.windows, device=True)
  TC.assert_same_arrays(got, host, '%s (device vs host entry)' % case.name)
  TC.assert_same_arrays(got, want, '%s (device vs the closed form)' % case.name)
  st = got['stats']
  assert st['pairs_tested'] == n_pairs and st['pairs_kept'] == len(got['src_row']) == int(kept.sum())
  assert st['words_written'] == len(got['cigar']) and st['launches'] == 3
  TC.assert_same_arrays(A.trim_arrays(table, case.windows, device=True), got, '%s (second call)' % case.name)


# ---------------------------------------------------------------- candidates
# The sizes count the regions WITH reads: only those get a workgroup of the pack kernels (see
# batch_edge_cases.edge_regions); the readless regions between them are part of every batch below.
@pytest.mark.parametrize('track', [False, True])
@pytest.mark.parametrize('n,overflow_at', [(257, None), (300, None), (300, 260)])
def test_candidates_past_256_regions(n, overflow_at, track):
  case = E.edge_regions(n, overflow_at)
  caller = HC._caller(track=track)                                              # pylint: disable=protected-access
  calls, counters = HC._two_ways(lambda positions: E.counters(case, positions, track), caller, track)   # pylint: disable=protected-access
  # an empty answer cannot pass: every SNP region has one call, every indel region two (the noisy region 400)
  assert len(calls) >= sum(kind == 'snp' for kind in case.kinds) + 2 * sum(kind == 'indels' for kind in case.kinds)
  per_region = [caller.calls_from_allele_counter(c) for c in counters]
  for kind, got in zip(case.kinds, per_region):
    assert len(got) == {'snp': 1, 'indels': 2, 'readless': 0, 'quiet': 0, 'noisy': 400}[kind], kind
  # the regions from slot 256 on as a batch of their own: no workgroup of theirs takes a second step of the sum
  lo = E.region_of_slot(case, E.REGION_STEP)
  positions = [[c.variant.start for c in got] for got in per_region]
  tail = E.counters(case, positions[lo:] if track else None, track, lo=lo)
  AL.AlleleCounter.run_batch(tail, call=caller.candidate_options())
  assert [caller.calls_from_allele_counter(c) for c in tail] == per_region[lo:]
  assert len(per_region[lo]) == 2 and (n == E.REGION_STEP + 1 or sum(map(len, per_region[lo + 1:])) > 20)
  for t, c in zip(tail, counters[lo:]):
    for x, y in zip(t._cand[1:], c._cand[1:]):                                  # sites, alleles, words   pylint: disable=protected-access
      assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---------------------------------------------------------------- gVCF
_GVCF = vc.GvcfOptions('s', include_med_dp=True)


@pytest.mark.parametrize('n', E.REGION_SIZES)
def test_gvcf_past_256_regions(n):
  case = E.edge_regions(n)
  together = E.counters(case)
  n_blocks = HG._check(together, _GVCF, min_blocks=len(together))              # pylint: disable=protected-access
  per_region = [len(c.gvcf_block_array(_GVCF)) for c in together]
  assert sum(per_region) == n_blocks and len(set(per_region)) > 1 and min(per_region) >= 1
  # the regions from slot 250 on against the same regions run as a batch of their own, byte for byte
  lo = E.region_of_slot(case, 250)
  alone = E.counters(case, lo=lo)
  AL.AlleleCounter.run_batch(alone, gvcf=_GVCF)
  for a, t in zip(alone, together[lo:]):
    assert a.gvcf_block_array(_GVCF).tobytes() == t.gvcf_block_array(_GVCF).tobytes()


def test_gvcf_and_candidates_in_one_pass_past_256_regions():
  """run_batch(gvcf=..., call=...) on 300 regions with reads: the records of run_batch(gvcf=...) bit for bit and
  the same candidates, as test_hip_candidates.test_with_gvcf_in_one_pass has it for four regions."""
  case = E.edge_regions(300)
  caller = HC._caller()                                                         # pylint: disable=protected-access
  calls, both = HC._two_ways(lambda positions: E.counters(case, positions), caller, gvcf=_GVCF)   # pylint: disable=protected-access
  assert len(calls) >= sum(kind == 'snp' for kind in case.kinds)
  only = E.counters(case)
  AL.AlleleCounter.run_batch(only, gvcf=_GVCF)
  for b, o in zip(both, only):
    assert b._gvcf is not None and b.gvcf_block_array(_GVCF).tobytes() == o.gvcf_block_array(_GVCF).tobytes()   # pylint: disable=protected-access
  for b in both[E.region_of_slot(case, 250):]:
    HG._same(b.gvcf_blocks(_GVCF), HG._host(b, _GVCF))                          # pylint: disable=protected-access
