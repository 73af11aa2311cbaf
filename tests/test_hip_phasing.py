"""dv_phase_reads_batch_device (csrc/phasing.hip: a workgroup per region) against dv_phase_reads_batch -- the checker
in a loop -- on the cases of phasing_cases.py: every output equal, the regions really phased on the device
(regions_on_host), one launch per call, the same answers twice, in reversed order and on a caller's stream; the dense
and the edge cases take the read sets to 16 words, the sites to 8 vertices and the scores past 2^16."""
import pytest

from tests import phasing_cases as pc

pytestmark = pytest.mark.gpu


def inside_cases():
  return pc.vector_cases() + [pc.EMPTY, pc.NO_CANDIDATES] + pc.named_cases() + pc.generated_cases(200)


@pytest.fixture(scope='module')
def inside():
  """(cases, the host entry's answers for min_alleles_to_phase 1 and 2): computed once, read only."""
  cases = inside_cases()
  want = {m: pc.run_batch(cases, m, device=False) for m in (1, 2)}
  for _, stats in want.values():
    assert stats['regions_on_host'] == 0          # or the device test would pass on host completion
  return cases, want


def assert_same(got, want, cases):
  assert len(got) == len(want) == len(cases)
  for case, g, w in zip(cases, got, want):
    assert pc.same(g, w), case['name']


@pytest.mark.parametrize('min_alleles_to_phase', [1, 2])
def test_same_cases_on_the_device(inside, min_alleles_to_phase):
  cases, want = inside
  got, stats = pc.run_batch(cases, min_alleles_to_phase, device=True)
  assert_same(got, want[min_alleles_to_phase][0], cases)
  host_stats = want[min_alleles_to_phase][1]
  assert stats['regions'] == len(cases) and stats['regions_on_host'] == 0 and stats['launches'] == 1
  assert stats['sites_in_graphs'] == host_stats['sites_in_graphs'] > 0
  assert stats['vertices'] == host_stats['vertices'] > 0
  assert stats['combinations'] > stats['sites_in_graphs']       # the kernel scored them, not the host


def test_limits():
  """A region at the reads-per-region limit and one at the vertices-per-site limit run on the device; one past
  either, a read under two alleles of one site and a text twice at a site get the checker's answer from the host
  code inside the same call."""
  at, over = pc.at_limit_cases(), pc.over_limit_cases()
  cases = at + over + pc.named_cases()[:2]
  want, _ = pc.run_batch(cases, 1, device=False)
  got, stats = pc.run_batch(cases, 1, device=True)
  assert_same(got, want, cases)
  assert stats['regions_on_host'] == len(over) and stats['launches'] == 1
  for case, g in zip(cases, got):
    assert pc.same(g, pc.reference(case, 1)), case['name']
  # only regions outside the limits: nothing is launched
  got, stats = pc.run_batch(over, 1, device=True)
  assert_same(got, want[len(at):len(at) + len(over)], over)
  assert stats['regions_on_host'] == len(over) and stats['launches'] == 0 and stats['combinations'] == 0


@pytest.fixture(scope='module')
def dense():
  """(the dense and the edge cases, the host entry's answers and stats for min_alleles_to_phase 1, 2 and 3): computed
  once, read only.  Read sets of 1-16 bitmap words, sites of up to MAX_VERTICES vertices with real edges, scores past
  2^16, vertices without reads (tests/test_phasing_batch_cpu.py asserts that the generator reaches them)."""
  cases = pc.dense_cases(126) + pc.edge_cases()
  want = {m: pc.run_batch(cases, m, device=False) for m in (1, 2, 3)}
  for _, stats in want.values():
    assert stats['regions_on_host'] == 0          # or the device test would pass on host completion
  return cases, want


@pytest.mark.parametrize('min_alleles_to_phase', [1, 2, 3])
def test_dense_regions_on_the_device(dense, min_alleles_to_phase):
  cases, want = dense
  got, stats = pc.run_batch(cases, min_alleles_to_phase, device=True)
  assert_same(got, want[min_alleles_to_phase][0], cases)
  host_stats = want[min_alleles_to_phase][1]
  assert stats['regions'] == len(cases) and stats['regions_on_host'] == 0 and stats['launches'] == 1
  assert stats['sites_in_graphs'] == host_stats['sites_in_graphs'] > 0
  assert stats['vertices'] == host_stats['vertices'] > 0
  assert stats['combinations'] > stats['vertices']              # the kernel scored them, not the host


def test_host_regions_between_large_device_regions(dense):
  """The host's regions among device regions of 1000-1024 reads: a device region's place in the downloaded phases
  (the device regions' reads before it) and in the call's phases (all reads before it) differ by thousands."""
  large = [c for c in dense[0] if c['name'].startswith('dense_') and c['n_reads'] >= 1000]
  over = pc.over_limit_cases()
  assert len(large) == 18 and len(over) == 4
  cases = []
  for k, case in enumerate(large):
    if k % 5 == 0:                                  # before large regions 0, 5, 10 and 15
      cases.append(over[k // 5])
    cases.append(case)
  assert len(cases) == 22 and cases[0] is over[0] and cases[-4] is over[3]
  want, _ = pc.run_batch(cases, 1, device=False)
  got, stats = pc.run_batch(cases, 1, device=True)
  assert_same(got, want, cases)
  for case, g in zip(cases, got):
    assert pc.same(g, pc.reference(case, 1)), case['name']
  assert stats['regions'] == len(cases) and stats['regions_on_host'] == 4 and stats['launches'] == 1
  backward, stats = pc.run_batch(cases[::-1], 1, device=True)
  assert_same(backward[::-1], got, cases)
  assert stats['regions_on_host'] == 4 and stats['launches'] == 1


def test_dense_determinism(dense):
  cases, want = dense
  first, stats1 = pc.run_batch(cases, 2, device=True)
  second, stats2 = pc.run_batch(cases, 2, device=True)
  backward, _ = pc.run_batch(cases[::-1], 2, device=True)
  assert_same(first, want[2][0], cases)
  assert_same(second, first, cases)
  assert_same(backward[::-1], first, cases)
  assert stats1 == stats2


def test_determinism(inside):
  cases, want = inside
  first, stats1 = pc.run_batch(cases, 2, device=True)
  second, stats2 = pc.run_batch(cases, 2, device=True)
  backward, _ = pc.run_batch(cases[::-1], 2, device=True)
  assert_same(first, want[2][0], cases)
  assert_same(second, first, cases)
  assert_same(backward[::-1], first, cases)
  assert stats1 == stats2


def test_callers_stream(inside):
  import torch
  cases, want = inside
  stream = torch.cuda.Stream()
  got, stats = pc.run_batch(cases, 1, device=True, stream=stream.cuda_stream)
  assert_same(got, want[1][0], cases)
  assert stats['launches'] == 1 and stats['regions_on_host'] == 0
