"""compact_batch_device (csrc/debruijn.hip: every window's graph, the choice of k and the cycle test included, in one
kernel launch) against compact_batch (the host's own constructor): identical arrays on the hand-made windows of
tests/assembly_cases.py and on the 160 seeded ones, stats that keep a run that never reached the device from passing,
and the windows past the kernel's limits -- the one sorted out before the launch and the ones the kernel finds at run
time (AC.limit_windows()) -- built by the host inside the same call."""
import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd.realigner import debruijn_graph
from tests import assembly_cases as AC

pytestmark = pytest.mark.gpu

_DEFAULT = debruijn_graph.DeBruijnGraphOptions()     # min_k 10, max_k 101, step_k 1: the realigner's


def _pairs(cases):
  return [(c[1], c[2]) for c in cases]


def _bases(case):
  return len(case[1]) + sum(len(r.aligned_sequence) for r in case[2])


def _compare(cases, opts, on_host=0):
  """One batch through both routes; -> (device graphs, stats).  on_host: the windows of `cases` that the kernel hands
  back to the host at run time."""
  want = debruijn_graph.compact_batch(_pairs(cases), opts)
  got, stats = debruijn_graph.compact_batch_device(_pairs(cases), opts, with_stats=True)
  assert len(got) == len(want) == len(cases)
  for case, a, b in zip(cases, got, want):
    assert a.k == b.k and a.k_tries == b.k_tries, case[0]
    for name in debruijn_graph.CompactGraph.ARRAYS:
      assert np.array_equal(getattr(a, name), getattr(b, name)), (case[0], name)
  # with on_host == 0 all are under the limits (checked on the host's graphs), so nothing may have gone back to the host
  past = sum(len(g.vertex_seq) > _lib.DV_DEBRUIJN_DEVICE_MAX_VERTICES or len(g.edge_from) > _lib.DV_DEBRUIJN_DEVICE_MAX_EDGES
             for g in want)
  assert past <= on_host                          # a window past them at a k that did not win has no such graph
  assert max(_bases(c) for c in cases) <= _lib.DV_DEBRUIJN_DEVICE_MAX_BASES
  assert stats.windows == len(cases) and stats.launches == 1 and stats.windows_on_host == on_host
  assert stats.windows_rejected == 0 and stats.kmers > 0
  assert stats.k_tries == sum(g.k_tries for g in want)
  return got, stats


def test_hand_made_windows_in_one_batch():
  cases = AC.hand_made()
  groups = AC.batches(cases)
  assert len(groups) == 2 and len(groups[0][1]) == len(cases) - 1          # all but step_k = 2 share their options
  for opts, group in groups:
    got, _ = _compare(group, opts)
    assert any(g.k == 0 for g in got) or len(group) == 1                  # the windows without a graph are among them
  # and all of them under one set of options, whatever each was made for
  _compare(cases, AC.options())


def test_zero_windows_need_no_launch():
  graphs, stats = debruijn_graph.compact_batch_device([], AC.options(), with_stats=True)
  assert graphs == [] and stats.launches == 0 and stats.windows == 0


@pytest.fixture(scope='module')
def generated():
  return [c for seed in AC.SEEDS for c in AC.generated(seed)]


def test_generated_windows_in_one_batch(generated):
  assert len(generated) == 160
  assert max(len(c[2]) for c in generated) <= 139 and max(len(c[1]) for c in generated) < 380
  got, _ = _compare(generated, _DEFAULT)
  assert sum(g.k > 0 for g in got) > 100 and len({g.k for g in got}) > 5


def test_generated_windows_under_their_own_options(generated):
  groups = AC.batches(generated)
  assert len(groups) > 6 and {opts.step_k for opts, _ in groups} == {1, 2}
  for opts, group in groups:
    _compare(group, opts)


def test_the_same_batch_twice_gives_identical_bytes(generated):
  cases = generated[:40] + AC.hand_made()
  first = debruijn_graph.compact_batch_device(_pairs(cases), _DEFAULT)
  second = debruijn_graph.compact_batch_device(_pairs(cases), _DEFAULT)
  for a, b in zip(first, second):
    assert (a.k, a.k_tries) == (b.k, b.k_tries)
    for name in debruijn_graph.CompactGraph.ARRAYS:
      assert getattr(a, name).tobytes() == getattr(b, name).tobytes()


_LONG = AC.options(min_k=18)       # random reads of this size repeat shorter k-mers by chance: fewer k to try


def _over_the_limit():
  """One window past DV_DEBRUIJN_DEVICE_MAX_BASES: many long random reads over a short reference."""
  rng = np.random.default_rng(5)
  ref = AC.random_bases(21, 200)
  n_reads, length = 64, _lib.DV_DEBRUIJN_DEVICE_MAX_BASES // 64 + 1
  reads = [AC.read(''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=length)), name='x%d' % i)
           for i in range(n_reads)]
  assert len(ref) + n_reads * length > _lib.DV_DEBRUIJN_DEVICE_MAX_BASES
  return ('over the limit', ref, reads, _LONG)


def test_a_window_over_the_limit_is_built_by_the_host_inside_the_call():
  big = _over_the_limit()
  cases = AC.hand_made()[:3] + [big]
  want = debruijn_graph.compact_batch(_pairs(cases), _LONG)
  got, stats = debruijn_graph.compact_batch_device(_pairs(cases), _LONG, with_stats=True)
  for a, b in zip(got, want):
    assert AC.same_graph(a, b)
  assert want[-1].k > 0
  assert stats.windows == 4 and stats.windows_on_host == 1 and stats.launches == 1
  # alone, it leaves nothing to launch
  got, stats = debruijn_graph.compact_batch_device(_pairs([big]), _LONG, with_stats=True)
  assert AC.same_graph(got[0], want[-1])
  assert stats.windows == 1 and stats.windows_on_host == 1 and stats.launches == 0


_HANDED_BACK = ('vertices_over', 'table_full', 'edges_over')       # of AC.limit_windows(), by the kernel at run time


def _among_neighbours(group):
  hand = AC.hand_made()
  return hand[:3] + group + hand[3:6]


def test_windows_at_and_past_the_run_time_limits():
  """AC.limit_windows() (tests/test_debruijn_compact_cpu.py asserts their sizes on the host's graphs) between small
  windows, in one launch per set of graph options: just_under is the device's own with its tables at their fullest;
  a graph past MAX_VERTICES or MAX_EDGES and a vertex table whose probe runs out are found by the kernel, built by the
  host inside the call, with the host's k_tries, and leave their neighbours' outputs alone."""
  groups = AC.batches(AC.limit_windows())
  assert [[c[0] for c in group] for _, group in groups] == [['just_under', 'vertices_over', 'table_full'], ['edges_over']]
  for opts, group in groups:
    cases = _among_neighbours(group)
    on_host = sum(c[0] in _HANDED_BACK for c in cases)
    assert on_host == len(group) - (group[0][0] == 'just_under') > 0
    got, _ = _compare(cases, opts, on_host=on_host)      # every window's arrays, the neighbours' included
    assert [g.k for g in got[3:3 + len(group)]] == [0 if c[0] == 'edges_over' else opts.min_k for c in group]
    # the same batch again: identical bytes
    again = debruijn_graph.compact_batch_device(_pairs(cases), opts)
    for a, b in zip(got, again):
      assert (a.k, a.k_tries) == (b.k, b.k_tries)
      for name in debruijn_graph.CompactGraph.ARRAYS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes()


def test_a_window_just_under_the_limits_is_the_devices():
  just_under = AC.limit_windows()[0]
  assert just_under[0] == 'just_under'
  got, stats = _compare([just_under], just_under[3])
  assert got[0].k == just_under[3].min_k and stats.k_tries == 1
  assert len(got[0].vertex_seq) >= 0.95 * _lib.DV_DEBRUIJN_DEVICE_MAX_VERTICES
