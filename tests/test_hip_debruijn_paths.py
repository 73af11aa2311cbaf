"""paths_batch_device (csrc/debruijn.hip: the graph launch and the paths launch behind it -- pruning, the count of
walks and the walks' text in lexicographic order) against paths_batch (DeBruijnGraph::build and candidate_haplotypes,
the host's own code): k, status and the haplotypes in order on every window of tests/path_cases.py, one call per set
of options.  windows_on_host must equal the number worked out from the host's own answer, so a run that quietly fell
back does not pass; the bytes of a second call and of a call on a caller's stream are identical; and the compact
entry still gives the host's graphs afterwards."""
import pytest
import torch

from deepvariant_amd import _lib
from deepvariant_amd.realigner import debruijn_graph
from tests import assembly_cases as AC
from tests import path_cases as PC

pytestmark = pytest.mark.gpu


def _pairs(cases):
  return [(c[1], c[2]) for c in cases]


@pytest.fixture(scope='module')
def batches():
  """[(options, cases, the host's answer, the host's compact graphs)] -- computed once, never changed."""
  out = []
  for opts, group in PC.batches(PC.all_cases()):
    out.append((opts, group, debruijn_graph.paths_batch(_pairs(group), opts),
                debruijn_graph.compact_batch(_pairs(group), opts)))
  return out


def _on_host(opts, want, graphs):
  """The windows of a call the host must have computed, from the host's own answer."""
  if opts.disable_graph_pruning or opts.max_num_paths > _lib.DV_DEBRUIJN_DEVICE_MAX_PATHS:
    return len(want)
  n = 0
  for (_, _, haps), g in zip(want, graphs):
    handed_back = (len(g.vertex_seq) > _lib.DV_DEBRUIJN_DEVICE_MAX_VERTICES or
                   len(g.edge_from) > _lib.DV_DEBRUIJN_DEVICE_MAX_EDGES)
    n += handed_back or sum(map(len, haps)) > _lib.DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES
  return n


def _check(opts, group, want, graphs, stream=0):
  got, stats = debruijn_graph.paths_batch_device(_pairs(group), opts, stream=stream, with_stats=True)
  assert len(got) == len(want) == len(group)
  for case, a, b in zip(group, got, want):
    assert a[0] == b[0] and a[1] == b[1], (case[0], a[:2], b[:2])
    assert a[2] == b[2], case[0]
  on_host = _on_host(opts, want, graphs)
  assert stats.windows == len(group) and stats.windows_on_host == on_host, [c[0] for c in group]
  assert stats.launches == (2 if on_host < len(group) else 0)
  assert (stats.bytes_down > 0) == (stats.launches > 0)
  return got, stats, on_host


def test_every_batch_equals_the_host(batches):
  total = {'windows': 0, 'on_host': 0, 'paths': 0, 'launches': 0}
  for opts, group, want, graphs in batches:
    got, stats, on_host = _check(opts, group, want, graphs)
    # paths and hap_bytes are the device's own: the windows the host computed do not count.  Which windows those are
    # is known only as a number, so the sums are checked where it is 0 or all.
    if on_host == 0:
      assert stats.paths == sum(len(h) for _, _, h in got)
      assert stats.hap_bytes == sum(len(s) for _, _, h in got for s in h)
    elif on_host == len(group):
      assert stats.paths == 0 and stats.hap_bytes == 0
    total['windows'] += stats.windows
    total['on_host'] += stats.windows_on_host
    total['paths'] += stats.paths
    total['launches'] += stats.launches
  assert total['windows'] == len(PC.all_cases())
  # the device's share: at least the bubble windows' walks (tests/test_debruijn_paths_cpu.py pins their counts)
  assert total['on_host'] < 0.2 * total['windows'] and total['paths'] > 8 + 8 + 256 + 512 + 1024
  assert total['launches'] == 2 * sum(_on_host(o, w, g) < len(c) for o, c, w, g in batches)


def _batch_of(batches, name):
  return next(b for b in batches if any(c[0] == name for c in b[1]))


def test_windows_handed_back_sit_between_the_devices_own(batches):
  """The batch with the windows just under and just over DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES: exactly one goes to the
  host, the 1024 walks of the other and the small neighbours are the device's."""
  opts, group, want, graphs = _batch_of(batches, 'haplotype bytes just over the limit')
  names = [c[0] for c in group]
  assert 'haplotype bytes just under the limit' in names and len(group) >= 6
  got, stats, on_host = _check(opts, group, want, graphs)
  assert on_host == 1
  device = [h for c, (_, _, h) in zip(group, got) if c[0] != 'haplotype bytes just over the limit']
  assert stats.paths == sum(map(len, device)) and stats.paths > 1024
  assert stats.hap_bytes == sum(len(s) for h in device for s in h) > _lib.DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES - 1024
  # and the graph kernel's own hand-back
  opts, group, want, graphs = _batch_of(batches, 'vertices_over')
  _, stats, on_host = _check(opts, group, want, graphs)
  assert on_host == 1 and len(group) == 3 and stats.launches == 2
  assert stats.paths == sum(len(h) for c, (_, _, h) in zip(group, want) if c[0] != 'vertices_over')


def test_calls_the_kernel_does_not_cover_launch_nothing(batches):
  for name in ('disable_graph_pruning=True', '3 bubbles, max_num_paths 2048'):
    opts, group, want, graphs = _batch_of(batches, name)
    _, stats, on_host = _check(opts, group, want, graphs)
    assert on_host == len(group) and stats.launches == 0 and stats.paths == 0 and stats.bytes_down == 0


def test_zero_windows_launch_nothing():
  got, stats = debruijn_graph.paths_batch_device([], AC.options(), with_stats=True)
  assert got == [] and (stats.windows, stats.windows_on_host, stats.launches, stats.paths, stats.bytes_down) == (0,) * 5


def _largest(batches, n=4):
  return sorted(batches, key=lambda b: -len(b[1]))[:n] + [_batch_of(batches, '9 bubbles, max_num_paths 1024')]


def test_a_second_call_gives_identical_bytes(batches):
  for opts, group, want, _ in _largest(batches):
    first = debruijn_graph.paths_batch_device(_pairs(group), opts)
    second = debruijn_graph.paths_batch_device(_pairs(group), opts)
    assert first == second == want


def test_on_a_callers_stream_with_work_queued_in_front(batches):
  stream = torch.cuda.Stream()
  a = torch.randn(2048, 2048, device='cuda')
  for opts, group, want, graphs in _largest(batches, 2):
    with torch.cuda.stream(stream):
      for _ in range(8):
        a = a @ a * 1e-3                       # still running when the call is made
    got, _, _ = _check(opts, group, want, graphs, stream=stream.cuda_stream)
    assert got == want
  torch.cuda.synchronize()


def test_the_compact_entry_is_unchanged_afterwards(batches):
  """After the paths calls (the calling thread's buffers are shared by kernel family, the tables by slice):
  compact_batch_device on the same batches still equals compact_batch."""
  for opts, group, _, graphs in _largest(batches, 3) + [_batch_of(batches, 'vertices_over')]:
    debruijn_graph.paths_batch_device(_pairs(group), opts)
    got = debruijn_graph.compact_batch_device(_pairs(group), opts)
    for case, a, b in zip(group, got, graphs):
      assert AC.same_graph(a, b), case[0]
