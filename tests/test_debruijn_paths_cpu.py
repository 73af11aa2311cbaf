"""paths_batch (dv_debruijn_paths_batch: DeBruijnGraph::build and candidate_haplotypes per window, the reference of the
device form) against build(...).candidate_haplotypes() and kmer_size on every window of tests/path_cases.py, the status
values, that every hand-made window holds what its name says -- on the host's answer, which is what the device is
compared with in tests/test_hip_debruijn_paths.py --, and the entry points' argument checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd.realigner import debruijn_graph
from tests import assembly_cases as AC
from tests import path_cases as PC

OK, NO_GRAPH, TOO_MANY = _lib.DV_DEBRUIJN_PATHS_OK, _lib.DV_DEBRUIJN_PATHS_NO_GRAPH, _lib.DV_DEBRUIJN_PATHS_TOO_MANY
LIMIT = _lib.DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES


@pytest.fixture(scope='module')
def answers():
  """{name: (case, (k, status, haplotypes))} from paths_batch, one call per set of options."""
  out = {}
  for opts, group in PC.batches(PC.all_cases()):
    got = debruijn_graph.paths_batch([(c[1], c[2]) for c in group], opts)
    assert len(got) == len(group)
    for case, answer in zip(group, got):
      assert case[0] not in out, case[0]
      out[case[0]] = (case, answer)
  return out


def _haps(answers, name):
  (k, status, haps) = answers[name][1]
  return k, status, haps


def test_equals_build_and_candidate_haplotypes_on_every_case(answers):
  assert len(answers) == len(PC.all_cases()) == len(AC.hand_made()) + 160 + len(PC.hand_made())
  seen = {OK: 0, NO_GRAPH: 0, TOO_MANY: 0}
  for name, ((_, ref, reads, opts), (k, status, haps)) in answers.items():
    graph = debruijn_graph.build(ref, reads, opts)
    if graph is None:
      assert (k, status, haps) == (0, NO_GRAPH, []), name
    else:
      want = graph.candidate_haplotypes()
      assert k == graph.kmer_size and haps == want, name
      assert status == (OK if want else TOO_MANY), name
      assert haps == sorted(haps)
    seen[status] += 1
  assert seen[OK] > 100 and seen[NO_GRAPH] >= 5 and seen[TOO_MANY] >= 10, seen
  assert sum(len(a[2]) > 1 for _, a in answers.values()) > 50


def test_every_case_kind_is_present():
  counts = {kind: len(make()) for kind, make in PC.KINDS.items()}
  assert counts == {'near_max_num_paths': 6, 'ordering': 5, 'pruning': 4, 'to_the_host': 12, 'general': 2}
  names = [c[0] for c in PC.all_cases()]
  assert len(set(names)) == len(names)
  groups = PC.batches(PC.all_cases())
  assert len(groups) > 20 and sum(len(g) for _, g in groups) == len(names)
  assert any(o.disable_graph_pruning for o, _ in groups) and any(o.max_num_paths > 1024 for o, _ in groups)


def test_walk_counts_around_max_num_paths(answers):
  assert [_haps(answers, '3 bubbles, max_num_paths %d' % m)[1] for m in (7, 8, 9)] == [TOO_MANY, OK, OK]
  assert [len(_haps(answers, '3 bubbles, max_num_paths %d' % m)[2]) for m in (7, 8, 9)] == [0, 8, 8]
  assert len(_haps(answers, '8 bubbles at the default')[2]) == 256 == debruijn_graph.DeBruijnGraphOptions().max_num_paths
  assert len(_haps(answers, '9 bubbles, max_num_paths 1024')[2]) == 512          # two strides of a 256-thread workgroup
  k, status, haps = _haps(answers, '33 bubbles')
  assert k > 0 and status == TOO_MANY and haps == []
  # its walks really are 2 ** 33: every site is a bubble of its own at this k
  case = answers['33 bubbles'][0]
  assert len(PC._sites(33)) == 33 and k < PC.SPACING and len(case[2]) == 4 * 33      # pylint: disable=protected-access
  few = debruijn_graph.paths_batch([(case[1], case[2][:4 * 5])], AC.options())[0]
  assert len(few[2]) == 2 ** 5


def test_order_and_lengths(answers):
  _, _, haps = _haps(answers, 'three-allele site')
  assert len(haps) == 3 and len({len(h) for h in haps}) == 1
  _, _, haps = _haps(answers, 'deletion over two bubbles and an insertion')
  ref = answers['deletion over two bubbles and an insertion'][0][1]
  cut = PC.SPACING + 9                                              # the deletion's bases; the insertion has 7
  assert len(haps) == 10 and {len(h) - len(ref) for h in haps} == {0, 7, -cut, 7 - cut}
  for name, place in (('N', 3), ('lower-case base', 4)):            # A C G N T; A C G T g
    case, (_, _, haps) = answers['reference with a %s after a branch point' % name]
    assert len(haps) == 5 and haps.index(case[1]) == place, name
  _, _, haps = _haps(answers, 'walks longer than 256 vertices')
  assert len(haps) == 4 and all(len(h) == 330 for h in haps)


def test_pruning_and_reachability(answers):
  for name, n in (('branch cut by min_edge_weight leaves a dead end', 2), ('alive branch that never rejoins', 2),
                  ('read-only start that joins the reference', 2), ('reads past both ends of the reference', 4)):
    case, (_, status, haps) = answers[name]
    assert status == OK and len(haps) == n and case[1] in haps, name
    assert all(len(h) == len(case[1]) for h in haps), name
  # what each leaves in the graph before pruning: more vertices than the kept walks visit
  for name in ('alive branch that never rejoins', 'read-only start that joins the reference',
               'reads past both ends of the reference'):
    case, (k, _, haps) = answers[name]
    graph = debruijn_graph.compact_batch([(case[1], case[2])], case[3])[0]
    on_walks = {h[i:i + k] for h in haps for i in range(len(h) - k + 1)}
    assert len(graph.vertex_seq) >= len(on_walks) + 10, name


def test_windows_and_calls_for_the_host(answers):
  _, status, haps = _haps(answers, 'haplotype bytes just under the limit')
  assert status == OK and len(haps) == 1024 and LIMIT - 1024 == sum(map(len, haps))
  _, status, haps = _haps(answers, 'haplotype bytes just over the limit')
  assert status == OK and len(haps) == 1024 and LIMIT + 1024 == sum(map(len, haps))
  assert len(_haps(answers, '3 bubbles, max_num_paths 2048')[2]) == 8
  assert _haps(answers, 'disable_graph_pruning=True')[1] == OK
  assert len(_haps(answers, '3 bubbles without pruning')[2]) >= 8
  case = answers['vertices_over'][0]
  graph = debruijn_graph.compact_batch([(case[1], case[2])], case[3])[0]
  assert len(graph.vertex_seq) > _lib.DV_DEBRUIJN_DEVICE_MAX_VERTICES
  # nothing else in the set passes the text limit
  over = [n for n, (_, a) in answers.items() if sum(map(len, a[2])) > LIMIT]
  assert over == ['haplotype bytes just over the limit']


def test_general(answers):
  case, (k, status, haps) = answers['no reads at all']
  assert (k, status, haps) == (AC.K, OK, [case[1]])
  assert _haps(answers, 'no graph') == (0, NO_GRAPH, [])


def _raw_call(fn, device, n_seqs=2, n_windows=1, options=None, table=True, out=True, windows=True):
  bases = np.frombuffer(b'ACGTACGTACGTTTGACCATGGACGTACGTACGT', np.uint8)
  quals = np.full(len(bases), 30, np.uint8)
  seq_off = np.array([0, 20, len(bases)], np.int64)
  mapq = np.array([0, 60], np.uint8)
  descs = (_lib.DvDebruijnWindow * 1)(_lib.DvDebruijnWindow(0, 1, 1, 0))
  opt = options or _lib.DvDebruijnOptions(10, 30, 1, 14, 15, 2, 256, 0)
  handle, arrays = C.c_void_p(), _lib.DvDebruijnPaths()
  args = [n_seqs, bases.ctypes.data, quals.ctypes.data, seq_off.ctypes.data if table else None, mapq.ctypes.data,
          n_windows, descs if windows else None, C.byref(opt)]
  if device:
    args.append(None)
  status = fn(*args, C.byref(handle) if out else None, C.byref(arrays))
  if handle.value:
    _lib.lib().dv_debruijn_paths_free(handle)
  return status


@pytest.mark.parametrize('device', [False, True])
def test_argument_errors_as_for_the_compact_entry(device):
  l = _lib.lib()
  fn = l.dv_debruijn_paths_batch_device if device else l.dv_debruijn_paths_batch
  compact = l.dv_debruijn_compact_batch_device if device else l.dv_debruijn_compact_batch
  bad = [dict(n_seqs=-1), dict(n_windows=-1), dict(table=False), dict(out=False), dict(windows=False),
         dict(options=_lib.DvDebruijnOptions(10, 30, 0, 14, 15, 2, 256, 0)),
         dict(options=_lib.DvDebruijnOptions(0, 30, 1, 14, 15, 2, 256, 0))]
  for how in bad:
    assert _raw_call(fn, device, **how) == _lib.DV_ERR_INVALID_ARGUMENT, how
    assert fn.__name__ in l.dv_last_error().decode()
  # a window outside the table: the same answer as the compact entry's
  descs = (_lib.DvDebruijnWindow * 1)(_lib.DvDebruijnWindow(0, 1, 5, 0))
  bases = np.frombuffer(b'ACGTACGTACGTTTGACCATGGACGTACGTACGT', np.uint8)
  seq_off = np.array([0, 20, len(bases)], np.int64)
  mapq = np.array([0, 60], np.uint8)
  opt = _lib.DvDebruijnOptions(10, 30, 1, 14, 15, 2, 256, 0)
  for f, arrays in ((fn, _lib.DvDebruijnPaths()), (compact, _lib.DvDebruijnCompact())):
    handle = C.c_void_p()
    args = [2, bases.ctypes.data, bases.ctypes.data, seq_off.ctypes.data, mapq.ctypes.data, 1, descs, C.byref(opt)]
    if device:
      args.append(None)
    assert f(*args, C.byref(handle), C.byref(arrays)) == _lib.DV_ERR_INVALID_ARGUMENT
    assert not handle.value


def test_the_device_entry_needs_no_device_without_device_work():
  """Zero windows, and a call the kernel does not cover, are the host's: they succeed whether or not there is a GPU."""
  result, stats = debruijn_graph.paths_batch_device([], AC.options(), with_stats=True)
  assert result == [] and (stats.windows, stats.windows_on_host, stats.launches, stats.bytes_down) == (0, 0, 0, 0)
  name, ref, reads, opts = PC.to_the_host()[0]
  assert name == 'disable_graph_pruning=True' and opts.disable_graph_pruning
  result, stats = debruijn_graph.paths_batch_device([(ref, reads)], opts, with_stats=True)
  assert result == debruijn_graph.paths_batch([(ref, reads)], opts)
  assert (stats.windows, stats.windows_on_host, stats.paths, stats.launches) == (1, 1, 0, 0)
