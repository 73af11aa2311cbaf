"""The compact form of the realigner's graphs on the host (include/dvhip.h, "compact form"): compact_batch returns
the graph of the winning k before pruning as integers, from_compact rebuilds the object from it.  On the hand-made
windows of tests/assembly_cases.py and the 160 seeded ones the rebuilt graph must be build()'s own -- k, haplotypes and
the graphviz dump, text for text -- and malformed compact graphs must be refused before anything is indexed by them."""
import dataclasses

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd.realigner import debruijn_graph
from tests import assembly_cases as AC


def _compact(cases):
  """compact_batch per group of equal graph options -> one CompactGraph per case, in order."""
  out = {}
  for opts, group in AC.batches(cases):
    for case, graph in zip(group, debruijn_graph.compact_batch([(c[1], c[2]) for c in group], opts)):
      out[case[0]] = graph
  return [out[c[0]] for c in cases]


def _check_round_trip(case, compact):
  name, ref, reads, opts = case
  want = debruijn_graph.build(ref, reads, opts)
  got = debruijn_graph.from_compact(ref, reads, opts, compact)
  assert (compact.k == 0) == (want is None), name
  assert (got is None) == (want is None), name
  if want is None:
    assert len(compact.vertex_seq) == 0 and len(compact.edge_from) == 0, name
    return None
  assert got.kmer_size == want.kmer_size == compact.k, name
  assert got.candidate_haplotypes() == want.candidate_haplotypes(), name
  assert got.graphviz() == want.graphviz(), name
  # canonical: sorted by first occurrence, the reference's vertices first and in order
  n_ref = len(ref) - compact.k + 1
  assert compact.vertex_seq[:n_ref].tolist() == [0] * n_ref and compact.vertex_pos[:n_ref].tolist() == list(range(n_ref)), name
  for seq, pos in ((compact.vertex_seq, compact.vertex_pos), (compact.edge_seq, compact.edge_pos)):
    keys = list(zip(seq.tolist(), pos.tolist()))
    assert keys == sorted(set(keys)), name
  assert (compact.vertex_seq[n_ref:] > 0).all() and compact.vertex_seq.max(initial=0) <= len(reads), name
  assert compact.edge_is_ref[:n_ref - 1].all() and (compact.edge_weight >= 1).all(), name
  return want


def test_hand_made_windows_round_trip():
  cases = AC.hand_made()
  graphs = _compact(cases)
  built = {}
  for case, compact in zip(cases, graphs):
    built[case[0]] = (_check_round_trip(case, compact), compact)
  # the windows do what their names say
  assert built['homopolymer reference'][0] is None and built['homopolymer reference'][1].k_tries == 21
  assert built['tandem repeat in the reference'][1].k >= AC.K + 5
  assert built['read-only cycle'][1].k == 13 and built['no reads'][1].k == AC.K
  assert built['step_k = 2'][1].k % 2 == 0 and built['step_k = 2'][1].k >= AC.K + 5
  assert built['reference of length min_k'][0] is None and built['reference of length min_k'][1].k_tries == 0
  assert built['reference of length min_k + 1'][1].k == AC.K
  assert built['max_num_paths exceeded'][0].candidate_haplotypes() == []
  lone = built['short segment after a bad base'][1]
  touched = set(lone.edge_from.tolist()) | set(lone.edge_to.tolist())
  assert any(v not in touched for v in range(len(lone.vertex_seq)))           # the vertex spanning the bad base
  low, n = built['low quality base'][1], built['N at the same place'][1]
  assert AC.same_graph(low, n)
  ignored = built['read below min_mapq'][1]
  assert set(ignored.vertex_seq.tolist()) <= {0, 1, 3}                          # reads 2 and 4 never occur


def test_zero_windows():
  assert debruijn_graph.compact_batch([], AC.options()) == []


@pytest.mark.parametrize('seed', AC.SEEDS)
def test_generated_windows_round_trip(seed):
  cases = AC.generated(seed)
  built = multi = 0
  for case, compact in zip(cases, _compact(cases)):
    want = _check_round_trip(case, compact)
    if want is not None:
      built += 1
      multi += len(want.candidate_haplotypes()) > 1
  assert built > 25 and multi > 8


def test_case_lists_keep_their_lengths():
  assert len(AC.hand_made()) == 22 and len(AC.limit_windows()) == 4
  assert [len(AC.generated(seed)) for seed in AC.SEEDS] == [40] * 4


def test_limit_windows_are_where_their_names_say():
  """The host's own graphs of AC.limit_windows(): the sizes that decide, in the device route, whether the kernel
  builds the window or hands it back (tests/test_hip_debruijn.py runs them there)."""
  max_v, max_e = _lib.DV_DEBRUIJN_DEVICE_MAX_VERTICES, _lib.DV_DEBRUIJN_DEVICE_MAX_EDGES
  table = 2 * max_v                                    # the kernel's vertex table at these windows' sizes
  cases = {c[0]: c for c in AC.limit_windows()}
  graphs = dict(zip(cases, _compact(list(cases.values()))))
  for name, (_, ref, reads, opts) in cases.items():
    bases = len(ref) + sum(len(r.aligned_sequence) for r in reads)
    assert bases <= _lib.DV_DEBRUIJN_DEVICE_MAX_BASES, name          # none is sorted out before the launch
    assert AC.distinct_kmers(ref, [], opts.min_k)[0] == len(ref) - opts.min_k + 1, name    # repeat-free: min_k is tried
    print(name, 'bases', bases, 'k', graphs[name].k, 'k_tries', graphs[name].k_tries, 'V', len(graphs[name].vertex_seq),
          'E', len(graphs[name].edge_from), 'distinct at min_k', AC.distinct_kmers(ref, reads, opts.min_k))
  for name in ('just_under', 'vertices_over', 'table_full'):
    g, (_, ref, reads, opts) = graphs[name], cases[name]
    assert g.k == opts.min_k and g.k_tries == 1, name                                      # one try, acyclic
    assert (len(g.vertex_seq), len(g.edge_from)) == AC.distinct_kmers(ref, reads, g.k), name
    _check_round_trip(cases[name], g)
  g = graphs['just_under']
  assert 0.95 * max_v <= len(g.vertex_seq) <= max_v and len(g.edge_from) <= max_e
  g = graphs['vertices_over']
  assert max_v < len(g.vertex_seq) <= 1.2 * max_v
  assert len(cases['vertices_over'][1]) + sum(len(r.aligned_sequence) for r in cases['vertices_over'][2]) < table
  g = graphs['table_full']
  assert table + 100 <= len(g.vertex_seq) <= table + 600
  # edges_over: the host finds a cycle at every k; at the first the graph has room for its vertices, not for its edges
  g, (_, ref, reads, opts) = graphs['edges_over'], cases['edges_over']
  schedule = list(range(opts.min_k, min(opts.max_k, len(ref) - 1) + 1, opts.step_k))
  assert g.k == 0 and g.k_tries == len(schedule) == 3 and len(g.vertex_seq) == 0
  vertices, edges = AC.distinct_kmers(ref, reads, opts.min_k)
  assert vertices <= max_v < edges <= table


def _malformed(compact, **changes):
  arrays = {name: getattr(compact, name).copy() for name in debruijn_graph.CompactGraph.ARRAYS}
  for name, (index, value) in changes.items():
    arrays[name][index] = value
  return dataclasses.replace(compact, **arrays)


def test_malformed_compact_graphs_are_refused():
  _, ref, reads, opts = AC.hand_made()[0]
  compact = debruijn_graph.compact_batch([(ref, reads)], opts)[0]
  assert debruijn_graph.from_compact(ref, reads, opts, compact) is not None
  n_ref = len(ref) - compact.k + 1
  last = len(compact.vertex_seq) - 1
  assert last >= n_ref + 1 and len(compact.edge_from) > n_ref
  swapped = _malformed(compact, vertex_pos=(last, int(compact.vertex_pos[last - 1])))
  swapped = _malformed(swapped, vertex_pos=(last - 1, int(compact.vertex_pos[last])))
  assert int(compact.vertex_seq[last]) == int(compact.vertex_seq[last - 1])
  bad = {
      'edge endpoint out of range': _malformed(compact, edge_to=(3, len(compact.vertex_seq))),
      'negative edge endpoint': _malformed(compact, edge_from=(3, -1)),
      'occurrence past the end of its sequence': _malformed(compact, vertex_pos=(last, len(reads[0].aligned_sequence))),
      'sequence number past the reads': _malformed(compact, vertex_seq=(last, len(reads) + 1)),
      'unsorted vertices': swapped,
      'wrong reference prefix': _malformed(compact, vertex_pos=(2, 3)),
      'a read vertex among the reference': _malformed(compact, vertex_seq=(n_ref - 1, 1)),
      'k past the reference': dataclasses.replace(compact, k=len(ref)),
  }
  for name, graph in bad.items():
    with pytest.raises(_lib.DvError) as raised:
      debruijn_graph.from_compact(ref, reads, opts, graph)
    assert raised.value.status == _lib.DV_ERR_BAD_INPUT, name
    assert 'dv_debruijn_from_compact' in _lib.last_error(), name


def test_bad_options_are_refused():
  _, ref, reads, _ = AC.hand_made()[0]
  compact = debruijn_graph.compact_batch([(ref, reads)], AC.options())[0]
  for changes in ({'min_k': 0}, {'min_k': -1}, {'step_k': 0}, {'step_k': -2}):
    opts = AC.options(**changes)
    with pytest.raises(_lib.DvError) as raised:
      debruijn_graph.compact_batch([(ref, reads)], opts)
    assert raised.value.status == _lib.DV_ERR_INVALID_ARGUMENT and 'dv_debruijn_compact_batch' in _lib.last_error()
    with pytest.raises(_lib.DvError) as raised:
      debruijn_graph.from_compact(ref, reads, opts, compact)
    assert raised.value.status == _lib.DV_ERR_INVALID_ARGUMENT and 'dv_debruijn_from_compact' in _lib.last_error()


def test_device_entry_point_needs_a_device():
  if _lib.device_count() > 0:
    pytest.skip('GPU present')
  _, ref, reads, opts = AC.hand_made()[0]
  with pytest.raises(_lib.DvError) as raised:
    debruijn_graph.compact_batch_device([(ref, reads)], opts)
  assert raised.value.status == _lib.DV_ERR_NO_DEVICE
