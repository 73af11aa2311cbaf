"""Host mirror of deepvariant/realigner/python/debruijn_graph (pybind of DeBruijnGraph) over
the C ABI: build(ref, reads, options) -> DeBruijnGraph or None; .kmer_size,
.candidate_haplotypes(), .graphviz().  All graph work is native (csrc/debruijn_graph.cpp).

compact_batch / compact_batch_device return the graphs of many windows before pruning as integer arrays (the "compact
form" of include/dvhip.h) -- the host's own constructor, or one kernel launch of csrc/debruijn.hip -- and from_compact
turns one back into the object build returns.  paths_batch / paths_batch_device return the windows' candidate
haplotypes themselves: build + candidate_haplotypes per window on the host, or the graph launch and the paths launch
of csrc/debruijn.hip."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Sequence

import numpy as np

from deepvariant_amd import _lib
from deepvariant_amd import packing


@dataclasses.dataclass
class DeBruijnGraphOptions:
  """deepvariant/protos/realigner.proto DeBruijnGraphOptions; defaults = realigner.py's flags."""
  min_k: int = 10
  max_k: int = 101
  step_k: int = 1
  min_mapq: int = 14
  min_base_quality: int = 15
  min_edge_weight: int = 2
  max_num_paths: int = 256
  disable_graph_pruning: bool = False


class DeBruijnGraph:
  def __init__(self, handle):
    self._h = handle

  def __del__(self):
    if getattr(self, '_h', None):
      _lib.lib().dv_debruijn_destroy(self._h)
      self._h = None

  @property
  def kmer_size(self) -> int:
    return int(_lib.lib().dv_debruijn_kmer_size(self._h))

  def candidate_haplotypes(self) -> List[str]:
    n = C.c_int32()
    arr = C.POINTER(C.c_char_p)()
    _lib.check(_lib.lib().dv_debruijn_haplotypes(self._h, C.byref(n), C.byref(arr)))
    return [arr[i].decode() for i in range(n.value)]

  def graphviz(self) -> str:
    text = C.c_char_p()
    _lib.check(_lib.lib().dv_debruijn_graphviz(self._h, C.byref(text)))
    return text.value.decode()


@dataclasses.dataclass
class CompactGraph:
  """One window's graph of the winning k before pruning; k = 0: build returns None.  Vertices and edges are in
  insertion order = ascending first occurrence (seq 0: the reference, seq 1 + j: read j; pos: the k-mer's offset)."""
  k: int
  k_tries: int
  vertex_seq: np.ndarray
  vertex_pos: np.ndarray
  edge_from: np.ndarray
  edge_to: np.ndarray
  edge_weight: np.ndarray
  edge_is_ref: np.ndarray
  edge_seq: np.ndarray
  edge_pos: np.ndarray

  ARRAYS = ('vertex_seq', 'vertex_pos', 'edge_from', 'edge_to', 'edge_weight', 'edge_is_ref', 'edge_seq', 'edge_pos')


def _native_options(options: DeBruijnGraphOptions) -> '_lib.DvDebruijnOptions':
  return _lib.DvDebruijnOptions(options.min_k, options.max_k, options.step_k, options.min_mapq,
                                options.min_base_quality, options.min_edge_weight, options.max_num_paths,
                                int(bool(options.disable_graph_pruning)))


def _sequence_table(windows):
  """windows: (ref, reads) pairs.  One sequence table: per window its reference, then its reads.  -> the leading
  arguments of the batch entry points (n_seqs .. windows) and the arrays they point into."""
  pieces, quals, lengths, mapq, descs = [], [], [], [], []
  for ref, reads in windows:
    first = len(lengths)
    raw = ref.encode()
    pieces.append(raw)
    quals.append(bytes(len(raw)))
    lengths.append(len(raw))
    mapq.append(0)
    for read in reads:
      seq = read.aligned_sequence.encode()
      pieces.append(seq)
      quals.append(bytes(bytearray(read.aligned_quality)))
      lengths.append(len(seq))
      mapq.append(min(255, max(0, int(read.alignment.mapping_quality))))
    descs.append(_lib.DvDebruijnWindow(first, first + 1, len(reads), 0))
  bases = np.frombuffer(b''.join(pieces), np.uint8)
  quality = np.frombuffer(b''.join(quals), np.uint8)
  assert len(bases) == len(quality), 'a read with other than one quality per base'
  seq_off = np.zeros(len(lengths) + 1, np.int64)
  np.cumsum(lengths, out=seq_off[1:])
  mapq = np.array(mapq, np.uint8)
  table = (_lib.DvDebruijnWindow * max(1, len(descs)))(*descs)
  args = [len(lengths), bases.ctypes.data, quality.ctypes.data, seq_off.ctypes.data, mapq.ctypes.data, len(descs), table]
  return args, (bases, quality, seq_off, mapq, table)


def _compact_call(windows, options, device, stream=0):
  args, keep = _sequence_table(windows)                  # pylint: disable=unused-variable
  opt = _native_options(options)
  handle, out = C.c_void_p(), _lib.DvDebruijnCompact()
  args.append(C.byref(opt))
  if device:
    _lib.check(_lib.lib().dv_debruijn_compact_batch_device(*args, stream, C.byref(handle), C.byref(out)))
  else:
    _lib.check(_lib.lib().dv_debruijn_compact_batch(*args, C.byref(handle), C.byref(out)))
  try:
    n = len(windows)
    view = lambda ptr, lo, hi: (np.ctypeslib.as_array(ptr, shape=(hi,))[lo:hi].copy() if hi > lo       # noqa: E731
                                else np.zeros(0, np.int32))
    k = view(out.k, 0, n)
    tries = view(out.k_tries, 0, n)
    v_off = np.ctypeslib.as_array(out.vertex_off, shape=(n + 1,)).copy()
    e_off = np.ctypeslib.as_array(out.edge_off, shape=(n + 1,)).copy()
    graphs = []
    for w in range(n):
      v0, v1, e0, e1 = int(v_off[w]), int(v_off[w + 1]), int(e_off[w]), int(e_off[w + 1])
      graphs.append(CompactGraph(
          int(k[w]), int(tries[w]), view(out.vertex_seq, v0, v1), view(out.vertex_pos, v0, v1),
          view(out.edge_from, e0, e1), view(out.edge_to, e0, e1), view(out.edge_weight, e0, e1),
          view(out.edge_is_ref, e0, e1), view(out.edge_seq, e0, e1), view(out.edge_pos, e0, e1)))
    return graphs
  finally:
    _lib.lib().dv_debruijn_compact_free(handle)


def compact_batch(windows: Sequence, options: DeBruijnGraphOptions) -> List[CompactGraph]:
  """The compact graphs of `windows` ((ref, reads) pairs) from the host code."""
  return _compact_call(list(windows), options, device=False)


def compact_batch_device(windows: Sequence, options: DeBruijnGraphOptions, stream: int = 0, with_stats: bool = False):
  """The same from one kernel launch over all windows (csrc/debruijn.hip); identical arrays.  with_stats: ->
  (graphs, _lib.DvDebruijnDeviceStats of the call).  Raises DvError(DV_ERR_NO_DEVICE) without a GPU."""
  graphs = _compact_call(list(windows), options, device=True, stream=stream)
  if not with_stats:
    return graphs
  stats = _lib.DvDebruijnDeviceStats()
  _lib.check(_lib.lib().dv_debruijn_device_last_stats(C.byref(stats)))
  return graphs, stats


def _paths_call(windows, options, device, stream=0):
  args, keep = _sequence_table(windows)                  # pylint: disable=unused-variable
  opt = _native_options(options)
  handle, out = C.c_void_p(), _lib.DvDebruijnPaths()
  args.append(C.byref(opt))
  if device:
    _lib.check(_lib.lib().dv_debruijn_paths_batch_device(*args, stream, C.byref(handle), C.byref(out)))
  else:
    _lib.check(_lib.lib().dv_debruijn_paths_batch(*args, C.byref(handle), C.byref(out)))
  try:
    n = len(windows)
    first = np.ctypeslib.as_array(out.hap_first, shape=(n + 1,))
    off = np.ctypeslib.as_array(out.hap_off, shape=(int(first[n]) + 1,))
    text = C.string_at(out.hap_text, int(off[-1])) if off[-1] else b''
    result = []
    for w in range(n):
      haps = [text[off[h]:off[h + 1]].decode() for h in range(int(first[w]), int(first[w + 1]))]
      result.append((int(out.k[w]), int(out.status[w]), haps))
    return result
  finally:
    _lib.lib().dv_debruijn_paths_free(handle)


def paths_batch(windows: Sequence, options: DeBruijnGraphOptions):
  """Per window of `windows` ((ref, reads) pairs) -> (k, status, [haplotypes]) from the host code: what
  build(ref, reads, options) gives -- kmer_size and candidate_haplotypes(), in its order.  status is
  _lib.DV_DEBRUIJN_PATHS_OK, _NO_GRAPH (build returns None; k = 0) or _TOO_MANY (more than max_num_paths walks)."""
  return _paths_call(list(windows), options, device=False)


def paths_batch_device(windows: Sequence, options: DeBruijnGraphOptions, stream: int = 0, with_stats: bool = False):
  """The same from the device: the graph launch and the paths launch of csrc/debruijn.hip over all windows; identical
  results.  with_stats: -> (results, _lib.DvDebruijnPathsStats of the call).  Raises DvError(DV_ERR_NO_DEVICE) without a
  GPU when there is device work."""
  result = _paths_call(list(windows), options, device=True, stream=stream)
  if not with_stats:
    return result
  stats = _lib.DvDebruijnPathsStats()
  _lib.check(_lib.lib().dv_debruijn_paths_last_stats(C.byref(stats)))
  return result, stats


def from_compact(ref: str, reads: Sequence, options: DeBruijnGraphOptions,
                 compact: CompactGraph) -> Optional[DeBruijnGraph]:
  """The graph build(ref, reads, options) returns, rebuilt from its compact form (validated first: a malformed
  one raises DvError(DV_ERR_BAD_INPUT)) and pruned as build prunes; None for k = 0."""
  table = packing.ReadTable.from_reads(list(reads))
  idx = np.arange(len(reads), dtype=np.int32)
  bases = np.ascontiguousarray(table.bases, np.uint8)
  quals = np.ascontiguousarray(table.quals, np.uint8)
  seq_off = np.ascontiguousarray(table.read_seq_off, np.uint32)
  mapq = np.ascontiguousarray(table.read_mapq, np.uint8)
  arrays = [np.ascontiguousarray(getattr(compact, name), np.int32) for name in CompactGraph.ARRAYS]
  opt = _native_options(options)
  raw = ref.encode()
  handle = C.c_void_p()
  _lib.check(_lib.lib().dv_debruijn_from_compact(
      raw, len(raw), bases.ctypes.data, quals.ctypes.data, len(bases), seq_off.ctypes.data, mapq.ctypes.data,
      table.n_reads, idx.ctypes.data, len(idx), C.byref(opt), int(compact.k), len(arrays[0]), arrays[0].ctypes.data,
      arrays[1].ctypes.data, len(arrays[2]), *[a.ctypes.data for a in arrays[2:]], C.byref(handle)))
  return DeBruijnGraph(handle) if handle.value else None


def build_from_table(ref: str, table: packing.ReadTable, read_indices: Sequence[int],
                     options: DeBruijnGraphOptions) -> Optional[DeBruijnGraph]:
  """build() on reads that are already packed: `read_indices` selects the window's reads from
  the region's read table, in the order the reference would add them."""
  opt = _lib.DvDebruijnOptions(options.min_k, options.max_k, options.step_k, options.min_mapq,
                               options.min_base_quality, options.min_edge_weight, options.max_num_paths,
                               int(bool(options.disable_graph_pruning)))
  idx = np.ascontiguousarray(read_indices, np.int32)
  bases = np.ascontiguousarray(table.bases, np.uint8)
  quals = np.ascontiguousarray(table.quals, np.uint8)
  seq_off = np.ascontiguousarray(table.read_seq_off, np.uint32)
  mapq = np.ascontiguousarray(table.read_mapq, np.uint8)
  raw = ref.encode()
  handle = C.c_void_p()
  _lib.check(_lib.lib().dv_debruijn_build(
      raw, len(raw), bases.ctypes.data, quals.ctypes.data, len(bases), seq_off.ctypes.data, mapq.ctypes.data,
      table.n_reads, idx.ctypes.data, len(idx), C.byref(opt), C.byref(handle)))
  return DeBruijnGraph(handle) if handle.value else None


def build(ref: str, reads: Sequence, options: DeBruijnGraphOptions) -> Optional[DeBruijnGraph]:
  """debruijn_graph.build(ref, reads, options)."""
  table = packing.ReadTable.from_reads(list(reads))
  return build_from_table(ref, table, range(len(reads)), options)
