"""Host mirror of deepvariant/python/direct_phasing (pybind of DirectPhasing) over the C ABI
(`dv_phase_reads`, csrc/direct_phasing.cpp):

  DirectPhasing(min_alleles_to_phase).phase(candidates, reads) -> [0 | 1 | 2 per read]
  .get_phased_variants(), .graphviz()          direct_phasing.h:114-160

Candidates are DeepVariantCalls with allele_support_ext / ref_support_ext (variant_calling.py
fills them); reads are matched by "<fragment_name>/<read_number>"."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Sequence

import numpy as np

from deepvariant_amd import _lib

K_UNCALLED_ALLELE = 'UNCALLED_ALLELE'


@dataclasses.dataclass
class PhasedVariant:
  position: int
  phase_1_bases: str
  phase_2_bases: str
  is_first_in_block: bool = False


# dv_phasing_candidate / dv_phasing_allele / dv_phasing_region (include/dvhip.h) as numpy records
CANDIDATE_DTYPE = np.dtype([('start', '<i8'), ('end', '<i8'), ('allele_off', '<i4'), ('n_alleles', '<i4')])
ALLELE_DTYPE = np.dtype([('bases_off', '<i8'), ('bases_len', '<i4'), ('is_ref', '<i4'), ('support_off', '<i8'),
                         ('n_support', '<i4'), ('reserved', '<i4')])
REGION_DTYPE = np.dtype([('candidate_off', '<i4'), ('n_candidates', '<i4'), ('allele_off', '<i4'), ('n_alleles', '<i4'),
                         ('support_off', '<i8'), ('n_support', '<i8'), ('first_read', '<i8'), ('n_reads', '<i4'),
                         ('reserved', '<i4')])
STATS_FIELDS = ('regions', 'regions_on_host', 'sites_in_graphs', 'vertices', 'combinations', 'launches')


def concat_regions(regions: Sequence):
  """[(candidates, alleles, bases, support_reads, support_low_quality, n_reads)] with every offset relative to the
  region's own arrays -> the concatenated tables of dv_phase_reads_batch with absolute offsets:
  (region table, candidates, alleles, bases, support_reads, support_low_quality, n_reads_total)."""
  table = np.zeros(len(regions), REGION_DTYPE)
  cands, alleles, bases, support, low = [], [], [], [], []
  n_cands = n_alleles = n_bases = n_support = n_reads = 0
  for k, (c, a, b, s, q, reads) in enumerate(regions):
    c = np.array(c, CANDIDATE_DTYPE, ndmin=1)
    a = np.array(a, ALLELE_DTYPE, ndmin=1)
    b = np.frombuffer(bytes(b), np.uint8) if isinstance(b, (bytes, bytearray)) else np.asarray(b, np.uint8)
    s = np.asarray(s, np.int32).reshape(-1)
    c['allele_off'] += n_alleles
    a['bases_off'] += n_bases
    a['support_off'] += n_support
    table[k] = (n_cands, len(c), n_alleles, len(a), n_support, len(s), n_reads, int(reads), 0)
    cands.append(c)
    alleles.append(a)
    bases.append(b)
    support.append(s)
    low.append(np.asarray(q, np.uint8).reshape(-1))
    n_cands, n_alleles, n_bases = n_cands + len(c), n_alleles + len(a), n_bases + len(b)
    n_support, n_reads = n_support + len(s), n_reads + int(reads)

  def cat(parts, dtype):
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dtype)
  return (table, cat(cands, CANDIDATE_DTYPE), cat(alleles, ALLELE_DTYPE), cat(bases, np.uint8), cat(support, np.int32),
          cat(low, np.uint8), n_reads)


def phase_tables(table, cands, alleles, bases, support, low, n_reads, min_alleles_to_phase, device=True, stream=0):
  """The native call on concatenated tables: -> (read_phases, allele_phases, allele_flags, stats)."""
  phases = np.zeros(max(n_reads, 1), np.int32)
  allele_phases = np.zeros(max(len(alleles), 1), np.int32)
  allele_flags = np.zeros(max(len(alleles), 1), np.uint8)
  stats = _lib.DvPhasingStats()
  args = [table.ctypes.data, len(table), cands.ctypes.data, len(cands), alleles.ctypes.data, len(alleles),
          bases.ctypes.data, len(bases), support.ctypes.data, low.ctypes.data, len(support), n_reads,
          int(min_alleles_to_phase), phases.ctypes.data, allele_phases.ctypes.data, allele_flags.ctypes.data,
          C.addressof(stats)]
  if device:
    _lib.check(_lib.lib().dv_phase_reads_batch_device(*args, C.c_void_p(int(stream) or None)))
  else:
    _lib.check(_lib.lib().dv_phase_reads_batch(*args))
  return phases, allele_phases, allele_flags, {f: int(getattr(stats, f)) for f in STATS_FIELDS}


def phase_arrays(regions: Sequence, min_alleles_to_phase: int, device: bool = True, stream: int = 0,
                 with_stats: bool = False):
  """PhaseReads for a batch of regions from arrays, in ONE native call (dv_phase_reads_batch_device: a workgroup per
  region; device=False: the checker in a loop).  `regions` as `concat_regions` takes them.
  -> [(read_phases, allele_phases, allele_flags)] per region (allele_phases: -1 = not a vertex of the graph);
  with_stats: (that, dv_phasing_stats as a dict)."""
  table, cands, alleles, bases, support, low, n_reads = concat_regions(regions)
  phases, allele_phases, allele_flags, stats = phase_tables(table, cands, alleles, bases, support, low, n_reads,
                                                            min_alleles_to_phase, device, stream)
  out = []
  for r in table:
    reads = slice(int(r['first_read']), int(r['first_read']) + int(r['n_reads']))
    als = slice(int(r['allele_off']), int(r['allele_off']) + int(r['n_alleles']))
    out.append((phases[reads], allele_phases[als], allele_flags[als]))
  return (out, stats) if with_stats else out


def read_key(read) -> str:
  return '%s/%d' % (read.fragment_name, read.read_number)


class DirectPhasing:
  def __init__(self, min_alleles_to_phase: int = 1):
    self._min_alleles_to_phase = int(min_alleles_to_phase)
    self._last = None

  def phase(self, candidates: Sequence, reads: Sequence) -> List[int]:
    """PhaseReads: the phase of every read; candidates must be strictly ordered by start."""
    index = {}
    for i, read in enumerate(reads):
      index[read_key(read)] = i                     # InitializeReadMaps: a later duplicate wins
    cands = (_lib.DvPhasingCandidate * max(len(candidates), 1))()
    alleles, bases, support, low_quality, names = [], [], [], [], []
    n_bases = 0
    for i, cand in enumerate(candidates):
      entries = []
      if cand.ref_support_ext:
        entries.append(('', 1, cand.ref_support_ext))
      for allele, infos in cand.allele_support_ext.items():
        if allele != K_UNCALLED_ALLELE:
          entries.append((allele, 0, infos))
      cands[i] = _lib.DvPhasingCandidate(cand.variant.start, cand.variant.end, len(alleles), len(entries))
      for allele, is_ref, infos in entries:
        raw = allele.encode()
        alleles.append(_lib.DvPhasingAllele(n_bases, len(raw), is_ref, len(support), len(infos), 0))
        names.append((i, allele, is_ref))
        bases.append(raw)
        n_bases += len(raw)
        for info in infos:
          support.append(index.get(info.read_name, -1))
          low_quality.append(1 if info.is_low_quality else 0)
    table = (_lib.DvPhasingAllele * max(len(alleles), 1))(*alleles)
    sup = np.ascontiguousarray(support, np.int32)
    lq = np.ascontiguousarray(low_quality, np.uint8)
    phases = np.zeros(max(len(reads), 1), np.int32)
    allele_phases = np.zeros(max(len(alleles), 1), np.int32)
    allele_flags = np.zeros(max(len(alleles), 1), np.uint8)
    dot = C.create_string_buffer(1 << 20)
    _lib.check(_lib.lib().dv_phase_reads(
        cands, len(candidates), table, len(alleles), b''.join(bases), n_bases, sup.ctypes.data, lq.ctypes.data,
        len(support), len(reads), self._min_alleles_to_phase, phases.ctypes.data, allele_phases.ctypes.data,
        allele_flags.ctypes.data, dot, len(dot)))
    self._last = (list(candidates), names, allele_phases, allele_flags, dot.value.decode())
    return [int(p) for p in phases[:len(reads)]]

  def get_phased_variants(self) -> List[PhasedVariant]:
    """GetPhasedVariants (direct_phasing.cc:326-360): sites where both phases got an allele."""
    if self._last is None:
      return []
    candidates, names, allele_phases, allele_flags, _ = self._last
    out = []
    per_candidate = {}
    for k, (i, allele, is_ref) in enumerate(names):
      if allele_phases[k] >= 0:
        per_candidate.setdefault(i, []).append((k, 'REF' if is_ref else allele))
    for i in sorted(per_candidate):
      # vertex order within a site: the reference vertex, then alleles by bases (AddCandidate)
      verts = sorted(per_candidate[i], key=lambda t: (0, '') if names[t[0]][2] else (1, t[1]))
      picked = ['', '']
      first = False
      for k, text in verts:
        if allele_phases[k] == 1:
          picked[0] = text
        elif allele_phases[k] == 2:
          picked[1] = text
        first = bool(allele_flags[k])
      if picked[0] and picked[1]:
        out.append(PhasedVariant(candidates[i].variant.start, picked[0], picked[1], first))
    return out

  def graphviz(self) -> str:
    return self._last[4] if self._last else ''
