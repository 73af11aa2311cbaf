"""The largest de Bruijn graphs of the realigner's windows, for DV_DEBRUIJN_DEVICE_MAX_* (include/dvhip.h): per window
the vertices and edges of the winning k's graph before pruning, the bases of the reference plus the reads, and (for
DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES) the number of candidate haplotypes and the sum of their lengths, over
the chr20 golden batch, the ten NA12878 regions of tests/test_hip_realigner_fast_pass.py and the 100-region batch of
tools/realign_bench.py.  Host code only (dv_debruijn_compact_batch; the windows come from the CPU allele counter of
the tests), so it runs without a GPU.  Prints one JSON line.

  python tools/assembly_limits.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepvariant_amd import dv_types as T                  # noqa: E402
from deepvariant_amd import packing                        # noqa: E402
from deepvariant_amd.realigner import debruijn_graph       # noqa: E402
from deepvariant_amd.realigner import realigner as R       # noqa: E402
from deepvariant_amd.realigner import utils as U           # noqa: E402
from tests import realigner_fixture as RF                  # noqa: E402


class _Ref:
  def __init__(self, seq, offset):
    self.seq, self.offset = seq, offset

  def n_bases(self, contig):
    return self.offset + len(self.seq)

  def get_bases(self, contig, start, end):
    lo, hi = max(start, self.offset), min(end, self.offset + len(self.seq))
    inner = self.seq[lo - self.offset:hi - self.offset] if hi > lo else ''
    return 'N' * max(0, min(lo, end) - start) + inner + 'N' * max(0, end - max(hi, start))


def _windows_of(ref, tables, regions):
  """(ref bases, reads) per candidate window, as dv_realign_regions gathers them."""
  job = R.Realigner(R.realigner_config(), ref, device_align=False).start_realign_tables(tables, regions)
  out = []
  for _, table, usable in job._jobs:                                          # pylint: disable=protected-access
    starts, ends = table.read_pos.astype(np.int64), table.read_end.astype(np.int64)
    bases, quals, off = table.bases.tobytes(), table.quals.tobytes(), table.read_seq_off
    for w in usable:
      reads = [types.SimpleNamespace(aligned_sequence=bases[off[i]:off[i + 1]].decode(),
                                     aligned_quality=quals[off[i]:off[i + 1]],
                                     alignment=types.SimpleNamespace(mapping_quality=int(table.read_mapq[i])))
               for i in np.nonzero((ends > w.start) & (starts < w.end))[0]]
      out.append((ref.get_bases(w.reference_name, w.start, w.end), reads))
  return out


def _na12878(first, n_regions):
  with np.load(os.path.join(ROOT, 'tests', 'golden', 'na12878_100kb.npz')) as z, tempfile.TemporaryDirectory() as tmp:
    bam = os.path.join(tmp, 'reads.bam')
    with open(bam, 'wb') as f:
      f.write(z['bam'].tobytes())
    with open(bam + '.bai', 'wb') as f:
      f.write(z['bai'].tobytes())
    ref = _Ref(z['ref_bases'].tobytes().decode(), int(z['ref_start'][0]))
    lo = ref.offset + first
    hi = min(lo + 1000 * n_regions, ref.offset + len(ref.seq))
    table = packing.ReadTable.from_bam(bam, 'chr20', max(ref.offset, lo - 500), hi + 500, min_mapping_quality=5)
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  regions = [T.Range('chr20', s, min(s + 1000, hi)) for s in range(lo, hi, 1000)]
  tables = [table.take(np.nonzero((ends > r.start) & (starts < r.end))[0]) for r in regions]
  keep = [i for i, t in enumerate(tables) if t.n_reads]
  return ref, [tables[i] for i in keep], [regions[i] for i in keep]


def _chr20():
  ref, sets = RF.load()
  reads = sets['wgs']
  spans = [U.read_range(r) for r in reads]
  regions = [T.Range('chr20', s, min(s + 1000, 10_010_000)) for s in range(9_999_999, 10_010_000, 1000)]
  tables = [packing.ReadTable.from_reads([r for r, s in zip(reads, spans) if U.ranges_overlap(s, region)])
            for region in regions]
  return ref, tables, regions


def main():
  result = {}
  with RF.oracle_allele_counter():
    batches = {'chr20_golden': _chr20(), 'na12878_10': _na12878(20_000, 10), 'na12878_100': _na12878(0, 100)}
    for name, (ref, tables, regions) in batches.items():
      windows = _windows_of(ref, tables, regions)
      graphs = debruijn_graph.compact_batch(windows, R.realigner_config().dbg_config)
      # for DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES: the haplotypes of a window, candidate_haplotypes()'s own
      paths = debruijn_graph.paths_batch(windows, R.realigner_config().dbg_config)
      result[name] = {
          'max_paths': max([len(h) for _, _, h in paths], default=0),
          'max_hap_bytes': max([sum(len(s) for s in h) for _, _, h in paths], default=0),
          'over_max_num_paths': sum(status == 2 for _, status, _ in paths),
          'windows': len(windows), 'no_graph': sum(g.k == 0 for g in graphs),
          'max_vertices': max([len(g.vertex_seq) for g in graphs], default=0),
          'max_edges': max([len(g.edge_from) for g in graphs], default=0),
          'max_bases': max([len(w[0]) + sum(len(r.aligned_sequence) for r in w[1]) for w in windows], default=0),
          'max_reads': max([len(w[1]) for w in windows], default=0),
          'max_k': max([g.k for g in graphs], default=0), 'k_tries': sum(g.k_tries for g in graphs)}
  print(json.dumps(result))


if __name__ == '__main__':
  main()
