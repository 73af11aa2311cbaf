"""gVCF blocks of the NA12878 100 kb BAM's 1 kb calling regions: the device pass
(AlleleCounter.run_batch(gvcf=...), dv_count_alleles_gvcf_batch) against the host route it replaces
(run_batch + AlleleCounter.summary_counts() + VariantCaller.make_gvcfs per region).  Prints one JSON
line: host wall times per batch of regions (median of --repeats after a warm-up), the records, and the
bytes the gVCF kernels move by construction (for a kernel trace's times: rocprofv3 --kernel-trace --stats).

  python tools/gvcf_bench.py [--batch 120] [--repeats 5] [--out result.json]
"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepvariant_amd import allelecounter as A   # noqa: E402
from deepvariant_amd import packing              # noqa: E402
from deepvariant_amd import variant_calling as vc   # noqa: E402


class _Ref:
  def __init__(self, seq, offset):
    self.seq, self.offset = seq, offset

  def n_bases(self, contig):
    return self.offset + len(self.seq)

  def get_bases(self, contig, start, end):
    lo, hi = max(start, self.offset), min(end, self.offset + len(self.seq))
    inner = self.seq[lo - self.offset:hi - self.offset] if hi > lo else ''
    return 'N' * max(0, min(lo, end) - start) + inner + 'N' * max(0, end - max(hi, start))


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=120, help='regions per device call')
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  import torch
  torch.cuda.init()
  with np.load(os.path.join(ROOT, 'tests', 'golden', 'na12878_100kb.npz')) as z, tempfile.TemporaryDirectory() as tmp:
    bam = os.path.join(tmp, 'reads.bam')
    with open(bam, 'wb') as f:
      f.write(z['bam'].tobytes())
    with open(bam + '.bai', 'wb') as f:
      f.write(z['bai'].tobytes())
    ref = _Ref(z['ref_bases'].tobytes().decode(), int(z['ref_start'][0]))
    lo, hi = ref.offset, ref.offset + len(ref.seq)
    table = packing.ReadTable.from_bam(bam, 'chr20', lo, hi, min_mapping_quality=5)
  ends = table.read_end.astype(np.int64)
  regions = []
  for start in range(lo, hi, 1000):
    end = min(start + 1000, hi)
    regions.append((start, end, table.take(np.nonzero((ends > start) & (table.read_pos.astype(np.int64) < end))[0])))
  regions = [r for r in regions if r[2].keys][:args.batch]
  opts = vc.GvcfOptions('NA12878', include_med_dp=True)
  caller = vc.VariantCaller(vc.VariantCallerOptions(sample_name='NA12878'))
  opts.table()
  caller.reference_confidence(0, 0)

  def counters():
    out = []
    for start, end, t in regions:
      c = A.AlleleCounter(ref, 'chr20', start, end, min_mapping_quality=5, min_base_quality=10)
      c.add_table(t)
      out.append(c)
    return out

  # the host route leaves ~10^6 objects behind: collect outside the timed windows, or a collection that the
  # next route's allocations trigger is charged to it
  def host_route():
    cs = counters()
    gc.collect()
    t0 = time.perf_counter()
    A.AlleleCounter.run_batch(cs)
    t1 = time.perf_counter()
    recs = [caller.make_gvcfs(c.summary_counts(), include_med_dp=True) for c in cs]
    return t1 - t0, time.perf_counter() - t1, recs

  def device_route():
    cs = counters()
    gc.collect()
    t0 = time.perf_counter()
    A.AlleleCounter.run_batch(cs, gvcf=opts)
    t1 = time.perf_counter()
    arrays = [c.gvcf_block_array(opts) for c in cs]
    t2 = time.perf_counter()
    recs = [c.gvcf_blocks(opts) for c in cs]
    return t1 - t0, t2 - t1, time.perf_counter() - t2, recs, cs, arrays

  host_route()
  device_route()
  host, dev = [], []
  for _ in range(args.repeats):
    host.append(host_route())
    dev.append(device_route())
  assert all(a == b for a, b in zip(host[-1][2], dev[-1][3])), 'device records differ from the host restatement'
  cs, arrays = dev[-1][4], dev[-1][5]
  sites = sum(c.interval_length() for c in cs)
  events = sum(len(c._events) for c in cs)             # pylint: disable=protected-access
  blocks = sum(len(a) for a in arrays)
  # bytes the five gVCF kernels move by construction: link reads events (16 B) and swaps a head / writes a
  # link (8 B); resolve reads events and walks the list (~16 B per entry) and adds a count (4 B); sites read
  # ref_count, alt, ref (9 B) and write key, gq, dp, tix (16 B); blocks read key (4 B) and write the run
  # arrays, then read gq, dp (8 B) per site; records 56 B written, read and written again by the pack
  gvcf_bytes = events * (16 + 8 + 16 + 16 + 4) + sites * (9 + 16 + 4 + 8) + blocks * 3 * 56
  med = lambda xs: float(np.median(xs)) * 1e3    # noqa: E731
  result = {
      'regions': len(cs), 'sites': sites, 'events': events, 'records': blocks,
      'host_count_ms': med([h[0] for h in host]), 'host_summary_make_gvcfs_ms': med([h[1] for h in host]),
      'device_count_and_gvcf_ms': med([d[0] for d in dev]), 'device_records_to_numpy_ms': med([d[1] for d in dev]),
      'device_records_to_variants_ms': med([d[2] for d in dev]),
      'gvcf_kernel_bytes': gvcf_bytes,
  }
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
