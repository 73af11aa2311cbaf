"""Candidates of the NA12878 100 kb BAM's 1 kb calling regions in one batch: the device caller
(AlleleCounter.run_batch(call=...), dv_call_candidates_batch, csrc/candidates.hip) against the host route
it replaces (run_batch + one Python Allele per event of the positions worth a look + VariantCaller's walk).
Prints one JSON line: host wall times per batch (medians of --repeats after a warm-up) of counting and of
calling apart, for both routes; the wall time of RegionProcessor.process_tables over the same batch (raw
reads, realigner off: the counting and calling share of a region driver); calls; bytes sent home per batch.
On a tree without the device route the host figures and process_tables are reported alone, so the same
file measures an older checkout (for the kernels' times: rocprofv3 --kernel-trace --stats).

  python tools/candidates_bench.py [--batch 120] [--repeats 5] [--track_ref_reads] [--out result.json]
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
from deepvariant_amd import dv_types as T        # noqa: E402
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


class _HostOnly:
  """The same counter without the device caller: VariantCaller walks its Python counts."""

  def __init__(self, counter):
    self._c = counter

  def __getattr__(self, name):
    if name in ('candidates', 'candidate_positions'):
      raise AttributeError(name)
    return getattr(self._c, name)


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=120, help='regions per device call')
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--track_ref_reads', action='store_true', help='the two-pass scheme')
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
  track = args.track_ref_reads
  caller = vc.VariantCaller(vc.VariantCallerOptions(2, 2, 0.12, 0.06, sample_name='NA12878', track_ref_reads=track))
  has_device = hasattr(A.AlleleCounter, 'candidates')

  def counters(positions=None):
    out = []
    for k, (start, end, t) in enumerate(regions):
      c = A.AlleleCounter(ref, 'chr20', start, end, candidate_positions=positions[k] if positions else (),
                          min_mapping_quality=5, min_base_quality=10, track_ref_reads=track)
      c.add_table(t)
      out.append(c)
    return out

  def home_bytes(cs):
    """Counts and events the counter sends home for these counters."""
    return sum(4 * c.interval_length() + 16 * len(c._events) for c in cs)   # pylint: disable=protected-access

  # the host route leaves ~10^5 objects behind: collect outside the timed windows, or a collection that the
  # next route's allocations trigger is charged to it
  def host_route():
    count = call = 0.0
    sent = 0
    positions = None
    if track:
      first = counters()
      gc.collect()
      t0 = time.perf_counter()
      A.AlleleCounter.run_batch(first)
      t1 = time.perf_counter()
      positions = [caller.call_positions_from_allele_counter(_HostOnly(c)) for c in first]
      count, call, sent = t1 - t0, time.perf_counter() - t1, home_bytes(first)
    cs = counters(positions)
    gc.collect()
    t0 = time.perf_counter()
    A.AlleleCounter.run_batch(cs)
    t1 = time.perf_counter()
    calls = [caller.calls_from_allele_counter(_HostOnly(c)) for c in cs]
    return count + t1 - t0, call + time.perf_counter() - t1, calls, sent + home_bytes(cs)

  def device_route():
    count = call = 0.0
    sent = 0
    positions = None
    if track:
      first = counters()
      gc.collect()
      t0 = time.perf_counter()
      A.AlleleCounter.run_batch(first, call=caller.candidate_options(positions_only=True))
      t1 = time.perf_counter()
      positions = [caller.call_positions_from_allele_counter(c) for c in first]
      count, call = t1 - t0, time.perf_counter() - t1
      sent = sum(16 + 8 + 20 * len(p) for p in positions)           # counters, record counts, site records
    cs = counters(positions)
    gc.collect()
    t0 = time.perf_counter()
    A.AlleleCounter.run_batch(cs, call=caller.candidate_options())
    t1 = time.perf_counter()
    calls = [caller.calls_from_allele_counter(c) for c in cs]
    t2 = time.perf_counter()
    for c in cs:
      _, sites, alleles, words = c._cand                            # pylint: disable=protected-access
      sent += 8 + sites.nbytes + alleles.nbytes + words.nbytes
    return count + t1 - t0, call + t2 - t1, calls, sent + home_bytes(cs)

  from deepvariant_amd import make_examples_core as mec
  from tests.golden.make_golden import wgs_options
  options = T.MakeExamplesOptions(pic_options=wgs_options(),
                                  sample_options=[T.SampleOptions(role='main', name='NA12878', pileup_height=100)])
  proc = mec.RegionProcessor(options, ref, mec.RegionProcessorOptions(realigner_enabled=False, track_ref_reads=track))
  ranges = [T.Range('chr20', s, e) for s, e, _ in regions]
  tables = [t for _, _, t in regions]

  def process_tables():
    gc.collect()
    t0 = time.perf_counter()
    out = proc.process_tables(ranges, tables, tables)
    return time.perf_counter() - t0, sum(len(calls) for calls, _ in out)

  host_route()
  process_tables()
  if has_device:
    device_route()
  host, dev, whole = [], [], []
  for _ in range(args.repeats):
    host.append(host_route())
    if has_device:
      dev.append(device_route())
    whole.append(process_tables())
  med = lambda xs: round(float(np.median(xs)) * 1e3, 3)    # noqa: E731
  result = {
      'regions': len(regions), 'track_ref_reads': track, 'device_route': has_device,
      'calls': sum(map(len, host[-1][2])),
      'host_count_ms': med([h[0] for h in host]), 'host_call_ms': med([h[1] for h in host]),
      'host_bytes_home': host[-1][3],
      'process_tables_ms': med([w[0] for w in whole]), 'process_tables_runs_ms': [round(w[0] * 1e3, 3) for w in whole],
      'process_tables_calls': whole[-1][1],
  }
  if has_device:
    assert host[-1][2] == dev[-1][2], 'device calls differ from the host restatement'
    result.update({'device_count_and_call_ms': med([d[0] for d in dev]), 'device_build_calls_ms': med([d[1] for d in dev]),
                   'device_bytes_home': dev[-1][3]})
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
