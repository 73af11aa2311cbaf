"""Read phasing of a batch of calling regions, three ways: (a) the Read-object route (RegionProcessor.process per
region: candidates_in_region with DirectPhasing.phase, supporting reads by name), (b) the table route
(RegionProcessor.process_tables) with direct_phasing.phase_arrays(device=False) -- the checker in a loop,
dv_phase_reads_batch -- and (c) the table route as it ships, phase_arrays(device=True): dv_phase_reads_batch_device,
csrc/phasing.hip.  All three count alleles and call candidates on the device; they differ in what phasing reads.
Input: the PacBio golden chain (tests/golden/pacbio_full_chr20.npz) in 5 kb regions (the first --max_regions), or
with --synthetic two haplotypes of 10-15 kb reads at 35x over 40 kb.  Candidates and HP values of the arms are
compared before anything is timed.  Prints one JSON line: medians of --repeats runs after a warm-up with min and
max, in milliseconds, the native call alone for (b) and (c) on the route's own arrays, and dv_phasing_stats (for the
kernel's own time: rocprofv3 --kernel-trace --stats -- python tools/phasing_bench.py --arms device).

  python tools/phasing_bench.py [--synthetic] [--repeats 7] [--arms objects,host,device] [--max_regions 8]
                                [--out result.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepvariant_amd import direct_phasing                # noqa: E402
from deepvariant_amd import dv_types as T                 # noqa: E402
from deepvariant_amd import make_examples_core as core    # noqa: E402
from deepvariant_amd import packing                       # noqa: E402
from deepvariant_amd import synth                         # noqa: E402

REGION = 5000


class SeqRef:
  def __init__(self, seq):
    self.seq = seq

  def n_bases(self, contig):
    return len(self.seq)

  def get_bases(self, contig, start, end):
    return self.seq[start:end]


def pacbio_input():
  from tests import pacbio_chain
  ref, reads, meta, _ = pacbio_chain.load()
  lo, hi = min(m[0] for m in meta), max(m[1] for m in meta)
  return ref, reads, 'chr20', lo - lo % REGION, hi


def synthetic_input(seed=3):
  """Two haplotypes that differ every ~300 bases over 40 kb, 10-15 kb reads at 35x with 0.2 % substitution errors."""
  rng = np.random.default_rng(seed)
  n, lo, hi = 70_000, 15_000, 55_000
  ref = ''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=n))
  haps = [list(ref), list(ref)]
  for k, pos in enumerate(np.nonzero(rng.random(n) < 1 / 300)[0].tolist()):
    haps[k % 2][pos] = 'ACGT'[('ACGT'.index(ref[pos]) + 1 + k % 3) % 4]
  reads, covered = [], 0
  while covered < 35 * (hi - lo):
    length = int(rng.integers(10_000, 15_001))
    start = int(rng.integers(lo - 10_000, hi - 2000))
    seq = haps[len(reads) % 2][start:start + length]
    for p in np.nonzero(rng.random(len(seq)) < 0.002)[0].tolist():
      seq[p] = 'ACGT'[int(rng.integers(0, 4))]
    covered += min(start + len(seq), hi) - max(start, lo)
    reads.append(T.cc_make_read('chr20', start, ''.join(seq), ['%dM' % len(seq)], 's%d' % len(reads)))
  reads.sort(key=lambda r: r.alignment.position.position)
  return SeqRef(ref), reads, 'chr20', lo, hi


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--synthetic', action='store_true')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--arms', default='objects,host,device')
  ap.add_argument('--max_regions', type=int, default=8)
  ap.add_argument('--out')
  args = ap.parse_args(argv)
  arms = args.arms.split(',')
  ref, reads, contig, lo, hi = synthetic_input() if args.synthetic else pacbio_input()
  regions = [T.Range(contig, s, min(s + REGION, hi)) for s in range(lo, hi, REGION)][:args.max_regions]
  pic = synth.longread_options('hifi')
  options = T.MakeExamplesOptions(pic_options=pic, sample_options=[T.SampleOptions(role='main', name='m')])
  proc = core.RegionProcessor(options, ref, core.RegionProcessorOptions(
      realigner_enabled=False, track_ref_reads=True, phase_reads=True))
  table = packing.ReadTable.from_reads(reads)
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  rows = [np.nonzero((ends > r.start) & (starts < r.end))[0] for r in regions]
  tables = [table.take(x) for x in rows]
  lists = [[reads[i] for i in x.tolist()] for x in rows]
  real = direct_phasing.phase_arrays
  captured = []

  def on_tables(device):
    def phase(regions_, min_alleles, **kw):
      captured[:] = [regions_, min_alleles]
      kw['device'] = device
      return real(regions_, min_alleles, **kw)
    direct_phasing.phase_arrays = phase
    try:
      return [(c, t.read_hp) for c, t in proc.process_tables(regions, tables)]
    finally:
      direct_phasing.phase_arrays = real

  def objects():
    out = []
    for region, in_reads in zip(regions, lists):
      cands, phased = proc.process(region, in_reads)
      out.append((cands, packing.ReadTable.from_reads(phased).read_hp))
    return out

  run = {'objects': objects, 'host': lambda: on_tables(False), 'device': lambda: on_tables(True)}
  # the arms agree before any of them is timed (this is the warm-up too)
  first = {arm: run[arm]() for arm in arms}
  for arm in arms[1:]:
    for k, ((c0, hp0), (c1, hp1)) in enumerate(zip(first[arms[0]], first[arm])):
      if c0 != c1 or hp0.tolist() != hp1.tolist():
        raise SystemExit('%s and %s differ in region %d' % (arms[0], arm, k))
  hp = np.concatenate([h for _, h in first[arms[0]]])
  result = {'input': 'synthetic' if args.synthetic else 'pacbio_full_chr20', 'reads': len(reads), 'regions': len(regions),
            'rows': int(sum(len(x) for x in rows)), 'candidates': int(sum(len(c) for c, _ in first[arms[0]])),
            'reads_phased': int(np.sum((hp == 1) | (hp == 2))), 'repeats': args.repeats, 'arms_equal': True}
  for arm, device in (('host', False), ('device', True)):
    if arm in arms and captured:
      concat = direct_phasing.concat_regions(captured[0])
      result[arm + '_stats'] = direct_phasing.phase_tables(*concat, captured[1], device=device)[3]
      times = []
      for _ in range(args.repeats):
        t0 = time.perf_counter()
        direct_phasing.phase_tables(*concat, captured[1], device=device)
        times.append((time.perf_counter() - t0) * 1e3)
      result[arm + '_native_call_only_ms'] = {'median': float(np.median(times)), 'min': min(times), 'max': max(times)}
      times = []
      for _ in range(args.repeats):
        t0 = time.perf_counter()
        real(captured[0], captured[1], device=device)
        times.append((time.perf_counter() - t0) * 1e3)
      result[arm + '_phase_arrays_ms'] = {'median': float(np.median(times)), 'min': min(times), 'max': max(times)}
  for arm in arms:
    times = []
    for _ in range(args.repeats):
      t0 = time.perf_counter()
      run[arm]()
      times.append((time.perf_counter() - t0) * 1e3)
    result[arm + '_ms'] = {'median': float(np.median(times)), 'min': min(times), 'max': max(times)}
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())
