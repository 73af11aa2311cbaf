"""Window trimming of one stretch of long reads, three ways: the Read-object route (alt_aligned_pileup_lib.trim_reads
per candidate + ReadTable.from_reads of the trimmed copies), alt_aligned_pileup_lib.trim_table(device=False) (the
host entry point dv_trim_reads_batch) and trim_table(device=True) (dv_trim_reads_batch_device, csrc/trim_reads.hip).
Input: the PacBio golden chain (tests/golden/pacbio_full_chr20.npz: 281 HiFi reads over 100 kb, one window of
width 147 per distinct golden variant), or with --synthetic 10-15 kb reads at 35x over 100 kb with 100 candidates.
The three tables are compared field by field before anything is timed.  Prints one JSON line: medians of
--repeats runs after a warm-up with min and max, in milliseconds, and the pair and word counts (for the kernels'
own times: rocprofv3 --kernel-trace --stats -- python tools/trim_bench.py --arms device).

  python tools/trim_bench.py [--synthetic] [--repeats 7] [--arms objects,host,device] [--out result.json]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepvariant_amd import alt_aligned_pileup_lib as A   # noqa: E402
from deepvariant_amd import dv_types as T                 # noqa: E402
from deepvariant_amd import packing                       # noqa: E402

BUFFER_BP = 5


def pacbio_input():
  from tests import pacbio_chain
  ref, reads, meta, _ = pacbio_chain.load()
  width = 147
  contig = ref.n_bases('chr20')
  sites = sorted({(start, end, refb) for start, end, refb, _, _ in meta})
  variants = [T.Variant('chr20', start, end, refb, ['N']) for start, end, refb in sites]
  return reads, variants, width, contig


def synthetic_input(seed=1):
  """10-15 kb reads at 35x over 100 kb, HiFi-like CIGARs (a short operation every ~150 bases), 100 candidates."""
  rng = np.random.default_rng(seed)
  span, contig, width = 100_000, 200_000, 147
  reads = []
  covered = 0
  while covered < 35 * span:
    ops, length = [], 0
    target = int(rng.integers(10_000, 15_001))
    while length < target:
      run = int(rng.integers(20, 300))
      ops.append(T.CigarUnit(1, run))
      length += run
      ops.append(T.CigarUnit(int(rng.choice((2, 3, 9))), int(rng.integers(1, 4))))
    ops.append(T.CigarUnit(1, 30))
    qlen = sum(u.operation_length for u in ops if u.operation in (1, 2, 9))
    covered += length
    reads.append(T.Read(
        fragment_name='s%d' % len(reads), read_number=0, number_reads=1,
        aligned_sequence=''.join('ACGT'[int(j)] for j in rng.integers(0, 4, size=qlen)),
        aligned_quality=bytes(rng.integers(0, 60, size=qlen).astype(np.uint8)),
        alignment=T.LinearAlignment(position=T.Position('chr20', int(rng.integers(40_000, 40_000 + span)), False),
                                    mapping_quality=60, cigar=ops)))
  reads.sort(key=lambda r: r.alignment.position.position)
  variants = [T.Variant('chr20', p, p + 1, 'A', ['C'])
              for p in sorted(set(rng.integers(55_000, 40_000 + span, size=100).tolist()))]
  return reads, variants, width, contig


def same_table(a, b):
  for f in dataclasses.fields(packing.ReadTable):
    x, y = getattr(a, f.name), getattr(b, f.name)
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
      if x is None or y is None or x.dtype != y.dtype or not np.array_equal(x, y):
        return f.name
    elif x != y:
      return f.name
  return None


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--synthetic', action='store_true')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--arms', default='objects,host,device')
  ap.add_argument('--out')
  args = ap.parse_args(argv)
  arms = args.arms.split(',')
  reads, variants, width, contig = synthetic_input() if args.synthetic else pacbio_input()
  hw = (width - 1) // 2
  table = packing.ReadTable.from_reads(reads)
  windows = []
  for v in variants:
    r0, r1 = A.calculate_alignment_region(v, hw, contig)
    windows.append((v.start - BUFFER_BP, v.end + BUFFER_BP, r0, r1, A.K_DEFAULT_MINIMUM_READ_OVERLAP))

  def objects():
    trimmed, starts = [], []
    for q0, q1, r0, r1, min_overlap in windows:
      kept, original = A.trim_reads([reads[int(k)] for k in table.query(q0, q1)], r0, r1, min_overlap)
      trimmed.extend(kept)
      starts.extend(original)
    return packing.ReadTable.from_reads(trimmed, alignment_positions=starts)

  run = {'objects': objects, 'host': lambda: A.trim_table(table, windows, device=False)[0],
         'device': lambda: A.trim_table(table, windows, device=True)[0]}
  # the arms agree before any of them is timed (this is the warm-up too)
  tables = {arm: run[arm]() for arm in arms}
  for arm in arms[1:]:
    differs = same_table(tables[arms[0]], tables[arm])
    if differs:
      raise SystemExit('%s and %s differ in %s' % (arms[0], arm, differs))
  result = {'input': 'synthetic' if args.synthetic else 'pacbio_full_chr20', 'reads': len(reads),
            'windows': len(windows), 'width': width, 'cigar_words': int(len(table.cigar)),
            'bases': int(len(table.bases)), 'rows_kept': int(tables[arms[0]].n_reads),
            'bases_kept': int(len(tables[arms[0]].bases)), 'repeats': args.repeats, 'tables_equal': True}
  if 'device' in arms:
    result['stats'] = A.trim_table(table, windows, device=True, with_stats=True)[2]
    arrays = []     # the native call alone, without building the table
    for _ in range(args.repeats):
      t0 = time.perf_counter()
      A.trim_arrays(table, windows, device=True)
      arrays.append((time.perf_counter() - t0) * 1e3)
    result['device_arrays_only_ms'] = {'median': float(np.median(arrays)), 'min': min(arrays), 'max': max(arrays)}
  if 'host' in arms:
    arrays = []
    for _ in range(args.repeats):
      t0 = time.perf_counter()
      A.trim_arrays(table, windows, device=False)
      arrays.append((time.perf_counter() - t0) * 1e3)
    result['host_arrays_only_ms'] = {'median': float(np.median(arrays)), 'min': min(arrays), 'max': max(arrays)}
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
