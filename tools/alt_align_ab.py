"""The alt-align step of make_examples (ExamplesGenerator._plan_region up to the alt tables: window trimming, then
RealignReadsToHaplotype per candidate and alt allele), two ways, alternating in one process: (a) the Read-object
route -- alt_aligned_pileup_lib.trim_reads, one FastPassAligner per (candidate, alt) through
fast_pass_aligner.realign_reads_to_haplotype, ReadTable.from_reads of the kept objects -- and (b) the table route
behind DV_ALT_ALIGN_TABLES=1 -- trim_table, then ONE alt_align_table call per region (dv_alt_align_batch_device,
csrc/alt_align.hip).  Input: the PacBio golden chain's reads as tests/pacbio_chain.py loads them, its golden
variants as candidates, the golden run's image options minus base_methylation, one region per 25 kb partition.
The two routes' alt tables and ranges are compared field by field before anything is timed.  Times are host clocks
around calls that end in a device synchronise (the table route) or never touch the device (the object route's
realignment); medians of --repeats alternating rounds after a warm-up, with min and max, in milliseconds.

  python tools/alt_align_ab.py [--repeats 7] [--out FILE]      (default: profiles/alt_align_ab.txt)
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

from deepvariant_amd import alt_aligned_pileup_lib as A        # noqa: E402
from deepvariant_amd import dv_types as T                      # noqa: E402
from deepvariant_amd import make_examples_core as core         # noqa: E402
from deepvariant_amd import make_examples_native as men        # noqa: E402
from deepvariant_amd import packing                            # noqa: E402
from deepvariant_amd.realigner import utils as U               # noqa: E402


def inputs():
  from tests import pacbio_chain as PC
  ref, reads, meta, _ = PC.load()
  pic = PC.pic_options(True)
  pic.channels = [c for c in pic.channels if c != 'base_methylation']
  pic.num_channels = len(pic.channels)
  options = T.MakeExamplesOptions(pic_options=pic, trim_reads_for_pileup=True,
                                  sample_options=[T.SampleOptions(role='main', name='s', pileup_height=100)])
  regions = []
  for region in core.partition(PC.REGION, PC.PARTITION):
    in_reads = [r for r in reads if U.ranges_overlap(U.read_range(r), region)]
    seen, cands = set(), []
    for start, end, refb, alts, _ in meta:
      if region.start <= start < region.end and (start, alts) not in seen:
        seen.add((start, alts))
        cands.append(T.DeepVariantCall(variant=T.Variant('chr20', start, end, refb, list(alts)), allele_support={}))
    regions.append((cands, in_reads, packing.ReadTable.from_reads(in_reads)))
  return options, ref, regions


def same_table(a, b):
  for field in dataclasses.fields(packing.ReadTable):
    x, y = getattr(a, field.name), getattr(b, field.name)
    if isinstance(y, np.ndarray):
      if x is None or x.dtype != y.dtype or not np.array_equal(x, y):
        return field.name
    elif x != y:
      return field.name
  return None


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'alt_align_ab.txt'))
  args = ap.parse_args(argv)
  options, ref, regions = inputs()
  gen = men.ExamplesGenerator(options, {}, test_mode=True, ref_reader=ref)
  pic = options.pic_options
  stats = []
  real = A.alt_align_arrays

  def recording(*a, **kw):
    d = real(*a, **kw)
    if 'stats' in d:
      stats.append(d['stats'])
    return d

  def step(cands, reads):
    """-> (alt tables, ranges, seconds for trimming, seconds for the realignment)."""
    need_alt = [A.need_alt_alignment(pic, c.variant) for c in cands]
    tables = [reads if isinstance(reads, packing.ReadTable) else packing.ReadTable.from_reads(reads)]
    t0 = time.perf_counter()
    _, trim_ranges = gen._trim_region_reads(cands, [reads], [0], tables, [True] * len(cands))   # pylint: disable=protected-access
    t1 = time.perf_counter()
    alt_tables, ranges = gen._realign_for_alt_images(cands, need_alt, [0], trim_ranges)         # pylint: disable=protected-access
    t2 = time.perf_counter()
    return alt_tables, ranges, t1 - t0, t2 - t1

  def arm(on_tables):
    os.environ['DV_ALT_ALIGN_TABLES'] = '1'
    out = [step(cands, table if on_tables else reads) for cands, reads, table in regions]
    return out, sum(o[2] for o in out) * 1e3, sum(o[3] for o in out) * 1e3

  A.alt_align_arrays = recording
  try:
    # the routes agree before either is timed (this is the warm-up too)
    objects, tables = arm(False)[0], arm(True)[0]
    for k, (o, t) in enumerate(zip(objects, tables)):
      bad = same_table(t[0][0], o[0][0])
      if bad or o[1] != t[1]:
        raise SystemExit('the routes differ in region %d: %s' % (k, bad or 'ranges'))
    call_stats = list(stats)
    times = {'objects': [], 'tables': []}
    for _ in range(args.repeats):
      for name, on_tables in (('objects', False), ('tables', True)):
        _, trim_ms, align_ms = arm(on_tables)
        times[name].append((trim_ms, align_ms))
  finally:
    A.alt_align_arrays = real
  total = {k: int(sum(s[k] for s in call_stats)) for k in call_stats[0]} if call_stats else {}
  result = {'input': 'pacbio_full_chr20', 'regions': len(regions), 'candidates': sum(len(r[0]) for r in regions),
            'reads': [len(r[1]) for r in regions], 'alt_rows': [int(o[0][0].n_reads) for o in objects],
            'repeats': args.repeats, 'routes_equal': True, 'stats_summed_over_regions': total,
            'stats_per_region': call_stats}
  for name, rows in times.items():
    for label, col in (('trim_ms', 0), ('alt_align_ms', 1)):
      v = [r[col] for r in rows]
      result['%s_%s' % (name, label)] = {'median': float(np.median(v)), 'min': min(v), 'max': max(v)}
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())
