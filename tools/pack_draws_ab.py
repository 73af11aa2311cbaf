"""From candidates to pixels for trimmed, alt-aligned regions, two ways, alternating in one process on one GPU:
(a) the per-region route -- ExamplesGenerator.encode_region_on_device: per region one trim call, one alt_align_table
call, a Python loop over candidate x combination x (1 + alts) with name strings, one upload of the region's
untrimmed + trimmed + alt tables, one encoder launch, one merge launch -- and (b) the batched route behind
DV_PACK_DEVICE=1 -- ExamplesGenerator.encode_regions_on_device: per region the trim call, then per BATCH one
alt_align_table call, one dv_pack_draws_device call (csrc/pack_regions.hip, items are row ranges), one upload of the
trimmed + alt tables, one encoder launch, one merge launch.  DV_ALT_ALIGN_TABLES=1 on both.

  1. the PacBio fixture (tests/golden, HiFi reads, width 147, diff_channels for indels, golden options minus
     base_methylation) in 1 kb regions, batches of --regions-per-batch (32)
  2. the synthetic long-read region of tests/test_hip_alt_align_route.py (width 99, 420 reads) cut in four

The two routes' outputs are compared before anything is timed.  "trim + alt-align + pack + encode" is a host clock
around the calls, ended by a device synchronise: medians of --repeats alternating rounds after a warm-up, with min
and max, in milliseconds per batch.  Upload bytes are those of the encoder batch (DeviceBatch.input_bytes: read
table, reference windows and, on the per-region route, the item and list arrays); what trim_table and
alt_align_table stage is the same on both routes up to the number of calls and is not counted.  Kernel times are not
measured (no trace run is made).

  python tools/pack_draws_ab.py [--repeats 7] [--out FILE]   (default: profiles/pack_draws_ab.txt)
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

from deepvariant_amd import dv_types as T                      # noqa: E402
from deepvariant_amd import make_examples_native as men        # noqa: E402
from deepvariant_amd import packing                            # noqa: E402
from deepvariant_amd import device_batch                       # noqa: E402


def pacbio_regions(size=1000):
  """-> (generator, image shape, [(candidates, table)] per `size` bp region of the fixture)."""
  from tests import pacbio_chain as PC
  ref, reads, meta, _ = PC.load()
  pic = PC.pic_options(True)
  pic.channels = [c for c in pic.channels if c != 'base_methylation']
  pic.num_channels = len(pic.channels)
  options = T.MakeExamplesOptions(pic_options=pic, trim_reads_for_pileup=True,
                                  sample_options=[T.SampleOptions(role='main', name='s', pileup_height=100)])
  gen = men.ExamplesGenerator(options, {}, test_mode=True, ref_reader=ref)
  table = packing.ReadTable.from_reads(reads)
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  regions = []
  for lo in range(PC.REGION.start, PC.REGION.end, size):
    seen, cands = set(), []
    for start, end, refb, alts, _ in meta:
      if lo <= start < lo + size and (start, alts) not in seen:
        seen.add((start, alts))
        cands.append(T.DeepVariantCall(variant=T.Variant('chr20', start, end, refb, list(alts)), allele_support={}))
    regions.append((cands, table.take(np.nonzero((ends > lo) & (starts < lo + size))[0])))
  return gen, [100, pic.width, len(pic.channels)], regions


def synthetic_regions():
  from tests.test_hip_alt_align_route import _region
  options, ref, reads, cands = _region('diff_channels', 'indels')
  options = dataclasses.replace(options, trim_reads_for_pileup=True)
  gen = men.ExamplesGenerator(options, {}, test_mode=True, ref_reader=ref)
  table = packing.ReadTable.from_reads(reads)
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  regions = []
  n = len(cands)
  for lo, hi in ((0, n // 4), (n // 4, n // 2), (n // 2, 3 * n // 4), (3 * n // 4, n)):
    part = cands[lo:hi]
    a, b = min(c.variant.start for c in part) - 150, max(c.variant.end for c in part) + 150
    regions.append((part, table.take(np.nonzero((ends > a) & (starts < b))[0])))
  pic = options.pic_options
  return gen, [pic.height, pic.width, len(pic.channels)], regions


def summary(values):
  return {'median': float(np.median(values)), 'min': float(min(values)), 'max': float(max(values))}


def measure(gen, shape, regions, per_batch, repeats):
  import torch
  batches = [regions[at:at + per_batch] for at in range(0, len(regions), per_batch)]
  uploaded = [0]
  real_init = device_batch.DeviceBatch.__init__

  def counting_init(self, *a, **kw):
    real_init(self, *a, **kw)
    uploaded[0] += self.input_bytes
  device_batch.DeviceBatch.__init__ = counting_init

  def per_region():
    out = []
    for batch in batches:
      for cands, table in batch:
        out.append(gen.encode_region_on_device(cands, [table], [0], [0.0], shape) if cands else (None, []))
    torch.cuda.synchronize()
    return out

  def batched():
    out = []
    for batch in batches:
      with_cands = [(c, t) for c, t in batch if c]
      drawn = iter(gen.encode_regions_on_device(with_cands, shape) if with_cands else [])
      out += [next(drawn) if c else (None, []) for c, _ in batch]
    torch.cuda.synchronize()
    return out

  try:
    bytes_of = {}
    uploaded[0] = 0
    a = per_region()                                              # the warm-up, and the comparison
    bytes_of['per_region'] = uploaded[0]
    uploaded[0] = 0
    b = batched()
    bytes_of['batched'] = uploaded[0]
    n_examples = 0
    for k, ((img_a, plan_a), (img_b, plan_b)) in enumerate(zip(a, b)):
      if plan_a != plan_b or (plan_a and img_a.cpu().numpy().tobytes() != img_b.cpu().numpy().tobytes()):
        raise SystemExit('the routes differ in region %d' % k)
      n_examples += len(plan_a)
    del a, b
    times = {'per_region': [], 'batched': []}
    for _ in range(repeats):
      for name, fn in (('per_region', per_region), ('batched', batched)):
        t0 = time.perf_counter()
        fn()
        times[name].append((time.perf_counter() - t0) * 1e3 / len(batches))
        print('%s: %.1f ms per batch' % (name, times[name][-1]), file=sys.stderr, flush=True)
  finally:
    device_batch.DeviceBatch.__init__ = real_init
  return {
      'regions': len(regions), 'regions_per_batch': per_batch, 'batches': len(batches),
      'candidates': sum(len(c) for c, _ in regions), 'examples': n_examples, 'outputs_equal': True,
      'trim_align_pack_encode_ms_per_batch_per_region_route': summary(times['per_region']),
      'trim_align_pack_encode_ms_per_batch_batched_route': summary(times['batched']),
      'encoder_upload_bytes_per_batch_per_region_route': bytes_of['per_region'] // len(batches),
      'encoder_upload_bytes_per_batch_batched_route': bytes_of['batched'] // len(batches)}


def main(argv=None):
  import torch
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--regions-per-batch', type=int, default=32)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pack_draws_ab.txt'))
  args = ap.parse_args(argv)
  torch.cuda.init()
  os.environ['DV_ALT_ALIGN_TABLES'] = '1'
  result = {'repeats': args.repeats,
            'not_measured': 'kernel times (no trace run); the staging of trim_table / alt_align_table; make_examples end to end'}
  gen, shape, regions = pacbio_regions()
  result['pacbio_1kb_regions'] = measure(gen, shape, regions, args.regions_per_batch, args.repeats)
  gen, shape, regions = synthetic_regions()
  result['synthetic_long_read_region'] = measure(gen, shape, regions, len(regions), args.repeats)
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())
