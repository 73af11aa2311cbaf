"""The step between the candidate caller and the encoder, two ways, alternating in one process on one GPU:
(a) the per-region route -- ExamplesGenerator.encode_region_on_device: dv_pack_region by read NAME, one upload
and one encoder launch per region -- and (b) the batched route behind DV_PACK_DEVICE=1 --
ExamplesGenerator.encode_regions_on_device: dv_pack_regions_device by read ROW for a batch of regions
(csrc/pack_regions.hip), one upload and one encoder launch per batch.

  1. "pack + encode" over the 1 kb calling regions of the NA12878 100 kb fixture (tests/golden/na12878_100kb.npz;
     candidates from RegionProcessor.process_tables, realigner off), in batches of make_examples' _REGION_BATCH
     regions: wall time per batch of regions.
  2. the pack step alone on the synthetic region of `bench.py --mode host` (--batch sites, 7,700 by default):
     packing.pack_region_native on 8 host threads against packing.pack_regions_device; both include their Python
     marshalling (key blob / key ids) because that is what the route pays.

The two routes' outputs are compared before anything is timed.  Times are host clocks around calls that end in a
device synchronise; medians of --repeats alternating rounds after a warm-up, with min and max, in milliseconds.
Kernel times are not measured (no trace run is made).

  python tools/pack_device_ab.py [--repeats 7] [--batch 7700] [--out FILE]   (default: profiles/pack_device_ab.txt)
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepvariant_amd import dv_types as T                      # noqa: E402
from deepvariant_amd import make_examples as me                # noqa: E402
from deepvariant_amd import make_examples_core as core         # noqa: E402
from deepvariant_amd import packing                            # noqa: E402
from deepvariant_amd import synth                              # noqa: E402


def na12878_regions(tmp):
  """-> (RegionProcessor, [(candidates, table)] per 1 kb calling region), as tests/test_hip_candidates.py sets them up."""
  import pathlib
  from tests import test_hip_gvcf as HG
  from tests.golden.make_golden import wgs_options
  bam, ref = HG._bam_fixture(pathlib.Path(tmp))                   # pylint: disable=protected-access
  regions = list(core.partition(T.Range('chr20', ref.offset, ref.offset + len(ref.seq)), 1000))
  table = packing.ReadTable.from_bam(bam, 'chr20', regions[0].start, regions[-1].end, min_mapping_quality=5)
  options = T.MakeExamplesOptions(pic_options=wgs_options(),
                                  sample_options=[T.SampleOptions(role='main', name='NA12878', pileup_height=100)])
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  tables = [table.take(np.nonzero((ends > r.start) & (starts < r.end))[0]) for r in regions]
  proc = core.RegionProcessor(options, ref, core.RegionProcessorOptions(realigner_enabled=False))
  return proc, proc.process_tables(regions, tables)


def summary(values):
  return {'median': float(np.median(values)), 'min': float(min(values)), 'max': float(max(values))}


def main(argv=None):
  import torch
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--batch', type=int, default=7700)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pack_device_ab.txt'))
  args = ap.parse_args(argv)
  torch.cuda.init()
  result = {'repeats': args.repeats, 'not_measured': 'kernel times (no trace run); make_examples end to end'}

  # ---- 1. pack + encode over the NA12878 regions
  with tempfile.TemporaryDirectory() as tmp:
    proc, called = na12878_regions(tmp)
  gen = proc.generator
  pic = proc.options.pic_options
  shape = [100, pic.width, len(pic.channels)]
  step = me._REGION_BATCH                                         # pylint: disable=protected-access
  batches = [called[at:at + step] for at in range(0, len(called), step)]

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

  a, b = per_region(), batched()                                  # the warm-up, and the comparison
  n_examples = 0
  for k, ((img_a, plan_a), (img_b, plan_b)) in enumerate(zip(a, b)):
    if plan_a != plan_b or (plan_a and img_a.cpu().numpy().tobytes() != img_b.cpu().numpy().tobytes()):
      raise SystemExit('the routes differ in region %d' % k)
    n_examples += len(plan_a)
  del a, b
  times = {'per_region': [], 'batched': []}
  for _ in range(args.repeats):
    for name, fn in (('per_region', per_region), ('batched', batched)):
      t0 = time.perf_counter()
      fn()
      times[name].append((time.perf_counter() - t0) * 1e3 / len(batches))
  result['na12878_100kb'] = {
      'regions': len(called), 'regions_per_batch': step, 'batches': len(batches),
      'candidates': sum(len(c) for c, _ in called), 'examples': n_examples, 'outputs_equal': True,
      'pack_encode_ms_per_batch_per_region_route': summary(times['per_region']),
      'pack_encode_ms_per_batch_batched_route': summary(times['batched'])}

  # ---- 2. the pack step alone on bench.py --mode host's synthetic region
  opts = synth.illumina_options(7)
  H, W, C = opts.height, opts.width, 7
  generated = synth.make_illumina_batch(args.batch, seed=synth.SEED, options=opts)
  table, cands, combos, windows = synth.region_inputs_from_batch(generated, opts)
  os.environ['DV_PACK_THREADS'] = '8'

  def host_pack():
    return packing.pack_region_native(table, cands, combos, windows, W, opts.read_overlap_buffer_bp, H, H * W * C,
                                      use_groups=True)

  def device_pack(download=False):
    packed, plan = packing.pack_regions_device([table], [cands], [combos], [windows], W, opts.read_overlap_buffer_bp, H,
                                               H * W * C)
    torch.cuda.synchronize()
    try:
      return (packed.download() if download else None), plan, packing.pack_device_stats()
    finally:
      packed.close()

  host, host_plan = host_pack()
  got, plan, stats = device_pack(download=True)
  if [(ci, combo) for _, ci, combo in plan] != host_plan:
    raise SystemExit('the packers give different plans')
  for name in ('item_variant_start', 'item_image_start', 'item_ref_idx', 'item_list_off', 'item_height', 'item_out_off',
               'list_read', 'list_code', 'list_group'):
    if not np.array_equal(got[name], getattr(host, name)):
      raise SystemExit('the packers differ in %s' % name)
  times = {'host': [], 'device': []}
  for _ in range(args.repeats):
    for name, fn in (('host', host_pack), ('device', device_pack)):
      t0 = time.perf_counter()
      fn()
      times[name].append((time.perf_counter() - t0) * 1e3)
  result['synthetic_region'] = {
      'sites': args.batch, 'candidates': len(cands), 'reads': int(table.n_reads), 'outputs_equal': True, 'stats': stats,
      'dv_pack_region_8_threads_ms': summary(times['host']), 'dv_pack_regions_device_ms': summary(times['device'])}
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())
