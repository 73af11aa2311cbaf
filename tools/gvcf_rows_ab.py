"""The gVCF's rows: the Python formatter over the host merge against the native rows on the host
(dv_gvcf_rows) and on the device (dv_gvcf_rows_device, csrc/gvcf_rows.hip), alternating in one process.

  fixture    the NA12878 100 kb slice, as tools/gvcf_merge_ab.py prepares it: the run's finished records and blocks
  synthetic  that tool's seeded layout of one large contig of --contig_kb, --blocks and --variants; the blocks' fields
             are drawn, the records are one SNP-like record per variant

Stretches, each the median, minimum and maximum wall time over --repeats runs after a warm-up, after the three outputs
were compared with ==:
  a            gvcf_rows + join + encode, the host merge inside (the baseline: the Python formatter)
  b, c         gvcf_body_native on the host and on the device: sorting, the variants' rows in Python, one native call
  *_blocks     the same three without records: no variant row is made, the blocks stay whole
  b_call, c_call   the native call alone, its arguments ready: what is left of b and c is Python's
  variant_rows     gvcf_variant_row + encode over the records alone
Prints one JSON line per layout.  Fails without a GPU.

  python tools/gvcf_rows_ab.py --layout fixture [--repeats 7] [--out result.json]
  python tools/gvcf_rows_ab.py --layout synthetic --blocks 8000000 --variants 400000
  python tools/gvcf_rows_ab.py --kernels_only --blocks 8000000 --variants 400000   # the device call three times and
                                                    # nothing else: run under rocprofv3 --kernel-trace --stats
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gvcf_merge_ab as AB                                          # noqa: E402
from deepvariant_amd import _lib                                    # noqa: E402
from deepvariant_amd import allelecounter                           # noqa: E402
from deepvariant_amd import postprocess_variants as pp              # noqa: E402


def synthetic_layout(n_blocks, n_variants, contig_kb, seed=23):
  """-> (records, {contig: blocks}, reference, contigs) over AB.synthetic_arguments' spans."""
  _, _, b_start, b_end, v_start, v_end = AB.synthetic_arguments(n_blocks, n_variants, int(contig_kb * 1000))
  rng = np.random.default_rng(seed)
  blocks = np.zeros(n_blocks, allelecounter.GVCF_BLOCK_DTYPE)
  blocks['start'], blocks['end'] = b_start, b_end
  blocks['likelihoods'] = -rng.random((n_blocks, 3)) * np.array([0.1, 9.0, 90.0])
  blocks['gq'] = rng.integers(0, 51, n_blocks)
  blocks['min_dp'] = rng.integers(0, 60, n_blocks)
  blocks['med_dp'] = -1
  blocks['ref_base'] = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, n_blocks)]
  blocks['has_valid_gl'] = rng.integers(0, 20, n_blocks) > 0
  records = [pp.VcfRecord('chr1', int(s), int(e), 'A' * int(e - s), ['C'], 30.0, 'PASS', [0, 1], 30, [-3.0, 0.0, -3.0],
                          30, [15, 15], [0.5]) for s, e in zip(v_start.tolist(), v_end.tolist())]
  return records, {'chr1': blocks}, AB._SyntheticReference(), [('chr1', int(b_end[-1]) + 1000)]


def native_arguments(records, blocks, ref_reader, contigs):
  """gvcf_rows_native's arguments as gvcf_body_native makes them, caught on their way."""
  caught = {}
  original = pp.gvcf_rows_native

  def catching(*args, **kwargs):
    caught['args'], caught['kwargs'] = args, {k: v for k, v in kwargs.items() if k not in ('device', 'stream')}
    return original(*args, **kwargs)

  pp.gvcf_rows_native = catching
  try:
    pp.gvcf_body_native(records, blocks, ref_reader, contigs)
  finally:
    pp.gvcf_rows_native = original
  return caught['args'], caught['kwargs']


def measure(records, blocks, ref_reader, contigs, repeats):
  import torch
  args, kwargs = native_arguments(records, blocks, ref_reader, contigs)
  routes = {
      'a': lambda: ''.join(pp.gvcf_rows(records, blocks, ref_reader, contigs)[0]).encode(),
      'b': lambda: pp.gvcf_body_native(records, blocks, ref_reader, contigs).text,
      'c': lambda: pp.gvcf_body_native(records, blocks, ref_reader, contigs, device=True).text,
      'a_blocks': lambda: ''.join(pp.gvcf_rows([], blocks, ref_reader, contigs)[0]).encode(),
      'b_blocks': lambda: pp.gvcf_body_native([], blocks, ref_reader, contigs).text,
      'c_blocks': lambda: pp.gvcf_body_native([], blocks, ref_reader, contigs, device=True).text,
      'b_call': lambda: pp.gvcf_rows_native(*args, **kwargs).text,
      'c_call': lambda: pp.gvcf_rows_native(*args, device=True, **kwargs).text,
      'variant_rows': lambda: [pp.gvcf_variant_row(r).encode() for r in records],
  }
  # the outputs first
  text = routes['a']()
  for route in ('b', 'c', 'b_call', 'c_call'):
    if routes[route]() != text:
      raise SystemExit('gvcf_rows_ab: route %s writes other bytes than the Python formatter' % route)
  stats = pp.last_rows_stats()
  whole = routes['a_blocks']()
  if routes['b_blocks']() != whole or routes['c_blocks']() != whole:
    raise SystemExit('gvcf_rows_ab: the routes differ on the blocks alone')
  n_bytes, n_rows = len(text), text.count(b'\n')
  del text, whole
  times = {route: [] for route in routes}
  for i in range(repeats + 1):            # the routes alternate, one warm-up run each
    for route, fn in routes.items():
      gc.collect()
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      out = fn()
      seconds = time.perf_counter() - t0
      del out
      if i:
        times[route].append(seconds)
  result = {route: AB._summary(t) for route, t in times.items()}
  result.update(rows=n_rows, text_bytes=n_bytes, device_stats=stats)
  return result


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--layout', choices=('fixture', 'synthetic'), default='fixture')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--contig_kb', type=float, default=230000.0)
  ap.add_argument('--blocks', type=int, default=8_000_000)
  ap.add_argument('--variants', type=int, default=400_000)
  ap.add_argument('--kernels_only', action='store_true')
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  if _lib.device_count() == 0:
    raise SystemExit('gvcf_rows_ab: no GPU')
  import torch
  torch.cuda.init()
  if args.kernels_only:
    call_args, kwargs = native_arguments(*synthetic_layout(args.blocks, args.variants, args.contig_kb))
    for _ in range(3):
      pp.gvcf_rows_native(*call_args, device=True, **kwargs)
    print(json.dumps({'kernels_only': pp.last_rows_stats()}))
    return
  if args.layout == 'fixture':
    records, blocks, ref_reader, contigs, kb = AB.fixture_run()
    result = {'layout': 'fixture', 'kb': kb}
  else:
    records, blocks, ref_reader, contigs = synthetic_layout(args.blocks, args.variants, args.contig_kb)
    result = {'layout': 'synthetic', 'contig_kb': args.contig_kb}
  result.update(blocks=sum(len(b) for b in blocks.values()), variants=len(records), repeats=args.repeats)
  result.update(measure(records, blocks, ref_reader, contigs, args.repeats))
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'a') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
