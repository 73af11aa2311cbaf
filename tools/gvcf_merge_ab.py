"""The gVCF merge: the host code (dv_gvcf_merge) against the device call
(dv_gvcf_merge_device, csrc/gvcf_merge.hip), alternating in one process, on two workloads.

  fixture    the NA12878 100 kb slice (tests/golden/na12878_100kb.npz, the seeded model): one fused run of
             make_examples --gvcf_outfile hands over the run's finished records and block arrays
  synthetic  a seeded layout of one large contig.  Its size is the fixture's blocks and records per kilobase times
             --contig_kb (230,000: the called part of chromosome 1), unless --blocks / --variants give it; the block
             lengths are drawn so that the density matches, the variants are mostly one to three bases with one in
             fifty of 40 to 400

Per workload and route: the median, minimum and maximum wall time of the merge call with its arguments ready, over
--repeats runs after a warm-up, every run's time, the device call's stats (bytes moved, launches) -- after both
routes' arrays were compared with == -- and beside it the time of the row text (gvcf_rows through the host merge; for
the synthetic layout one run, with made-up block values and reference).  Prints one JSON line.  Fails without a GPU.

  python tools/gvcf_merge_ab.py [--repeats 7] [--contig_kb 230000] [--blocks B --variants V] [--out result.json]
  python tools/gvcf_merge_ab.py --kernels_only      # the synthetic device call three times and nothing else: run under
                                                    # rocprofv3 --kernel-trace --stats for the kernels' times
"""
import argparse
import gc
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepvariant_amd import _lib                                    # noqa: E402
from deepvariant_amd import allelecounter                           # noqa: E402
from deepvariant_amd import dv_types as T                           # noqa: E402
from deepvariant_amd import genomics_io                             # noqa: E402
from deepvariant_amd import make_examples as me                     # noqa: E402
from deepvariant_amd import postprocess_variants as pp              # noqa: E402

FIELDS = ('piece_start', 'piece_end', 'piece_block', 'piece_slot', 'var_slot')


def _summary(seconds):
  ms = [1e3 * s for s in seconds]
  return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3),
          'runs_ms': [round(x, 3) for x in ms]}


def fixture_run():
  """-> (records, {contig: blocks}, reference reader's file kept alive by the caller's directory, contigs, kb)."""
  kept = {}
  original = pp.write_gvcf

  def keeping(path, records, blocks, ref_reader, contigs, sample_name, **kwargs):
    kept.update(records=list(records), blocks=dict(blocks), contigs=list(contigs))
    return original(path, records, blocks, ref_reader, contigs, sample_name, **kwargs)

  tmp = tempfile.mkdtemp()
  with np.load(os.path.join(ROOT, 'tests', 'golden', 'na12878_100kb.npz')) as z:
    bam = os.path.join(tmp, 'reads.bam')
    with open(bam, 'wb') as f:
      f.write(z['bam'].tobytes())
    with open(bam + '.bai', 'wb') as f:
      f.write(z['bai'].tobytes())
    fasta = os.path.join(tmp, 'ref.fa')
    start = int(z['ref_start'][0])
    bases = z['ref_bases'].tobytes().decode()
  genomics_io.write_fasta(fasta, [('chr20', 'N' * start + bases)])
  regions = 'chr20:%d-%d' % (start + 1, start + len(bases))
  argv = ['--ref', fasta, '--reads', bam, '--regions', regions, '--sample_name', 'NA12878', '--channel_list',
          ','.join(T.PILEUP_CHANNELS_WITH_INSERT_SIZE), '--checkpoint', 'random:7', '--gvcf_outfile',
          os.path.join(tmp, 'out.g.vcf')]
  parser = me.build_arg_parser()
  argv = me.absl_booleans(parser, argv)
  flags = parser.parse_args(argv)
  me.apply_flags_for_calling(parser, flags, argv)
  pp.write_gvcf = keeping
  try:
    me.make_examples_runner(flags)
  finally:
    pp.write_gvcf = original
  return kept['records'], kept['blocks'], genomics_io.FastaReader(fasta), kept['contigs'], len(bases) / 1000.0


def fixture_arguments(records, blocks, contigs):
  """The arguments gvcf_rows hands to the merge."""
  order = {name: k for k, (name, _) in enumerate(contigs)}
  records = sorted(records, key=lambda r: (order[r.reference_name], r.start, r.end))
  block_off, var_off, arrays, at = [0], [0], [], 0
  for name, _ in contigs:
    arr = blocks.get(name, np.zeros(0, allelecounter.GVCF_BLOCK_DTYPE))
    arrays.append(arr)
    block_off.append(block_off[-1] + arr.size)
    while at < len(records) and records[at].reference_name == name:
      at += 1
    var_off.append(at)
  every = np.concatenate(arrays)
  return (np.array(block_off, np.int64), np.array(var_off, np.int64), every['start'].copy(), every['end'].copy(),
          np.array([r.start for r in records], np.int64), np.array([r.end for r in records], np.int64))


def synthetic_arguments(n_blocks, n_variants, contig_bases, seed=22):
  rng = np.random.default_rng(seed)
  mean = max(2.0, contig_bases / max(n_blocks, 1))
  lengths = rng.integers(1, int(2 * mean), size=n_blocks)
  gaps = np.where(rng.integers(0, 200, size=n_blocks) == 0, rng.integers(1, 300, size=n_blocks), 0)
  ends = np.cumsum(lengths + gaps)
  starts = ends - lengths
  v_start = np.sort(rng.integers(0, int(ends[-1]), size=n_variants))
  v_len = np.where(rng.integers(0, 50, size=n_variants) == 0, rng.integers(40, 400, size=n_variants),
                   rng.integers(1, 4, size=n_variants))
  v_end = v_start + v_len
  order = np.lexsort((v_end, v_start))
  return (np.array([0, n_blocks], np.int64), np.array([0, n_variants], np.int64), starts.astype(np.int64),
          ends.astype(np.int64), v_start[order].astype(np.int64), v_end[order].astype(np.int64))


def compare(arguments):
  host, device = pp.merge_blocks_and_variants(*arguments), pp.merge_blocks_and_variants_device(*arguments)
  for field in FIELDS:
    if not (getattr(host, field) == getattr(device, field)).all():
      raise SystemExit('gvcf_merge_ab: the routes differ in %s' % field)
  return pp.last_merge_stats()


def timed(arguments, repeats):
  import torch
  routes = {'host': pp.merge_blocks_and_variants, 'device': pp.merge_blocks_and_variants_device}
  times = {'host': [], 'device': []}
  for i in range(repeats + 1):            # the routes alternate, one warm-up run each
    for route, fn in routes.items():
      gc.collect()
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn(*arguments)
      if i:
        times[route].append(time.perf_counter() - t0)
  return {route: _summary(t) for route, t in times.items()}


class _SyntheticReference:
  def get_bases(self, contig, start, end):
    return 'ACGT' * ((end - start) // 4 + 1)


def synthetic_row_text_s(arguments):
  """One run of gvcf_rows over the synthetic blocks alone (made-up values), the host merge inside."""
  n = arguments[2].size
  blocks = np.zeros(n, allelecounter.GVCF_BLOCK_DTYPE)
  blocks['start'], blocks['end'] = arguments[2], arguments[3]
  blocks['likelihoods'] = np.array([-0.0, -3.01, -30.1])
  blocks['gq'], blocks['min_dp'], blocks['med_dp'], blocks['ref_base'], blocks['has_valid_gl'] = 30, 25, -1, ord('A'), 1
  records = [pp.VcfRecord('chr1', int(s), int(e), 'A' * int(e - s), ['C'], 30.0, 'PASS', [0, 1], 30,
                          [-3.0, 0.0, -3.0], 30, [15, 15], [0.5]) for s, e in zip(arguments[4].tolist(), arguments[5].tolist())]
  t0 = time.perf_counter()
  rows, _ = pp.gvcf_rows(records, {'chr1': blocks}, _SyntheticReference(), [('chr1', int(arguments[3][-1]) + 1000)])
  return time.perf_counter() - t0, len(rows)


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--contig_kb', type=float, default=230000.0)
  ap.add_argument('--blocks', type=int, default=0)
  ap.add_argument('--variants', type=int, default=0)
  ap.add_argument('--kernels_only', action='store_true')
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  if _lib.device_count() == 0:
    raise SystemExit('gvcf_merge_ab: no GPU')
  import torch
  torch.cuda.init()
  if args.kernels_only:
    arguments = synthetic_arguments(args.blocks or 8_000_000, args.variants or 400_000, int(args.contig_kb * 1000))
    for _ in range(3):
      pp.merge_blocks_and_variants_device(*arguments)
    print(json.dumps({'kernels_only': pp.last_merge_stats()}))
    return
  records, blocks, ref_reader, contigs, kb = fixture_run()
  fixture = fixture_arguments(records, blocks, contigs)
  result = {'repeats': args.repeats}
  n_blocks, n_variants = int(fixture[2].size), int(fixture[4].size)
  stats = compare(fixture)
  row_times = []
  for i in range(args.repeats + 1):
    t0 = time.perf_counter()
    rows, _ = pp.gvcf_rows(records, blocks, ref_reader, contigs)
    if i:
      row_times.append(time.perf_counter() - t0)
  result['fixture'] = {'kb': kb, 'blocks': n_blocks, 'variants': n_variants, 'pieces': stats['pieces'],
                       'blocks_per_kb': round(n_blocks / kb, 3), 'variants_per_kb': round(n_variants / kb, 3),
                       'merge_call': timed(fixture, args.repeats), 'device_stats': stats,
                       'row_text_with_host_merge': _summary(row_times), 'rows': len(rows)}
  guess = (8_000_000, 400_000)
  by_ratio = (int(round(n_blocks / kb * args.contig_kb)), int(round(n_variants / kb * args.contig_kb)))
  size = (args.blocks or by_ratio[0], args.variants or by_ratio[1])
  synthetic = synthetic_arguments(size[0], size[1], int(args.contig_kb * 1000))
  stats = compare(synthetic)
  result['synthetic'] = {'contig_kb': args.contig_kb, 'size_guessed': guess, 'size_by_fixture_ratio': by_ratio,
                         'blocks': size[0], 'variants': size[1], 'pieces': stats['pieces'],
                         'merge_call': timed(synthetic, args.repeats), 'device_stats': stats}
  seconds, n_rows = synthetic_row_text_s(synthetic)
  result['synthetic']['row_text_with_host_merge_one_run_s'] = round(seconds, 3)
  result['synthetic']['rows'] = n_rows
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
