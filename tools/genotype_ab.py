"""From the classifier's output to finished VCF rows on the NA12878 100 kb slice (tests/golden/na12878_100kb.npz, the
seeded model): the device merge (dv_genotype_sites_device on the output tensor, csrc/genotype.hip) against
DV_GENOTYPE_HOST=1 (the tensor downloaded, dv_genotype_sites), alternating in one process.

One fused run of make_examples --vcf_outfile collects what every flush of the queue hands to
RegionProcessor._genotype_queue (the regions' plans and the output tensor, which stays on the device).  A timed run
replays those calls -- site tables from the plans, the merge, the status check, step 4 -- and formats every row;
nothing before the classifier's output is in it.  One pass over the slice is about 305 examples; a timed run replays
the flushes --passes times (10, as `bench.py --mode bam --repeat 10` does for its 3,040).  The two routes' rows are
compared before anything is timed.  Prints one JSON line: per route the median, minimum and maximum wall time over
--repeats runs after a warm-up and every run's time, for the whole stretch (`classifier_output_to_vcf_rows`) and for
the merge call alone with the site tables ready (`merge_call_alone`: the download plus dv_genotype_sites against
dv_genotype_sites_device); the examples, sites and flushes per run; and the device route's dv_genotype_device_stats
summed over one pass.  Fails without a GPU.

  python tools/genotype_ab.py [--repeats 7] [--passes 10] [--regions chr20:10,000,000-10,100,000] [--out result.json]
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
from deepvariant_amd import dv_types as T                           # noqa: E402
from deepvariant_amd import genomics_io                             # noqa: E402
from deepvariant_amd import make_examples as me                     # noqa: E402
from deepvariant_amd import make_examples_core as core              # noqa: E402
from deepvariant_amd import postprocess_variants as pp              # noqa: E402

SWITCH = 'DV_GENOTYPE_HOST'


def _set(route):
  if route == 'host':
    os.environ[SWITCH] = '1'
  else:
    os.environ.pop(SWITCH, None)


def _summary(seconds):
  ms = [1e3 * s for s in seconds]
  return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3),
          'runs_ms': [round(x, 3) for x in ms]}


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--passes', type=int, default=10)
  ap.add_argument('--regions', default='')
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  if _lib.device_count() == 0:
    raise SystemExit('genotype_ab: no GPU (the classifier has no CPU fallback)')
  import torch
  torch.cuda.init()
  flushes = []
  original = core.RegionProcessor._genotype_queue            # pylint: disable=protected-access

  def collecting(self, queue, probs):
    flushes.append((self, [(c, plan, None) for c, plan, _ in queue], probs.clone()))
    return original(self, queue, probs)

  with np.load(os.path.join(ROOT, 'tests', 'golden', 'na12878_100kb.npz')) as z, tempfile.TemporaryDirectory() as tmp:
    bam = os.path.join(tmp, 'reads.bam')
    with open(bam, 'wb') as f:
      f.write(z['bam'].tobytes())
    with open(bam + '.bai', 'wb') as f:
      f.write(z['bai'].tobytes())
    fasta = os.path.join(tmp, 'ref.fa')
    start = int(z['ref_start'][0])
    bases = z['ref_bases'].tobytes().decode()
    genomics_io.write_fasta(fasta, [('chr20', 'N' * start + bases)])
    regions = args.regions or 'chr20:%d-%d' % (start + 1, start + len(bases))
    argv = ['--ref', fasta, '--reads', bam, '--regions', regions, '--sample_name', 'NA12878', '--channel_list',
            ','.join(T.PILEUP_CHANNELS_WITH_INSERT_SIZE), '--checkpoint', 'random:7', '--vcf_outfile',
            os.path.join(tmp, 'out.vcf')]
    parser = me.build_arg_parser()
    argv = me.absl_booleans(parser, argv)
    flags = parser.parse_args(argv)
    me.apply_flags_for_calling(parser, flags, argv)
    core.RegionProcessor._genotype_queue = collecting          # pylint: disable=protected-access
    try:
      _set('device')
      run_stats = me.make_examples_runner(flags)
    finally:
      core.RegionProcessor._genotype_queue = original          # pylint: disable=protected-access

  def replay():
    rows, device = [], {}
    for proc, queue, probs in flushes:
      proc.vcf = core.VcfSink(want_records=False)
      original(proc, queue, probs)
      rows.extend(pp.vcf_row(r) for r in proc.vcf.records)
      for name, value in proc.vcf.device_stats.items():
        device[name] = device.get(name, 0) + value
    return rows, device

  answers = {}
  for route in ('host', 'device'):
    _set(route)
    answers[route] = replay()
  if answers['host'][0] != answers['device'][0]:
    raise SystemExit('genotype_ab: the routes differ')
  tables = [core.RegionProcessor.queue_sites(queue)[1] for _, queue, _ in flushes]

  def merge_alone(route):
    for (_, _, probs), t in zip(flushes, tables):
      if route == 'host':
        pp.genotype_sites(probs.cpu().numpy(), *t)
      else:
        pp.genotype_sites_device(probs, *t)

  def timed(fn):
    """-> {route: [seconds]}: the routes alternate, one warm-up run each."""
    times = {'host': [], 'device': []}
    for i in range(args.repeats + 1):
      for route in ('host', 'device'):
        _set(route)
        gc.collect()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.passes):
          fn(route)
        if i:
          times[route].append(time.perf_counter() - t0)
    _set('device')
    return times

  whole = timed(lambda route: replay())
  merge = timed(merge_alone)
  result = {'examples': int(run_stats['n_examples']) * args.passes, 'sites': len(answers['device'][0]) * args.passes,
            'flushes': len(flushes) * args.passes, 'passes': args.passes, 'repeats': args.repeats,
            'classifier_output_to_vcf_rows': {r: _summary(whole[r]) for r in whole},
            'merge_call_alone': {r: _summary(merge[r]) for r in merge},
            'device_stats_per_pass': answers['device'][1]}
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
