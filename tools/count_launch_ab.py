"""Counting launches of a batch: one per region (the default) against one for the whole batch (DV_COUNT_ONE_LAUNCH=1,
count_alleles_batch_kernel in csrc/allele_counter.hip), over the NA12878 100 kb BAM's 1 kb calling regions in one
batch, the two arms alternating in one process.  Every row's outputs are compared between the arms before anything is
timed.  Prints one JSON line: per row and arm the median, minimum and maximum host wall time over --repeats batches
after a warm-up (every timed call ends in a stream synchronisation inside the library), every run's time, the last
call's dv_count_batch_last_stats, and the host time of building the batch's counters and requests, which neither arm
changes.  Rows:

  run_batch                 AlleleCounter.run_batch(counters)
  run_batch_call            AlleleCounter.run_batch(counters, call=...)        (dv_call_candidates_batch)
  select_windows_of_tables  window_selector.select_windows_of_tables with DV_WINDOWS_DEVICE=1
  process_tables            RegionProcessor.process_tables, realigner off, the device caller
  realign_tables            Realigner.realign_tables with DV_WINDOWS_DEVICE=1

On a tree without the switch the default arm is measured alone, so the same file measures an older checkout.  Fails
without a GPU.  Kernel time is not measured here; run the tool on its own under
`rocprofv3 --kernel-trace --stats -- python tools/count_launch_ab.py --rows run_batch --repeats 1`: `batches` in the
output says how many batches each arm ran, so count_alleles_batch_kernel (one launch a batch) can be set against the
sum of a batch's count_alleles_kernel launches.

  python tools/count_launch_ab.py [--regions 102] [--repeats 7] [--rows run_batch,process_tables] [--out result.json]
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
from deepvariant_amd import allelecounter as A                      # noqa: E402
from deepvariant_amd import dv_types as T                           # noqa: E402
from deepvariant_amd import packing                                 # noqa: E402
from deepvariant_amd import variant_calling as vc                   # noqa: E402

SWITCH = 'DV_COUNT_ONE_LAUNCH'
ROWS = ('run_batch', 'run_batch_call', 'select_windows_of_tables', 'process_tables', 'realign_tables')


class _Ref:
  def __init__(self, seq, offset):
    self.seq, self.offset = seq, offset

  def n_bases(self, contig):
    return self.offset + len(self.seq)

  def get_bases(self, contig, start, end):
    lo, hi = max(start, self.offset), min(end, self.offset + len(self.seq))
    inner = self.seq[lo - self.offset:hi - self.offset] if hi > lo else ''
    return 'N' * max(0, min(lo, end) - start) + inner + 'N' * max(0, end - max(hi, start))


def _set(arm):
  if arm == 'one_launch':
    os.environ[SWITCH] = '1'
  else:
    os.environ.pop(SWITCH, None)


def _summary(seconds):
  ms = [1e3 * s for s in seconds]
  return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3),
          'runs_ms': [round(x, 3) for x in ms]}


def _stats():
  if not hasattr(A, 'last_batch_stats'):
    return None
  return dict(A.last_batch_stats()._asdict())


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--regions', type=int, default=102, help='calling regions per batch')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--rows', default=','.join(ROWS))
  ap.add_argument('--label', default='')
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  rows = [r for r in args.rows.split(',') if r]
  if any(r not in ROWS for r in rows):
    raise SystemExit('count_launch_ab: rows are %s' % ', '.join(ROWS))
  if _lib.device_count() == 0:
    raise SystemExit('count_launch_ab: no GPU (the allele counter has no CPU fallback)')
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
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  batch = []
  for start in range(lo, hi, 1000):
    end = min(start + 1000, hi)
    batch.append((T.Range('chr20', start, end), table.take(np.nonzero((ends > start) & (starts < end))[0])))
  batch = [b for b in batch if b[1].n_reads][:args.regions]
  regions, tables = [b[0] for b in batch], [b[1] for b in batch]
  has_switch = hasattr(A, 'count_one_launch')
  arms = ['per_region', 'one_launch'] if has_switch else ['per_region']
  caller = vc.VariantCaller(vc.VariantCallerOptions(2, 2, 0.12, 0.06, sample_name='NA12878'))

  def counters():
    out = []
    for region, t in zip(regions, tables):
      c = A.AlleleCounter(ref, 'chr20', region.start, region.end, min_mapping_quality=5, min_base_quality=10)
      c.add_table(t)
      out.append(c)
    return out

  def counted(c):
    return (c.ref_supporting_read_counts().tobytes(), c.n_counted_reads(), c._events.tobytes())   # pylint: disable=protected-access

  # every row: prepare() outside the clock -> state; run(state) inside it -> what the arms are compared on
  def run_batch_row():
    def run(cs):
      A.AlleleCounter.run_batch(cs)
      return cs
    return counters, run, lambda cs: [counted(c) for c in cs]

  def run_batch_call_row():
    def run(cs):
      A.AlleleCounter.run_batch(cs, call=caller.candidate_options())
      return cs
    return counters, run, lambda cs: [counted(c) + tuple(x.tobytes() for x in c._cand[1:]) for c in cs]   # pylint: disable=protected-access

  def select_windows_row():
    from deepvariant_amd.realigner import realigner as R
    from deepvariant_amd.realigner import window_selector as ws
    if not hasattr(ws, 'windows_on_device'):
      return None
    config = R.realigner_config().ws_config
    return (lambda: None), (lambda _: ws.select_windows_of_tables(config, ref, tables, regions)), (lambda out: out)

  def process_tables_row():
    from deepvariant_amd import make_examples_core as mec
    from tests.golden.make_golden import wgs_options
    options = T.MakeExamplesOptions(pic_options=wgs_options(),
                                    sample_options=[T.SampleOptions(role='main', name='NA12878', pileup_height=100)])
    proc = mec.RegionProcessor(options, ref, mec.RegionProcessorOptions(realigner_enabled=False))
    return (lambda: None), (lambda _: proc.process_tables(regions, tables, tables)), \
        (lambda out: [calls for calls, _ in out])

  def realign_tables_row():
    from deepvariant_amd.realigner import realigner as R
    realigner = R.Realigner(R.realigner_config(), ref)

    def key(out):
      return [([(c.span, c.haplotypes) for c in ch], t.read_pos.tobytes(), t.cigar.tobytes(), t.bases.tobytes())
              for ch, t in out]
    return (lambda: None), (lambda _: realigner.realign_tables(tables, regions)), key

  makers = {'run_batch': run_batch_row, 'run_batch_call': run_batch_call_row,
            'select_windows_of_tables': select_windows_row, 'process_tables': process_tables_row,
            'realign_tables': realign_tables_row}
  result = {'label': args.label, 'regions': len(regions), 'reads': int(sum(t.n_reads for t in tables)),
            'repeats': args.repeats, 'has_switch': has_switch, 'arms': arms, 'rows': {}, 'batches': {a: 0 for a in arms}}
  # what neither arm changes: the Python side of a batch before the library is called
  build = []
  for _ in range(args.repeats + 1):
    gc.collect()
    t0 = time.perf_counter()
    requests = [c._request() for c in counters()]                     # pylint: disable=protected-access
    build.append(time.perf_counter() - t0)
    del requests
  result['build_counters_and_requests'] = _summary(build[1:])
  for name in rows:
    if name in ('select_windows_of_tables', 'realign_tables'):
      os.environ['DV_WINDOWS_DEVICE'] = '1'
    made = makers[name]()
    if made is None:
      result['rows'][name] = None
      continue
    prepare, run, key = made
    answers, stats = {}, {}
    for arm in arms:                                                  # compared before anything is timed
      _set(arm)
      answers[arm] = key(run(prepare()))
      stats[arm] = _stats()
      result['batches'][arm] += 1
    if has_switch and answers['one_launch'] != answers['per_region']:
      raise SystemExit('count_launch_ab: the arms differ (%s)' % name)
    times = {arm: [] for arm in arms}
    for i in range(args.repeats + 1):                                 # the first round is the warm-up
      for arm in arms:
        _set(arm)
        state = prepare()
        gc.collect()
        t0 = time.perf_counter()
        run(state)
        if i:
          times[arm].append(time.perf_counter() - t0)
        result['batches'][arm] += 1
    _set('per_region')
    os.environ.pop('DV_WINDOWS_DEVICE', None)
    result['rows'][name] = {arm: dict(_summary(times[arm]), last_stats=stats[arm]) for arm in arms}
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
