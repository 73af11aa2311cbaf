"""Window selection over the NA12878 100 kb BAM's 1 kb calling regions in one batch: the host route of
window_selector.select_windows_of_tables (counts and events downloaded, scored in numpy / Python, merged in Python)
against the device route (DV_WINDOWS_DEVICE=1: dv_select_windows_batch, csrc/window_select.hip), alternating in one
process.  The two routes' windows are compared before anything is timed.  Prints one JSON line: per window selector
model (VARIANT_READS = the realigner's default flags, ALLELE_COUNT_LINEAR = ws_use_window_selector_model) and per
route the median, minimum and maximum wall time of select_windows_of_tables and of Realigner.realign_tables over
--repeats batches after a warm-up, every run's time, and the bytes each route brings home per batch (from the sizes
of what it downloads: counters, counts and events on the host route; counters, window counts and windows on the
device route).  On a tree without the device route the host route is measured alone, so the same file measures an
older checkout.  Fails without a GPU.  Kernel time is not measured here: run this under
`rocprofv3 --kernel-trace --stats -- python tools/window_select_ab.py --repeats 1`.

  python tools/window_select_ab.py [--regions 102] [--repeats 7] [--out result.json]
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
from deepvariant_amd import packing                                 # noqa: E402
from deepvariant_amd.realigner import realigner as R                # noqa: E402
from deepvariant_amd.realigner import window_selector as ws         # noqa: E402

SWITCH = 'DV_WINDOWS_DEVICE'


class _Ref:
  def __init__(self, seq, offset):
    self.seq, self.offset = seq, offset

  def n_bases(self, contig):
    return self.offset + len(self.seq)

  def get_bases(self, contig, start, end):
    lo, hi = max(start, self.offset), min(end, self.offset + len(self.seq))
    inner = self.seq[lo - self.offset:hi - self.offset] if hi > lo else ''
    return 'N' * max(0, min(lo, end) - start) + inner + 'N' * max(0, end - max(hi, start))


def _set(route):
  if route == 'device':
    os.environ[SWITCH] = '1'
  else:
    os.environ.pop(SWITCH, None)


def _timed(fn, routes, repeats):
  """Alternates the routes; -> {route: [seconds]} after one warm-up run each."""
  times = {r: [] for r in routes}
  for i in range(repeats + 1):
    for route in routes:
      _set(route)
      gc.collect()
      t0 = time.perf_counter()
      fn()
      if i:
        times[route].append(time.perf_counter() - t0)
  _set('host')
  return times


def _summary(seconds):
  ms = [1e3 * s for s in seconds]
  return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3),
          'runs_ms': [round(x, 3) for x in ms]}


def _bytes_home(config, ref, tables, regions, windows):
  """Per batch: what each route downloads, from the sizes of its arrays."""
  counters = [ws._make_counter(config, ref, (), region, table=table)[0]             # pylint: disable=protected-access
              for table, region in zip(tables, regions) if table.n_reads]
  from deepvariant_amd import allelecounter
  allelecounter.AlleleCounter.run_batch(counters)
  n = len(counters)
  host = sum(16 + 4 * c.interval_length() + 16 * len(c._events) for c in counters)  # pylint: disable=protected-access
  return {'host': host, 'device': n * (16 + 4) + 16 * sum(len(w) for w in windows)}


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--regions', type=int, default=102, help='calling regions per batch')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  if _lib.device_count() == 0:
    raise SystemExit('window_select_ab: no GPU (the allele counter has no CPU fallback)')
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
  has_device = hasattr(ws, 'windows_on_device')
  routes = ['host', 'device'] if has_device else ['host']
  result = {'regions': len(regions), 'reads': int(sum(t.n_reads for t in tables)), 'repeats': args.repeats,
            'has_device_route': has_device, 'models': {}}
  for name, use_model in (('VARIANT_READS', False), ('ALLELE_COUNT_LINEAR', True)):
    options = R.realigner_config(ws_use_window_selector_model=use_model)
    config = options.ws_config
    answers = {}
    for route in routes:
      _set(route)
      answers[route] = ws.select_windows_of_tables(config, ref, tables, regions)
    _set('host')
    if has_device and answers['device'] != answers['host']:
      raise SystemExit('window_select_ab: the routes differ (%s)' % name)
    realigner = R.Realigner(options, ref)
    select = _timed(lambda: ws.select_windows_of_tables(config, ref, tables, regions), routes, args.repeats)
    realign = _timed(lambda: realigner.realign_tables(tables, regions), routes, args.repeats)
    result['models'][name] = {
        'windows': sum(len(w) for w in answers['host']), 'regions_with_windows': sum(1 for w in answers['host'] if w),
        'select_windows_of_tables': {r: _summary(select[r]) for r in routes},
        'realign_tables': {r: _summary(realign[r]) for r in routes},
        'bytes_home_per_batch': _bytes_home(config, ref, tables, regions, answers['host'])}
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
