"""The window realigner over the NA12878 100 kb BAM's 1 kb calling regions in one batch, through
Realigner.realign_tables: the host route (dv_realign_regions) against the device route
(dv_realign_regions_device: the local alignments of all windows in one kernel launch, csrc/local_align.hip),
alternating in one process.  The two routes' tables and haplotypes are compared before anything is timed.
Prints one JSON line: per DV_REALIGN_THREADS setting (16 and 4) and per route the median wall time of
realign_tables over --repeats batches after a warm-up, the share of it spent in the native call, every run's
time (the spread), and the device route's stats: pairs, forward-pass cells, share of pairs aligned on the host.
Where the library has the device trace-back, the device route is measured in two arms that alternate with the
host route: `device` with DV_REALIGN_DEVICE_TRACEBACK=0 (every CIGAR's banded trace-back on the host) and
`device_traceback` with =1 (in the kernel); the split of the trace-backs and the widest band are in `stats`.
Where it has the device fast pass, `device_fast_pass` is one more alternating arm: DV_REALIGN_DEVICE_FASTPASS=1 with the
trace-back on the host, against `device` with both switches 0; its (haplotype, read) pairs and diagonal cells are in
`stats`.  Where it has the device assembly, `device_assembly` (DV_REALIGN_DEVICE_ASSEMBLY=1, the other two switches 0:
phase 1's graphs in one launch of csrc/debruijn.hip) and `device_all` (all three switches 1) alternate with them too;
windows, k-mer occurrences hashed and k values tried are in `stats`.  Where it has the device paths, `device_all_paths`
(all four switches 1: DV_REALIGN_DEVICE_PATHS=1 on top of `device_all`, pruning and the haplotypes from the device too)
is one more arm, compared with `device_all`; its windows, haplotypes and download size are in `stats`, next to the
size of `device_all`'s download of the graphs' pools.  Where it has the device finish, `device_all_finish` (all five
switches 1: DV_REALIGN_DEVICE_FINISH=1 on top of `device_all_paths`, the alignments finished by csrc/realign_finish.hip)
is one more arm, compared with `device_all_paths`; its windows, reads, words and download size are in `stats`.  Fails
without a GPU.  On a tree without the device route the host route is measured alone, so the same file
measures an older checkout.  Kernel time is not measured here: run this under
`rocprofv3 --kernel-trace --stats -- python tools/realign_bench.py --repeats 1 --threads 16` and divide
`cells` by local_align_sweeps' time per call (fast_pass_kernel: `fast_pass_cells`, with DV_REALIGN_DEVICE_FASTPASS=1
-- the tool sets the switches per arm itself, so profile with `--arms device_fast_pass`; debruijn_kernel:
`assembly_kmers`, with `--arms device_assembly`).

  python tools/realign_bench.py [--regions 100] [--repeats 7] [--threads 16,4] [--arms a,b] [--out result.json]
"""
import argparse
import dataclasses
import gc
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepvariant_amd import _lib                           # noqa: E402
from deepvariant_amd import dv_types as T                  # noqa: E402
from deepvariant_amd import packing                        # noqa: E402
from deepvariant_amd.realigner import realigner as R       # noqa: E402


class _Ref:
  def __init__(self, seq, offset):
    self.seq, self.offset = seq, offset

  def n_bases(self, contig):
    return self.offset + len(self.seq)

  def get_bases(self, contig, start, end):
    lo, hi = max(start, self.offset), min(end, self.offset + len(self.seq))
    inner = self.seq[lo - self.offset:hi - self.offset] if hi > lo else ''
    return 'N' * max(0, min(lo, end) - start) + inner + 'N' * max(0, end - max(hi, start))


def _same(a, b):
  for f in dataclasses.fields(packing.ReadTable):
    x, y = getattr(a, f.name), getattr(b, f.name)
    if not (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y):
      return False
  return True


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--regions', type=int, default=100, help='calling regions per batch')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--threads', default='16,4', help='DV_REALIGN_THREADS settings to measure')
  ap.add_argument('--arms', default='', help='time only these arms (comma-separated); default: every arm')
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  if _lib.device_count() == 0:
    raise SystemExit('realign_bench: no GPU (the device route has no CPU fallback)')
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
  has_device = hasattr(_lib, 'DvRealignDeviceStats')
  has_traceback = hasattr(_lib, 'DvRealignTracebackStats')
  has_fast_pass = hasattr(_lib, 'DvFastPassStats')
  has_assembly = hasattr(_lib, 'DvDebruijnDeviceStats')
  switch, fast_pass_switch = 'DV_REALIGN_DEVICE_TRACEBACK', 'DV_REALIGN_DEVICE_FASTPASS'
  assembly_switch = 'DV_REALIGN_DEVICE_ASSEMBLY'
  has_paths = hasattr(_lib, 'DvDebruijnPathsStats')
  paths_switch = 'DV_REALIGN_DEVICE_PATHS'
  has_finish = hasattr(_lib, 'DvRealignFinishStats')
  finish_switch = 'DV_REALIGN_DEVICE_FINISH'
  if has_device:
    routes = {'host': R.Realigner(R.realigner_config(), ref, device_align=False),
              'device': R.Realigner(R.realigner_config(), ref, device_align=True)}
    if has_traceback:
      routes['device_traceback'] = routes['device']
    if has_fast_pass:
      routes['device_fast_pass'] = routes['device']
    if has_assembly:
      routes['device_assembly'] = routes['device']
      routes['device_all'] = routes['device']
    if has_paths:
      routes['device_all_paths'] = routes['device']
    if has_finish:
      routes['device_all_finish'] = routes['device']
  else:
    routes = {'host': R.Realigner(R.realigner_config(), ref)}

  def run(route):
    if has_traceback:
      # read by the library at each call
      os.environ[switch] = '1' if route in ('device_traceback', 'device_all', 'device_all_paths', 'device_all_finish') else '0'
    if has_fast_pass:
      os.environ[fast_pass_switch] = '1' if route in ('device_fast_pass', 'device_all', 'device_all_paths', 'device_all_finish') else '0'
    if has_assembly:
      os.environ[assembly_switch] = '1' if route in ('device_assembly', 'device_all', 'device_all_paths', 'device_all_finish') else '0'
    if has_paths:
      os.environ[paths_switch] = '1' if route in ('device_all_paths', 'device_all_finish') else '0'
    if has_finish:
      os.environ[finish_switch] = '1' if route == 'device_all_finish' else '0'
    gc.collect()
    t0 = time.perf_counter()
    job = routes[route].start_realign_tables(tables, regions, want_haplotypes=False)    # window selection
    t1 = time.perf_counter()
    out = job.result()                                                                    # the native call + write-back
    t2 = time.perf_counter()
    return t2 - t0, t2 - t1, out, job

  # the routes must agree before either is timed (this is the warm-up too)
  _, _, want, _ = run('host')
  ms = lambda x: round(x * 1e3, 3)                         # noqa: E731
  result = {'regions': len(regions), 'reads': int(sum(t.n_reads for t in tables)), 'device_route': has_device,
            'threads': {}}
  if has_device:
    _, _, got, job = run('device')
    stats = job.device_stats
    assert len(want) == len(got) and all(_same(a[1], b[1]) for a, b in zip(want, got)), 'the device route differs'
    assert stats.pairs > 0 and stats.launches == 1
    result['stats'] = {'pairs': stats.pairs, 'cells': stats.cells, 'pairs_on_host': stats.pairs_on_host,
                       'share_on_host': round(stats.pairs_on_host / stats.pairs, 6), 'launches': stats.launches}
  if has_traceback:
    _, _, got, job = run('device_traceback')
    assert len(want) == len(got) and all(_same(a[1], b[1]) for a, b in zip(want, got)), 'the device trace-back differs'
    tb = job.traceback_stats
    assert job.device_stats.launches == 1 and tb.traced_on_device > 0
    result['stats'].update({'traced_on_device': tb.traced_on_device, 'traced_on_host': tb.traced_on_host,
                            'band_cells': tb.band_cells, 'widest_band': tb.widest_band})
  if has_fast_pass:
    _, _, got, job = run('device_fast_pass')
    assert len(want) == len(got) and all(_same(a[1], b[1]) for a, b in zip(want, got)), 'the device fast pass differs'
    fp = job.fast_pass_stats
    assert job.device_stats.launches == 1 and fp.launches == 1 and fp.haplotypes > 0
    result['stats'].update({'fast_pass_haplotypes': fp.haplotypes, 'fast_pass_haplotypes_on_host': fp.haplotypes_on_host,
                            'fast_pass_pairs': fp.pairs, 'fast_pass_cells': fp.cells, 'fast_pass_launches': fp.launches})
  if has_assembly:
    for route in ('device_assembly', 'device_all'):
      _, _, got, job = run(route)
      assert len(want) == len(got) and all(_same(a[1], b[1]) for a, b in zip(want, got)), 'the device assembly differs'
      asm = job.assembly_stats
      assert job.device_stats.launches == 1 and asm.launches == 1 and asm.windows > 0
      assert asm.windows_on_host == 0 and asm.windows_rejected == 0
      assert (job.fast_pass_stats.launches == 1) == (route == 'device_all')
    result['stats'].update({'assembly_windows': asm.windows, 'assembly_windows_on_host': asm.windows_on_host,
                            'assembly_kmers': asm.kmers, 'assembly_k_tries': asm.k_tries,
                            'assembly_launches': asm.launches, 'assembly_windows_rejected': asm.windows_rejected})
  if has_paths:
    _, _, got, job = run('device_all_paths')
    assert len(want) == len(got) and all(_same(a[1], b[1]) for a, b in zip(want, got)), 'the device paths differ'
    ps, asm = job.paths_stats, job.assembly_stats
    assert job.device_stats.launches == 1 and job.fast_pass_stats.launches == 1
    assert ps.launches == 2 and ps.windows == asm.windows > 0 and ps.windows_on_host == 0 and asm.windows_rejected == 0
    result['stats'].update({'paths_windows': ps.windows, 'paths_windows_on_host': ps.windows_on_host,
                            'paths_haplotypes': ps.paths, 'paths_hap_bytes': ps.hap_bytes,
                            'paths_launches': ps.launches, 'paths_bytes_down': ps.bytes_down})
  if has_finish:
    _, _, got, job = run('device_all_finish')
    assert len(want) == len(got) and all(_same(a[1], b[1]) for a, b in zip(want, got)), 'the device finish differs'
    fs = job.finish_stats
    assert job.device_stats.launches == 1 and fs.launches == 4 and fs.windows > 0 and fs.reads > 0
    result['stats'].update({'finish_windows': fs.windows, 'finish_windows_on_host': fs.windows_on_host,
                            'finish_reads': fs.reads, 'finish_cigar_words': fs.cigar_words,
                            'finish_launches': fs.launches, 'finish_bytes_down': fs.bytes_down,
                            'parent_sweep_bytes_down': job.device_stats.pairs * 72 * 4})
  for threads in [int(t) for t in args.threads.split(',')]:
    R._NATIVE_THREADS = threads                             # pylint: disable=protected-access
    runs = {route: [] for route in routes if not args.arms or route in args.arms.split(',')}
    for route in runs:
      run(route)
    for _ in range(args.repeats):
      for route in runs:                                    # alternating arms
        whole, native, _, _ = run(route)
        runs[route].append((whole, native))
    entry = {}
    for route, r in runs.items():
      entry[route] = {'realign_tables_ms': ms(float(np.median([x[0] for x in r]))),
                      'native_call_ms': ms(float(np.median([x[1] for x in r]))),
                      'realign_tables_runs_ms': [ms(x[0]) for x in r],
                      'native_call_runs_ms': [ms(x[1]) for x in r]}
    if 'device' in entry and 'host' in entry:
      entry['device_over_host_native'] = round(entry['device']['native_call_ms'] / entry['host']['native_call_ms'], 4)
    if 'device_traceback' in entry and 'device' in entry:
      entry['traceback_over_device_native'] = round(entry['device_traceback']['native_call_ms'] /
                                                    entry['device']['native_call_ms'], 4)
    if 'device_fast_pass' in entry and 'device' in entry:
      entry['fast_pass_over_device_native'] = round(entry['device_fast_pass']['native_call_ms'] /
                                                    entry['device']['native_call_ms'], 4)
      entry['fast_pass_median_below_device_min'] = (entry['device_fast_pass']['native_call_ms'] <
                                                    min(entry['device']['native_call_runs_ms']))
    for arm in ('device_assembly', 'device_all'):
      if arm in entry and 'device' in entry:
        entry[arm + '_over_device_native'] = round(entry[arm]['native_call_ms'] / entry['device']['native_call_ms'], 4)
        entry[arm + '_median_below_device_min'] = (entry[arm]['native_call_ms'] <
                                                   min(entry['device']['native_call_runs_ms']))
    if 'device_all_paths' in entry and 'device_all' in entry:
      entry['device_all_paths_over_device_all_native'] = round(entry['device_all_paths']['native_call_ms'] /
                                                               entry['device_all']['native_call_ms'], 4)
      entry['device_all_paths_median_below_device_all_min'] = (entry['device_all_paths']['native_call_ms'] <
                                                               min(entry['device_all']['native_call_runs_ms']))
    if 'device_all_finish' in entry and 'device_all_paths' in entry:
      entry['device_all_finish_over_device_all_paths_native'] = round(entry['device_all_finish']['native_call_ms'] /
                                                                      entry['device_all_paths']['native_call_ms'], 4)
      entry['device_all_finish_median_below_device_all_paths_min'] = (
          entry['device_all_finish']['native_call_ms'] < min(entry['device_all_paths']['native_call_runs_ms']))
    result['threads'][str(threads)] = entry
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
