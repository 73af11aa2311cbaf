"""The device route of the window realigner (dv_realign_regions_device: the local alignments of all windows
of a batch of regions in one kernel launch, csrc/local_align.hip) against the host route, dv_realign_regions:
every array of dv_realign_output must be identical.  stats.pairs > 0, pairs_on_host == 0 and launches == 1 keep
a run that never reached the device from passing."""
import concurrent.futures
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from deepvariant_amd.realigner import realigner as R
from deepvariant_amd.realigner import utils as U
from tests import realigner_fixture as RF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _output_arrays(job):
  """Runs the job's native call and copies every array of dv_realign_output out of the result."""
  handle, out = job._call()                                                   # pylint: disable=protected-access
  try:
    n = len(job._jobs)                                                        # pylint: disable=protected-access
    view = lambda ptr, count: np.ctypeslib.as_array(ptr, shape=(count,)).copy() if count else np.zeros(0)   # noqa: E731
    a = {'region_row_off': view(out.region_row_off, n + 1)}
    rows = int(a['region_row_off'][-1])
    for name in ('order', 'status', 'position'):
      a[name] = view(getattr(out, name), rows)
    a['cigar_off'] = view(out.cigar_off, rows + 1)
    a['cigar'] = view(out.cigar, int(a['cigar_off'][-1]))
    a['region_assembled_off'] = view(out.region_assembled_off, n + 1)
    n_asm = int(a['region_assembled_off'][-1])
    a['assembled_window'] = view(out.assembled_window, n_asm)
    a['assembled_hap_off'] = view(out.assembled_hap_off, n_asm + 1)
    n_haps = int(a['assembled_hap_off'][-1])
    a['hap_text_off'] = view(out.hap_text_off, n_haps + 1)
    a['hap_text'] = C.string_at(out.hap_text, int(a['hap_text_off'][-1])) if n_haps else b''
    return a
  finally:
    _lib.lib().dv_realign_result_free(handle)


def _chr20_batch():
  ref, sets = RF.load()
  reads = sets['wgs']
  spans = [U.read_range(r) for r in reads]
  regions = [T.Range('chr20', s, min(s + 1000, 10_010_000)) for s in range(9_999_999, 10_010_000, 1000)]
  tables = [packing.ReadTable.from_reads([r for r, s in zip(reads, spans) if U.ranges_overlap(s, region)])
            for region in regions]
  return ref, tables, regions


class _Ref:
  def __init__(self, seq, offset):
    self.seq, self.offset = seq, offset

  def n_bases(self, contig):
    return self.offset + len(self.seq)

  def get_bases(self, contig, start, end):
    lo, hi = max(start, self.offset), min(end, self.offset + len(self.seq))
    inner = self.seq[lo - self.offset:hi - self.offset] if hi > lo else ''
    return 'N' * max(0, min(lo, end) - start) + inner + 'N' * max(0, end - max(hi, start))


def _na12878_batch(tmp_path, n_regions=10):
  with np.load(os.path.join(ROOT, 'tests', 'golden', 'na12878_100kb.npz')) as z:
    bam = str(tmp_path / 'reads.bam')
    with open(bam, 'wb') as f:
      f.write(z['bam'].tobytes())
    with open(bam + '.bai', 'wb') as f:
      f.write(z['bai'].tobytes())
    ref = _Ref(z['ref_bases'].tobytes().decode(), int(z['ref_start'][0]))
  lo = ref.offset + 20_000
  table = packing.ReadTable.from_bam(bam, 'chr20', lo - 500, lo + 1000 * n_regions + 500, min_mapping_quality=5)
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  regions = [T.Range('chr20', s, s + 1000) for s in range(lo, lo + 1000 * n_regions, 1000)]
  tables = [table.take(np.nonzero((ends > r.start) & (starts < r.end))[0]) for r in regions]
  return ref, tables, regions


def _compare_routes(ref, tables, regions):
  host = R.Realigner(R.realigner_config(), ref, device_align=False).start_realign_tables(tables, regions)
  device = R.Realigner(R.realigner_config(), ref, device_align=True).start_realign_tables(tables, regions)
  want, got = _output_arrays(host), _output_arrays(device)
  assert host.device_stats is None
  assert sorted(got) == sorted(want)
  for name in want:
    assert np.array_equal(got[name], want[name]) if isinstance(want[name], np.ndarray) else got[name] == want[name], name
  stats = device.device_stats
  assert stats.pairs > 0 and stats.pairs_on_host == 0 and stats.launches == 1 and stats.cells > 0
  assert int((want['status'] == 1).sum()) > 0           # reads did move
  return stats


def test_chr20_golden_regions_every_output_array():
  _compare_routes(*_chr20_batch())


def test_na12878_ten_regions_in_one_batch(tmp_path):
  _compare_routes(*_na12878_batch(tmp_path))


def _same_tables(a, b):
  for f in dataclasses.fields(packing.ReadTable):
    x, y = getattr(a, f.name), getattr(b, f.name)
    if isinstance(x, np.ndarray):
      assert np.array_equal(x, y), f.name
    else:
      assert x == y, f.name


def test_realign_tables_on_the_main_thread_and_on_an_executor_thread():
  ref, tables, regions = _chr20_batch()
  want = R.Realigner(R.realigner_config(), ref, device_align=False).realign_tables(tables, regions)
  rl = R.Realigner(R.realigner_config(), ref, device_align=True)
  with concurrent.futures.ThreadPoolExecutor(max_workers=1) as pool:
    first = rl.start_realign_tables(tables[:4], regions[:4], executor=pool)      # two jobs in flight, as the runner has
    second = rl.start_realign_tables(tables[4:], regions[4:], executor=pool)
    threaded = first.result() + second.result()
  assert first.device_stats.launches == 1 and second.device_stats.launches == 1
  for got in (rl.realign_tables(tables, regions), threaded):
    assert len(got) == len(want)
    for (ch_a, t_a), (ch_b, t_b) in zip(want, got):
      assert [(c.span, c.haplotypes) for c in ch_a] == [(c.span, c.haplotypes) for c in ch_b]
      _same_tables(t_a, t_b)


def test_device_route_is_off_unless_asked_for():
  ref, _ = RF.load()
  assert os.environ.get('DV_REALIGN_DEVICE', '0') == '1' or not R.Realigner(R.realigner_config(), ref).device_align


def test_golden_illumina_chain_with_device_realigner_in_a_child_process():
  env = dict(os.environ, DV_REALIGN_DEVICE='1')
  done = subprocess.run([sys.executable, '-m', 'tests.realign_device_chain'], cwd=ROOT, env=env, capture_output=True,
                        text=True, timeout=600)
  assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
  assert '84/84' in done.stdout
