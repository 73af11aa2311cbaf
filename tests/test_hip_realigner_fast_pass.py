"""dv_realign_regions_device with the fast pass on the device (DV_REALIGN_DEVICE_FASTPASS=1: every (window,
haplotype) of the batch in one launch of csrc/fast_pass.hip, no k-mer index on the host) against the host route,
dv_realign_regions: every array of dv_realign_output must be identical, on the golden chr20 regions and on ten NA12878
regions, alone and together with the device trace-back.  The stats keep a run that never reached the device from
passing, and the sweep kernel's own count stays at one launch."""
import contextlib
import ctypes as C
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
SWITCH, TRACEBACK = 'DV_REALIGN_DEVICE_FASTPASS', 'DV_REALIGN_DEVICE_TRACEBACK'


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


@contextlib.contextmanager
def _environment(**values):
  """Sets (a string) or unsets (None) variables the library reads at each call."""
  before = {name: os.environ.get(name) for name in values}
  try:
    for name, value in values.items():
      if value is None:
        os.environ.pop(name, None)
      else:
        os.environ[name] = value
    yield
  finally:
    for name, value in before.items():
      if value is None:
        os.environ.pop(name, None)
      else:
        os.environ[name] = value


def _device_run(ref, tables, regions, fast_pass, traceback=None):
  with _environment(**{SWITCH: fast_pass, TRACEBACK: traceback}):
    job = R.Realigner(R.realigner_config(), ref, device_align=True).start_realign_tables(tables, regions)
    return _output_arrays(job), job


def _same(got, want):
  assert sorted(got) == sorted(want)
  for name in want:
    assert np.array_equal(got[name], want[name]) if isinstance(want[name], np.ndarray) else got[name] == want[name], name


def _compare_routes(ref, tables, regions):
  host = R.Realigner(R.realigner_config(), ref, device_align=False).start_realign_tables(tables, regions)
  want = _output_arrays(host)
  assert host.device_stats is None and host.fast_pass_stats is None
  assert int((want['status'] == 1).sum()) > 0           # reads did move
  seen = {}
  for traceback in (None, '1'):
    got, job = _device_run(ref, tables, regions, '1', traceback)
    _same(got, want)
    fp, sweeps = job.fast_pass_stats, job.device_stats
    assert fp.haplotypes > 0 and fp.haplotypes_on_host == 0 and fp.launches == 1 and fp.pairs > 0 and fp.cells > 0
    assert sweeps.pairs > 0 and sweeps.pairs_on_host == 0 and sweeps.launches == 1      # the sweep kernel's own count
    assert (job.traceback_stats.traced_on_device > 0) == (traceback == '1')
    seen[traceback] = (fp.haplotypes, fp.pairs, fp.cells, sweeps.pairs)
  assert seen[None] == seen['1']
  # unset and 0: the fast pass stays on the host threads, and the pairs it leaves to the sweeps are the same
  for value in (None, '0'):
    got, job = _device_run(ref, tables, regions, value)
    _same(got, want)
    fp = job.fast_pass_stats
    assert (fp.haplotypes, fp.haplotypes_on_host, fp.pairs, fp.cells, fp.launches) == (0, 0, 0, 0, 0)
    assert job.device_stats.launches == 1 and job.device_stats.pairs == seen[None][3]


def test_chr20_golden_regions_every_output_array():
  _compare_routes(*_chr20_batch())


def test_na12878_ten_regions_in_one_batch(tmp_path):
  _compare_routes(*_na12878_batch(tmp_path))


def test_golden_illumina_chain_with_device_fast_pass_in_a_child_process():
  env = dict(os.environ, DV_REALIGN_DEVICE='1', **{SWITCH: '1'})
  done = subprocess.run([sys.executable, '-m', 'tests.realign_device_chain'], cwd=ROOT, env=env, capture_output=True,
                        text=True, timeout=600)
  assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
  assert '84/84' in done.stdout
