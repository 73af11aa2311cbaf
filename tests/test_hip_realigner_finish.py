"""dv_realign_regions_device with the alignments finished on the device (DV_REALIGN_DEVICE_FINISH=1 together with
DV_REALIGN_DEVICE_TRACEBACK=1: the sweep launch's result stays there and the kernels of csrc/realign_finish.hip pick
the haplotype and merge the CIGARs of every read) against the host route, dv_realign_regions: every array of
dv_realign_output must be identical on the golden chr20 regions and on ten NA12878 regions, with the switch unset, 0
and 1.  Without the switch, and without the trace-back switch, the stats are zero and the other kernels' counts are
what they were."""
import dataclasses

import numpy as np
import pytest

from deepvariant_amd import packing
from deepvariant_amd.realigner import realigner as R
from tests import test_hip_realigner_assembly as RA
from tests import test_hip_realigner_fast_pass as FP

pytestmark = pytest.mark.gpu
FINISH, PATHS = 'DV_REALIGN_DEVICE_FINISH', 'DV_REALIGN_DEVICE_PATHS'


def _device_run(ref, tables, regions, finish, traceback, others=None):
  with FP._environment(**{FINISH: finish, RA.TRACEBACK: traceback, RA.FASTPASS: others, RA.SWITCH: others,   # pylint: disable=protected-access
                          PATHS: others}):
    job = R.Realigner(R.realigner_config(), ref, device_align=True).start_realign_tables(tables, regions)
    return FP._output_arrays(job), job                                                # pylint: disable=protected-access


def _finish(job):
  s = job.finish_stats
  return (s.windows, s.windows_on_host, s.reads, s.cigar_words, s.launches, s.bytes_down)


def _sweeps(job):
  s, t = job.device_stats, job.traceback_stats
  return (s.pairs, s.pairs_on_host, s.cells, s.launches, t.traced_on_device, t.traced_on_host, t.band_cells, t.widest_band)


def _compare_routes(ref, tables, regions):
  host = R.Realigner(R.realigner_config(), ref, device_align=False).start_realign_tables(tables, regions)
  want = FP._output_arrays(host)                                                      # pylint: disable=protected-access
  assert host.finish_stats is None
  assert int((want['status'] == 1).sum()) > 0
  for others in (None, '1'):
    _, parent = _device_run(ref, tables, regions, None, '1', others)
    for value in (None, '0'):
      got, job = _device_run(ref, tables, regions, value, '1', others)
      FP._same(got, want)                                                             # pylint: disable=protected-access
      assert _finish(job) == (0,) * 6 and _sweeps(job) == _sweeps(parent)
    got, job = _device_run(ref, tables, regions, '1', '1', others)
    FP._same(got, want)                                                               # pylint: disable=protected-access
    s = job.finish_stats
    assert s.windows > 0 and 0 <= s.windows_on_host < s.windows and s.reads > 0 and s.launches == 4
    assert s.cigar_words > 0
    if s.windows_on_host == 0:                       # every word of the result came from the kernels
      assert s.cigar_words == len(want['cigar'])
    # 8 words per pair instead of 72; the finish step's own download: header, 16 + 4 bytes per read, and 4 words per
    # read or, where there are more, every word (each section padded to 16 bytes)
    assert 0 < s.bytes_down <= job.device_stats.pairs * 8 * 4 + 16 + 20 * s.reads + 4 * max(4 * s.reads, s.cigar_words) + 48
    assert _sweeps(job) == _sweeps(parent)
    # the switch without the trace-back switch is ignored
    for traceback in (None, '0'):
      got, job = _device_run(ref, tables, regions, '1', traceback, others)
      FP._same(got, want)                                                             # pylint: disable=protected-access
      assert _finish(job) == (0,) * 6 and job.traceback_stats.traced_on_device == 0


def test_chr20_golden_regions_every_output_array():
  _compare_routes(*FP._chr20_batch())                                                 # pylint: disable=protected-access


def test_na12878_ten_regions_in_one_batch(tmp_path):
  _compare_routes(*FP._na12878_batch(tmp_path))                                       # pylint: disable=protected-access


def test_realign_tables_with_all_five_switches(tmp_path):
  ref, tables, regions = FP._na12878_batch(tmp_path)                                  # pylint: disable=protected-access
  want = R.Realigner(R.realigner_config(), ref, device_align=False).realign_tables(tables, regions)
  with FP._environment(**{FINISH: '1', RA.TRACEBACK: '1', RA.FASTPASS: '1', RA.SWITCH: '1', PATHS: '1'}):   # pylint: disable=protected-access
    job = R.Realigner(R.realigner_config(), ref, device_align=True).start_realign_tables(tables, regions)
    got = job.result()
  assert job.finish_stats.windows > 0 and job.finish_stats.launches == 4
  assert len(got) == len(want)
  for a, b in zip(want, got):
    assert a[0] == b[0]
    for f in dataclasses.fields(packing.ReadTable):
      x, y = getattr(a[1], f.name), getattr(b[1], f.name)
      assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, f.name
