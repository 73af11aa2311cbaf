"""dv_realign_regions_device with phase 1's graphs on the device (DV_REALIGN_DEVICE_ASSEMBLY=1: every window of the
batch in one launch of csrc/debruijn.hip, the host threads prune and enumerate from the compact graphs) against the
host route, dv_realign_regions: every array of dv_realign_output must be identical, hap_text included, on the golden
chr20 regions and on ten NA12878 regions -- with the switch alone, with the fast-pass and trace-back switches on as
well, and with it unset or 0.  The stats keep a run that never reached the device from passing, and the other
kernels' own counts do not move."""
import os
import subprocess
import sys

import pytest

from deepvariant_amd.realigner import realigner as R
from tests import test_hip_realigner_fast_pass as FP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH, FASTPASS, TRACEBACK = 'DV_REALIGN_DEVICE_ASSEMBLY', 'DV_REALIGN_DEVICE_FASTPASS', 'DV_REALIGN_DEVICE_TRACEBACK'


def _device_run(ref, tables, regions, assembly, others=None):
  with FP._environment(**{SWITCH: assembly, FASTPASS: others, TRACEBACK: others}):    # pylint: disable=protected-access
    job = R.Realigner(R.realigner_config(), ref, device_align=True).start_realign_tables(tables, regions)
    return FP._output_arrays(job), job                                                # pylint: disable=protected-access


def _counts(job):
  fp, sweeps, tb = job.fast_pass_stats, job.device_stats, job.traceback_stats
  return ((fp.haplotypes, fp.haplotypes_on_host, fp.pairs, fp.cells, fp.launches),
          (sweeps.pairs, sweeps.pairs_on_host, sweeps.cells, sweeps.launches),
          (tb.traced_on_device, tb.traced_on_host, tb.band_cells, tb.widest_band))


def _assembly(job):
  a = job.assembly_stats
  return (a.windows, a.windows_on_host, a.kmers, a.k_tries, a.launches, a.windows_rejected)


def _compare_routes(ref, tables, regions):
  host = R.Realigner(R.realigner_config(), ref, device_align=False).start_realign_tables(tables, regions)
  want = FP._output_arrays(host)                                                      # pylint: disable=protected-access
  assert host.assembly_stats is None
  assert int((want['status'] == 1).sum()) > 0 and len(want['hap_text']) > 0
  for others in (None, '1'):
    # the switch unset and 0: today's code path, and what the other kernels then count
    off = {}
    for value in (None, '0'):
      got, job = _device_run(ref, tables, regions, value, others)
      FP._same(got, want)                                                             # pylint: disable=protected-access
      assert _assembly(job) == (0, 0, 0, 0, 0, 0)
      off[value] = _counts(job)
    assert off[None] == off['0']
    got, job = _device_run(ref, tables, regions, '1', others)
    FP._same(got, want)                                                               # pylint: disable=protected-access
    a = job.assembly_stats
    assert a.windows > 0 and a.windows_on_host == 0 and a.windows_rejected == 0 and a.launches == 1
    assert a.kmers > 0 and a.k_tries >= a.windows
    assert _counts(job) == off[None]
    assert (job.fast_pass_stats.launches == 1) == (others == '1')


def test_chr20_golden_regions_every_output_array():
  _compare_routes(*FP._chr20_batch())                                                 # pylint: disable=protected-access


def test_na12878_ten_regions_in_one_batch(tmp_path):
  _compare_routes(*FP._na12878_batch(tmp_path))                                       # pylint: disable=protected-access


def test_golden_illumina_chain_with_all_three_switches_in_a_child_process():
  env = dict(os.environ, DV_REALIGN_DEVICE='1', **{SWITCH: '1', FASTPASS: '1', TRACEBACK: '1'})
  done = subprocess.run([sys.executable, '-m', 'tests.realign_device_chain'], cwd=ROOT, env=env, capture_output=True,
                        text=True, timeout=600)
  assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
  assert '84/84' in done.stdout
