"""dv_realign_regions_device with phase 1 wholly on the device (DV_REALIGN_DEVICE_ASSEMBLY=1 and
DV_REALIGN_DEVICE_PATHS=1: graphs, pruning and the haplotypes of every window of the batch from the two launches of
csrc/debruijn.hip, the host threads only compare with the reference) against the host route, dv_realign_regions: every
array of dv_realign_output must be identical, hap_text included, on the golden chr20 regions and on ten NA12878
regions.  With the new switch unset or 0 the route is the one it was: paths_stats all zero, the assembly stats and the
other kernels' counts unchanged; with it on but the assembly switch off nothing changes either.  The stats keep a run
that never reached the device from passing."""
import os
import subprocess
import sys

import pytest

from deepvariant_amd.realigner import realigner as R
from tests import test_hip_realigner_assembly as RA
from tests import test_hip_realigner_fast_pass as FP

pytestmark = pytest.mark.gpu
PATHS = 'DV_REALIGN_DEVICE_PATHS'


def _device_run(ref, tables, regions, assembly, paths, others=None):
  with FP._environment(**{RA.SWITCH: assembly, PATHS: paths, RA.FASTPASS: others, RA.TRACEBACK: others}):   # pylint: disable=protected-access
    job = R.Realigner(R.realigner_config(), ref, device_align=True).start_realign_tables(tables, regions)
    return FP._output_arrays(job), job                                                # pylint: disable=protected-access


def _paths(job):
  p = job.paths_stats
  return (p.windows, p.windows_on_host, p.paths, p.hap_bytes, p.launches, p.bytes_down)


def _compare_routes(ref, tables, regions):
  host = R.Realigner(R.realigner_config(), ref, device_align=False).start_realign_tables(tables, regions)
  want = FP._output_arrays(host)                                                      # pylint: disable=protected-access
  assert host.paths_stats is None
  assert int((want['status'] == 1).sum()) > 0 and len(want['hap_text']) > 0
  for others in (None, '1'):
    # the parent route: the assembly switch alone
    _, parent = RA._device_run(ref, tables, regions, '1', others)                     # pylint: disable=protected-access
    for value in (None, '0'):
      got, job = _device_run(ref, tables, regions, '1', value, others)
      FP._same(got, want)                                                             # pylint: disable=protected-access
      assert _paths(job) == (0,) * 6
      assert RA._assembly(job) == RA._assembly(parent) and RA._counts(job) == RA._counts(parent)   # pylint: disable=protected-access
    got, job = _device_run(ref, tables, regions, '1', '1', others)
    FP._same(got, want)                                                               # pylint: disable=protected-access
    p, a = job.paths_stats, job.assembly_stats
    assert p.windows == a.windows == parent.assembly_stats.windows > 0
    assert p.windows_on_host == 0 and p.launches == 2 and p.paths >= p.windows - 2 and p.hap_bytes > 0 and p.bytes_down > 0
    assert a.windows_rejected == 0 and a.windows_on_host == 0 and a.launches == 1
    assert (a.kmers, a.k_tries) == (parent.assembly_stats.kmers, parent.assembly_stats.k_tries)
    assert RA._counts(job) == RA._counts(parent)                                      # pylint: disable=protected-access
  # the paths switch without the assembly switch: phase 1 stays on the host threads
  _, plain = RA._device_run(ref, tables, regions, None, None)                         # pylint: disable=protected-access
  got, job = _device_run(ref, tables, regions, None, '1')
  FP._same(got, want)                                                                 # pylint: disable=protected-access
  assert _paths(job) == (0,) * 6 and RA._assembly(job) == (0,) * 6                    # pylint: disable=protected-access
  assert RA._counts(job) == RA._counts(plain)                                         # pylint: disable=protected-access


def test_chr20_golden_regions_every_output_array():
  _compare_routes(*FP._chr20_batch())                                                 # pylint: disable=protected-access


def test_na12878_ten_regions_in_one_batch(tmp_path):
  _compare_routes(*FP._na12878_batch(tmp_path))                                       # pylint: disable=protected-access


def test_golden_illumina_chain_with_all_four_switches_in_a_child_process():
  env = dict(os.environ, DV_REALIGN_DEVICE='1', **{RA.SWITCH: '1', PATHS: '1', RA.FASTPASS: '1', RA.TRACEBACK: '1'})
  done = subprocess.run([sys.executable, '-m', 'tests.realign_device_chain'], cwd=RA.ROOT, env=env, capture_output=True,
                        text=True, timeout=600)
  assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
  assert '84/84' in done.stdout
