"""dv_realign_regions_device with the banded trace-back on the device (DV_REALIGN_DEVICE_TRACEBACK=1) against the
same call with the trace-back on the host (=0) and against the host route, dv_realign_regions, on the golden
chr20 regions of test_hip_realigner_device.py: every array of dv_realign_output must be identical.

The split between device and host trace-backs is pinned exactly.  The batch's (haplotype, reference) and
(read, haplotype) pairs are rebuilt here from the aligner inputs of every assembled window, as
FastPassAligner::prepare_alignments collects them; their number must be the call's own stats.pairs, and
dv_local_align_band then says for each of them whether the kernel has to trace it back itself.
"""
import ctypes as C
import os

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import dv_types as T
from deepvariant_amd import fast_pass_aligner as F
from deepvariant_amd import packing
from deepvariant_amd.realigner import realigner as R
from deepvariant_amd.realigner import utils as U
from tests import realigner_fixture as RF

pytestmark = pytest.mark.gpu
SWITCH = 'DV_REALIGN_DEVICE_TRACEBACK'
MAX_BAND = _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND
MAX_RUNS = _lib.DV_LOCAL_ALIGN_DEVICE_MAX_RUNS
BUILD_INDEX = 0      # DV_ALIGNER_BUILD_INDEX


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
  per_region = [[r for r, s in zip(reads, spans) if U.ranges_overlap(s, region)] for region in regions]
  tables = [packing.ReadTable.from_reads(rs) for rs in per_region]
  return ref, tables, regions, per_region


def _device_run(ref, tables, regions, traceback):
  before = os.environ.get(SWITCH)
  os.environ[SWITCH] = '1' if traceback else '0'
  try:
    job = R.Realigner(R.realigner_config(), ref, device_align=True).start_realign_tables(tables, regions)
    return _output_arrays(job), job
  finally:
    if before is None:
      del os.environ[SWITCH]
    else:
      os.environ[SWITCH] = before


class _Recorder:
  """Stands in for Realigner._aligner: builds the real aligner and notes what it was given."""

  def __init__(self, realigner, log):
    self._make, self._log = realigner._aligner, log      # pylint: disable=protected-access

  def __call__(self, read_size, force_alignment, prefix_len, suffix_len):
    aligner = self._make(read_size, force_alignment, prefix_len, suffix_len)
    entry = dict(read_size=read_size, prefix_len=prefix_len, suffix_len=suffix_len)
    log = self._log
    set_reference, set_haplotypes, realign_reads = aligner.set_reference, aligner.set_haplotypes, aligner.realign_reads

    def note_reference(reference, ref_start=0):
      entry['reference'], entry['ref_start'] = reference, ref_start
      return set_reference(reference, ref_start)

    def note_haplotypes(haplotypes):
      entry['haplotypes'] = list(haplotypes)
      return set_haplotypes(haplotypes)

    def note_reads(reads):
      entry['sequences'] = [r.aligned_sequence for r in reads]
      log.append(entry)
      return realign_reads(reads)

    aligner.set_reference, aligner.set_haplotypes, aligner.realign_reads = note_reference, note_haplotypes, note_reads
    return aligner


def _batch_pairs(ref, regions, per_region):
  """(reference, query) of every local alignment of the batch: per assembled window the haplotypes that differ
  from the reference against it, then every read the fast pass placed nowhere against every haplotype the fast
  pass gave a score (FastPassAligner::collect_haplotype_pairs / collect_read_pairs, force_alignment off)."""
  windows = []
  rl = R.Realigner(R.realigner_config(), ref)
  make = rl._aligner                                     # pylint: disable=protected-access
  rl._aligner = _Recorder(rl, windows)                   # pylint: disable=protected-access
  for region, reads in zip(regions, per_region):
    rl.realign_reads(reads, region)
  pairs = []
  for w in windows:
    reads = [s.upper() for s in w['sequences']]
    a = make(w['read_size'], False, w['prefix_len'], w['suffix_len'])
    a.set_reference(w['reference'], w['ref_start'])
    a.set_haplotypes(w['haplotypes'])
    a.set_reads(reads)
    a.stage(BUILD_INDEX)
    pairs += [(w['reference'], h) for h in w['haplotypes'] if h != w['reference']]
    targets, placed = [], [False] * len(reads)
    for h in w['haplotypes']:
      score, alignments = a.fast_align_reads_to_haplotype(h)
      if score != 0:
        targets.append(h)
        placed = [p or ra.score > 0 for p, ra in zip(placed, alignments)]
    pairs += [(h, read) for read, p in zip(reads, placed) if not p for h in targets]
  return pairs


def test_traceback_on_off_and_host_route_every_output_array(capsys):
  ref, tables, regions, per_region = _chr20_batch()
  host = R.Realigner(R.realigner_config(), ref, device_align=False).start_realign_tables(tables, regions)
  want = _output_arrays(host)
  assert host.device_stats is None and host.traceback_stats is None
  on, job_on = _device_run(ref, tables, regions, True)
  off, job_off = _device_run(ref, tables, regions, False)
  for got in (on, off):
    assert sorted(got) == sorted(want)
    for name in want:
      assert np.array_equal(got[name], want[name]) if isinstance(want[name], np.ndarray) else got[name] == want[name], name
  assert int((want['status'] == 1).sum()) > 0           # reads did move
  for job in (job_on, job_off):
    assert job.device_stats.pairs > 0 and job.device_stats.pairs_on_host == 0 and job.device_stats.launches == 1

  pairs = _batch_pairs(ref, regions, per_region)
  assert len(pairs) == job_on.device_stats.pairs == job_off.device_stats.pairs      # the batch's own pair list
  scoring = R.realigner_config().aln_config
  shapes = [F.local_align_band(r, q, scoring.match, scoring.mismatch, scoring.gap_open, scoring.gap_extend)
            for r, q in pairs]
  traceable = sum(1 for band, _ in shapes if band > 0)
  predicted = sum(1 for band, runs in shapes if 0 < band <= MAX_BAND and runs <= MAX_RUNS)
  tb_on, tb_off = job_on.traceback_stats, job_off.traceback_stats
  with capsys.disabled():
    print('\n%d pairs, %d hold an alignment; traced on the device %d (%.2f %%), predicted %d; widest band %d'
          % (len(pairs), traceable, tb_on.traced_on_device, 100.0 * tb_on.traced_on_device / max(traceable, 1),
             predicted, tb_on.widest_band))
  assert (tb_off.traced_on_device, tb_off.traced_on_host, tb_off.band_cells, tb_off.widest_band) == (0, traceable, 0, 0)
  assert tb_on.traced_on_device > 0
  assert tb_on.traced_on_device + tb_on.traced_on_host == traceable
  assert tb_on.traced_on_device >= predicted                # the same exact count:
  assert tb_on.traced_on_device == predicted
  assert tb_on.widest_band == max(band for band, runs in shapes if band <= MAX_BAND and runs <= MAX_RUNS)
