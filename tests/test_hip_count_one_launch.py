"""DV_COUNT_ONE_LAUNCH=1 (count_alleles_batch_kernel, deepvariant_amd/csrc/allele_counter.hip; GPU): every batch entry
point counts its batched regions in ONE launch, and nothing it returns differs from the launch-per-region route in
the same process -- nor, where stated, from each region counted alone by dv_count_alleles.  Every comparison is an
equality: reference counts, counted reads, the sorted events as bytes, sites, alleles, event words, gVCF blocks,
windows, and the window scores as uint32 bit patterns.  dv_count_batch_last_stats says which way a call went."""
import ctypes as C

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import allelecounter as A
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from deepvariant_amd import variant_calling as vc
from deepvariant_amd.realigner import realigner as R
from oracle import allelecounter_ref as REF
from tests import allelecounter_vectors as V
from tests import batch_edge_cases as E
from tests import count_launch_cases as L
from tests import test_hip_allelecounter as HA
from tests import test_hip_candidates as HC
from tests import test_hip_gvcf as HG
from tests import test_hip_window_select as HW
from tests import window_select_cases as W

pytestmark = pytest.mark.gpu
SWITCH = 'DV_COUNT_ONE_LAUNCH'
GVCF = vc.GvcfOptions('s', include_med_dp=True)


def _switch(monkeypatch, on):
  if on:
    monkeypatch.setenv(SWITCH, '1')
  else:
    monkeypatch.delenv(SWITCH, raising=False)


def _run(monkeypatch, on, counters, **kwargs):
  """One run_batch with the switch on or off -> its stats."""
  _switch(monkeypatch, on)
  A.AlleleCounter.run_batch(counters, **kwargs)
  stats = A.last_batch_stats()
  _switch(monkeypatch, False)
  return stats


def _same_counts(a, b):
  assert np.array_equal(a.ref_supporting_read_counts(), b.ref_supporting_read_counts())
  assert a.n_counted_reads() == b.n_counted_reads()
  assert a._events.dtype == b._events.dtype and a._events.tobytes() == b._events.tobytes()   # pylint: disable=protected-access


def _same_passes(a, b, call=False, gvcf=False):
  if call:
    assert a._cand is not None and b._cand is not None               # pylint: disable=protected-access
    for x, y in zip(a._cand[1:], b._cand[1:]):                        # sites, alleles, event words   pylint: disable=protected-access
      assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
  if gvcf:
    assert a.gvcf_block_array(GVCF).tobytes() == b.gvcf_block_array(GVCF).tobytes()


# ---------------------------------------------------------------- 1. the block mapping

@pytest.mark.parametrize('track', [False, True])
@pytest.mark.parametrize('make', [L.block_edge_batch, L.special_batch])
def test_block_edges(monkeypatch, make, track):
  """Switch on == switch off == every region counted alone, and the stats name the route.  (Fails before the
  switch existed: there is no last_batch_stats.)"""
  case = make()
  slots = L.batched_regions(case)
  off, on = L.counters(case, track), L.counters(case, track)
  stats_off = _run(monkeypatch, False, off)
  stats_on = _run(monkeypatch, True, on)
  n = len(case.spans)
  assert stats_on == A.BatchStats(n, len(slots), 0, 1, case.total_blocks)
  assert stats_off == A.BatchStats(n, len(slots), 0, len(slots), case.total_blocks)
  for k in range(n):
    alone = L.counters(case, track, only=k)[0]
    alone.counts()                                                    # dv_count_alleles
    _same_counts(on[k], off[k])
    _same_counts(on[k], alone)
    if k in slots:                                                    # something to get wrong in every region
      assert len(on[k]._events) and on[k].ref_supporting_read_counts().any()      # pylint: disable=protected-access
  if track:
    positions = L.candidate_positions(case)
    for k in slots:
      kinds = (on[k]._events['length_type'] >> 28) & 7                # pylint: disable=protected-access
      assert bool((kinds == A.REFERENCE).any()) == bool(positions[k])
  if case.name == 'special':
    assert len(on[2]._events) > L.BLOCK_EVENTS                        # pylint: disable=protected-access
    assert on[3].n_counted_reads() < len(case.reads[3])               # the legacy region's own mapping quality bar
    assert on[0].n_counted_reads() == len(case.reads[0])
    assert on[1].ref_supporting_read_counts()[L.WINDOW + 100:].any()  # counted past the LDS window


def test_reference_vectors_in_one_launch(monkeypatch):
  """The reference's own vectors (deepvariant/allelecounter_test.cc), each a region of one batch."""
  cases = V.cases()
  counters, oracles = [], []
  for _, contig, start, end, reads, _ in cases:
    counter = A.AlleleCounter(V.TestRef(), contig, start, end, min_base_quality=V.MIN_BQ)
    oracle = REF.AlleleCounter(V.TestRef(), contig, start, end, min_base_quality=V.MIN_BQ)
    for r in reads:
      counter.add(r)
      oracle.add(r)
    counters.append(counter)
    oracles.append(oracle)
  stats = _run(monkeypatch, True, counters)
  assert stats.count_launches == 1 and stats.regions_batched == sum(1 for c in cases if c[4] and c[3] > c[2])
  for (name, _, _, _, reads, expected), counter, oracle in zip(cases, counters, oracles):
    assert counter.n_counted_reads() == len(reads)
    for i, (ac, want) in enumerate(zip(counter.counts(), expected)):
      assert sorted((a.bases, a.type, a.count) for a in A.sum_allele_counts(ac)) == sorted(want), (name, i)
    HA._compare(counter.counts(), oracle)                             # pylint: disable=protected-access


# ---------------------------------------------------------------- 2. past 256 regions

@pytest.mark.parametrize('n,overflow_at', L.MANY_REGIONS)
def test_past_256_regions(monkeypatch, n, overflow_at):
  case = L.many_regions(n, overflow_at)
  caller = HC._caller()                                               # pylint: disable=protected-access
  tracked = [tuple(range(s, e, 7)) for s, e in case.spans]
  ways = [dict(call=caller.candidate_options()), dict(call=caller.candidate_options(), track=True), dict(gvcf=GVCF),
          dict(gvcf=GVCF, call=caller.candidate_options())]
  for way in ways:
    track = way.pop('track', False)
    off = E.counters(case, tracked if track else None, track)
    on = E.counters(case, tracked if track else None, track)
    stats_off = _run(monkeypatch, False, off, **way)
    stats_on = _run(monkeypatch, True, on, **way)
    alone = 0 if overflow_at is None else 1
    blocks = sum(-(-len(rs) // 64) for rs in case.reads)
    assert stats_on == A.BatchStats(len(case.spans), n, alone, 1, blocks)
    assert stats_off == A.BatchStats(len(case.spans), n, alone, n, blocks)
    for a, b in zip(on, off):
      _same_counts(a, b)
      _same_passes(a, b, call='call' in way, gvcf='gvcf' in way)
    if overflow_at is not None:
      k = E.region_of_slot(case, overflow_at)
      assert case.kinds[k] == 'noisy' and len(on[k]._events) > 300 + 300 * 100 // 16 + 4096   # pylint: disable=protected-access


# ---------------------------------------------------------------- 3. the window pass

@pytest.mark.parametrize('seed,long_reads,track', [(31, False, False), (32, True, False), (33, False, True)])
def test_window_pass(monkeypatch, seed, long_reads, track):
  make = HW._fuzz_makers(seed, long_reads, track)                     # pylint: disable=protected-access
  for distance in (0, 80):
    for config in (W.linear_config(distance), W.threshold_config(distance)):
      off, on = make(), make()
      _run(monkeypatch, False, off, windows=config, window_debug=True)
      stats = _run(monkeypatch, True, on, windows=config, window_debug=True)
      assert stats == A.BatchStats(3, 3, 0, 1, sum(-(-len(c._reads) // 64) for c in on))   # pylint: disable=protected-access
      for a, b in zip(on, off):
        got, want = a.windows(config, want_debug=True), b.windows(config, want_debug=True)
        assert len(want[0]) and want[3].dtype == np.uint32
        for x, y in zip(got, want):                                   # starts, ends, mask, score bit patterns
          assert x.dtype == y.dtype and np.array_equal(x, y)


# ---------------------------------------------------------------- 4. real reads: NA12878, 102 regions

def test_na12878_run_batch(tmp_path, monkeypatch):
  make = HC._na12878_counters(tmp_path)                               # pylint: disable=protected-access
  off, on = make(None), make(None)
  stats_off = _run(monkeypatch, False, off)
  stats_on = _run(monkeypatch, True, on)
  assert stats_on.regions >= 100 and stats_on.count_launches == 1 and stats_off.count_launches == stats_off.regions_batched
  assert stats_on.count_workgroups == stats_off.count_workgroups > stats_on.regions_batched
  for a, b in zip(on, off):
    _same_counts(a, b)


@pytest.mark.parametrize('track', [False, True])
def test_na12878_process_tables(tmp_path, monkeypatch, track):
  from deepvariant_amd import make_examples_core as mec
  from tests.golden.make_golden import wgs_options
  bam, ref = HG._bam_fixture(tmp_path)                                # pylint: disable=protected-access
  regions = list(mec.partition(T.Range('chr20', ref.offset, ref.offset + len(ref.seq)), 1000))
  table = packing.ReadTable.from_bam(bam, 'chr20', regions[0].start, regions[-1].end, min_mapping_quality=5)
  options = T.MakeExamplesOptions(pic_options=wgs_options(),
                                  sample_options=[T.SampleOptions(role='main', name='NA12878', pileup_height=100)])
  ends = table.read_end.astype(np.int64)
  tables = [table.take(np.nonzero((ends > r.start) & (table.read_pos.astype(np.int64) < r.end))[0]) for r in regions]
  po = mec.RegionProcessorOptions(realigner_enabled=False, track_ref_reads=track, gvcf=not track)

  def run(on):
    _switch(monkeypatch, on)
    proc = mec.RegionProcessor(options, ref, po)
    calls = [calls for calls, _ in proc.process_tables(regions, tables)]
    stats = A.last_batch_stats()
    _switch(monkeypatch, False)
    return calls, proc.gvcf_records, stats
  want, want_records, stats_off = run(False)
  got, got_records, stats_on = run(True)
  assert got == want and got_records == want_records and bool(want_records) == (not track)
  assert sum(map(len, want)) >= HC.NA12878_HOST_CALLS // 2
  assert stats_on.count_launches == 1 and stats_off.count_launches == stats_off.regions_batched > 1


def test_na12878_realign_tables(tmp_path, monkeypatch):
  ref, tables, regions = HW._na12878_tables(tmp_path)                 # pylint: disable=protected-access
  monkeypatch.setenv('DV_WINDOWS_DEVICE', '1')

  def run(on):
    _switch(monkeypatch, on)
    out = R.Realigner(R.realigner_config(), ref).realign_tables(tables, regions)
    _switch(monkeypatch, False)
    return out
  want, got = run(False), run(True)
  HW._same_results(want, got)                                         # pylint: disable=protected-access
  assert sum(len(ch) for ch, _ in want) > 0


# ---------------------------------------------------------------- 5. mixed and repeated batches

def _on_device(counter):
  """Makes the counter hand over its read table in device memory: plan_batch gives it no slot."""
  import torch
  host_request = counter._request                                     # pylint: disable=protected-access

  def request():
    b, opt, keep, ctx = host_request()
    tensors = []
    for name, dtype in (('read_pos', np.int32), ('read_seq_off', np.uint32), ('read_cigar_off', np.uint32),
                        ('read_mapq', np.uint8), ('bases', np.uint8), ('quals', np.uint8), ('cigar', np.uint32)):
      host = np.ascontiguousarray(getattr(ctx[0], name), dtype).view(np.uint8)
      tensors.append(torch.from_numpy(host.copy()).cuda())
      setattr(b, name, tensors[-1].data_ptr())
    torch.cuda.synchronize()
    b.memory = _lib.DV_MEM_DEVICE
    return b, opt, (keep, tensors), ctx
  counter._request = request                                          # pylint: disable=protected-access


def test_device_resident_table_and_a_counter_that_has_run(monkeypatch):
  """Region 0's table is device-resident (it goes alone), no read reaches region 1's interval, region 2 has already
  counted (it is counted again): the batched regions take slots 0 to 2 while they are regions 1 to 3."""
  ref, reads = HC._synthetic_with_candidates()                        # pylint: disable=protected-access
  spans = [(1000, 1200), (2500, 2600), (1200, 1450), (1450, 1800)]
  caller = HC._caller()                                               # pylint: disable=protected-access

  def make():
    out = []
    for s, e in spans:
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    _on_device(out[0])
    out[2].counts()
    return out
  off, on = make(), make()
  stats_off = _run(monkeypatch, False, off, call=caller.candidate_options())
  stats_on = _run(monkeypatch, True, on, call=caller.candidate_options())
  assert (stats_on.regions, stats_on.regions_batched, stats_on.regions_alone, stats_on.count_launches) == (4, 3, 1, 1)
  assert (stats_off.regions_batched, stats_off.regions_alone, stats_off.count_launches) == (3, 1, 3)
  for a, b in zip(on, off):
    _same_counts(a, b)
    _same_passes(a, b, call=True)
  assert {1070, 1220, 1620} <= {c.variant.start for k in range(4) for c in caller.calls_from_allele_counter(on[k])}


def test_one_slot(monkeypatch):
  case = L.block_edge_batch()
  pair = lambda: L.counters(case)[2:4]                                # the read-less region and the 64-read region
  off, on = pair(), pair()
  _run(monkeypatch, False, off)
  assert _run(monkeypatch, True, on) == A.BatchStats(2, 1, 0, 1, 1)
  for a, b in zip(on, off):
    _same_counts(a, b)
  assert on[0].n_counted_reads() == 0 and on[1].n_counted_reads() == 64


def test_a_small_batch_after_a_large_one(monkeypatch):
  """300 regions, then three: the thread's staging buffers are reused, and the second batch's table and prefix lie
  where the first one's reads lay."""
  many, few = L.many_regions(300), L.block_edge_batch()
  caller = HC._caller()                                               # pylint: disable=protected-access
  off_many, on_many = E.counters(many), E.counters(many)
  off_few, on_few = L.counters(few)[3:6], L.counters(few)[3:6]
  _run(monkeypatch, False, off_many, call=caller.candidate_options())
  _run(monkeypatch, False, off_few)
  assert _run(monkeypatch, True, on_many, call=caller.candidate_options()).count_launches == 1
  assert _run(monkeypatch, True, on_few) == A.BatchStats(3, 3, 0, 1, 1 + 2 + 2)
  for a, b in zip(on_many, off_many):
    _same_counts(a, b)
    _same_passes(a, b, call=True)
  for a, b in zip(on_few, off_few):
    _same_counts(a, b)


# ---------------------------------------------------------------- 6. the error that comes from the counters

def test_reference_window_too_small(monkeypatch):
  """A deletion anchored inside the interval whose bases lie past the end of the reference window handed over: the
  kernels report it in a counter and the call returns DV_ERR_BAD_INPUT, on either route."""
  ref = HC._corner_ref()                                              # pylint: disable=protected-access
  spans = [(1990, 2070), (1000, 1100), (2100, 2180)]
  sets = [HC._quiet_reads(ref), HC._pile(ref, 'ref', 6) + HC._indel_reads(ref, 'del', 3, 1095, deleted=20, start=1060),   # pylint: disable=protected-access
          HC._quiet_reads(ref, 2110)]                                 # pylint: disable=protected-access

  def make():
    out = []
    for (s, e), reads in zip(spans, sets):
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    host_request = out[1]._request                                    # pylint: disable=protected-access

    def request():                                                    # the window without the deletion's margin
      b, opt, keep, ctx = host_request()
      opt.n_ref_bases = opt.reads_interval_end - opt.ref_start
      return b, opt, keep, ctx
    out[1]._request = request                                         # pylint: disable=protected-access
    return out
  for on in (False, True):
    _switch(monkeypatch, on)
    with pytest.raises(_lib.DvError) as err:
      A.AlleleCounter.run_batch(make())
    assert err.value.status == _lib.DV_ERR_BAD_INPUT and 'outside the reference window' in str(err.value)
    stats = _lib.DvCountBatchStats()
    assert _lib.lib().dv_count_batch_last_stats(C.byref(stats)) == _lib.DV_OK
    assert stats.count_launches == (1 if on else 3)
  _switch(monkeypatch, False)
