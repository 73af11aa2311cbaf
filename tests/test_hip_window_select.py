"""The device window pass (dv_select_windows_batch, deepvariant_amd/csrc/window_select.hip; GPU) against the host
functions of deepvariant_amd/realigner/window_selector.py on separately counted plain counters
(tests/window_select_cases.py): candidate masks, windows, and the float32 scores as bit patterns -- a wrong
summation order changes 42 % of the scores of the fuzz reads and not one window, so windows alone show nothing."""

import numpy as np
import pytest

from deepvariant_amd import allelecounter as A
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from deepvariant_amd.realigner import realigner as R
from deepvariant_amd.realigner import window_selector as ws
from tests import realigner_fixture as RF
from tests import test_hip_candidates as HC
from tests import test_hip_gvcf as HG
from tests import window_select_cases as W
from tests import window_selector_vectors as V
from tests.test_hip_allelecounter import _fuzz_reads

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the reference's vectors

def _vector_counters(cases):
  """One counter per vector, as ws._candidates_from_reads makes it (the region expanded by 20, clipped)."""
  out = []
  for (cfg_name, reads, expected, kw), min_mapq in cases:
    config = V.linear_config() if cfg_name == 'linear' else V.threshold_config()
    if min_mapq is not None:
      config.min_mapq = min_mapq
    start, end = kw.get('start', 0), kw.get('end', 20)
    made = [V.mk(*r) for r in reads]
    chrom = made[0].alignment.position.reference_name
    ref = RF.StringRef(chrom, kw.get('ref') or 'A' * (end - start + 512))
    counter, _ = ws._make_counter(config, ref, made, T.Range(chrom, start, end))   # pylint: disable=protected-access
    out.append(counter)
  return out


@pytest.mark.parametrize('cfg_name', ['linear', 'threshold'])
def test_reference_vectors(cfg_name):
  cases = [(c, None) for c in V.CASES if c[0] == cfg_name]
  if cfg_name == 'threshold':                       # the mapq sweep of test_window_selector_vectors_device_counts
    for read_mapq in range(10, 15):
      for min_mapq in range(8, 17):
        cases.append((('threshold', [('AGA', 10, '3M', None, read_mapq)], [11] if read_mapq >= min_mapq else [], {}),
                      min_mapq))
  config = V.linear_config() if cfg_name == 'linear' else V.threshold_config()
  counters = _vector_counters(cases)
  A.AlleleCounter.run_batch(counters, windows=config, window_debug=True)
  for (case, _), counter in zip(cases, counters):
    _, _, mask, _ = counter.windows(config, want_debug=True)
    got = [counter.interval_start() + int(p) for p in np.nonzero(mask)[0]]
    assert got == case[2], (case, got)
  W.check(lambda: _vector_counters(cases), config)


# ---------------------------------------------------------------- 2. fuzz

_FUZZ_REGIONS = (((1000, 2000), (700, 2100)), ((0, 400), (0, 420)), ((5600, 6000), (5300, 5990)))


def _fuzz_makers(seed, long_reads, track):
  """test_hip_candidates.py::test_fuzz's reference, regions and reads -> make() for the three counters."""
  rng = np.random.default_rng(seed)
  seq = ''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=6000))
  ref = HC._SeqRef(seq)                                                 # pylint: disable=protected-access
  read_sets = []
  for _, (lo, hi) in _FUZZ_REGIONS:
    reads = _fuzz_reads(rng, ref, 700 if not long_reads else 200, lo, hi, long_reads)
    read_sets.append(reads + reads[:40])

  def make():
    out = []
    for ((start, end), _), reads in zip(_FUZZ_REGIONS, read_sets):
      # with `track`, REFERENCE events at every seventh position take part in the linear model
      c = A.AlleleCounter(ref, 'c', start, end, candidate_positions=range(start, end, 7) if track else (),
                          min_mapping_quality=10, min_base_quality=20, track_ref_reads=track)
      for r in reads:
        c.add(r)
      out.append(c)
    return out
  return make


@pytest.mark.parametrize('seed,long_reads,track', [(31, False, False), (32, True, False), (33, False, True)])
def test_fuzz(seed, long_reads, track):
  make = _fuzz_makers(seed, long_reads, track)
  for distance in (0, 4, 80):
    configs = [W.linear_config(distance), W.threshold_config(distance), W.threshold_config(distance, strict=True)]
    for config in configs:
      want = W.check(make, config)
      for k, (mask, windows, _) in enumerate(want):
        assert mask.any() and windows, (k, config)                      # every (region, model) selects something
        if distance == 0:
          assert len(windows) == int(mask.sum())


# ---------------------------------------------------------------- 3. the float32 order decides

def test_float32_summation_order_decides():
  """The boundary is put on a host score that an order-free sum misses by one float32 step: a kernel that sums in
  another order selects a different set there."""
  make = _fuzz_makers(31, False, False)
  plain = make()[0]
  model = W.linear_config().window_selector_model.allele_count_linear_model
  want = ws.allele_count_linear_candidates_from_allele_counter(plain, model)
  alt = W.order_free_scores(plain, model)
  differ = want.view(np.uint32) != alt.view(np.uint32)
  print('order-free sum differs in bits at %d of %d positions' % (int(differ.sum()), len(want)))
  assert differ.any()
  above, below = np.nonzero(alt > want)[0], np.nonzero(alt < want)[0]
  assert len(above) and len(below)
  j = int(above[0])
  config = W.linear_config(4, decision_boundary=float(want[j]))         # the host leaves j out; alt[j] is past it
  mask = W.check(lambda: [make()[0]], config)[0][0]
  assert not mask[j] and float(alt[j]) > config.window_selector_model.allele_count_linear_model.decision_boundary
  j = int(below[0])
  boundary = float(np.nextafter(want[j], np.float32(-np.inf)))         # just below want[j]: the host takes j
  config = W.linear_config(4, decision_boundary=boundary)
  mask = W.check(lambda: [make()[0]], config)[0][0]
  assert mask[j] and not float(alt[j]) > boundary


# ---------------------------------------------------------------- 4. the allele filter's edges

def _piles(n_ref):
  reads = [('AAAAT', 10, '4M1I')] + [('AAAA', 10, '4M')] * n_ref
  return lambda: _vector_counters([(('threshold', reads, None, {}), None)])


@pytest.mark.parametrize('n_ref,kept', [(12, False), (11, True)])
def test_strict_insertion_filter_edge(n_ref, kept):
  """1 of 13 reads = 7.7 % is dropped, 1 of 12 = 8.3 % is kept (tests/test_window_selector_cpu.py)."""
  config = V.threshold_config()
  config.window_selector_model.variant_reads_model.max_num_supporting_reads = 100
  off = W.check(_piles(n_ref), config)[0]
  assert [int(p) for p in np.nonzero(off[0])[0]] == [13, 14]
  config.enable_strict_insertion_filter = True
  on = W.check(_piles(n_ref), config)[0]
  assert [int(p) for p in np.nonzero(on[0])[0]] == ([13, 14] if kept else [])


@pytest.mark.parametrize('n_reads,expected', [(1, []), (2, [12])])
def test_min_allele_support(n_reads, expected):
  config = V.threshold_config()
  config.min_allele_support = 2
  make = lambda: _vector_counters([(('threshold', [('AAGA', 10, '4M')] * n_reads, None, {}), None)])   # noqa: E731
  mask = W.check(make, config)[0][0]
  assert [int(p) for p in np.nonzero(mask)[0]] == expected


# ---------------------------------------------------------------- 5. real reads

def _na12878_tables(tmp_path):
  bam, ref = HG._bam_fixture(tmp_path)                                  # pylint: disable=protected-access
  lo, hi = ref.offset, ref.offset + len(ref.seq)
  table = packing.ReadTable.from_bam(bam, 'chr20', lo, hi, min_mapping_quality=5, keep_supplementary=True)
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  regions = [T.Range('chr20', s, min(s + 1000, hi)) for s in range(lo, hi, 1000)]
  tables = [table.take(np.nonzero((ends > r.start) & (starts < r.end))[0]) for r in regions]
  return ref, tables, regions


def _both_routes(monkeypatch, config, ref, tables, regions):
  monkeypatch.delenv('DV_WINDOWS_DEVICE', raising=False)
  want = ws.select_windows_of_tables(config, ref, tables, regions)
  monkeypatch.setenv('DV_WINDOWS_DEVICE', '1')
  got = ws.select_windows_of_tables(config, ref, tables, regions)
  monkeypatch.delenv('DV_WINDOWS_DEVICE', raising=False)
  assert got == want
  return want


@pytest.mark.parametrize('use_model', [True, False])
def test_na12878_100kb_every_region_in_one_batch(tmp_path, monkeypatch, use_model):
  ref, tables, regions = _na12878_tables(tmp_path)
  assert len(regions) >= 100
  config = R.realigner_config(ws_use_window_selector_model=use_model).ws_config
  want = _both_routes(monkeypatch, config, ref, tables, regions)
  with_windows = sum(1 for w in want if w)
  print('NA12878 100 kb: %d windows in %d of %d regions' % (sum(len(w) for w in want), with_windows, len(regions)))
  assert with_windows * 10 >= len(regions)


def _chr20_batch():
  from deepvariant_amd.realigner import utils as U
  ref, sets = RF.load()
  reads = sets['wgs']
  spans = [U.read_range(r) for r in reads]
  regions = [T.Range('chr20', s, min(s + 1000, 10_010_000)) for s in range(9_999_999, 10_010_000, 1000)]
  tables = [packing.ReadTable.from_reads([r for r, s in zip(reads, spans) if U.ranges_overlap(s, region)])
            for region in regions]
  return ref, tables, regions


@pytest.mark.parametrize('use_model', [True, False])
def test_golden_illumina_read_table(monkeypatch, use_model):
  ref, tables, regions = _chr20_batch()
  config = R.realigner_config(ws_use_window_selector_model=use_model).ws_config
  want = _both_routes(monkeypatch, config, ref, tables, regions)
  assert sum(1 for w in want if w) >= 1


# ---------------------------------------------------------------- 6. edges of the batch machinery

def test_readless_region_in_a_batch_and_a_counter_that_has_run():
  ref, reads = HC._synthetic_with_candidates()                          # pylint: disable=protected-access
  spans = [(1000, 1200), (2500, 2600), (1200, 1450), (1450, 1800)]      # the second has no reads

  def make():
    out = []
    for s, e in spans:
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    out[2].counts()                                                     # has already run
    return out
  for config in (W.linear_config(4), W.threshold_config(4)):
    want = W.check(make, config)
    assert not want[1][1] and any(w[1] for w in want)
    alone = [W.device_answer(config, make()[k])[1] for k in range(len(spans))]   # the one-region form of the pass
    assert alone == [w[1] for w in want]


def test_events_beyond_the_first_guess():
  """A region whose events overflow the batch's first guess goes alone afterwards, next to an ordinary one."""
  ref = HC._corner_ref()                                                # pylint: disable=protected-access
  noisy, quiet = HC._noisy_reads(ref), HC._quiet_reads(ref)             # pylint: disable=protected-access

  def make():
    out = []
    for (s, e), reads in (((1990, 2070), quiet), ((1000, 1400), noisy), ((1990, 2070), quiet)):
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    return out
  plain = make()[1]
  assert len(plain.counts()) and len(plain._events) > 300 + 300 * 100 // 16 + 4096    # pylint: disable=protected-access
  for config in (W.linear_config(4, decision_boundary=-30.0), W.threshold_config(4, lo=1, hi=1000)):
    want = W.check(make, config)
    assert want[1][0].any() and want[0][1] == want[2][1]


def _long_region_counter(ref, start, end, rng_seed=3):
  """10x of reference reads, a third with one substitution, and every 300 bases four reads with a two-base
  insertion and three with a substitution."""
  rng = np.random.default_rng(rng_seed)
  reads = []
  for i in range(400):
    at = int(rng.integers(max(start - 40, 0), end - 20))
    seq = list(ref.seq[at:at + 60])
    if i % 3 == 0 and len(seq) > 30:
      seq[30] = HC._other(seq[30])                                      # pylint: disable=protected-access
    reads.append(HG._read('l%d' % i, 1, at, ''.join(seq), [(len(seq), 'M')]))      # pylint: disable=protected-access
  for locus in range(start + 100, end - 100, 300):
    reads += HC._indel_reads(ref, 'ins%d' % locus, 4, locus, inserted='TT', start=locus - 25)    # pylint: disable=protected-access
    reads += HC._pile(ref, 'sub%d' % locus, 3, start=locus + 90, edit=HC._sub_at(locus + 120, locus + 90))   # pylint: disable=protected-access
  c = A.AlleleCounter(ref, 'c', start, end, min_mapping_quality=10, min_base_quality=10)
  for r in reads:
    c.add(r)
  return c


def test_region_past_one_scan_chunk():
  """2,500 positions: ten rounds of the 256-lane scan, windows carried from round to round."""
  ref = HC._corner_ref()                                                # pylint: disable=protected-access
  for config in (W.linear_config(0), W.linear_config(4), W.threshold_config(4, lo=1), W.threshold_config(80, lo=1)):
    want = W.check(lambda: [_long_region_counter(ref, 300, 2800)], config)
    assert len(want[0][1]) >= (3 if config.min_windows_distance < 80 else 1)


def test_three_hundred_tiny_regions():
  ref = HC._corner_ref()                                                # pylint: disable=protected-access
  reads = HC._quiet_reads(ref, 2000) + HC._quiet_reads(ref, 2100)       # pylint: disable=protected-access

  def make():
    out = []
    for k in range(300):
      s = 1990 + (k % 40) * 5
      c = A.AlleleCounter(ref, 'c', s, s + 1 + k % 7, min_mapping_quality=10, min_base_quality=10)
      c.add_table(table)
      out.append(c)
    return out
  table = packing.ReadTable.from_reads(reads)
  want = W.check(make, W.threshold_config(0, lo=1))
  assert sum(len(w[1]) for w in want) >= 5


def test_windows_reach_below_zero_and_past_the_contig():
  """Windows are not clamped: [first - d, last + d) with d = 80 around candidates at the contig's two ends."""
  ref = HC._corner_ref()                                                # pylint: disable=protected-access
  n = len(ref.seq)
  reads = HC._pile(ref, 'lo', 4, start=0, edit=HC._sub_at(5, 0)) + \
      HC._pile(ref, 'hi', 4, start=n - 60, edit=HC._sub_at(n - 5, n - 60))   # pylint: disable=protected-access

  def make():
    out = []
    for s, e in ((0, 300), (n - 300, n)):
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    return out
  want = W.check(make, W.threshold_config(80, lo=1))
  assert want[0][1] == [(5 - 80, 5 + 80)] and want[1][1] == [(n - 5 - 80, n - 5 + 80)]


# ---------------------------------------------------------------- 7. the route

def _same_results(a, b):
  assert len(a) == len(b)
  for (ch_a, t_a), (ch_b, t_b) in zip(a, b):
    assert [(c.span, c.haplotypes) for c in ch_a] == [(c.span, c.haplotypes) for c in ch_b]
    assert np.array_equal(t_a.read_pos, t_b.read_pos) and np.array_equal(t_a.cigar, t_b.cigar)
    assert np.array_equal(t_a.bases, t_b.bases)


@pytest.mark.parametrize('device_align', [False, True])
def test_realign_tables_with_and_without_the_switch(monkeypatch, device_align):
  """DV_WINDOWS_DEVICE=1 alone and together with the device aligner (what DV_REALIGN_DEVICE=1 turns on)."""
  ref, tables, regions = _chr20_batch()
  monkeypatch.delenv('DV_WINDOWS_DEVICE', raising=False)
  want = R.Realigner(R.realigner_config(), ref, device_align=device_align).realign_tables(tables, regions)
  monkeypatch.setenv('DV_WINDOWS_DEVICE', '1')
  got = R.Realigner(R.realigner_config(), ref, device_align=device_align).realign_tables(tables, regions)
  _same_results(want, got)
  assert sum(len(ch) for ch, _ in want) > 0
