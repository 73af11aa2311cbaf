"""The device candidate caller (dv_call_candidates_batch, deepvariant_amd/csrc/candidates.hip; GPU)
against the host restatement variant_calling.VariantCaller.calls_from_allele_counts(counter.counts()):
the un-narrowed walk over every position's Python AlleleCount, which shares nothing with the device
route but the counter's events.  Every comparison is == on the DeepVariantCall dataclasses: variant,
info DP / AD / VAF, allele_support, allele_support_ext, ref_support, ref_support_ext and the orders
of their lists."""
import os

import numpy as np
import pytest

from deepvariant_amd import allelecounter as A
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from deepvariant_amd import variant_calling as vc
from tests import test_hip_gvcf as HG
from tests.test_hip_allelecounter import _fuzz_reads

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def _caller(min_snps=2, min_indels=2, f_snps=0.12, f_indels=0.06, track=False):
  """make_examples' defaults: vsc_min_count 2 / 2, vsc_min_fraction 0.12 / 0.06."""
  return vc.VariantCaller(vc.VariantCallerOptions(min_snps, min_indels, f_snps, f_indels, sample_name='s',
                                                  track_ref_reads=track))


def _host_calls(caller, counter):
  return caller.calls_from_allele_counts(counter.counts())


def _two_ways(make, caller, track=False, gvcf=None, fresh=True):
  """`make(positions)` -> fresh counters (positions: one list per counter, or None).  Runs the
  make_examples scheme on the device route -- a positions-only pass, then the calls (at the first
  pass' positions with `track`) -- and checks both against the host.  `fresh`: no counter has run
  before.  -> (all device calls, the counters that made them)."""
  first = make(None)
  A.AlleleCounter.run_batch(first, call=caller.candidate_options(positions_only=True))
  positions = [caller.call_positions_from_allele_counter(c) for c in first]
  assert not fresh or all(c._events is None for c in first)     # nothing but positions came home   pylint: disable=protected-access
  plain = make(None)
  A.AlleleCounter.run_batch(plain)
  assert positions == [caller.call_positions_from_allele_counts(c.counts()) for c in plain]
  counters = make(positions if track else None)
  A.AlleleCounter.run_batch(counters, gvcf=gvcf, call=caller.candidate_options())
  calls = []
  for c, pos in zip(counters, positions):
    got = caller.calls_from_allele_counter(c)
    assert got == _host_calls(caller, c)
    assert [g.variant.start for g in got] == pos
    assert caller.call_positions_from_allele_counter(c) == pos    # answered from the full pass
    calls += got
  return calls, counters


# ---------------------------------------------------------------- real reads

def _na12878_counters(tmp_path):
  bam, ref = HG._bam_fixture(tmp_path)                              # pylint: disable=protected-access
  lo, hi = ref.offset, ref.offset + len(ref.seq)
  table = packing.ReadTable.from_bam(bam, 'chr20', lo, hi, min_mapping_quality=5, keep_supplementary=True)
  ends = table.read_end.astype(np.int64)
  spans = [(start, min(start + 1000, hi)) for start in range(lo, hi, 1000)]
  tables = [table.take(np.nonzero((ends > s) & (table.read_pos.astype(np.int64) < e))[0]) for s, e in spans]

  def make(positions, track=False):
    out = []
    for k, ((s, e), t) in enumerate(zip(spans, tables)):
      c = A.AlleleCounter(ref, 'chr20', s, e, candidate_positions=positions[k] if positions else (),
                          min_mapping_quality=5, min_base_quality=10, track_ref_reads=track)
      c.add_table(t)
      out.append(c)
    return out
  return make


# Calls the host route yields on the raw reads of the slice (first GPU run of this test): 298.
NA12878_HOST_CALLS = 298


@pytest.mark.parametrize('track', [False, True])
def test_na12878_100kb_every_calling_region(tmp_path, track):
  """Every 1 kb calling region of the NA12878 100 kb BAM in one batch, make_examples' default
  thresholds, track_ref_reads off and on.  The host route yields 298 calls on these raw reads; the
  floor is half of that, so that an empty answer cannot pass."""
  make = _na12878_counters(tmp_path)
  caller = _caller(track=track)
  calls, _ = _two_ways(lambda positions: make(positions, track), caller, track)
  print('NA12878 100 kb: %d calls, %d reference-supporting reads named' % (len(calls), sum(len(c.ref_support) for c in calls)))
  assert len(calls) >= NA12878_HOST_CALLS // 2
  if track:
    assert sum(len(c.ref_support) for c in calls) > len(calls)
  else:
    assert not any(c.ref_support for c in calls)


@pytest.mark.parametrize('fixture', ['illumina_wgs_chr20.npz', 'pacbio_chr20.npz'])
def test_golden_read_tables(fixture):
  from tests import golden_io
  from tests import test_oracle_golden as G
  caller = _caller()
  calls, _ = _two_ways(lambda positions: [HG._golden_counter(fixture)], caller)      # pylint: disable=protected-access
  assert len(calls) > 20
  if fixture.startswith('illumina'):
    # golden_candidate_agreement's three figures (tests/test_hip_allelecounter.py holds them for the host
    # route), with the device route's calls in the place of call_variant
    _, examples, _ = golden_io.load(os.path.join(GOLDEN, fixture))
    by_start = {c.variant.start: c for c in calls}
    gold = {}
    for ex in examples:
      v = ex['call'].variant
      gold[(v.start, v.reference_bases, tuple(v.alternate_bases))] = ex['call']
    same = same_support = 0
    for (start, ref, alts), g in gold.items():
      call = by_start.get(start)
      if call is None or (call.variant.reference_bases, tuple(call.variant.alternate_bases)) != (ref, alts):
        continue
      same += 1
      same_support += ({k: sorted(s.read_names) for k, s in call.allele_support.items()} ==
                       {k: sorted(s.read_names) for k, s in g.allele_support.items()})
    assert (len(gold), same, same_support) == (78, 72, 47)
    counts = HG._golden_counter(fixture).counts()                   # pylint: disable=protected-access
    lo = counts[0].position.position
    assert G.golden_candidate_agreement(examples, lambda pos: counts[pos - lo]) == (78, 72, 47)


# ---------------------------------------------------------------- fuzz

class _SeqRef:
  def __init__(self, seq):
    self.seq = seq

  def n_bases(self, contig):
    return len(self.seq)

  def get_bases(self, contig, start, end):
    return self.seq[start:end]


@pytest.mark.parametrize('seed,long_reads,track', [(31, False, False), (32, True, False), (33, False, True)])
def test_fuzz(seed, long_reads, track):
  """The regions, seeds and threshold triples of
  test_hip_allelecounter.py::test_narrowed_visit_gives_the_same_candidates (duplicate read keys,
  low-quality alleles, soft clips, long reads, tracked reference reads), plus min_count 0 and 1."""
  rng = np.random.default_rng(seed)
  seq = ''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=6000))
  ref = _SeqRef(seq)
  n_calls = 0
  for (start, end), (lo, hi) in (((1000, 2000), (700, 2100)), ((0, 400), (0, 420)), ((5600, 6000), (5300, 5990))):
    reads = _fuzz_reads(rng, ref, 700 if not long_reads else 200, lo, hi, long_reads)
    reads += reads[:40]
    for min_snps, min_indels in ((2, 2), (3, 2), (2, 4), (0, 0), (1, 1), (1, 0)):
      caller = _caller(min_snps, min_indels, track=track)

      def make(positions):
        c = A.AlleleCounter(ref, 'c', start, end, candidate_positions=positions[0] if positions else (),
                            min_mapping_quality=10, min_base_quality=20, track_ref_reads=track)
        for r in reads:
          c.add(r)
        return [c]

      calls, _ = _two_ways(make, caller, track)
      if min(min_snps, min_indels) >= 2:
        n_calls += len(calls)
  assert n_calls > 20 or long_reads


# ---------------------------------------------------------------- hand-built corners

def _corner_ref():
  rng = np.random.default_rng(77)
  seq = list(''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=3000)))
  seq[1500], seq[1520] = 'N', 'R'
  return _SeqRef(''.join(seq))


def _other(base):
  return 'A' if base != 'A' else 'C'


def _pile(ref, name, n, start=1000, length=60, edit=None, qual=30, **kw):
  """`n` 60M reads at `start`; edit(sequence as a list) changes their bases."""
  out = []
  for i in range(n):
    s = list(ref.seq[start:start + length])
    if edit:
      edit(s)
    out.append(HG._read('%s%d' % (name, i), 1, start, ''.join(s), [(length, 'M')], qual=qual, **kw))   # pylint: disable=protected-access
  return out


def _one_region(ref, reads, caller, start=900, end=1700, track=False):
  def make(positions):
    c = A.AlleleCounter(ref, 'c', start, end, candidate_positions=positions[0] if positions else (),
                        min_mapping_quality=10, min_base_quality=10, track_ref_reads=track)
    for r in reads:
      c.add(r)
    return [c]
  calls, _ = _two_ways(make, caller, track)
  return {c.variant.start: c for c in calls}


def _sub_at(p, start=1000):
  def edit(s):
    s[p - start] = _other(s[p - start])
  return edit


def test_float32_threshold_edges():
  """The thresholds are float32 (proto `float`): with min_fraction_snps 0.1, 2 of 20 reads is rejected,
  because float32(0.1) = 0.10000000149 lies above 2 / 20 -- a plain double comparison keeps it; with the
  default 0.12, 3 of 25 is kept, float32(0.12) = 0.11999999732 lying below it."""
  assert 2 / 20 >= 0.1 and not 2 / 20 >= float(np.float32(0.1))
  assert 3 / 25 >= float(np.float32(0.12))
  ref = _corner_ref()
  reads = _pile(ref, 'ref', 18) + _pile(ref, 'alt', 2, edit=_sub_at(1030))
  assert 1030 not in _one_region(ref, reads, _caller(f_snps=0.1))
  assert 1030 in _one_region(ref, reads, _caller(f_snps=0.0999))
  reads = _pile(ref, 'ref', 22) + _pile(ref, 'alt', 3, edit=_sub_at(1030))
  call = _one_region(ref, reads, _caller())[1030]
  assert [v.int_value for v in call.variant.calls[0].info['DP'].values] == [25]
  assert [v.int_value for v in call.variant.calls[0].info['AD'].values] == [22, 3]


def _indel_reads(ref, name, n, at, inserted='', deleted=0, anchor=None, start=1000, length=60):
  """Reads with an insertion of `inserted` or a deletion of `deleted` bases anchored on `at`; `anchor`
  replaces the read's base at `at` (a mismatch the indel supersedes)."""
  k = at - start + 1
  out = []
  for i in range(n):
    head = list(ref.seq[start:at + 1])
    if anchor:
      head[-1] = anchor
    tail = ref.seq[at + 1 + deleted:start + length + deleted]
    cigar = [(k, 'M'), (len(inserted), 'I') if inserted else (deleted, 'D'), (len(tail), 'M')]
    out.append(HG._read('%s%d' % (name, i), 1, start, ''.join(head) + inserted + tail, cigar))   # pylint: disable=protected-access
  return out


def test_alleles_that_differ_in_text_only():
  ref = _corner_ref()
  reads = _pile(ref, 'ref', 10)
  # two insertions of equal length and different bases at 1020
  reads += _indel_reads(ref, 'insTT', 3, 1020, inserted='TT') + _indel_reads(ref, 'insGG', 2, 1020, inserted='GG')
  # two deletions of equal length with different anchor bases at 1040
  reads += _indel_reads(ref, 'del', 3, 1040, deleted=2)
  reads += _indel_reads(ref, 'delx', 2, 1040, deleted=2, anchor=_other(ref.seq[1040]))
  calls = _one_region(ref, reads, _caller())
  assert len(calls[1020].variant.alternate_bases) == 2 and len(calls[1040].variant.alternate_bases) == 2
  assert sorted(len(s.read_names) for s in calls[1020].allele_support.values()) == [2, 3]
  # with min_count 3 the rarer ones are uncalled
  calls = _one_region(ref, reads, _caller(3, 3))
  assert len(calls[1020].allele_support[vc.K_SUPPORTING_UNCALLED_ALLELE].read_names) == 2
  assert len(calls[1040].allele_support[vc.K_SUPPORTING_UNCALLED_ALLELE].read_names) == 2


def test_low_quality_and_overwritten_events():
  ref = _corner_ref()
  reads = _pile(ref, 'ref', 10)
  # a low-quality event whose text equals a called allele: supports it, does not count
  reads += _pile(ref, 'alt', 3, edit=_sub_at(1030)) + _pile(ref, 'low', 1, edit=_sub_at(1030), qual=3)
  # a read key whose later (supplementary, low-quality) event overwrites its good allele at 1045
  reads += _pile(ref, 'good', 2, edit=_sub_at(1045))
  reads += [HG._read('chimera', 1, 1000, ''.join(r.aligned_sequence), [(60, 'M')]) for r in _pile(ref, 'x', 1, edit=_sub_at(1045))]   # pylint: disable=protected-access
  reads += [HG._read('chimera', 1, 1040, ''.join(r.aligned_sequence), [(20, 'M')], qual=3, supplementary=True)                       # pylint: disable=protected-access
            for r in _pile(ref, 'x', 1, start=1040, length=20, edit=_sub_at(1045, 1040))]
  calls = _one_region(ref, reads, _caller())
  info = calls[1030].variant.calls[0].info
  assert [v.int_value for v in info['AD'].values] == [13, 3]
  support = [s for ext in calls[1030].allele_support_ext.values() for s in ext]
  assert len(support) == 4 and sum(s.is_low_quality for s in support) == 1
  info = calls[1045].variant.calls[0].info
  assert [v.int_value for v in info['AD'].values][1] == 2            # the chimera's good allele is gone
  support = [s for ext in calls[1045].allele_support_ext.values() for s in ext]
  assert len(support) == 3 and sum(s.is_low_quality for s in support) == 1


def test_non_acgt_reference_base_is_never_a_candidate():
  ref = _corner_ref()

  def edit(s):
    s[0], s[20], s[40] = 'A', 'C', _other(s[40])
  reads = _pile(ref, 'alt', 6, start=1500, edit=edit) + _pile(ref, 'ref', 6, start=1500)
  calls = _one_region(ref, reads, _caller())
  assert 1500 not in calls and 1520 not in calls and 1540 in calls


def test_deletion_reaching_past_another_allele():
  """A 3-base deletion and a substitution selected at one position: the variant's reference bases are the
  deletion's, and the substitution's key carries their suffix."""
  ref = _corner_ref()
  reads = _pile(ref, 'ref', 8) + _pile(ref, 'sub', 3, edit=_sub_at(1030)) + _indel_reads(ref, 'del', 3, 1030, deleted=3)
  reads += _pile(ref, 'next', 3, edit=_sub_at(1032))                 # and a candidate inside the deleted bases
  calls = _one_region(ref, reads, _caller())
  call = calls[1030]
  assert call.variant.reference_bases == ref.seq[1030:1034]
  assert sorted(map(len, call.allele_support)) == [1, 4] and 1032 in calls


def test_insertion_longer_than_16_bits():
  ref = _corner_ref()
  rng = np.random.default_rng(3)
  long_text = ''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=66_000))
  reads = _pile(ref, 'ref', 4)
  reads += _indel_reads(ref, 'ins', 2, 1030, inserted=long_text)
  reads += _indel_reads(ref, 'other', 1, 1030, inserted=long_text[:-1] + _other(long_text[-1]))
  calls = _one_region(ref, reads, _caller())
  call = calls[1030]
  assert [len(a) for a in call.variant.alternate_bases] == [66_001]
  assert len(call.allele_support[vc.K_SUPPORTING_UNCALLED_ALLELE].read_names) == 1


def _synthetic_with_candidates():
  """test_hip_gvcf.py's synthetic reads (12x background, shared read keys, a 150-deep site whose third
  read carries an alternate base at 1620) plus four reads each with a substitution at 1070 and a
  deletion at 1220: one certain candidate in each of three regions."""
  ref, reads = HG._synthetic()                                      # pylint: disable=protected-access
  reads += _pile(ref, 'sub', 4, start=1050, edit=_sub_at(1070, 1050))
  reads += _indel_reads(ref, 'del', 4, 1220, deleted=2, start=1205)
  return ref, reads


def test_readless_region_in_a_batch_and_a_counter_that_has_run():
  ref, reads = _synthetic_with_candidates()
  spans = [(1000, 1200), (2500, 2600), (1200, 1450), (1450, 1800)]  # the second has no reads
  caller = _caller()

  def make(positions):
    out = []
    for s, e in spans:
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    out[2].counts()                                                 # has already run: it is counted again
    return out
  calls, counters = _two_ways(make, caller, fresh=False)
  assert {1070, 1220, 1620} <= {c.variant.start for c in calls} and caller.calls_from_allele_counter(counters[1]) == []
  # each region alone (the one-region entry of the same pass) gives the same calls
  alone = [c for k in range(len(spans)) for c in caller.calls_from_allele_counter(make(None)[k])]
  assert alone == calls


def _noisy_reads(ref):
  """300 reads of 100 bases over [950, 1450), every base a mismatch."""
  rng = np.random.default_rng(11)
  noisy = []
  for i in range(300):
    start = int(rng.integers(950, 1350))
    seq = ''.join(_other(b) if i % 3 else ('G' if b != 'G' else 'T') for b in ref.seq[start:start + 100])
    noisy.append(HG._read('n%d' % i, 1, start, seq, [(100, 'M')]))    # pylint: disable=protected-access
  return noisy


def _quiet_reads(ref, start=2000):
  """Ten reference reads and four with a substitution at start + 30."""
  return _pile(ref, 'ref', 10, start=start) + _pile(ref, 'alt', 4, start=start, edit=_sub_at(start + 30, start))


def test_events_beyond_the_first_guess():
  """A region whose events overflow the batch's first guess (every base of every read is a mismatch) is
  counted alone and takes the same kernels from its counts (the one-region path), next to an ordinary
  region of the same batch."""
  ref = _corner_ref()
  noisy = _noisy_reads(ref)
  quiet = _quiet_reads(ref)
  caller = _caller()

  def make(positions):
    out = []
    for (s, e), reads in (((1000, 1400), noisy), ((1990, 2070), quiet)):
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    return out
  calls, counters = _two_ways(make, caller)
  n_events = len(counters[0]._events)                                # pylint: disable=protected-access
  assert n_events > 300 + 300 * 100 // 16 + 4096                      # dv_count_alleles_batch's first guess
  assert len(calls) == 400 + 1 and sum(len(c.variant.alternate_bases) == 2 for c in calls) > 300


# ---------------------------------------------------------------- with the gVCF pass

def test_with_gvcf_in_one_pass():
  """run_batch(gvcf=..., call=...): the gVCF records of run_batch(gvcf=...) bit for bit, and the same
  candidates."""
  ref, reads = _synthetic_with_candidates()
  spans = [(1000, 1200), (1200, 1450), (2500, 2600), (1450, 1800)]
  opts = vc.GvcfOptions('s', include_med_dp=True)
  caller = _caller()

  def make(positions):
    out = []
    for s, e in spans:
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    return out
  calls, both = _two_ways(make, caller, gvcf=opts)
  assert {1070, 1220, 1620} <= {c.variant.start for c in calls}
  only = make(None)
  A.AlleleCounter.run_batch(only, gvcf=opts)
  for b, o in zip(both, only):
    assert b._gvcf is not None and b.gvcf_block_array(opts).tobytes() == o.gvcf_block_array(opts).tobytes()   # pylint: disable=protected-access
    HG._same(b.gvcf_blocks(opts), HG._host(o, opts))                # pylint: disable=protected-access


# ---------------------------------------------------------------- the overflow route inside a batch

_OVERFLOW_SPANS = ((1990, 2070), (1000, 1400), (2100, 2180))       # quiet, noisy, quiet
_OVERFLOW_GVCF = vc.GvcfOptions('s', include_med_dp=True)
_overflow_cache = {}


def _overflow_counters(track):
  """Three fresh counters: the noisy region of test_events_beyond_the_first_guess between two quiet ones.
  With `track` every region has candidate positions; the noisy one few enough that it still overflows."""
  ref = _corner_ref()
  reads = (_quiet_reads(ref), _noisy_reads(ref), _quiet_reads(ref, 2110))
  positions = ([2030], list(range(1000, 1400, 8)), [2140]) if track else ((), (), ())
  out = []
  for (s, e), rs, pos in zip(_OVERFLOW_SPANS, reads, positions):
    c = A.AlleleCounter(ref, 'c', s, e, candidate_positions=pos, min_mapping_quality=10, min_base_quality=10,
                        track_ref_reads=track)
    for r in rs:
      c.add(r)
    out.append(c)
  return out


def _overflow_reference(track):
  """Once per `track`: each region counted alone by the one-region entry, and the host's records, calls
  and call positions from those counts."""
  if track not in _overflow_cache:
    caller = _caller(track=track)
    alone = _overflow_counters(track)
    for c in alone:
      c.counts()
    # the noisy region's events exceed dv_count_alleles_batch's first guess
    n_positions = len(alone[1]._candidate_positions) if track else 0   # pylint: disable=protected-access
    assert len(alone[1]._events) > 300 + 300 * 100 // 16 + 4096 + 64 * n_positions   # pylint: disable=protected-access
    assert len(alone[0]._events) < 14 + 14 * 60 // 16 + 4096           # pylint: disable=protected-access
    _overflow_cache[track] = dict(
        caller=caller, alone=alone,
        records=[HG._host(c, _OVERFLOW_GVCF) for c in alone],          # pylint: disable=protected-access
        calls=[_host_calls(caller, c) for c in alone],
        positions=[caller.call_positions_from_allele_counts(c.counts()) for c in alone])
    assert len(_overflow_cache[track]['calls'][1]) == 400 and [len(x) for x in _overflow_cache[track]['positions']] == [1, 400, 1]
  return _overflow_cache[track]


def _run_overflow(track, way, groups):
  """Runs the three regions in `groups` (lists of region indices, one run_batch each) -> the counters."""
  want = _overflow_reference(track)
  caller = want['caller']
  kwargs = {'gvcf': dict(gvcf=_OVERFLOW_GVCF),
            'gvcf+call': dict(gvcf=_OVERFLOW_GVCF, call=caller.candidate_options()),
            'positions': dict(call=caller.candidate_options(positions_only=True)),
            'plain': {}}[way]
  counters = _overflow_counters(track)
  for group in groups:
    A.AlleleCounter.run_batch([counters[k] for k in group], **kwargs)
  return counters


@pytest.mark.parametrize('way', ['gvcf', 'gvcf+call', 'positions', 'plain'])
@pytest.mark.parametrize('track', [False, True])
def test_overflowing_region_in_the_middle_of_a_batch(track, way):
  """Quiet, noisy, quiet: the noisy region leaves the batch (its events exceed the first guess) and the
  packed records behind it still land in the right region.  Every way of running the batch against the
  host, and against the same regions run one per batch."""
  want = _overflow_reference(track)
  caller = want['caller']
  together = _run_overflow(track, way, [[0, 1, 2]])
  one_each = _run_overflow(track, way, [[0], [1], [2]])
  for k, (t, o, a) in enumerate(zip(together, one_each, want['alone'])):
    for c in (t, o):
      if way == 'positions':
        assert c._events is None                                      # pylint: disable=protected-access
        assert caller.call_positions_from_allele_counter(c) == want['positions'][k]
        continue
      assert np.array_equal(c._events, a._events)                     # pylint: disable=protected-access
      assert np.array_equal(c.ref_supporting_read_counts(), a.ref_supporting_read_counts())
      assert c.n_counted_reads() == a.n_counted_reads()
      if 'gvcf' in way:
        assert c._gvcf is not None                                    # pylint: disable=protected-access
        HG._same(c.gvcf_blocks(_OVERFLOW_GVCF), want['records'][k])   # pylint: disable=protected-access
      if 'call' in way:
        assert c._cand is not None                                    # pylint: disable=protected-access
        assert caller.calls_from_allele_counter(c) == want['calls'][k]
    if 'gvcf' in way:
      assert t.gvcf_block_array(_OVERFLOW_GVCF).tobytes() == o.gvcf_block_array(_OVERFLOW_GVCF).tobytes()
    if 'call' in way:
      for x, y in zip(t._cand[1:], o._cand[1:]):                      # pylint: disable=protected-access
        assert x.tobytes() == y.tobytes()


def test_device_resident_read_table_in_a_batch_with_call():
  """A region whose read table is in device memory takes the one-region path and the candidate pass from
  its counts, reading the bases where the caller left them; next to a host-resident region of the same
  batch it gives the sites, alleles and words of the same region passed host-resident."""
  import torch
  from deepvariant_amd import _lib
  ref, reads = _synthetic_with_candidates()
  caller = _caller()

  def make():
    out = []
    for s, e in ((1000, 1200), (1200, 1450)):                         # the first has shared read keys
      c = A.AlleleCounter(ref, 'c', s, e, min_mapping_quality=10, min_base_quality=10)
      for r in reads:
        c.add(r)
      out.append(c)
    return out

  def on_device(counter):
    host_request = counter._request                                   # pylint: disable=protected-access

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
    counter._request = request                                        # pylint: disable=protected-access

  host = make()
  A.AlleleCounter.run_batch(host, call=caller.candidate_options())
  mixed = make()
  on_device(mixed[0])
  A.AlleleCounter.run_batch(mixed, call=caller.candidate_options())
  for m, h in zip(mixed, host):
    assert len(m._cand[1]) and len(m._cand[2]) and len(m._cand[3])    # pylint: disable=protected-access
    for x, y in zip(m._cand[1:], h._cand[1:]):                        # sites, alleles, words   pylint: disable=protected-access
      assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert np.array_equal(m._events, h._events)                       # pylint: disable=protected-access
    assert caller.calls_from_allele_counter(m) == _host_calls(caller, m)
  assert 1070 in [c.variant.start for c in caller.calls_from_allele_counter(mixed[0])]


# ---------------------------------------------------------------- through the product

@pytest.mark.parametrize('track,gvcf', [(False, False), (True, False), (False, True)])
def test_process_tables_with_and_without_the_device_route(tmp_path, monkeypatch, track, gvcf):
  from deepvariant_amd import make_examples_core as mec
  from tests.golden.make_golden import wgs_options
  bam, ref = HG._bam_fixture(tmp_path)                              # pylint: disable=protected-access
  regions = list(mec.partition(T.Range('chr20', ref.offset, ref.offset + len(ref.seq)), 1000))
  table = packing.ReadTable.from_bam(bam, 'chr20', regions[0].start, regions[-1].end, min_mapping_quality=5)
  options = T.MakeExamplesOptions(pic_options=wgs_options(),
                                  sample_options=[T.SampleOptions(role='main', name='NA12878', pileup_height=100)])
  ends = table.read_end.astype(np.int64)
  tables = [table.take(np.nonzero((ends > r.start) & (table.read_pos.astype(np.int64) < r.end))[0]) for r in regions]
  po = mec.RegionProcessorOptions(realigner_enabled=False, track_ref_reads=track, gvcf=gvcf)

  def run():
    proc = mec.RegionProcessor(options, ref, po)
    return [calls for calls, _ in proc.process_tables(regions, tables)], proc.gvcf_records
  device, device_records = run()
  monkeypatch.delattr(A.AlleleCounter, 'candidates')                # the host walk, as before the device route
  monkeypatch.delattr(A.AlleleCounter, 'candidate_positions')
  host, host_records = run()
  assert device == host and sum(map(len, host)) >= NA12878_HOST_CALLS // 2
  assert device_records == host_records and bool(host_records) == gvcf
  if track:
    assert sum(len(c.ref_support) for calls in device for c in calls) > 100
