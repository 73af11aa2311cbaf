"""gVCF blocks on the device (dv_count_alleles_gvcf_batch, gvcf.hip) against the host restatement
(VariantCaller.make_gvcfs over AlleleCounter.summary_counts(), i.e. over counter.counts()): every field
of every record, bit for bit, on real reads (the NA12878 100 kb BAM, the Illumina and PacBio golden
read tables), on synthetic corner cases (read keys shared by supplementary alignments, two alleles of
one read at one position, zero-coverage gaps, N runs, sites deeper than the table) and through a
multi-region batch and the region processor's table path."""
import os

import numpy as np
import pytest

from deepvariant_amd import allelecounter as A
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from deepvariant_amd import variant_calling as vc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


class _Ref:
  def __init__(self, seq, offset=0):
    self.seq, self.offset = seq, offset

  def n_bases(self, contig):
    return self.offset + len(self.seq)

  def get_bases(self, contig, start, end):
    lo, hi = max(start, self.offset), min(end, self.offset + len(self.seq))
    inner = self.seq[lo - self.offset:hi - self.offset] if hi > lo else ''
    return 'N' * max(0, min(lo, end) - start) + inner + 'N' * max(0, end - max(hi, start))


def _host(counter, opts):
  caller = vc.VariantCaller(vc.VariantCallerOptions(sample_name=opts.sample_name, gq_resolution=opts.gq_resolution,
                                                    max_cache_coverage=opts.max_cache_coverage))
  return caller.make_gvcfs(counter.summary_counts(opts.left_padding, opts.right_padding),
                           include_med_dp=opts.include_med_dp)


def _same(device, host):
  """Every field, the likelihood doubles bit for bit."""
  assert len(device) == len(host)
  for d, h in zip(device, host):
    assert (d.reference_name, d.start, d.end, d.reference_bases, d.alternate_bases) == \
        (h.reference_name, h.start, h.end, h.reference_bases, h.alternate_bases)
    dc, hc = d.calls[0], h.calls[0]
    assert (dc.call_set_name, dc.genotype, dc.info) == (hc.call_set_name, hc.genotype, hc.info)
    assert np.array_equal(np.array(dc.genotype_likelihood).view(np.int64), np.array(hc.genotype_likelihood).view(np.int64))


def _check(counters, opts, min_blocks=1):
  A.AlleleCounter.run_batch(counters, gvcf=opts)
  n = 0
  for c in counters:
    got = c.gvcf_blocks(opts)
    _same(got, _host(c, opts))
    n += len(got)
  assert n >= min_blocks
  return n


# ---------------------------------------------------------------- real reads

def _bam_fixture(tmp_path):
  with np.load(os.path.join(GOLDEN, 'na12878_100kb.npz')) as z:
    bam = str(tmp_path / 'reads.bam')
    with open(bam, 'wb') as f:
      f.write(z['bam'].tobytes())
    with open(bam + '.bai', 'wb') as f:
      f.write(z['bai'].tobytes())
    ref = _Ref(z['ref_bases'].tobytes().decode(), int(z['ref_start'][0]))
  return bam, ref


@pytest.mark.parametrize('include_med_dp', [False, True])
def test_na12878_100kb_every_calling_region(tmp_path, include_med_dp):
  bam, ref = _bam_fixture(tmp_path)
  lo, hi = ref.offset, ref.offset + len(ref.seq)
  table = packing.ReadTable.from_bam(bam, 'chr20', lo, hi, min_mapping_quality=5, keep_supplementary=True)
  ends = table.read_end.astype(np.int64)
  counters = []
  for start in range(lo, hi, 1000):
    end = min(start + 1000, hi)
    rows = np.nonzero((ends > start) & (table.read_pos.astype(np.int64) < end))[0]
    c = A.AlleleCounter(ref, 'chr20', start, end, min_mapping_quality=5, min_base_quality=10)
    c.add_table(table.take(rows))
    counters.append(c)
  opts = vc.GvcfOptions('NA12878', include_med_dp=include_med_dp)
  n = _check(counters, opts, min_blocks=200)
  assert n < sum(c.interval_length() for c in counters) // 5      # blocks, not sites


def _golden_counter(fixture):
  from tests import golden_io
  from tests import test_oracle_golden as G
  reads, examples, _ = golden_io.load(os.path.join(GOLDEN, fixture))
  ref = G._WindowRef(examples)                                          # pylint: disable=protected-access
  lo = min(ex['call'].variant.start for ex in examples)
  hi = max(ex['call'].variant.end for ex in examples)
  c = A.AlleleCounter(ref, 'chr20', lo, hi, min_mapping_quality=5, min_base_quality=10)
  for r in reads:
    c.add(r)
  return c


@pytest.mark.parametrize('fixture', ['illumina_wgs_chr20.npz', 'pacbio_chr20.npz'])
def test_golden_read_tables(fixture):
  c = _golden_counter(fixture)
  _check([c], vc.GvcfOptions('NA12878', include_med_dp=True), min_blocks=20)
  _check([c], vc.GvcfOptions('NA12878', gq_resolution=1, left_padding=13, right_padding=7), min_blocks=20)


# ---------------------------------------------------------------- synthetic corner cases

def _read(name, number, start, seq, cigar, mapq=60, qual=30, supplementary=False):
  ops = []
  for n, op in cigar:
    ops.append(T.CigarUnit({'M': 1, 'I': 2, 'D': 3, 'N': 4, 'S': 5}[op], n))
  return T.Read(fragment_name=name, read_number=number, number_reads=2, aligned_sequence=seq,
                aligned_quality=bytes([qual] * len(seq)), supplementary_alignment=supplementary,
                alignment=T.LinearAlignment(position=T.Position('c', start, False), mapping_quality=mapq, cigar=ops))


def _synthetic():
  rng = np.random.default_rng(5)
  seq = list(''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=3000)))
  seq[1300:1320] = 'N' * 20                                            # an N run inside the region
  seq[1400] = 'R'                                                      # a lone IUPAC code
  ref = _Ref(''.join(seq))
  reads = []
  # background: 12x over [1000, 1250) and [1500, 1800); nothing over [1250, 1500) but the N run
  for i in range(300):
    start = int(rng.integers(990, 1700))
    if 1250 - 60 < start < 1500:
      continue
    s = ''.join(ref.seq[start:start + 60])
    s = ''.join(b if rng.random() > 0.02 else 'ACGT'[int(rng.integers(0, 4))] for b in s)
    reads.append(_read('bg%d' % i, 1, start, s, [(60, 'M')], qual=int(rng.integers(5, 40))))
  # supplementary alignments sharing a key: a low-quality allele of the second at 1100 overwrites the first's good
  # one (chimera2); with track_ref_reads the second's REFERENCE allele there overwrites it too (chimera)
  s = ref.seq[1080:1120]
  alt = s[:20] + ('A' if s[20] != 'A' else 'C') + s[21:]
  reads.append(_read('chimera', 1, 1080, alt, [(40, 'M')]))
  reads.append(_read('chimera', 1, 1090, ref.seq[1090:1130], [(40, 'M')], supplementary=True))
  reads.append(_read('chimera2', 1, 1080, alt, [(40, 'M')], qual=35))
  reads.append(_read('chimera2', 1, 1095, alt[15:], [(25, 'M')], qual=3, supplementary=True))
  # one read, two alleles at one position: 4M 1I 4S(with N, unusable) 2D 4M -> INS and DEL anchored at 1203
  reads.append(_read('twoalleles', 1, 1200, ref.seq[1200:1204] + 'T' + 'ANAA' + ref.seq[1206:1210],
                     [(4, 'M'), (1, 'I'), (4, 'S'), (2, 'D'), (4, 'M')]))
  # a mismatch directly before an insertion (the insertion supersedes the substitution)
  reads.append(_read('subins', 1, 1210, ref.seq[1210:1214] + ('A' if ref.seq[1214] != 'A' else 'G') + 'TT' +
                     ref.seq[1215:1220], [(5, 'M'), (2, 'I'), (5, 'M')]))
  # a site deeper than M = 100: 150 reads over [1600, 1640), a third of them with an alternate base at 1620
  for i in range(150):
    s = ref.seq[1600:1640]
    if i % 3 == 0:
      s = s[:20] + ('A' if s[20] != 'A' else 'T') + s[21:]
    reads.append(_read('deep%d' % i, 2, 1600, s, [(40, 'M')]))
  return ref, reads


@pytest.mark.parametrize('include_med_dp,binsize', [(False, 5), (True, 5), (True, 1), (True, 50)])
def test_synthetic_corner_cases(include_med_dp, binsize):
  ref, reads = _synthetic()
  c = A.AlleleCounter(ref, 'c', 1000, 1800, min_mapping_quality=10, min_base_quality=10)
  for r in reads:
    c.add(r)
  opts = vc.GvcfOptions('s', gq_resolution=binsize, include_med_dp=include_med_dp)
  _check([c], opts, min_blocks=5)
  blocks = c.gvcf_blocks(opts)
  covered = set()
  for b in blocks:
    covered.update(range(b.start, b.end))
  assert not covered & set(range(1300, 1320)) and 1400 not in covered      # N / R sites: no record
  assert set(range(1250, 1300)) <= covered                                  # zero coverage still gets records
  dp = {p: n for _, p, _, _, n in c.summary_counts()}
  assert dp[1620] > 100 and dp[1260] == 0
  # the key rule moved the counts where the host's read_alleles maps put them
  assert c.counts()[1203 - 1000].read_alleles['twoalleles/1'].type == A.DELETION


def test_track_ref_reads_and_padding():
  ref, reads = _synthetic()
  c = A.AlleleCounter(ref, 'c', 1000, 1800, min_mapping_quality=10, min_base_quality=10, track_ref_reads=True,
                      candidate_positions=[1100, 1203, 1620])
  for r in reads:
    c.add(r)
  _check([c], vc.GvcfOptions('s', include_med_dp=True, left_padding=150, right_padding=40))


def test_multi_region_batch_equals_each_alone():
  ref, reads = _synthetic()
  spans = [(1000, 1200), (1200, 1450), (1450, 1800), (2500, 2600), (1000, 1800)]   # one region without reads

  def make(k):
    start, end = spans[k]
    c = A.AlleleCounter(ref, 'c', start, end, min_mapping_quality=10, min_base_quality=10)
    for r in reads:
      c.add(r)
    return c

  opts = vc.GvcfOptions('s', include_med_dp=True)
  together = [make(k) for k in range(len(spans))]
  A.AlleleCounter.run_batch(together, gvcf=opts)
  for k, t in enumerate(together):
    alone = make(k)
    a = alone.gvcf_block_array(opts)
    assert a.tobytes() == t.gvcf_block_array(opts).tobytes()
    _same(alone.gvcf_blocks(opts), _host(alone, opts))
  assert together[3].gvcf_block_array(opts)['min_dp'].tolist() == [0]       # the readless region: one GQ-1 block
  # counts are those of the plain batch
  plain = [make(k) for k in range(len(spans))]
  A.AlleleCounter.run_batch(plain)
  for p, t in zip(plain, together):
    assert np.array_equal(p.ref_supporting_read_counts(), t.ref_supporting_read_counts())
    assert np.array_equal(p._events, t._events)                           # pylint: disable=protected-access


# ---------------------------------------------------------------- region processor

def test_region_processor_table_path(tmp_path):
  from deepvariant_amd import make_examples_core as mec
  from tests.golden.make_golden import wgs_options
  bam, ref = _bam_fixture(tmp_path)
  lo = ref.offset + 20_000
  regions = list(mec.partition(T.Range('chr20', lo, lo + 8000), 1000))
  table = packing.ReadTable.from_bam(bam, 'chr20', regions[0].start, regions[-1].end, min_mapping_quality=5)
  options = T.MakeExamplesOptions(pic_options=wgs_options(),
                                  sample_options=[T.SampleOptions(role='main', name='NA12878', pileup_height=100)])
  ends = table.read_end.astype(np.int64)
  tables = [table.take(np.nonzero((ends > r.start) & (table.read_pos.astype(np.int64) < r.end))[0]) for r in regions]
  results = {}
  for gvcf in (False, True):
    po = mec.RegionProcessorOptions(realigner_enabled=False, gvcf=gvcf, include_med_dp=True)
    proc = mec.RegionProcessor(options, ref, po)
    results[gvcf] = proc.process_tables(regions, tables)
    records = proc.gvcf_records
  assert [[c.variant for c in cs] for cs, _ in results[False]] == [[c.variant for c in cs] for cs, _ in results[True]]
  assert len(records) == len(regions) and sum(map(len, records)) > 50
  rr = options.pic_options.read_requirements
  opts = vc.GvcfOptions('NA12878', include_med_dp=True)
  for region, t, got in zip(regions, tables, records):
    c = A.AlleleCounter(ref, 'chr20', region.start, region.end, min_mapping_quality=rr.min_mapping_quality,
                        min_base_quality=rr.min_base_quality)
    c.add_table(t)
    _same(got, _host(c, opts))
