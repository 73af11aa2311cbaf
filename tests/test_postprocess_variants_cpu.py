"""deepvariant_amd.postprocess_variants on the host: step 4 against answers worked out here
with `math` alone, the VCF writer as text, and the command line on CallVariantsOutput records.  No GPU."""
import gzip
import math

import numpy as np
import pytest

from deepvariant_amd import call_variants as cv
from deepvariant_amd import dv_types as T
from deepvariant_amd import genomics_io
from deepvariant_amd import postprocess_variants as pp
from deepvariant_amd import protowire as pw
from deepvariant_amd import tfrecord

MAXC = 1.0 - 1e-15


def phred(p):
  return -10.0 * math.log10(1.0 - min(p, MAXC))


def make_variant(contig, start, ref, alts, ad, vaf, sample='NA12878'):
  info = {'AD': T.ListValue([T.Value(int_value=v) for v in ad]), 'DP': T.ListValue([T.Value(int_value=sum(ad))]),
          'VAF': T.ListValue([T.Value(number_value=v) for v in vaf])}
  call = T.VariantCall(call_set_name=sample, genotype=[-1, -1], info=info)
  return T.Variant(reference_name=contig, start=start, end=start + len(ref), reference_bases=ref,
                   alternate_bases=list(alts), calls=[call])


SNP = make_variant('chr1', 99, 'A', ['G'], [10, 10], [0.5])


def test_compute_quals_and_genotypes():
  gq, qual = pp.compute_quals([0.0, 1.0, 0.0], 1)
  # both probabilities are capped at 1 - 1e-15, whose distance from one is 9 * 2^-53 = 9.992e-16 as a double
  bounded = -10.0 * math.log10(1.0 - MAXC)
  assert 1.0 - MAXC == 9 * 2.0 ** -53 and 150 < bounded < 150.01 and gq == 150 and qual == round(bounded, 7)
  gq, qual = pp.compute_quals([0.9, 0.06, 0.04], 0)
  assert gq == 10 and qual == round(-10.0 * math.log10(1.0 - (0.06 + 0.04)), 7)
  assert [pp.genotype_of_index(k) for k in range(10)] == [[0, 0], [0, 1], [1, 1], [0, 2], [1, 2], [2, 2], [0, 3], [1, 3],
                                                          [2, 3], [3, 3]]
  assert pp.most_likely_genotype([0.2, 0.4, 0.4]) == (1, [0, 1])     # the first of the largest


def test_add_call_to_variant_known_answers():
  r = pp.add_call_to_variant(SNP, [0.0, 1.0, 0.0], 1)
  assert (r.genotype, r.filter, r.gq) == ([0, 1], 'PASS', 150)
  floor = math.log10(1.0 - MAXC)
  assert r.genotype_likelihood == [floor, 0.0, floor]
  assert (r.reference_name, r.start, r.end, r.reference_bases, r.alternate_bases) == ('chr1', 99, 100, 'A', ['G'])
  assert (r.dp, r.ad, r.vaf, r.call_set_name) == (20, [10, 10], [0.5], 'NA12878')
  # 0/0 below GQ 20 becomes ./. and keeps its filter; at 30 it stays
  low = pp.add_call_to_variant(SNP, [0.9, 0.06, 0.04], 0)
  assert (low.genotype, low.filter, low.gq) == ([-1, -1], 'RefCall', 10)
  high = pp.add_call_to_variant(SNP, [0.999, 0.0006, 0.0004], 0)
  assert (high.genotype, high.filter, high.gq) == ([0, 0], 'RefCall', 30)
  assert pp.add_call_to_variant(SNP, [0.9, 0.06, 0.04], 0, cnn_homref_call_min_gq=10).genotype == [0, 0]
  # a het call whose QUAL = phred(0.55) = 3.47 passes the default filter and is LowQual under 5
  assert 3.4 < phred(0.55) < 3.5
  assert pp.add_call_to_variant(SNP, [0.45, 0.5, 0.05], 1).filter == 'PASS'
  lq = pp.add_call_to_variant(SNP, [0.45, 0.5, 0.05], 1, qual_filter=5.0)
  assert (lq.filter, lq.genotype, lq.quality) == ('LowQual', [0, 1], round(phred(0.5 + 0.05), 7))


def test_pruning_and_suffix_stripping():
  v = make_variant('chr1', 10, 'CAAA', ['CAA', 'C', 'CAAAA'], [5, 1, 7, 2], [0.1, 0.5, 0.2])
  assert pp.prune_alleles(v, 0b001) == (['C', 'CAAAA'], [5, 7, 2], [0.5, 0.2])
  assert pp.prune_alleles(v, 0b110) == (['CAA'], [5, 1], [0.1])
  assert pp.prune_alleles(v, 0) == (['CAA', 'C', 'CAAAA'], [5, 1, 7, 2], [0.1, 0.5, 0.2])
  assert pp.simplify_variant_alleles('CAAA', ['CAA', 'CAAAA']) == ('CA', ['C', 'CAA'])
  assert pp.simplify_variant_alleles('CAAA', ['CAA', 'C']) == ('CAAA', ['CAA', 'C'])          # 'C' is one base already
  assert pp.simplify_variant_alleles('AT', ['GT']) == ('A', ['G'])
  assert pp.simplify_variant_alleles('TT', ['TT']) == ('T', ['T'])                            # down to one base
  assert pp.simplify_variant_alleles('A', ['G']) == ('A', ['G'])
  # alts 1 and 2 removed: the record keeps CAA alone, simplified, and `end` follows
  r = pp.add_call_to_variant(v, [0.1, 0.2, 0.7], 2, removed=0b110)
  assert (r.reference_bases, r.alternate_bases, r.start, r.end) == ('CA', ['C'], 10, 12)
  assert (r.ad, r.vaf, r.genotype) == ([5, 1], [0.1], [1, 1])


CONTIGS = [('chr1', 1000), ('chr2', 500)]
THREE_RECORDS = '''##fileformat=VCFv4.2
##FILTER=<ID=PASS,Description="All filters passed">
##FILTER=<ID=RefCall,Description="Genotyping model thinks this site is reference.">
##FILTER=<ID=LowQual,Description="Confidence in this variant being real is below calling threshold.">
##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">
##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Conditional genotype quality">
##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read depth">
##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Read depth for each allele">
##FORMAT=<ID=VAF,Number=A,Type=Float,Description="Variant allele fractions.">
##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods rounded to the closest integer">
##contig=<ID=chr1,length=1000>
##contig=<ID=chr2,length=500>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA12878
chr1\t100\t.\tA\tG\t150\tPASS\t.\tGT:GQ:DP:AD:VAF:PL\t0/1:150:20:10,10:0.5:150,0,150
chr1\t201\t.\tCA\tC\t0.5\tRefCall\t.\tGT:GQ:DP:AD:VAF:PL\t./.:10:12:11,1:0.0833333:0,12,14
chr2\t8\t.\tT\tTG\t0\tRefCall\t.\tGT:GQ:DP:AD:VAF:PL\t0/0:30:30:29,1:0.0333333:0,32,34
'''


def three_records():
  deletion = make_variant('chr1', 200, 'CA', ['C'], [11, 1], [1 / 12])
  insertion = make_variant('chr2', 7, 'T', ['TG'], [29, 1], [1 / 30])
  return [pp.add_call_to_variant(insertion, [0.999, 0.0006, 0.0004], 0),
          pp.add_call_to_variant(deletion, [0.9, 0.06, 0.04], 0),
          pp.add_call_to_variant(SNP, [0.0, 1.0, 0.0], 1)]


def test_three_record_vcf_as_text(tmp_path):
  # the figures of the rows, by hand: PL = round(-10 log10 p) less the smallest
  assert [round(-10 * math.log10(p)) for p in (0.9, 0.06, 0.04)] == [0, 12, 14]
  assert [round(-10 * math.log10(p)) for p in (0.999, 0.0006, 0.0004)] == [0, 32, 34]
  assert round(phred(0.1), 1) == 0.5 and round(phred(0.001), 1) == 0.0 and round(phred(1.0), 1) == 150.0
  records = three_records()
  assert pp.vcf_text(records, CONTIGS, 'NA12878') == THREE_RECORDS
  plain, zipped = str(tmp_path / 'out.vcf'), str(tmp_path / 'out.vcf.gz')
  pp.write_vcf(plain, records, CONTIGS, 'NA12878')
  pp.write_vcf(zipped, records, CONTIGS, 'NA12878')
  assert open(plain).read() == THREE_RECORDS and gzip.open(zipped, 'rt').read() == THREE_RECORDS
  with pytest.raises(ValueError, match='not a contig'):
    pp.vcf_text(records, [('chr1', 1000)], 'NA12878')


def test_rows_sort_stably_by_contig_start_end():
  a = pp.add_call_to_variant(make_variant('chr1', 50, 'AC', ['A'], [5, 5], [0.5]), [0.0, 1.0, 0.0], 1)
  b = pp.add_call_to_variant(make_variant('chr1', 50, 'A', ['T'], [5, 5], [0.5]), [0.0, 1.0, 0.0], 1)
  c = pp.add_call_to_variant(make_variant('chr1', 50, 'A', ['G'], [5, 5], [0.5]), [0.0, 1.0, 0.0], 1)
  rows = pp.vcf_text([a, b, c], CONTIGS, 's').splitlines()[-3:]
  assert [r.split('\t')[3:5] for r in rows] == [['A', 'T'], ['A', 'G'], ['AC', 'A']]     # end first, then input order


def cvo(variant, indices, probs):
  gls = cv.round_gls_batch(np.array([probs], np.float32), 10)[0].tolist()
  return cv.create_cvo(pw.encode_variant(variant), gls, pw.encode_alt_allele_indices(indices))


def test_command_line_on_call_variants_outputs(tmp_path):
  fasta = str(tmp_path / 'ref.fa')
  genomics_io.write_fasta(fasta, [('chr1', 'ACGT' * 250), ('chr2', 'TTGCA' * 100)])
  multi = make_variant('chr1', 300, 'CAA', ['C', 'CA'], [4, 1, 9], [1 / 14, 9 / 14])
  records = [
      cvo(SNP, [0], [0.001, 0.99, 0.009]),
      cvo(multi, [0], [0.93, 0.05, 0.02]),            # alt 0 scores 0.07 < t: removed
      cvo(multi, [1], [0.02, 0.18, 0.8]),
      cvo(multi, [0, 1], [0.6, 0.3, 0.1]),
      cvo(make_variant('chr2', 7, 'T', ['TG'], [29, 1], [1 / 30]), [0], [0.999, 0.0006, 0.0004]),
  ]
  outputs = []
  for k, order in enumerate(([0, 1, 2, 3, 4], [3, 4, 2, 0, 1])):
    infile, outfile = str(tmp_path / ('cvo%d.tfrecord.gz' % k)), str(tmp_path / ('out%d.vcf' % k))
    with tfrecord.Writer(infile) as w:
      for i in order:
        w.write(records[i])
    assert pp.main(['--infile', infile, '--ref', fasta, '--outfile', outfile]) == 0
    outputs.append(open(outfile, 'rb').read())
  assert outputs[0] == outputs[1]
  rows = [line.split('\t') for line in outputs[0].decode().splitlines() if not line.startswith('#')]
  assert [(r[0], r[1], r[3], r[4], r[6]) for r in rows] == [
      ('chr1', '100', 'A', 'G', 'PASS'), ('chr1', '301', 'CA', 'C', 'PASS'), ('chr2', '8', 'T', 'TG', 'RefCall')]
  # the pruned site: alt CA alone, from the single-alt item {1} only, AD and VAF pruned with it
  sample = dict(zip(rows[1][8].split(':'), rows[1][9].split(':')))
  assert sample['GT'] == '1/1' and sample['AD'] == '4,9' and sample['VAF'] == '%g' % (9 / 14) and sample['DP'] == '14'
  assert '##contig=<ID=chr2,length=500>' in outputs[0].decode() and rows[0][9].startswith('0/1:')
  # --sample_name, --qual_filter and --cnn_homref_call_min_gq reach step 4
  out = str(tmp_path / 'named.vcf')
  assert pp.main(['--infile', str(tmp_path / 'cvo0.tfrecord.gz'), '--ref', fasta, '--outfile', out, '--sample_name', 'X',
                  '--qual_filter', '35', '--cnn_homref_call_min_gq', '40']) == 0
  text = open(out).read()
  assert '\tFORMAT\tX\n' in text
  rows = [line.split('\t') for line in text.splitlines() if not line.startswith('#')]
  assert rows[0][6] == 'LowQual' and rows[2][9].startswith('./.:30:')


def test_merge_predictions_and_errors():
  multi = make_variant('chr1', 300, 'CAA', ['C', 'CA'], [4, 1, 9], [1 / 14, 9 / 14])
  items = [(multi, [0, 1], [0.6, 0.3, 0.1]), (multi, [1], [0.02, 0.18, 0.8]), (multi, [0], [0.93, 0.05, 0.02])]
  removed, predictions, best = pp.merge_predictions(items)
  assert removed == 1 and len(predictions) == 3 and best == 2
  total = np.float32(0.02).item() + np.float32(0.18).item() + np.float32(0.8).item()
  assert predictions == [np.float32(v).item() / total for v in (0.02, 0.18, 0.8)]
  assert pp.merge_predictions(items, qual_filter=0.0)[0] == 0
  with pytest.raises(ValueError, match='do not cover every genotype'):
    pp.merge_predictions(items[1:], qual_filter=0.0)       # singles only: genotype 1/2 has no example
  with pytest.raises(ValueError, match='do not sum to one'):
    pp.merge_predictions([(SNP, [0], [0.5, 0.3, 0.3])])


def test_make_examples_flags_for_the_vcf():
  from deepvariant_amd import make_examples as me
  ap = me.build_arg_parser()

  def check(extra):
    me.check_flags(ap.parse_args(['--ref', 'r.fa', '--reads', 'r.bam'] + extra))
  check(['--vcf_outfile', 'x.vcf', '--checkpoint', 'random:1'])
  check(['--vcf_outfile', 'x.vcf.gz', '--checkpoint', 'random:1', '--call_variants_outfile', 'cvo.tfrecord.gz'])
  with pytest.raises(ValueError, match='needs --checkpoint'):
    check(['--vcf_outfile', 'x.vcf'])
  with pytest.raises(ValueError, match='two routes'):
    check(['--vcf_outfile', 'x.vcf', '--checkpoint', 'random:1', '--examples', 'e.tfrecord.gz'])
  with pytest.raises(ValueError, match='one rank'):       # the multi-rank gather of the sites is left out
    check(['--vcf_outfile', 'x.vcf', '--checkpoint', 'random:1', '--gpus', '2', '--call_variants_outfile', 'c@2.gz'])
  with pytest.raises(ValueError, match='one rank'):
    check(['--vcf_outfile', 'x.vcf', '--checkpoint', 'random:1', '--ranks_per_gpu', '2', '--call_variants_outfile', 'c@2.gz'])


def test_the_queue_merges_its_sites_through_the_host_code(monkeypatch):
  """RegionProcessor._genotype_queue under DV_GENOTYPE_HOST=1, on a queue of two regions made by hand: the sites are the
  candidates, the records collect in the sink, and the rows it returns are round_gls_batch's."""
  import types
  import torch
  from deepvariant_amd import make_examples_core as core
  monkeypatch.setenv('DV_GENOTYPE_HOST', '1')
  multi = make_variant('chr1', 300, 'CAA', ['C', 'CA'], [4, 1, 9], [1 / 14, 9 / 14])
  region1 = ([types.SimpleNamespace(variant=SNP)], [(0, ['G'])], None)
  region2 = ([types.SimpleNamespace(variant=multi)], [(0, ['C']), (0, ['CA']), (0, ['C', 'CA'])], None)
  probs = np.array([[0.001, 0.99, 0.009], [0.93, 0.05, 0.02], [0.02, 0.18, 0.8], [0.6, 0.3, 0.1]], np.float32)
  variants, (item_alts, site_off, n_alts) = core.RegionProcessor.queue_sites([region1, ([], [], None), region2])
  assert variants == [SNP, multi] and site_off.tolist() == [0, 1, 4] and n_alts.tolist() == [1, 2]
  assert item_alts.tolist() == [[0, -1], [0, -1], [1, -1], [0, 1]]
  stub = types.SimpleNamespace(vcf=core.VcfSink(), queue_sites=core.RegionProcessor.queue_sites)
  rounded = core.RegionProcessor._genotype_queue(stub, [region1, region2], torch.from_numpy(probs))
  assert (rounded == cv.round_gls_batch(probs, 10)).all()
  assert stub.vcf.n_examples == 4 and stub.vcf.device_stats == {}
  got = [(r.start, r.reference_bases, r.alternate_bases, r.genotype, r.filter) for r in stub.vcf.records]
  assert got == [(99, 'A', ['G'], [0, 1], 'PASS'), (300, 'CA', ['C'], [1, 1], 'PASS')]
  bad = torch.from_numpy(np.array([[0.5, 0.3, 0.3]], np.float32))
  with pytest.raises(ValueError, match='do not sum to one'):
    core.RegionProcessor._genotype_queue(stub, [region1], bad)
