"""The gVCF writer of deepvariant_amd.postprocess_variants as text, on a layout written by hand,
and the command line on CallVariantsOutput records plus a GvcfShardWriter file.  The host merge; no GPU."""
import gzip

import numpy as np
import pytest

from deepvariant_amd import allelecounter
from deepvariant_amd import call_variants as cv
from deepvariant_amd import dv_types as T
from deepvariant_amd import genomics_io
from deepvariant_amd import make_examples_core as core
from deepvariant_amd import postprocess_variants as pp
from deepvariant_amd import protowire as pw
from deepvariant_amd import tfrecord
from deepvariant_amd import variant_calling

CHR1, CHR2 = 'ACGT' * 250, 'TTGCA' * 100
CONTIGS = [('chr1', 1000), ('chr2', 500)]


class Reference:
  """get_bases alone, counting the fetches."""

  def __init__(self):
    self.fetches = []

  def get_bases(self, contig, start, end):
    self.fetches.append((contig, start, end))
    return {'chr1': CHR1, 'chr2': CHR2}[contig][start:end]


def make_variant(contig, start, ref, alts, ad, vaf, sample='NA12878'):
  info = {'AD': T.ListValue([T.Value(int_value=v) for v in ad]), 'DP': T.ListValue([T.Value(int_value=sum(ad))]),
          'VAF': T.ListValue([T.Value(number_value=v) for v in vaf])}
  call = T.VariantCall(call_set_name=sample, genotype=[-1, -1], info=info)
  return T.Variant(reference_name=contig, start=start, end=start + len(ref), reference_bases=ref,
                   alternate_bases=list(alts), calls=[call])


SNP = make_variant('chr1', 99, 'T', ['G'], [10, 10], [0.5])                          # CHR1[99] is T
MULTI = make_variant('chr1', 120, 'ACG', ['A', 'AC'], [4, 1, 9], [1 / 14, 9 / 14])   # CHR1[120:123] is ACG


def block(start, end, base, likelihoods, gq, min_dp, med_dp=-1, valid=1):
  return (start, end, likelihoods, gq, min_dp, med_dp, ord(base), valid, (0, 0))


def blocks(med_dp):
  """chr1: [90, 110) whose own base is written as N (the FASTA has G there), so that a row shows where its base came
  from; [110, 130) without valid likelihoods.  chr2: [0, 20)."""
  m = (lambda v: v) if med_dp else (lambda v: -1)
  return {
      'chr2': np.array([block(0, 20, 'T', [0.0, -1.25, -12.5], 1, 3, m(4))], allelecounter.GVCF_BLOCK_DTYPE),
      'chr1': np.array([block(90, 110, 'N', [-0.0, -3.0, -30.0], 30, 12, m(15)),
                        block(110, 130, 'G', [-0.1, -0.2, -0.3], 0, 0, m(0), valid=0)], allelecounter.GVCF_BLOCK_DTYPE),
  }


def records():
  return [pp.add_call_to_variant(MULTI, [0.01, 0.02, 0.03, 0.04, 0.8, 0.1], 4),
          pp.add_call_to_variant(SNP, [0.0, 1.0, 0.0], 1)]


HEADER = '''##fileformat=VCFv4.2
##FILTER=<ID=PASS,Description="All filters passed">
##FILTER=<ID=RefCall,Description="Genotyping model thinks this site is reference.">
##FILTER=<ID=LowQual,Description="Confidence in this variant being real is below calling threshold.">
##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">
##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Conditional genotype quality">
##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read depth">
##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Read depth for each allele">
##FORMAT=<ID=VAF,Number=A,Type=Float,Description="Variant allele fractions.">
##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods rounded to the closest integer">
##INFO=<ID=END,Number=1,Type=Integer,Description="End position (for use with symbolic alleles)">
##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description="Minimum DP observed within the GVCF block.">
%s##contig=<ID=chr1,length=1000>
##contig=<ID=chr2,length=500>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA12878
'''
MED_DP_LINE = ('##FORMAT=<ID=MED_DP,Number=1,Type=Integer,Description="Median DP observed within the GVCF block rounded '
               'to the nearest integer.">\n')

# By hand.  [90, 110) loses base 99 to the SNP: [90, 99) keeps the block's own base N, [100, 110) starts anew and reads
# CHR1[100] = A.  [110, 130) loses [120, 123): [110, 120) keeps G, [123, 130) reads CHR1[123] = T.  PL = round(-10 GL)
# less the smallest: (0, 30, 300); (1, 2, 3) -> (0, 1, 2); (0, 12.5 -> 12 by half to even, 125).
# The SNP: 150,0,150 as in the plain VCF, then its three <*> genotypes at 990 - 0.  The two-alt site: round(-10 log10 p)
# of (0.01, 0.02, 0.03, 0.04, 0.8, 0.1) = (20, 17, 15, 14, 1, 10), less 1; its four <*> genotypes 990 - 1.  GQ =
# round(-10 log10(1 - 0.8)) = 7, QUAL = -10 log10(1 - 0.99) = 20.
ROWS_WITH_MED_DP = '''chr1\t91\t.\tN\t<*>\t0\t.\tEND=99\tGT:GQ:MIN_DP:MED_DP:PL\t0/0:30:12:15:0,30,300
chr1\t100\t.\tT\tG,<*>\t150\tPASS\t.\tGT:GQ:DP:AD:VAF:PL\t0/1:150:20:10,10,0:0.5,0:150,0,150,990,990,990
chr1\t101\t.\tA\t<*>\t0\t.\tEND=110\tGT:GQ:MIN_DP:MED_DP:PL\t0/0:30:12:15:0,30,300
chr1\t111\t.\tG\t<*>\t0\t.\tEND=120\tGT:GQ:MIN_DP:MED_DP:PL\t./.:0:0:0:0,1,2
chr1\t121\t.\tACG\tA,AC,<*>\t20\tPASS\t.\tGT:GQ:DP:AD:VAF:PL\t1/2:7:14:4,1,9,0:0.0714286,0.642857,0:19,16,14,13,0,9,989,989,989,989
chr1\t124\t.\tT\t<*>\t0\t.\tEND=130\tGT:GQ:MIN_DP:MED_DP:PL\t./.:0:0:0:0,1,2
chr2\t1\t.\tT\t<*>\t0\t.\tEND=20\tGT:GQ:MIN_DP:MED_DP:PL\t0/0:1:3:4:0,12,125
'''


def without_med_dp(rows):
  out = []
  for line in rows.splitlines():
    cols = line.split('\t')
    if cols[4] == '<*>':
      cols[8] = 'GT:GQ:MIN_DP:PL'
      sample = cols[9].split(':')
      cols[9] = ':'.join(sample[:3] + sample[4:])
    out.append('\t'.join(cols))
  return '\n'.join(out) + '\n'


def test_gvcf_text_by_hand():
  assert (CHR1[99], CHR1[100], CHR1[120:123], CHR1[123]) == ('T', 'A', 'ACG', 'T')
  ref = Reference()
  text = pp.gvcf_text(records(), blocks(True), ref, CONTIGS, 'NA12878')
  assert text == HEADER % MED_DP_LINE + ROWS_WITH_MED_DP
  # one fetch per contig with a moved start, over the moved starts alone
  assert ref.fetches == [('chr1', 100, 124)]


def test_gvcf_text_without_med_dp(tmp_path):
  text = pp.gvcf_text(records(), blocks(False), Reference(), CONTIGS, 'NA12878')
  assert text == HEADER % '' + without_med_dp(ROWS_WITH_MED_DP)
  assert 'MED_DP' not in text
  plain, zipped = str(tmp_path / 'out.g.vcf'), str(tmp_path / 'out.g.vcf.gz')
  pp.write_gvcf(plain, records(), blocks(False), Reference(), CONTIGS, 'NA12878')
  pp.write_gvcf(zipped, records(), blocks(False), Reference(), CONTIGS, 'NA12878')
  assert open(plain).read() == text and gzip.open(zipped, 'rt').read() == text
  assert open(zipped, 'rb').read()[4:8] == b'\x00' * 4          # no time stamp: the same bytes on every run


def test_variant_row_extension():
  one, two = records()[1], records()[0]
  cols = pp.gvcf_variant_row(one).rstrip('\n').split('\t')
  plain = pp.vcf_row(one).rstrip('\n').split('\t')
  assert cols[:4] == plain[:4] and cols[4] == plain[4] + ',<*>' and cols[5:9] == plain[5:9]
  got, was = dict(zip(cols[8].split(':'), cols[9].split(':'))), dict(zip(plain[8].split(':'), plain[9].split(':')))
  assert got['AD'] == was['AD'] + ',0' and got['VAF'] == was['VAF'] + ',0' and got['PL'] == was['PL'] + ',990,990,990'
  assert (got['GT'], got['GQ'], got['DP']) == (was['GT'], was['GQ'], was['DP'])
  cols = pp.gvcf_variant_row(two).rstrip('\n').split('\t')
  pl = dict(zip(cols[8].split(':'), cols[9].split(':')))['PL'].split(',')
  assert len(pl) == 10 and pl[6:] == ['989'] * 4           # (A + 2)(A + 3) / 2 genotypes of A + 1 = 3 alts
  # a record without AD or VAF keeps its dots
  import dataclasses
  bare = dataclasses.replace(one, ad=None, vaf=None)
  assert pp.gvcf_variant_row(bare).split('\t')[9].split(':')[3:5] == ['.', '.']
  with pytest.raises(ValueError, match='one likelihood per genotype'):
    pp.gvcf_variant_row(dataclasses.replace(one, genotype_likelihood=[0.0, -1.0]))


def test_blocks_only_variants_only_and_unknown_contigs():
  text = pp.gvcf_text([], blocks(False), Reference(), CONTIGS, 's')
  rows = [line.split('\t') for line in text.splitlines() if not line.startswith('#')]
  assert [(r[0], r[1], r[7]) for r in rows] == [('chr1', '91', 'END=110'), ('chr1', '111', 'END=130'), ('chr2', '1', 'END=20')]
  assert rows[0][3] == 'N'                       # an untouched block keeps its own base
  text = pp.gvcf_text(records(), {}, Reference(), CONTIGS, 's')
  assert [line.split('\t')[1] for line in text.splitlines() if not line.startswith('#')] == ['100', '121']
  with pytest.raises(ValueError, match='not a contig'):
    pp.gvcf_text([], {'chrX': blocks(False)['chr2']}, Reference(), CONTIGS, 's')
  with pytest.raises(Exception, match='overlaps'):
    both = np.concatenate([blocks(False)['chr1'], blocks(False)['chr1']])
    pp.gvcf_text([], {'chr1': both}, Reference(), CONTIGS, 's')


def test_blocks_from_variants_round_trip():
  arrays = blocks(True)
  variants = [variant_calling.gvcf_record(contig, int(b['start']), int(b['end']), chr(b['ref_base']),
                                          b['likelihoods'].tolist(), int(b['gq']), int(b['min_dp']), int(b['med_dp']),
                                          bool(b['has_valid_gl']), 's')
              for contig in ('chr1', 'chr2') for b in arrays[contig]]
  decoded = [pw.decode_variant(pw.encode_variant(v)) for v in reversed(variants)]
  back = pp.blocks_from_variants(decoded)
  assert sorted(back) == ['chr1', 'chr2']
  for contig in back:
    assert back[contig].dtype == allelecounter.GVCF_BLOCK_DTYPE and (back[contig] == arrays[contig]).all()


# ---------------------------------------------------------------------------------------------- the command line
def cvo(variant, indices, probs):
  gls = cv.round_gls_batch(np.array([probs], np.float32), 10)[0].tolist()
  return cv.create_cvo(pw.encode_variant(variant), gls, pw.encode_alt_allele_indices(indices))


def test_command_line_writes_the_gvcf(tmp_path):
  fasta = str(tmp_path / 'ref.fa')
  genomics_io.write_fasta(fasta, [('chr1', CHR1), ('chr2', CHR2)])
  cvos = [cvo(SNP, [0], [0.001, 0.99, 0.009]), cvo(MULTI, [0], [0.02, 0.9, 0.08]), cvo(MULTI, [1], [0.02, 0.18, 0.8]),
          cvo(MULTI, [0, 1], [0.1, 0.3, 0.6]),
          cvo(make_variant('chr2', 7, 'G', ['GT'], [29, 1], [1 / 30]), [0], [0.999, 0.0006, 0.0004])]
  arrays = blocks(True)
  arrays['chr2'] = np.array([block(0, 20, 'T', [0.0, -1.25, -12.5], 1, 3, 4), block(25, 40, 'T', [0.0, -2.0, -20.0], 20, 9, 9)],
                            allelecounter.GVCF_BLOCK_DTYPE)
  nonvariants = [variant_calling.gvcf_record(contig, int(b['start']), int(b['end']), chr(b['ref_base']),
                                             b['likelihoods'].tolist(), int(b['gq']), int(b['min_dp']), int(b['med_dp']),
                                             bool(b['has_valid_gl']), 'NA12878')
                 for contig in ('chr1', 'chr2') for b in arrays[contig]]
  outputs = []
  for k, (cvo_order, block_order) in enumerate((([0, 1, 2, 3, 4], [0, 1, 2, 3]), ([3, 4, 2, 0, 1], [3, 1, 0, 2]))):
    infile, spec = str(tmp_path / ('cvo%d.tfrecord.gz' % k)), str(tmp_path / ('gvcf%d.tfrecord@2.gz' % k))
    with tfrecord.Writer(infile) as w:
      for i in cvo_order:
        w.write(cvos[i])
    for task in range(2):                       # two shards, as two make_examples tasks write them
      with core.GvcfShardWriter(spec, task) as w:
        w.write_all(nonvariants[i] for i in block_order[task::2])
    vcf, gvcf = str(tmp_path / ('out%d.vcf' % k)), str(tmp_path / ('out%d.g.vcf' % k))
    assert pp.main(['--infile', infile, '--ref', fasta, '--outfile', vcf, '--nonvariant_site_tfrecord_path', spec,
                    '--gvcf_outfile', gvcf]) == 0
    outputs.append((open(vcf, 'rb').read(), open(gvcf, 'rb').read()))
  assert outputs[0] == outputs[1]
  # without the new flags: the same VCF, which is write_vcf's of the same records
  alone = str(tmp_path / 'alone.vcf')
  assert pp.main(['--infile', str(tmp_path / 'cvo0.tfrecord.gz'), '--ref', fasta, '--outfile', alone]) == 0
  assert open(alone, 'rb').read() == outputs[0][0]
  finished = pp.records_from_cvos([pw.decode_call_variants_output(r) for r in cvos])
  assert pp.vcf_text(finished, CONTIGS, 'NA12878').encode() == outputs[0][0]
  # the gVCF is gvcf_text of the same records and arrays
  text = outputs[0][1].decode()
  assert text == pp.gvcf_text(finished, arrays, genomics_io.FastaReader(fasta), CONTIGS, 'NA12878')
  rows = [line.split('\t') for line in text.splitlines() if not line.startswith('#')]
  assert [(r[0], r[1], r[4], r[7]) for r in rows] == [
      ('chr1', '91', '<*>', 'END=99'), ('chr1', '100', 'G,<*>', '.'), ('chr1', '101', '<*>', 'END=110'),
      ('chr1', '111', '<*>', 'END=120'), ('chr1', '121', 'A,AC,<*>', '.'), ('chr1', '124', '<*>', 'END=130'),
      ('chr2', '1', '<*>', 'END=7'), ('chr2', '8', 'GT,<*>', '.'), ('chr2', '9', '<*>', 'END=20'),
      ('chr2', '26', '<*>', 'END=40')]
  assert rows[8][3] == CHR2[8]                  # a moved start on the second contig reads its own contig
  vcf_rows = [line for line in outputs[0][0].decode().splitlines() if not line.startswith('#')]
  assert [r[1] for r in rows if r[4] != '<*>'] == [line.split('\t')[1] for line in vcf_rows]


def test_flag_pairing():
  with pytest.raises(ValueError, match='need each other'):
    pp.main(['--infile', 'x', '--ref', 'r.fa', '--outfile', 'o.vcf', '--gvcf_outfile', 'o.g.vcf'])
  with pytest.raises(ValueError, match='need each other'):
    pp.main(['--infile', 'x', '--ref', 'r.fa', '--outfile', 'o.vcf', '--nonvariant_site_tfrecord_path', 'g.tfrecord.gz'])


def test_region_processor_collects_block_arrays():
  """RegionProcessorOptions.gvcf_arrays_only: the field beside gvcf_records, and gvcf_records' default behaviour."""
  import types
  calls = []

  class Counter:
    def gvcf_block_array(self, opts):
      calls.append('array')
      return blocks(False)['chr2']

    def gvcf_blocks(self, opts):
      calls.append('objects')
      return ['a Variant']

  for arrays_only, want_records, want_calls in ((False, [['a Variant']], ['array', 'objects']), (True, [[]], ['array'])):
    del calls[:]
    stub = types.SimpleNamespace(processor_options=core.RegionProcessorOptions(gvcf=True, gvcf_arrays_only=arrays_only),
                                 gvcf_records=[[]], gvcf_block_arrays=[None])
    core.RegionProcessor._keep_gvcf(stub, 0, Counter(), None)
    assert stub.gvcf_records == want_records and calls == want_calls
    assert (stub.gvcf_block_arrays[0] == blocks(False)['chr2']).all()
