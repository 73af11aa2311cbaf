"""The native gVCF rows on the host (dv_gvcf_rows, csrc/gvcf_rows.h) against the Python formatter:
pp.gvcf_rows joined and encoded, compared with ==.  The layouts are those of the merge's tests, filled with seeded
block fields and records (tests/gvcf_rows_cases.py); then the number edges, the refused inputs, the by-hand text of
tests/test_gvcf_text_cpu.py and the command line with DV_GVCF_ROWS_NATIVE=1.  No GPU."""
import gzip

import numpy as np
import pytest

from deepvariant_amd import genomics_io
from deepvariant_amd import make_examples_core as core
from deepvariant_amd import postprocess_variants as pp
from deepvariant_amd import tfrecord
from deepvariant_amd import variant_calling
from tests import gvcf_merge_cases as M
from tests import gvcf_rows_cases as R
from tests import test_gvcf_text_cpu as H

CASES = M.named_cases()
CHUNK_CASES = M.chunk_cases(pp.merge_scan_chunk())
EDGES = R.number_edges()
VARIANT_CASES = R.variant_cases()


def host_equals_reference(arguments, n_pieces=None):
  records, blocks, contigs = arguments
  ref = R.CyclingReference()
  body = pp.gvcf_body_native(records, blocks, ref, contigs, want_row_off=True)
  R.assert_body(body, R.reference(*arguments), n_pieces)
  return body, ref


def merged_pieces(layout):
  return pp.merge_blocks_and_variants(*M.arguments(layout)).piece_slot.size


@pytest.mark.parametrize('name', sorted(CASES))
def test_named_case(name):
  host_equals_reference(R.fill(CASES[name]), merged_pieces(CASES[name]))


@pytest.mark.parametrize('name', sorted(CHUNK_CASES))
def test_chunk_case(name):
  host_equals_reference(R.fill(CHUNK_CASES[name]), merged_pieces(CHUNK_CASES[name]))


def test_random_layouts():
  rng = np.random.default_rng(23)
  for k in range(2000):
    layout = M.random_layout(rng)
    host_equals_reference(R.fill(layout, seed=k, med_dp=('some', 'all', 'none')[k % 3]), merged_pieces(layout))


def test_a_row_shows_where_its_base_came_from():
  """[10, 20) loses [12, 15): the first piece keeps the block's N, the second reads the FASTA at 15 ('ACGT'[3])."""
  body, ref = host_equals_reference(R.fill(CASES['variant_inside_block']))
  rows = [r.split(b'\t') for r in body.text.splitlines()]
  assert [(r[1], r[3]) for r in rows if r[4] == b'<*>'] == [(b'1', b'N'), (b'11', b'N'), (b'16', b'T'), (b'26', b'N')]
  assert ref.fetches == [('c0', 15, 16)]          # one fetch, over the variant ends


@pytest.mark.parametrize('name', sorted(EDGES))
def test_number_edge(name):
  body, _ = host_equals_reference(R.edge_arguments(EDGES[name]), len(EDGES[name][1]))
  if name == 'med_dp_all_missing':
    assert b'MED_DP' not in body.text and not body.med_dp
  if name == 'med_dp_missing_among_present':
    assert [r.split(b':')[-2] for r in body.text.splitlines()] == [b'17', b'.', b'0']
  if name == 'pl_half_12.5':
    assert body.text.endswith(b':12,40,0\n')            # half to even
  if name == 'start_%d' % (10 ** 12 - 1):
    assert body.text.startswith(b'chr1\t1000000000000\t.\tN\t<*>\t0\t.\tEND=1000000000000\t')


@pytest.mark.parametrize('name', sorted(VARIANT_CASES))
def test_variant_case(name):
  body, ref = host_equals_reference(VARIANT_CASES[name])
  if name == 'variant_ends_at_the_contig_length':
    assert ref.fetches == [('chr1', 23, 24)]      # the end at the contig's length is not fetched
  else:
    assert max(len(row) for row in body.text.splitlines()) > 5000


# ---------------------------------------------------------------------------------------------- the plain entry point
def plain_call(**changes):
  """One group 'chr7': blocks [0, 10) and [10, 30), a variant [12, 15) whose end base is T.  -> gvcf_rows_native's
  arguments as a dict, with `changes` applied."""
  row = b'chr7\t13\t.\tGGG\tG,<*>\trest\n'
  a = dict(block_off=[0, 2], var_off=[0, 1], blocks=np.array([R.block(0, 10), R.block(10, 30)], R.DTYPE),
           var_start=[12], var_end=[15], var_end_base=[ord('T')], var_text_off=[0, len(row)], var_text=row,
           name_off=[0, 4], names=b'chr7')
  a.update(changes)
  return a


PLAIN = (b'chr7\t1\t.\tN\t<*>\t0\t.\tEND=10\tGT:GQ:MIN_DP:PL\t0/0:30:12:0,30,300\n'
         b'chr7\t11\t.\tN\t<*>\t0\t.\tEND=12\tGT:GQ:MIN_DP:PL\t0/0:30:12:0,30,300\n'
         b'chr7\t13\t.\tGGG\tG,<*>\trest\n'
         b'chr7\t16\t.\tT\t<*>\t0\t.\tEND=30\tGT:GQ:MIN_DP:PL\t0/0:30:12:0,30,300\n')


def test_plain_call_and_med_dp_forced():
  body = pp.gvcf_rows_native(**plain_call())
  assert body.text == PLAIN and body.n_pieces == 3 and body.row_off is None and not body.med_dp
  assert pp.gvcf_rows_native(**plain_call(med_dp=0)).text == PLAIN
  forced = pp.gvcf_rows_native(**plain_call(med_dp=1))
  assert forced.med_dp
  assert forced.text == PLAIN.replace(b'MIN_DP:PL', b'MIN_DP:MED_DP:PL').replace(b':12:0,30,300', b':12:.:0,30,300')
  # blocks that carry one, and the column switched off
  with_med = plain_call(blocks=np.array([R.block(0, 10, med_dp=4), R.block(10, 30, med_dp=-1)], R.DTYPE))
  decided = pp.gvcf_rows_native(**with_med)
  assert decided.med_dp and decided.text == pp.gvcf_rows_native(**dict(with_med, med_dp=1)).text
  assert decided.text.splitlines()[0].endswith(b'0/0:30:12:4:0,30,300')
  assert pp.gvcf_rows_native(**dict(with_med, med_dp=0)).text == PLAIN
  # the Python formatter with the same flag
  pieces = pp._piece_rows('chr7', with_med['blocks'], np.array([0, 10, 15]), np.array([10, 12, 30]), np.array([0, 1, 1]),
                          R.CyclingReference(), True)
  assert [r for r in decided.text.decode().splitlines(True) if '<*>\t0' in r] == pieces


def test_empty_calls():
  none = pp.gvcf_rows_native([0], [0], [], [], [], [], [0], b'', [0], b'', want_row_off=True)
  assert none.text == b'' and none.row_off.tolist() == [0] and none.n_pieces == 0
  one = pp.gvcf_rows_native([0, 0], [0, 0], [], [], [], [], [0], b'', [0, 3], b'chr', want_row_off=True)
  assert one.text == b'' and one.row_off.tolist() == [0]


REFUSED = {
    # what dv_gvcf_merge refuses
    'blocks_out_of_order': (dict(blocks=np.array([R.block(10, 30), R.block(0, 10)], R.DTYPE)), 'out of order or overlaps'),
    'blocks_overlap': (dict(blocks=np.array([R.block(0, 11), R.block(10, 30)], R.DTYPE)), 'out of order or overlaps'),
    'empty_block': (dict(blocks=np.array([R.block(0, 10), R.block(10, 10)], R.DTYPE)), 'block 1 is empty'),
    'empty_variant': (dict(var_end=[12]), 'variant 0 is empty'),
    'variants_out_of_order': (dict(var_off=[0, 2], var_start=[12, 11], var_end=[15, 16], var_end_base=[84, 84],
                                   var_text_off=[0, 2, 4], var_text=b'a\nb\n'), r'out of order: \(start, end\) must ascend'),
    'offsets_start_past_0': (dict(block_off=[1, 2]), 'the offsets must start at 0'),
    'offsets_descend': (dict(block_off=[0, 2, 1, 2], var_off=[0, 1, 1, 1], name_off=[0, 4, 4, 4]), 'the offsets descend at group 1'),
    # what the rows add
    'var_text_off_starts_past_0': (dict(var_text_off=[1, 25]), 'var_text_off must ascend from 0'),
    'var_text_off_descends': (dict(var_off=[0, 2], var_start=[12, 13], var_end=[15, 16], var_end_base=[84, 84],
                                   var_text_off=[0, 4, 2], var_text=b'a\nb\n'), 'var_text_off must ascend from 0'),
    'variant_row_empty': (dict(var_text_off=[0, 0]), "variant 0's row is empty or does not end in a newline"),
    'variant_row_without_newline': (dict(var_text_off=[0, 5]), "variant 0's row is empty or does not end in a newline"),
    'name_off_descends': (dict(name_off=[4, 0]), 'name_off must ascend'),
    'ref_base_space': (dict(blocks=np.array([R.block(0, 10), R.block(10, 30, base=' ')], R.DTYPE)),
                       'block 1: ref_base 0x20 is not a printable character'),
    'ref_base_del': (dict(blocks=np.array([R.block(0, 10, base='\x7f'), R.block(10, 30)], R.DTYPE)),
                     'block 0: ref_base 0x7F is not a printable character'),
    'ref_base_latin1': (dict(blocks=np.array([R.block(0, 10, base='\xe9'), R.block(10, 30)], R.DTYPE)),
                        'block 0: ref_base 0xE9 is not a printable character'),
    'used_var_end_base': (dict(var_end_base=[0]), 'variant 0: var_end_base 0x00 is not a printable character'),
    'likelihood_nan': (dict(blocks=np.array([R.block(0, 10, likelihoods=(0.0, float('nan'), -1.0)), R.block(10, 30)], R.DTYPE)),
                       'block 0: a likelihood is not finite or too large to round'),
    'likelihood_infinite': (dict(blocks=np.array([R.block(0, 10), R.block(10, 30, likelihoods=(0.0, -1.0, float('-inf')))], R.DTYPE)),
                            'block 1: a likelihood is not finite or too large to round'),
    'likelihood_past_2_53': (dict(blocks=np.array([R.block(0, 10, likelihoods=(-2.0 ** 53 / 10, 0.0, 0.0)), R.block(10, 30)], R.DTYPE)),
                             'block 0: a likelihood is not finite or too large to round'),
    'med_dp_flag': (dict(med_dp=2), 'med_dp must be -1, 0 or 1'),
}


@pytest.mark.parametrize('name', sorted(REFUSED))
def test_refused(name):
  changes, message = REFUSED[name]
  with pytest.raises(Exception, match=message):
    pp.gvcf_rows_native(**plain_call(**changes))


def test_an_unused_var_end_base_is_not_read():
  """The variant [12, 30) ends where its block ends: no piece starts there, so its base may be anything."""
  body = pp.gvcf_rows_native(**plain_call(var_end=[30], var_end_base=[0]))
  assert body.text == b''.join(PLAIN.splitlines(True)[:3])
  with pytest.raises(ValueError, match='one end, one base and one row per variant'):
    pp.gvcf_rows_native(**plain_call(var_end_base=[]))


# ---------------------------------------------------------------------------------------------- the writer
def test_by_hand_text_and_files(tmp_path):
  text = pp.gvcf_text(H.records(), H.blocks(True), H.Reference(), H.CONTIGS, 'NA12878', rows='native')
  assert text == H.HEADER % H.MED_DP_LINE + H.ROWS_WITH_MED_DP
  bare = pp.gvcf_text(H.records(), H.blocks(False), H.Reference(), H.CONTIGS, 'NA12878', rows='native')
  assert bare == H.HEADER % '' + H.without_med_dp(H.ROWS_WITH_MED_DP)
  ref = H.Reference()
  pp.gvcf_body_native(H.records(), H.blocks(True), ref, H.CONTIGS)
  assert ref.fetches == [('chr1', 100, 124)]      # the two variant ends of chr1; chr2 has no variant
  plain, zipped = str(tmp_path / 'out.g.vcf'), str(tmp_path / 'out.g.vcf.gz')
  pp.write_gvcf(plain, H.records(), H.blocks(True), H.Reference(), H.CONTIGS, 'NA12878', rows='native')
  pp.write_gvcf(zipped, H.records(), H.blocks(True), H.Reference(), H.CONTIGS, 'NA12878', rows='native')
  assert open(plain).read() == text and gzip.open(zipped, 'rt').read() == text
  assert open(zipped, 'rb').read()[4:8] == b'\x00' * 4
  again = str(tmp_path / 'python.g.vcf.gz')
  pp.write_gvcf(again, H.records(), H.blocks(True), H.Reference(), H.CONTIGS, 'NA12878')
  assert open(again, 'rb').read() == open(zipped, 'rb').read()
  with pytest.raises(ValueError, match="'python' or 'native'"):
    pp.gvcf_text(H.records(), H.blocks(True), H.Reference(), H.CONTIGS, 'NA12878', rows='fast')
  with pytest.raises(ValueError, match='not a contig'):
    pp.gvcf_text([], {'chrX': H.blocks(False)['chr2']}, H.Reference(), H.CONTIGS, 's', rows='native')


def test_command_line_with_the_switch(tmp_path, monkeypatch):
  fasta = str(tmp_path / 'ref.fa')
  genomics_io.write_fasta(fasta, [('chr1', H.CHR1), ('chr2', H.CHR2)])
  cvos = [H.cvo(H.SNP, [0], [0.001, 0.99, 0.009]), H.cvo(H.MULTI, [0], [0.02, 0.9, 0.08]),
          H.cvo(H.MULTI, [1], [0.02, 0.18, 0.8]), H.cvo(H.MULTI, [0, 1], [0.1, 0.3, 0.6]),
          H.cvo(H.make_variant('chr2', 7, 'G', ['GT'], [29, 1], [1 / 30]), [0], [0.999, 0.0006, 0.0004])]
  arrays = H.blocks(True)
  infile, spec = str(tmp_path / 'cvo.tfrecord.gz'), str(tmp_path / 'gvcf.tfrecord@1.gz')
  with tfrecord.Writer(infile) as w:
    for c in cvos:
      w.write(c)
  with core.GvcfShardWriter(spec, 0) as w:
    w.write_all(variant_calling.gvcf_record(contig, int(b['start']), int(b['end']), chr(b['ref_base']),
                                            b['likelihoods'].tolist(), int(b['gq']), int(b['min_dp']), int(b['med_dp']),
                                            bool(b['has_valid_gl']), 'NA12878')
                for contig in ('chr1', 'chr2') for b in arrays[contig])
  outputs = []
  for switch in ('0', '1'):
    monkeypatch.setenv('DV_GVCF_ROWS_NATIVE', switch)
    assert pp.gvcf_rows_switch() == ('native' if switch == '1' else 'python')
    vcf, gvcf = str(tmp_path / ('out%s.vcf' % switch)), str(tmp_path / ('out%s.g.vcf' % switch))
    assert pp.main(['--infile', infile, '--ref', fasta, '--outfile', vcf, '--nonvariant_site_tfrecord_path', spec,
                    '--gvcf_outfile', gvcf]) == 0
    outputs.append((open(vcf, 'rb').read(), open(gvcf, 'rb').read()))
  assert outputs[0] == outputs[1]
  assert outputs[0][1].count(b'<*>\t0\t.\tEND=') == 6 and outputs[0][1].count(b',<*>') == 3
  monkeypatch.delenv('DV_GVCF_ROWS_NATIVE')
  assert pp.gvcf_rows_switch() == 'python'
