"""dv_bgzf_compress and dv_gvcf_rows_bgzf (csrc/bgzf.hip, csrc/gvcf_rows.hip), the host code:
the file with == against the plain-Python restatement of tests/bgzf_cases.py on the named texts and on 500 seeded ones,
every member inflated alone, the refused arguments, and DV_BGZF=1 through write_vcf, write_gvcf and the command line."""
import ctypes as C
import gzip
import io
import zlib

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import postprocess_variants as pp
from tests import bgzf_cases as Z
from tests import gvcf_rows_cases as R
from tests import test_gvcf_text_cpu as G

TEXTS = Z.named_texts()


def check_file(text, got):
  """got: a BgzfFile of `text`.  Everything the format asks of it, without the restatement."""
  assert gzip.decompress(got.data) == text              # Python checks every member's CRC-32 and ISIZE
  members = Z.members(got.data)
  assert len(members) == (len(text) + Z.B - 1) // Z.B + 1 == got.block_coff.size
  assert [at for at, _ in members] == got.block_coff.tolist()
  for k, (_, member) in enumerate(members[:-1]):
    assert len(member) <= 65536
    assert zlib.decompress(member[18:-8], -15) == text[k * Z.B:(k + 1) * Z.B]
  assert members[-1][1] == Z.EOF == got.data[-28:]
  assert got.stored_blocks == sum((member[18] & 6) == 0 for _, member in members[:-1])


def matches(text):
  return [t for at in range(0, len(text), Z.B) for t in Z.tokens_of_block(text[at:at + Z.B]) if not isinstance(t, int)]


def test_the_parameters():
  assert set(Z.PARAMS) == {'block', 'tile', 'seg', 'hash_bits'}
  assert 0 < Z.TILE <= Z.SEG <= Z.B and Z.B + 5 + 26 <= 65536 and 8 <= Z.HASH_BITS <= 16


def test_the_restatement_reads_zlibs_streams_back():
  """The restatement's own tables: what it writes, zlib inflates."""
  for name in ('every_byte_twice', 'one_letter', 'gvcf_by_hand', 'distance_257', 'noise_2000'):
    assert gzip.decompress(Z.restated(TEXTS[name])[0]) == TEXTS[name]


@pytest.mark.parametrize('name', sorted(TEXTS))
def test_named_text(name):
  text = TEXTS[name]
  got = pp.bgzf_file(text)
  want, coff, stored = Z.restated(text)
  assert got.data == want and got.block_coff.tolist() == coff and got.stored_blocks == stored
  check_file(text, got)


def test_what_the_named_texts_exercise():
  """The texts do what their names say, by the restatement's tokens."""
  assert len(TEXTS['row_400_times']) == 32000 and len(pp.bgzf_compress(TEXTS['row_400_times'])) * 8 < 32000
  noise = pp.bgzf_file(TEXTS['noise_2000'])
  assert noise.stored_blocks == 1 and len(noise.data) == 2000 + 5 + 26 + 28
  assert matches(TEXTS['repeat_of_3']) == [] and matches(TEXTS['repeat_of_4']) == [(4, 100)]
  assert matches(TEXTS['same_tile']) == []
  for name in TEXTS:
    if name.startswith('distance_'):
      assert (40, int(name[9:])) in matches(TEXTS[name]), name
  assert all(d == 1 for _, d in matches(TEXTS['one_letter'])) and len(matches(TEXTS['one_letter'])) >= Z.B // Z.SEG
  cap = min(258, Z.SEG)
  assert [n for n, _ in matches(TEXTS['stretch_of_300_twice'])][:2] == [cap, min(cap, 300 - cap)]
  assert sum(n for n, _ in matches(TEXTS['every_byte_twice'])) == 256


def test_500_seeded_texts():
  longest = 0
  for seed in range(500):
    text = Z.seeded_text(seed)
    got = pp.bgzf_file(text)
    assert got.data == Z.restated(text)[0], seed
    check_file(text, got)
    longest = max(longest, len(text))
  assert longest > 2 * Z.B


def test_refused_arguments():
  l = _lib.lib()
  handle = C.c_void_p(1)
  text = C.cast(C.c_char_p(b'abc'), C.c_void_p)
  assert l.dv_bgzf_compress(text, -1, C.byref(handle)) == _lib.DV_ERR_INVALID_ARGUMENT and handle.value is None
  assert l.dv_bgzf_compress(None, 3, C.byref(handle)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_bgzf_compress(text, 3, None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_bgzf_compress_device(text, _lib.DV_MEM_HOST, -1, C.byref(handle), None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_bgzf_compress_device(None, _lib.DV_MEM_HOST, 3, C.byref(handle), None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_bgzf_compress_device(text, _lib.DV_MEM_HOST, 3, None, None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_bgzf_compress_device(text, 7, 3, C.byref(handle), None) == _lib.DV_ERR_INVALID_ARGUMENT
  for call in (l.dv_bgzf_params, l.dv_bgzf_last_stats):
    assert call(None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_bgzf_arrays(None, None) == _lib.DV_ERR_INVALID_ARGUMENT
  l.dv_bgzf_free(None)
  # an empty text needs no device, whichever entry point takes it
  assert pp.bgzf_compress(b'') == pp.bgzf_compress(b'', device=True) == Z.EOF
  stats = pp.last_bgzf_stats()
  assert stats['launches'] == 0 and stats['file_bytes'] == 28 and stats['bytes_up'] == stats['bytes_down'] == 0


# ---------------------------------------------------------------------------------------------- the rows, compressed
def rows_arguments():
  layout = R.split_blocks(300, range(0, 120, 7))
  return R.plain_arguments(layout)


def test_rows_bgzf_is_the_compressed_header_and_body():
  arguments = rows_arguments()
  prefix = b'##fileformat=VCFv4.2\n#CHROM\tPOS\n'
  for med_dp in (0, 1):
    body = pp.gvcf_rows_native(**arguments, med_dp=med_dp, want_row_off=True)
    got = pp.gvcf_rows_bgzf_native(prefix, **arguments, med_dp=med_dp, want_row_off=True)
    assert got.file.data == pp.bgzf_compress(prefix + body.text)
    assert (got.row_off == body.row_off + len(prefix)).all()
    assert (got.text_bytes, got.n_rows, got.n_pieces) == (len(prefix) + len(body.text), body.row_off.size - 1, body.n_pieces)
    check_file(prefix + body.text, got.file)
  without = pp.gvcf_rows_bgzf_native(b'', **arguments, med_dp=0)
  assert without.row_off is None and gzip.decompress(without.file.data) == pp.gvcf_rows_native(**arguments, med_dp=0).text
  empty = pp.gvcf_rows_bgzf_native(prefix, [0, 0], [0, 0], [], [], [], [], [0], b'', [0, 3], b'chr', med_dp=0,
                                   want_row_off=True)
  assert gzip.decompress(empty.file.data) == prefix and empty.row_off.tolist() == [len(prefix)] and empty.n_rows == 0


def test_rows_bgzf_refuses_what_the_rows_refuse():
  arguments = rows_arguments()
  with pytest.raises(_lib.DvError, match='med_dp must be 0 or 1'):
    pp.gvcf_rows_bgzf_native(b'x', **arguments, med_dp=-1)
  bad = dict(arguments, var_end_base=np.zeros_like(arguments['var_end_base']))
  with pytest.raises(_lib.DvError, match='var_end_base 0x00 is not a printable character'):
    pp.gvcf_rows_bgzf_native(b'x', **bad, med_dp=0)
  l = _lib.lib()
  arg, _alive = pp._rows_input(**arguments, med_dp=0, want_row_off=False)   # pylint: disable=protected-access
  handle, meta = C.c_void_p(1), _lib.DvGvcfRowsMeta()
  assert l.dv_gvcf_rows_bgzf(C.byref(arg), None, -1, C.byref(meta), C.byref(handle)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert handle.value is None
  assert l.dv_gvcf_rows_bgzf(C.byref(arg), None, 3, C.byref(meta), C.byref(handle)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_gvcf_rows_bgzf(C.byref(arg), None, 0, None, C.byref(handle)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_gvcf_rows_bgzf(C.byref(arg), None, 0, C.byref(meta), None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_gvcf_rows_bgzf(None, None, 0, C.byref(meta), C.byref(handle)) == _lib.DV_ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------- the switch
def test_the_switch_writes_bgzf_and_nothing_else_changes(tmp_path, monkeypatch):
  records, contigs = G.records(), G.CONTIGS

  def write(tag):
    names = [str(tmp_path / (tag + end)) for end in ('.vcf', '.vcf.gz', '.g.vcf', '.g.vcf.gz', '.native.g.vcf.gz')]
    pp.write_vcf(names[0], records, contigs, 'NA12878')
    pp.write_vcf(names[1], records, contigs, 'NA12878')
    pp.write_gvcf(names[2], records, G.blocks(True), G.Reference(), contigs, 'NA12878')
    pp.write_gvcf(names[3], records, G.blocks(True), G.Reference(), contigs, 'NA12878')
    pp.write_gvcf(names[4], records, G.blocks(True), G.Reference(), contigs, 'NA12878', rows='native')
    return [open(name, 'rb').read() for name in names]

  monkeypatch.delenv('DV_BGZF', raising=False)
  off = write('off')
  # the parent's bytes: one gzip stream without a time stamp
  for plain, zipped in ((off[0], off[1]), (off[2], off[3]), (off[2], off[4])):
    stream = io.BytesIO()
    with gzip.GzipFile(filename='', fileobj=stream, mode='wb', mtime=0) as z:
      z.write(plain)
    assert zipped == stream.getvalue() and zipped[3] & 4 == 0            # no extra field: not BGZF
  assert off[2] == (G.HEADER % G.MED_DP_LINE + G.ROWS_WITH_MED_DP).encode()
  monkeypatch.setenv('DV_BGZF', '1')
  on = write('on')
  assert (on[0], on[2]) == (off[0], off[2])                     # a name without .gz is unaffected
  for plain, zipped in ((on[0], on[1]), (on[2], on[3]), (on[2], on[4])):
    assert zipped == pp.bgzf_compress(plain)
    check_file(plain, pp.BgzfFile(zipped, np.array([at for at, _ in Z.members(zipped)]),
                                  sum((m[18] & 6) == 0 for _, m in Z.members(zipped)[:-1])))
  monkeypatch.setenv('DV_BGZF', '0')
  assert write('zero') == off


def test_the_command_line_with_the_switch(tmp_path, monkeypatch):
  from deepvariant_amd import genomics_io, tfrecord
  from deepvariant_amd import make_examples_core as core
  from deepvariant_amd import variant_calling
  fasta = str(tmp_path / 'ref.fa')
  genomics_io.write_fasta(fasta, [('chr1', G.CHR1), ('chr2', G.CHR2)])
  infile, spec = str(tmp_path / 'cvo.tfrecord.gz'), str(tmp_path / 'gvcf.tfrecord@1.gz')
  with tfrecord.Writer(infile) as w:
    w.write(G.cvo(G.SNP, [0], [0.001, 0.99, 0.009]))
  arrays = G.blocks(True)
  with core.GvcfShardWriter(spec, 0) as w:
    w.write_all(variant_calling.gvcf_record(contig, int(b['start']), int(b['end']), chr(b['ref_base']),
                                            b['likelihoods'].tolist(), int(b['gq']), int(b['min_dp']), int(b['med_dp']),
                                            bool(b['has_valid_gl']), 'NA12878')
                for contig in ('chr1', 'chr2') for b in arrays[contig])

  def run(tag, end):
    vcf, gvcf = str(tmp_path / (tag + '.vcf' + end)), str(tmp_path / (tag + '.g.vcf' + end))
    assert pp.main(['--infile', infile, '--ref', fasta, '--outfile', vcf, '--nonvariant_site_tfrecord_path', spec,
                    '--gvcf_outfile', gvcf]) == 0
    return open(vcf, 'rb').read(), open(gvcf, 'rb').read()

  monkeypatch.delenv('DV_BGZF', raising=False)
  monkeypatch.delenv('DV_GVCF_ROWS_NATIVE', raising=False)
  monkeypatch.delenv('DV_GVCF_MERGE_DEVICE', raising=False)
  plain = run('plain', '')
  gz = run('gz', '.gz')
  assert [gzip.decompress(data) for data in gz] == list(plain) and all(data[3] == 0 for data in gz)
  monkeypatch.setenv('DV_BGZF', '1')
  bgzf = run('bgzf', '.gz')
  assert list(bgzf) == [pp.bgzf_compress(data) for data in plain]
  monkeypatch.setenv('DV_GVCF_ROWS_NATIVE', '1')
  assert run('native', '.gz') == bgzf
