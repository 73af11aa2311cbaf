"""dv_bgzf_compress_device and dv_gvcf_rows_bgzf_device (csrc/bgzf.hip, csrc/gvcf_rows.hip)
against their host twins, the file with ==: the named texts of tests/bgzf_cases.py from host and from device memory,
block counts around the offset scan's chunk, a caller's stream, the stats, the rows compressed behind the merge, and the
fused route's --gvcf_outfile on the Illumina golden fixture with DV_BGZF=1."""
import gzip

import numpy as np
import pytest
import torch

from deepvariant_amd import postprocess_variants as pp
from tests import bgzf_cases as Z
from tests import gvcf_merge_cases as M
from tests import gvcf_rows_cases as R
from tests import test_hip_gvcf_merge as G
from tests import test_hip_gvcf_rows as HR

pytestmark = pytest.mark.gpu

TEXTS = Z.named_texts()
CHUNK = pp.merge_scan_chunk()
CASES = M.named_cases()
CHUNK_CASES = M.chunk_cases(CHUNK)
PREFIX = b'##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\n'


def assert_stats(text_bytes, got, from_host):
  """What dv_bgzf_last_stats says of the device call that returned `got`."""
  stats = pp.last_bgzf_stats()
  blocks = got.block_coff.size - 1
  assert (stats['text_bytes'], stats['file_bytes'], stats['blocks']) == (text_bytes, len(got.data), blocks)
  assert stats['stored_blocks'] == got.stored_blocks
  if text_bytes == 0:
    assert stats['launches'] == stats['bytes_up'] == stats['bytes_down'] == 0
    return
  assert stats['launches'] == 5                 # the blocks, the offsets' three, the copy
  assert stats['bytes_down'] == 16 + len(got.data) + 8 * (blocks + 1)
  assert 0 < stats['bytes_up'] - (text_bytes if from_host else 0) < 4096        # the CRC tables


def device_equals_host(text, **kwargs):
  host = pp.bgzf_file(text)
  device = pp.bgzf_file(text, device=True, **kwargs)
  assert_stats(len(text), device, True)
  assert device.data == host.data and (device.block_coff == host.block_coff).all()
  assert device.stored_blocks == host.stored_blocks
  return device


@pytest.mark.parametrize('name', sorted(TEXTS))
def test_named_text(name):
  text = TEXTS[name]
  host = device_equals_host(text)
  # the same from device memory, at an address that is no multiple of four as well
  for lead in (0, 1):
    whole = torch.frombuffer(bytearray(b'?' * lead + text + b'!'), dtype=torch.uint8).cuda()
    tensor = whole[lead:lead + len(text)]
    assert len(text) == 0 or tensor.data_ptr() % 4 == lead
    got = pp.bgzf_file(tensor, device=True)
    assert_stats(len(text), got, False)
    assert got.data == host.data and (got.block_coff == host.block_coff).all()


@pytest.mark.parametrize('blocks', (1, 2, 255, 256, 257, CHUNK + 1))
def test_block_counts(blocks):
  text = Z.block_counts_text(blocks)
  got = device_equals_host(text)
  assert got.block_coff.size == blocks + 1 and gzip.decompress(got.data) == text


def test_on_a_callers_stream():
  stream = torch.cuda.Stream()
  text = TEXTS['gvcf_2049_rows']
  device_equals_host(text, stream=stream.cuda_stream)
  with torch.cuda.stream(stream):
    tensor = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    doubled = torch.cat([tensor, tensor])       # written on the stream the compressor reads it on
  got = pp.bgzf_file(doubled, device=True, stream=stream.cuda_stream)
  assert got.data == pp.bgzf_compress(text + text)


def test_an_empty_text_launches_nothing():
  got = pp.bgzf_file(b'', device=True)
  assert got.data == Z.EOF and got.block_coff.tolist() == [0]
  assert_stats(0, got, True)


# ---------------------------------------------------------------------------------------------- the rows, compressed
def rows_device_equals_host(arguments, med_dp=1):
  host = pp.gvcf_rows_bgzf_native(PREFIX, **arguments, med_dp=med_dp, want_row_off=True)
  device = pp.gvcf_rows_bgzf_native(PREFIX, **arguments, med_dp=med_dp, want_row_off=True, device=True)
  assert device.file.data == host.file.data and (device.file.block_coff == host.file.block_coff).all()
  assert (device.row_off == host.row_off).all()
  assert (device.text_bytes, device.n_rows, device.n_pieces) == (host.text_bytes, host.n_rows, host.n_pieces)
  assert_stats(host.text_bytes, device.file, False)
  rows, blocks, variants = pp.last_rows_stats(), arguments['blocks'].size, arguments['var_start'].size
  assert (rows['blocks'], rows['variants'], rows['rows'], rows['text_bytes']) == (blocks, variants, host.n_rows, host.text_bytes)
  if blocks + variants:
    # the text stays where it is: the header and row_off alone come back from the rows
    assert rows['bytes_down'] == 16 + 8 * host.n_rows
  return device


@pytest.mark.parametrize('name', sorted(CASES))
def test_rows_of_a_named_case(name):
  arguments = R.plain_arguments(CASES[name])
  for med_dp in (0, 1):
    got = rows_device_equals_host(arguments, med_dp)
    assert gzip.decompress(got.file.data) == PREFIX + pp.gvcf_rows_native(**arguments, med_dp=med_dp).text


@pytest.mark.parametrize('name', sorted(CHUNK_CASES))
def test_rows_around_the_merge_scans_chunk(name):
  rows_device_equals_host(R.plain_arguments(CHUNK_CASES[name]))


def test_rows_with_a_long_variant_row():
  arguments = R.plain_arguments(R.split_blocks(CHUNK + 50, [CHUNK - 2]), long_row=0)
  got = rows_device_equals_host(arguments)
  assert np.diff(got.row_off).max() > 5000


def test_rows_of_the_large_layout_and_the_plain_rows_after_it():
  arguments = R.plain_arguments(M.large_layout())
  got = rows_device_equals_host(arguments)
  assert 300000 <= got.n_pieces <= 340000 and got.file.block_coff.size > 100
  # dv_gvcf_rows_device straight after: its own launches and bytes, the text downloaded as before
  HR.device_equals_host(R.plain_arguments(CHUNK_CASES['both_%d' % (CHUNK + 1)]))
  assert pp.last_rows_stats()['launches'] == 16


def test_rows_without_records_compress_the_prefix():
  got = pp.gvcf_rows_bgzf_native(PREFIX, [0, 0], [0, 0], [], [], [], [], [0], b'', [0, 3], b'chr', med_dp=0,
                                 want_row_off=True, device=True)
  assert got.file.data == pp.bgzf_compress(PREFIX) and got.row_off.tolist() == [len(PREFIX)]
  assert pp.last_rows_stats()['launches'] == 0 and pp.last_bgzf_stats()['launches'] == 5


# ---------------------------------------------------------------------------------------------- the fused route
def test_gvcf_gz_from_the_fused_route(tmp_path, monkeypatch):
  """The Illumina golden fixture as tests/test_hip_gvcf_merge.py prepares it: with DV_BGZF=1 every route writes a
  .g.vcf.gz that decompresses to the default run's text, and the device's file is the host's."""
  from deepvariant_amd import dv_types as T
  from deepvariant_amd import genomics_io
  from tests import realigner_fixture as RF
  ref, sets = RF.load()
  stretch_start = 9_995_000
  fasta = str(tmp_path / 'ref.fa.gz')
  genomics_io.write_fasta(fasta, [('chr20', 'N' * stretch_start + ref.get_bases('chr20', stretch_start, 10_100_600))])
  bam = str(tmp_path / 'reads.bam')
  genomics_io.write_bam(bam, [('chr20', 10_100_600)], sets['wgs'], sample_name='NA12878')
  common = ['--ref', fasta, '--reads', bam, '--regions', 'chr20:10,000,000-10,010,000', '--sample_name', 'NA12878',
            '--channel_list', ','.join(T.PILEUP_CHANNELS_WITH_INSERT_SIZE), '--checkpoint', 'random:7']
  for name in ('DV_BGZF', 'DV_GVCF_ROWS_NATIVE', 'DV_GVCF_MERGE_HOST'):
    monkeypatch.delenv(name, raising=False)
  default = str(tmp_path / 'default.g.vcf')
  stats = G._run(common + ['--gvcf_outfile', default])            # pylint: disable=protected-access
  assert 'gvcf_bgzf' not in stats
  text = open(default, 'rb').read()
  files = {}
  for native in (False, True):
    for host in (False, True):
      monkeypatch.setenv('DV_BGZF', '1')
      monkeypatch.setenv('DV_GVCF_ROWS_NATIVE', '1' if native else '0')
      monkeypatch.setenv('DV_GVCF_MERGE_HOST', '1' if host else '0')
      path = str(tmp_path / ('native%d_host%d.g.vcf.gz' % (native, host)))
      stats = G._run(common + ['--gvcf_outfile', path])           # pylint: disable=protected-access
      files[native, host] = open(path, 'rb').read()
      assert gzip.decompress(files[native, host]) == text
      if native and not host:
        bgzf = stats['gvcf_bgzf']
        assert (bgzf['text_bytes'], bgzf['file_bytes'], bgzf['launches']) == (len(text), len(files[native, host]), 5)
        assert stats['gvcf_rows']['launches'] == 16 and stats['gvcf_rows']['bytes_down'] == 16
      else:
        assert stats['gvcf_bgzf'] == {}
  assert len(set(files.values())) == 1 and files[True, False] == pp.bgzf_compress(text)
