"""dv_gvcf_rows_device (csrc/gvcf_rows.hip) against its host twin and the Python formatter, the
text with ==: the named cases and the number edges of tests/gvcf_rows_cases.py, row counts around the length scan's
chunk, long variant rows on both sides of a chunk edge, one large layout, the stats; and the fused route's
--gvcf_outfile on the Illumina golden fixture with DV_GVCF_ROWS_NATIVE=1."""
import numpy as np
import pytest
import torch

from deepvariant_amd import postprocess_variants as pp
from tests import gvcf_merge_cases as M
from tests import gvcf_rows_cases as R
from tests import test_hip_gvcf_merge as G

pytestmark = pytest.mark.gpu

CASES = M.named_cases()
CHUNK = pp.merge_scan_chunk()
CHUNK_CASES = M.chunk_cases(CHUNK)
EDGES = R.number_edges()
VARIANT_CASES = R.variant_cases()
SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)


def assert_stats(body, blocks, variants, want_row_off=True):
  """What dv_gvcf_rows_last_stats says of the device call that returned `body`."""
  stats = pp.last_rows_stats()
  rows = body.n_pieces + variants
  assert (stats['blocks'], stats['variants'], stats['pieces'], stats['rows']) == (blocks, variants, body.n_pieces, rows)
  assert stats['text_bytes'] == len(body.text)
  # the merge's (4 with variants, 5 with blocks); the lengths and their sum's three; with blocks the bases and the
  # piece rows; with variants their copy
  assert stats['launches'] == ((4 if variants else 0) + (7 if blocks else 0) + (1 if variants else 0) + 4
                               if blocks + variants else 0)
  if blocks + variants:
    # the header, the text and row_off -- not the bound the buffer was sized by
    assert stats['bytes_down'] == 16 + len(body.text) + (8 * rows if want_row_off else 0)
    assert stats['bytes_up'] >= 72 * blocks + 25 * variants
  else:
    assert stats['bytes_up'] == stats['bytes_down'] == 0


def device_equals_host_and_reference(arguments, n_pieces=None):
  records, blocks, contigs = arguments
  device = pp.gvcf_body_native(records, blocks, R.CyclingReference(), contigs, device=True, want_row_off=True)
  assert_stats(device, sum(len(b) for b in blocks.values()), len(records))
  host = pp.gvcf_body_native(records, blocks, R.CyclingReference(), contigs, want_row_off=True)
  assert device.text == host.text and (device.row_off == host.row_off).all()
  assert (device.med_dp, device.n_pieces) == (host.med_dp, host.n_pieces)
  R.assert_body(device, R.reference(*arguments), n_pieces)
  return device


def device_equals_host(arguments, **kwargs):
  """arguments: gvcf_rows_native's, as R.plain_arguments makes them."""
  device = pp.gvcf_rows_native(**arguments, device=True, want_row_off=True, **kwargs)
  assert_stats(device, arguments['blocks'].size, arguments['var_start'].size)
  host = pp.gvcf_rows_native(**arguments, want_row_off=True)
  assert device.text == host.text and (device.row_off == host.row_off).all()
  assert (device.med_dp, device.n_pieces) == (host.med_dp, host.n_pieces)
  return device


@pytest.mark.parametrize('name', sorted(CASES))
def test_named_case(name):
  layout = CASES[name]
  device_equals_host_and_reference(R.fill(layout), pp.merge_blocks_and_variants(*M.arguments(layout)).piece_slot.size)


@pytest.mark.parametrize('name', sorted(EDGES))
def test_number_edge(name):
  device_equals_host_and_reference(R.edge_arguments(EDGES[name]), len(EDGES[name][1]))


@pytest.mark.parametrize('name', sorted(VARIANT_CASES))
def test_variant_case(name):
  device_equals_host_and_reference(VARIANT_CASES[name])


@pytest.mark.parametrize('name', sorted(CHUNK_CASES))
def test_around_the_merge_scans_chunk(name):
  """The merge's own chunk cases, a group boundary at a chunk edge among them, carried on to the text."""
  device_equals_host(R.plain_arguments(CHUNK_CASES[name]))


@pytest.mark.parametrize('rows', SIZES)
def test_rows_around_the_length_scans_chunk(rows):
  """P + V = rows: 100 cut blocks give two pieces and a variant each."""
  layout = R.split_blocks(rows - 200, range(0, 500, 5))
  body = device_equals_host(R.plain_arguments(layout))
  assert body.row_off.size == rows + 1 and body.n_pieces == rows - 100
  reference = R.fill(layout)
  R.assert_body(pp.gvcf_body_native(reference[0], reference[1], R.CyclingReference(), reference[2], device=True,
                                    want_row_off=True), R.reference(*reference))


@pytest.mark.parametrize('blocks', SIZES)
def test_blocks_alone(blocks):
  body = device_equals_host(R.plain_arguments(R.split_blocks(blocks, [])))
  assert body.n_pieces == blocks and body.row_off.size == blocks + 1


def test_variants_alone():
  layout = [([], [(3 * j, 3 * j + 2) for j in range(CHUNK + 1)]), ([], [(5, 9)])]
  body = device_equals_host(R.plain_arguments(layout, long_row=CHUNK))
  assert body.n_pieces == 0 and body.row_off.size == CHUNK + 3


@pytest.mark.parametrize('slot', (CHUNK - 1, CHUNK))
def test_long_variant_row_at_a_chunk_edge(slot):
  """A row of 5,000 bytes in the last slot of the length scan's first chunk, and in the first slot of its second."""
  layout = R.split_blocks(CHUNK + 50, [slot - 1])            # the variant in block k takes slot k + 1
  body = device_equals_host(R.plain_arguments(layout, long_row=0))
  lengths = np.diff(body.row_off)
  assert int(np.argmax(lengths)) == slot and lengths[slot] > 5000
  assert body.text[body.row_off[slot]:body.row_off[slot] + 3] == b'v0\t'


def test_large_layout():
  body = device_equals_host(R.plain_arguments(M.large_layout()))
  assert 300000 <= body.n_pieces <= 340000 and body.row_off.size == body.n_pieces + 40001


def test_on_a_callers_stream_and_without_row_off():
  arguments = R.plain_arguments(CHUNK_CASES['both_%d' % (2 * CHUNK + 1)])
  stream = torch.cuda.Stream()
  with_off = device_equals_host(arguments, stream=stream.cuda_stream)
  without = pp.gvcf_rows_native(**arguments, device=True, stream=stream.cuda_stream)
  assert_stats(without, arguments['blocks'].size, arguments['var_start'].size, want_row_off=False)
  assert without.row_off is None and without.text == with_off.text


def test_an_empty_call_launches_nothing():
  body = pp.gvcf_rows_native([0, 0], [0, 0], [], [], [], [], [0], b'', [0, 3], b'chr', device=True, want_row_off=True)
  assert body.text == b'' and body.row_off.tolist() == [0]
  assert_stats(body, 0, 0)
  assert pp.last_rows_stats()['launches'] == 0


def test_refused_before_any_device_work():
  arguments = R.plain_arguments(CASES['variant_inside_block'])
  arguments['var_end_base'] = np.zeros(1, np.uint8)
  with pytest.raises(Exception, match='var_end_base 0x00 is not a printable character'):
    pp.gvcf_rows_native(**arguments, device=True)
  assert pp.last_rows_stats()['launches'] == 0 and pp.last_rows_stats()['bytes_up'] == 0


def test_the_merge_still_runs_its_nine_launches():
  layout = CHUNK_CASES['both_%d' % (CHUNK + 1)]
  body = device_equals_host(R.plain_arguments(layout))
  merged = pp.merge_blocks_and_variants_device(*M.arguments(layout))
  G.assert_stats(layout, merged)
  assert pp.last_merge_stats()['launches'] == 9 and merged.piece_slot.size == body.n_pieces
  assert pp.last_rows_stats()['launches'] == 16


# ---------------------------------------------------------------------------------------------- the fused route
def test_gvcf_from_the_fused_route(tmp_path, monkeypatch):
  """The Illumina golden fixture as tests/test_hip_gvcf_merge.py prepares it: DV_GVCF_ROWS_NATIVE=1 writes the default
  run's bytes, on the device and with DV_GVCF_MERGE_HOST=1 on the host."""
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
  monkeypatch.delenv('DV_GVCF_ROWS_NATIVE', raising=False)
  monkeypatch.delenv('DV_GVCF_MERGE_HOST', raising=False)
  default = str(tmp_path / 'default.g.vcf')
  stats = G._run(common + ['--gvcf_outfile', default])
  assert stats['n_vcf_records'] == 78 and stats['gvcf_merge']['launches'] == 9 and 'gvcf_rows' not in stats
  text = open(default, 'rb').read()
  n_rows = len(G._rows(default))
  monkeypatch.setenv('DV_GVCF_ROWS_NATIVE', '1')
  native = str(tmp_path / 'native.g.vcf')
  stats = G._run(common + ['--gvcf_outfile', native])
  assert open(native, 'rb').read() == text
  rows = stats['gvcf_rows']
  assert stats['gvcf_merge'] == {} and rows['rows'] == n_rows and rows['variants'] == 78
  assert (rows['blocks'], rows['launches']) == (stats['n_gvcf_blocks'], 16)
  monkeypatch.setenv('DV_GVCF_MERGE_HOST', '1')
  host = str(tmp_path / 'host.g.vcf')
  stats = G._run(common + ['--gvcf_outfile', host])
  assert open(host, 'rb').read() == text and stats['gvcf_merge'] == {} and stats['gvcf_rows'] == {}
