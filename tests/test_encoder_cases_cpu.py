"""The inputs of tests/encoder_cases.py are what they claim to be -- proven with the oracle alone, so that a machine
without a GPU verifies that the cases of tests/test_hip_encoder_paths.py reach the code they are meant for: exact CIGAR
operation counts, operations past the 64th and 128th that draw inside the window, wide windows filled (indel anchors
included) beyond columns 256 and 512 with reads across the pass boundaries, and in every case a read the site gate
rejects next to one it accepts."""
import numpy as np
import pytest

from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from tests import encoder_cases as E
from tests import fuzz_inputs as F


def _image(case, reads, built):
  from oracle import oracle as O
  call, ref, _, start, combo = built
  return O.build_pileup(case.options(), call, ref, reads, start, combo, pileup_height=case.height,
                        mean_coverage=case.mean_coverage, channels_to_blank=case.blank_enums())


def _all_cases():
  return [c for w in E.BOUNDARY_WIDTHS for c in E.boundary_cases(w)] + \
         [c for w in E.PASS_WIDTHS for c in E.pass_cases(w)] + \
         [E.padded_case(n, ch, w) for n, ch in (('c7', T.PILEUP_CHANNELS_WITH_INSERT_SIZE), ('c16', E.CHANNELS_16),
                                                ('c6', T.PILEUP_DEFAULT_CHANNELS)) for w in (61, 221)]


def test_exact_operation_counts_and_placement():
  rng = np.random.default_rng(7)
  seen = set()
  for n in E.OP_COUNTS + (1, 2):
    at = [(int(rng.integers(0, n)), int(rng.integers(0, 61))) for _ in range(6)]
    reads = E.reads_with_ops(rng, 61, n, n_reads=6, image_start=970, at=at)
    table = packing.ReadTable.from_reads(reads)
    np.testing.assert_array_equal(np.diff(table.read_cigar_off.astype(np.int64)), n)
    for r, (idx, col) in zip(reads, at):
      cig = r.alignment.cigar
      kinds = [c.operation for c in cig]
      assert all(a != b for a, b in zip(kinds, kinds[1:])), 'neighbouring operations of one kind could be merged'
      assert all(1 <= c.operation_length <= 4 for c in cig)
      assert r.alignment.position.position + E.ref_offset(cig, idx) == 970 + col
      assert len(r.aligned_sequence) == F.query_len(cig) >= 1
      assert max(r.aligned_quality) <= 59
      seen.update(kinds)
  assert seen == set(range(1, 10)), 'not all nine operation kinds are drawn'


@pytest.mark.parametrize('case', _all_cases(), ids=lambda c: c.name)
def test_case_conditions(case):
  from oracle import oracle as O
  built = case.build()
  call, ref, reads, start, combo = built
  opts = case.options()
  assert [len(r.alignment.cigar) for r in reads] == list(case.ops)
  table = packing.ReadTable.from_reads(reads)
  batch = packing.PackedBatch(table=table, width=case.width)
  batch.add_item(call.variant.start, start, batch.add_ref_window(ref), np.arange(len(reads), dtype=np.uint32),
                 np.zeros(len(reads), np.uint8), height=case.height, out_off=0)
  assert batch.size_hints() == (case.max_ops, case.height)
  # the site gate: reads 0 and 1 pass the mapping-quality gate (60); only the base at the variant column differs
  assert reads[0].alignment.mapping_quality == reads[1].alignment.mapping_quality == 60 >= E.MIN_MAPQ
  assert O.encode_read(opts, call, ref, reads[0], start, combo) is None, 'read 0 passes the site gate'
  assert O.encode_read(opts, call, ref, reads[1], start, combo) is not None, 'read 1 fails the site gate'
  full = _image(case, reads, built)
  band = opts.reference_band_height
  assert full[band:].any()
  # operations past the first (and second) chunk of 64 draw inside the window
  for chunk_end in (64, 128):
    if case.max_ops > chunk_end:
      assert not np.array_equal(_image(case, E.cut_reads(reads, chunk_end), built), full), \
          'nothing past operation %d is drawn' % chunk_end
  # wide windows: pixels and indel anchors in the later column passes, a read across every pass boundary
  rows = full[band:]
  strand = case.channels.index('strand')
  for edge in (256, 512):
    if case.width > edge:
      assert rows[:, edge:].any(), 'no read pixel in columns >= %d' % edge
      anchors = (rows[:, edge:, 0] == 0) & (rows[:, edge:, strand] != 0)    # '*' has no base colour
      assert anchors.any(), 'no indel anchor in columns >= %d' % edge
      assert (rows[:, edge - 1].any(axis=-1) & rows[:, edge].any(axis=-1)).any(), \
          'no read row spans columns %d | %d' % (edge - 1, edge)


def test_mixed_batch_has_items_of_both_routes():
  from oracle import oracle as O
  opts, batch = E.mixed_batch()
  assert batch.size_hints() == (200, E.MIXED_HEIGHT)
  n_ops = np.diff(batch.table.read_cigar_off.astype(np.int64))
  off = np.asarray(batch.item_list_off)
  longest = [int(n_ops[batch.list_read[off[i]:off[i + 1]]].max()) for i in range(batch.n_items)]
  assert all(n <= 16 for n in longest[0::2]) and all(n > 16 for n in longest[1::2])
  assert {32, 33, 64, 65} <= set(int(n) for n in n_ops)
  shared = set(batch.list_read[off[0]:off[1]].tolist()) & set(batch.list_read[off[1]:off[2]].tolist())
  assert shared, 'neighbouring items share no read'
  assert (np.diff(off) > E.MIXED_HEIGHT - opts.reference_band_height).any(), 'no item deeper than the image'
  out, rows = O.encode_packed(opts, batch, 7)
  assert (rows > 0).all() and (rows < np.diff(off)).any()
  img = out.reshape(batch.n_items, E.MIXED_HEIGHT, E.MIXED_WIDTH, 7)
  assert all(img[i, opts.reference_band_height:].any() for i in range(batch.n_items))


def test_gpu_shapes_stay_below_48_kib_of_lds():
  """Every shape tests/test_hip_encoder_paths.py launches, by dv_encode_batch's own formula; the refused shape is far
  above the 64 KiB limit."""
  sizes = {}
  for c in _all_cases():
    oc = len(c.channels)
    sizes[c.name] = E.lds_bytes(c.width, oc, oc, c.height, c.options().reference_band_height, c.max_ops)
  for name, channels, oc in E.PADDED:
    for w in E.padded_widths(oc):
      sizes['%s_%d_w%d' % (name, oc, w)] = E.lds_bytes(w, oc, len(channels), 20, 5, 70)
  for cache in (8, 16, 32, 64):
    sizes['mixed_cache%d' % cache] = E.lds_bytes(E.MIXED_WIDTH, 7, 7, E.MIXED_HEIGHT, 5, cig_cache=cache)
  worst = max(sizes, key=sizes.get)
  print('largest LDS request: %d bytes (%s)' % (sizes[worst], worst))
  assert sizes[worst] < 48 * 1024
  # the knob run with tables for 256 kept reads (DV_CIG_CACHE=32 with DV_CIG_KEPT_MAX) is the one larger request
  kept_max = E.lds_bytes(E.MIXED_WIDTH, 7, 7, E.MIXED_HEIGHT, 5, cig_cache=32, kept_cap=256)
  print('with DV_CIG_CACHE=32 and DV_CIG_KEPT_MAX: %d bytes' % kept_max)
  assert kept_max < 64 * 1024
  assert E.lds_bytes(2049, 64, 7, 100, 5) > 64 * 1024
  # DV_CIG_CACHE=64 with DV_CIG_KEPT_MAX asks for 64 words x 256 reads: the cache alone is 64 KiB
  assert E.lds_bytes(E.MIXED_WIDTH, 7, 7, E.MIXED_HEIGHT, 5, cig_cache=64, kept_cap=256) > 64 * 1024
