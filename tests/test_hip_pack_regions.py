"""dv_pack_regions_device (csrc/pack_regions.hip: count, scan, emit) against its checker dv_pack_region: the
downloaded device arrays equal the host's, array for array and region by region -- keys rendered as strings for
the host, offsets and rows shifted for the batch -- on the cases of tests/pack_cases.py: shared keys, reads
listed under several alts, a ghost key, shuffled and sorted rows, a 1,100-read pile, lists of exactly 0, 1, 63, 64,
65, 255, 256, 257, 1,024 and 1,025 reads, 32 alts with mask bit 31, an empty region and one without candidates."""
import ctypes as C

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import packing
from tests import pack_cases as PC

pytestmark = pytest.mark.gpu

_NAMES = ('item_variant_start', 'item_image_start', 'item_ref_idx', 'item_list_off', 'item_height', 'item_out_off',
          'item_candidate', 'item_combo', 'list_read', 'list_code')


def _device(regions, use_groups, stream=None, with_keys=True, mean_coverage=0.0):
  """-> (downloaded arrays, what fill_batch says, stats)."""
  inputs = PC.DeviceInputs(regions, mean_coverage=mean_coverage, with_keys=with_keys)
  status, handle = inputs.call(stream)
  assert status == _lib.DV_OK, _lib.last_error()
  stats = packing.pack_device_stats()
  packed = packing.PackedRegions(handle, 0, [], [])
  try:
    got = packed.download()
    b = _lib.DvBatch()
    b.memory = _lib.DV_MEM_DEVICE
    packed.fill_batch(b, use_groups)
    filled = dict(n_items=b.n_items, n_list=b.n_list, max_list_len=b.max_list_len, has_groups=bool(b.list_group),
                  blank=b.item_blank_mask, has_lists=bool(b.list_read))
  finally:
    packed.close()
  return got, filled, stats


def _assert_same(got, want, use_groups, what):
  for name in _NAMES + (('list_group',) if use_groups else ()):
    assert got[name].dtype == want[name].dtype, (what, name)
    np.testing.assert_array_equal(got[name], want[name], err_msg='%s: %s' % (what, name))
  assert got['max_list_len'] == want['max_list_len'], what


_WANT = {}


def _want(use_groups):
  if use_groups not in _WANT:
    _WANT[use_groups] = PC.expected(PC.batch(), use_groups)
  return _WANT[use_groups]


@pytest.mark.parametrize('use_groups', [0, 1])
def test_the_batch_equals_the_host_packer(use_groups):
  regions = PC.batch()
  want = _want(use_groups)
  got, filled, stats = _device(regions, use_groups, mean_coverage=3.5)
  _assert_same(got, want, use_groups, 'batch')
  n_items, n_list = len(want['item_height']), len(want['list_read'])
  assert n_items > 300 and n_list > 30000
  assert np.array_equal(got['item_mean_coverage'], np.full(n_items, 3.5, np.float32))
  assert filled == dict(n_items=n_items, n_list=n_list, max_list_len=1100, has_groups=bool(use_groups), blank=None,
                        has_lists=True)
  # the stats add up
  assert stats == dict(regions=len(regions), candidates=sum(len(r.candidates) for r in regions), items=n_items,
                       list_entries=n_list, regions_unsorted=1, launches=3)


@pytest.mark.parametrize('k', range(6))
def test_each_region_alone_equals_the_host_packer(k):
  region = PC.batch()[k]
  want = PC.expected([region], use_groups=True)
  got, filled, stats = _device([region], 1)
  _assert_same(got, want, True, region.name)
  n_items = len(want['item_height'])
  assert filled['n_items'] == n_items and stats['launches'] == (3 if n_items else 0)
  assert stats['regions_unsorted'] == int(not region.sorted and bool(region.candidates))


def test_identical_bytes_twice_and_on_a_callers_stream():
  import torch
  regions = PC.batch()
  first, _, _ = _device(regions, 1)
  second, _, _ = _device(regions, 1)
  stream = torch.cuda.Stream()
  with torch.cuda.stream(stream):
    busy = torch.ones(1 << 24, device='cuda')
    for _ in range(8):
      busy = busy * 1.0001                       # work queued in front of the call on the caller's stream
    third, _, stats = _device(regions, 1, stream=stream.cuda_stream)
  assert stats['launches'] == 3
  for name in _NAMES + ('list_group', 'item_mean_coverage'):
    assert first[name].tobytes() == second[name].tobytes() == third[name].tobytes(), name
  _assert_same(third, _want(1), True, 'caller stream')


def test_rows_as_their_own_keys():
  """read_key NULL: every row is its own key, and support entries name rows of the concatenated table."""
  regions = [PC.pile_region(), PC.no_candidates_region(), PC.edges_region()]
  want = PC.expected(regions, use_groups=True)
  got, _, _ = _device(regions, 1, with_keys=False)
  _assert_same(got, want, True, 'rows as keys')


def test_the_golden_slice_gives_84_items():
  """packing.pack_regions_device (names resolved through one dict per table: these calls carry no rows) against
  packing.pack_region_native on the golden HG001 slice, whole and split into two regions' candidates."""
  from deepvariant_amd import dv_types as T
  from deepvariant_amd import make_examples_native as men
  from tests import golden_io
  from tests.golden.make_golden import wgs_options
  from tests.test_oracle_golden import FIXTURE
  from tests.test_hip_pipeline import _WindowRef
  reads, examples, _ = golden_io.load(FIXTURE)
  pic = wgs_options()
  cands, seen = [], set()
  for ex in examples:
    key = (ex['call'].variant.start, tuple(ex['call'].variant.alternate_bases))
    if key not in seen:
      seen.add(key)
      cands.append(ex['call'])
  ref = _WindowRef(examples, pic.width)
  table = packing.ReadTable.from_reads(reads)
  windows = [men.get_reference_bases_for_pileup(ref, c.variant, pic.width) for c in cands]
  combos = [list(men.alt_allele_combinations(c, pic.multi_allelic_mode)) if w else [] for c, w in zip(cands, windows)]
  example_bytes = 100 * pic.width * len(pic.channels)
  host, host_plan = packing.pack_region_native(table, cands, combos, windows, pic.width, pic.read_overlap_buffer_bp, 100,
                                               example_bytes, use_groups=True)
  assert host.n_items == 84
  half = len(cands) // 2
  for split in ([cands], [cands[:half], cands[half:]]):
    tables = [table] * len(split)
    at, wins, cmbs = 0, [], []
    for part in split:
      wins.append(windows[at:at + len(part)])
      cmbs.append(combos[at:at + len(part)])
      at += len(part)
    packed, plan = packing.pack_regions_device(tables, split, cmbs, wins, pic.width, pic.read_overlap_buffer_bp, 100,
                                               example_bytes)
    try:
      got = packed.download()
    finally:
      packed.close()
    assert packed.n_items == 84 and len(got['item_height']) == 84
    base = [0, half]
    assert [(base[k] + ci, combo) for k, ci, combo in plan] == host_plan
    assert packed.ref_windows_list == host.ref_windows_list
    # rows of the second region's copy of the table are shifted by the first's rows
    rows = got['list_read'].astype(np.int64)
    if len(split) == 2:
      first_items = sum(1 for k, _, _ in plan if k == 0)
      cut = int(got['item_list_off'][first_items])
      assert rows[cut:].min() >= table.n_reads
      rows[cut:] -= table.n_reads
    np.testing.assert_array_equal(rows, host.list_read)
    for name in ('item_variant_start', 'item_image_start', 'item_ref_idx', 'item_list_off', 'item_height', 'item_out_off',
                 'list_code', 'list_group'):
      np.testing.assert_array_equal(got[name], getattr(host, name), err_msg=name)
