"""dv_pack_draws_device (csrc/pack_regions.hip, pack_draws_kernel: one wave per draw) against the per-read rule
transcribed in plain Python, on the batch of tests/pack_draw_cases.py: draws of exactly 0, 1, 63, 64, 65, 255, 256
and 257 rows, several masks over the same rows, 32 alts with mask bit 31, a candidate without support, reads under
two alts, ghost keys, one read name in two regions, and alt draws whose keys come through two src_row hops."""
import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import packing
from tests import pack_draw_cases as DC

pytestmark = pytest.mark.gpu

_NAMES = ('item_variant_start', 'item_image_start', 'item_ref_idx', 'item_list_off', 'item_height', 'item_out_off',
          'item_mean_coverage', 'item_candidate', 'item_combo', 'list_read', 'list_code', 'list_group')


def _device(b, use_groups, stream=None, **kw):
  """-> (downloaded arrays, what fill_batch says, stats)."""
  packed = DC.call(b, stream=stream, **kw)
  stats = packing.pack_draws_stats()
  try:
    got = packed.download()
    c = _lib.DvBatch()
    c.memory = _lib.DV_MEM_DEVICE
    packed.fill_batch(c, use_groups)
    filled = dict(n_items=c.n_items, n_list=c.n_list, max_list_len=c.max_list_len, has_groups=bool(c.list_group),
                  blank=c.item_blank_mask, has_lists=bool(c.list_read), has_coverage=bool(c.item_mean_coverage))
  finally:
    packed.close()
  return got, filled, stats


def _assert_same(got, want, what):
  for name in _NAMES:
    assert got[name].dtype == want[name].dtype, (what, name)
    np.testing.assert_array_equal(got[name], want[name], err_msg='%s: %s' % (what, name))
  assert got['max_list_len'] == want['max_list_len'], what


@pytest.mark.parametrize('use_groups', [0, 1])
def test_the_batch_equals_the_transcription(use_groups):
  b, want = DC.batch(), DC.expected()
  got, filled, stats = _device(b, use_groups)
  _assert_same(got, want, 'batch')
  n_items, n_list = len(b.draws), int(b.draws['n_rows'].sum())
  assert n_items > 50 and n_list > 5000
  assert filled == dict(n_items=n_items, n_list=n_list, max_list_len=257, has_groups=bool(use_groups), blank=None,
                        has_lists=True, has_coverage=True)
  # the stats add up
  assert stats == dict(draws=n_items, candidates=len(b.cands), list_entries=n_list, launches=1)


def test_identical_bytes_twice_and_on_a_callers_stream():
  import torch
  b = DC.batch()
  first, _, _ = _device(b, 1)
  second, _, _ = _device(b, 1)
  stream = torch.cuda.Stream()
  with torch.cuda.stream(stream):
    busy = torch.ones(1 << 24, device='cuda')
    for _ in range(8):
      busy = busy * 1.0001                       # work queued in front of the call on the caller's stream
    third, _, stats = _device(b, 1, stream=stream.cuda_stream)
  assert stats['launches'] == 1
  for name in _NAMES:
    assert first[name].tobytes() == second[name].tobytes() == third[name].tobytes(), name
  _assert_same(third, DC.expected(), 'caller stream')


def test_rows_as_their_own_keys():
  """rows_key NULL: every row is its own key and a support entry names a row of the concatenated table -- here the
  FIRST row that carries the key, so the other copies of a read (its alt copies, a second row with its key) read as
  unsupported."""
  b = DC.batch()
  first_row = {}
  for row, key in enumerate(b.rows_key.tolist()):
    first_row.setdefault(key, row)
  support_key = np.array([first_row.get(k, DC.NO_KEY) for k in b.support_key.tolist()], np.int32)
  want = DC.transcription(None, b.draws, b.n_alts, b.first_support, b.n_support, support_key, b.support_alt)
  assert (want['list_code'] != DC.expected()['list_code']).sum() > 500          # the alt draws and later copies differ
  got, _, _ = _device(b, 1, rows_key=None, support_key=support_key)
  _assert_same(got, want, 'rows as keys')


def test_draws_without_rows_and_a_single_draw():
  b = DC.batch()
  empty = b.draws[b.draws['n_rows'] == 0]
  assert len(empty) >= 1
  got, filled, stats = _device(b, 1, draws=empty)
  assert filled['n_items'] == len(empty) and filled['n_list'] == 0 and stats['launches'] == 1
  np.testing.assert_array_equal(got['item_list_off'], np.zeros(len(empty) + 1, np.uint32))
  np.testing.assert_array_equal(got['item_out_off'], empty['out_off'])
  one = b.draws[b.draws['n_rows'] == 257][:1]
  want = DC.transcription(b.rows_key, one, b.n_alts, b.first_support, b.n_support, b.support_key, b.support_alt)
  got, _, _ = _device(b, 1, draws=one)
  _assert_same(got, want, 'one draw')
