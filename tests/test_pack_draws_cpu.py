"""dv_pack_draws_device's host side -- its argument checks, which come back before any device work, the limits, the
empty call -- the cases its GPU tests run (tests/pack_draw_cases.py) against the name-string functions the per-region
route uses (packing.support_codes / allele_groups), and the source rows trim_table remembers.  No GPU needed."""
import ctypes as C
import types

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from tests import pack_draw_cases as DC


class _Args:
  """The C call's arguments for the shared batch, each replaceable."""

  def __init__(self):
    b = DC.batch()
    self.rows_key = b.rows_key.copy()
    self.n_rows = b.n_rows
    self.draws = b.draws.copy()
    self.n_draws = len(b.draws)
    self.cands = np.zeros(len(b.n_alts), packing._CAND_DTYPE)                 # pylint: disable=protected-access
    self.cands['n_alts'], self.cands['first_support'], self.cands['n_support'] = b.n_alts, b.first_support, b.n_support
    self.n_cands = len(self.cands)
    self.support_key, self.support_alt = b.support_key.copy(), b.support_alt.copy()
    self.n_support = len(self.support_key)
    self.null = set()

  def call(self, out=True):
    ptr = lambda name: None if name in self.null else getattr(self, name).ctypes.data       # noqa: E731
    handle = C.c_void_p(1)
    status = _lib.lib().dv_pack_draws_device(
        ptr('rows_key'), self.n_rows, ptr('draws'), self.n_draws, ptr('cands'), self.n_cands, ptr('support_key'),
        ptr('support_alt'), self.n_support, None, C.byref(handle) if out else None)
    return status, handle


def _set(arr, index, name, value):
  arr[name][index] = value


@pytest.mark.parametrize('name,edit', [
    ('null draws', lambda a: a.null.add('draws')),
    ('null cands', lambda a: a.null.add('cands')),
    ('null support_key', lambda a: a.null.add('support_key')),
    ('null support_alt', lambda a: a.null.add('support_alt')),
    ('negative n_rows', lambda a: setattr(a, 'n_rows', -1)),
    ('negative n_draws', lambda a: setattr(a, 'n_draws', -1)),
    ('negative n_cands', lambda a: setattr(a, 'n_cands', -1)),
    ('rows past the table', lambda a: _set(a.draws, len(a.draws) - 1, 'n_rows', a.draws['n_rows'][-1] + 1)),
    ('negative first row', lambda a: _set(a.draws, 3, 'row_first', -1)),
    ('negative row count', lambda a: _set(a.draws, 3, 'n_rows', -1)),
    ('a table shorter than the draws', lambda a: setattr(a, 'n_rows', a.n_rows - 1)),
    ('candidate below cands', lambda a: _set(a.draws, 5, 'cand', -1)),
    ('candidate past cands', lambda a: _set(a.draws, 5, 'cand', a.n_cands)),
    ('height 0', lambda a: _set(a.draws, 7, 'height', 0)),
    ('support outside its arrays', lambda a: _set(a.cands, 2, 'first_support', a.n_support)),
    ('support past its arrays', lambda a: _set(a.cands, a.n_cands - 1, 'n_support', a.cands['n_support'][-1] + 1)),
    ('n_alts > 32', lambda a: _set(a.cands, 0, 'n_alts', 33)),
    ('negative n_alts', lambda a: _set(a.cands, 0, 'n_alts', -1)),
    ('support_alt >= n_alts', lambda a: a.support_alt.__setitem__(int(a.cands['first_support'][1]), 40)),
    ('a mask bit at n_alts', lambda a: _set(a.draws, 0, 'combo_mask', 1 << int(a.cands['n_alts'][a.draws['cand'][0]]))),
    ('mask bit 31 of a narrow candidate', lambda a: _set(a.draws, 0, 'combo_mask', 1 << 31)),
])
def test_argument_errors_come_back_before_device_work(name, edit):
  args = _Args()
  edit(args)
  status, handle = args.call()
  assert status == _lib.DV_ERR_INVALID_ARGUMENT, (name, status, _lib.last_error())
  assert handle.value is None, name                  # *out is NULL
  assert 'dv_pack_draws_device' in _lib.last_error()


def test_null_out_and_null_stats_are_refused():
  status, _ = _Args().call(out=False)
  assert status == _lib.DV_ERR_INVALID_ARGUMENT
  assert _lib.lib().dv_pack_draws_device_last_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT


def test_the_limits_are_decided_on_the_host():
  """More than 2^31 - 1 draws, and more than 2^32 - 1 list entries: DV_ERR_BAD_INPUT before anything is read or
  launched (the counts alone decide; three draws over a table of 2^31 - 1 rows that are their own keys)."""
  args = _Args()
  args.n_draws = 1 << 31
  status, handle = args.call()
  assert status == _lib.DV_ERR_BAD_INPUT and handle.value is None and '2^31' in _lib.last_error()
  args = _Args()
  big = (1 << 31) - 1
  args.draws = args.draws[:3].copy()
  args.draws['row_first'], args.draws['n_rows'] = 0, big
  args.n_draws, args.n_rows = 3, big
  args.null.add('rows_key')
  status, handle = args.call()
  assert status == _lib.DV_ERR_BAD_INPUT and handle.value is None and '2^32' in _lib.last_error()


def test_no_draw_needs_no_device_and_anything_else_does():
  lib = _lib.lib()
  args = _Args()
  args.n_draws = 0
  args.null.add('draws')
  status, handle = args.call()
  assert status == _lib.DV_OK, _lib.last_error()
  try:
    view = _lib.DvPackedRegionsView()
    _lib.check(lib.dv_packed_regions_download(handle, C.byref(view)))
    assert (view.n_items, view.n_list, view.max_list_len) == (0, 0, 0)
    assert C.cast(view.item_list_off, C.POINTER(C.c_uint32))[0] == 0
    assert lib.dv_packed_regions_items(handle, None, None) == 0
    b = _lib.DvBatch()
    b.memory = _lib.DV_MEM_DEVICE
    _lib.check(lib.dv_packed_regions_fill_batch(handle, 1, C.byref(b)))
    assert (b.n_items, b.n_list, b.max_list_len) == (0, 0, 0)
    assert packing.pack_draws_stats() == dict(draws=0, candidates=args.n_cands, list_entries=0, launches=0)
  finally:
    lib.dv_packed_regions_free(handle)
  # everything NULL and zero is the same empty call
  handle = C.c_void_p(1)
  assert lib.dv_pack_draws_device(None, 0, None, 0, None, 0, None, None, 0, None, C.byref(handle)) == _lib.DV_OK
  lib.dv_packed_regions_free(handle)
  if lib.dv_device_count() == 0:
    status, handle = _Args().call()
    assert status == _lib.DV_ERR_NO_DEVICE and handle.value is None
    # a draw without rows is still an item: it needs the device too
    args = _Args()
    args.draws = args.draws[:1].copy()
    args.draws['n_rows'] = 0
    args.n_draws = 1
    status, handle = args.call()
    assert status == _lib.DV_ERR_NO_DEVICE and handle.value is None


def _calls(b):
  """The batch's candidates as DeepVariantCalls, support by name."""
  calls = []
  for c in b.cands:
    support = {}
    for key, alt in c.support:
      support.setdefault(c.alts[alt], T.SupportingReads()).read_names.append(key)
    calls.append(T.DeepVariantCall(variant=T.Variant('chr1', 10, 11, 'A', list(c.alts)), allele_support=support))
  return calls


def test_the_transcription_is_what_the_name_strings_give():
  """Per draw, list_code / list_group of the integer transcription equal packing.support_codes / allele_groups on
  the rows' key STRINGS (traced through src_row, twice for the alt segment) and the call's read names."""
  b, want = DC.batch(), DC.expected()
  calls = _calls(b)
  off = want['item_list_off'].astype(np.int64)
  n_codes = 0
  for d, draw in enumerate(b.draws):
    c = b.cands[int(draw['cand'])]
    rows = range(int(draw['row_first']), int(draw['row_first']) + int(draw['n_rows']))
    names = [DC.key_string(b, r) for r in rows]
    assert all(region == c.region for _, region in names)          # a draw lists rows of its own region only
    table = types.SimpleNamespace(keys=[key for key, _ in names])
    combo = [alt for i, alt in enumerate(c.alts) if (int(draw['combo_mask']) >> i) & 1]
    idx = np.arange(len(names))
    np.testing.assert_array_equal(want['list_code'][off[d]:off[d + 1]], packing.support_codes(calls[int(draw['cand'])], combo, table, idx))
    np.testing.assert_array_equal(want['list_group'][off[d]:off[d + 1]], packing.allele_groups(calls[int(draw['cand'])], table, idx))
    np.testing.assert_array_equal(want['list_read'][off[d]:off[d + 1]], np.arange(rows.start, rows.stop))
    n_codes += len(names)
  assert n_codes == len(want['list_code']) > 5000


def test_the_cases_contain_what_they_promise():
  b, want = DC.batch(), DC.expected()
  sizes = b.draws['n_rows'].tolist()
  for size in DC.SIZES:
    assert sizes.count(size) >= 1, size
  assert want['max_list_len'] == 257 and b.n_trimmed > 1000 and b.n_rows - b.n_trimmed > 400
  assert len({k for c in b.cands for k in [c.region]}) == 3
  # draws over the same rows with different masks
  same = {}
  for d in b.draws:
    same.setdefault((int(d['row_first']), int(d['n_rows']), int(d['cand'])), set()).add(int(d['combo_mask']))
  assert sum(1 for masks in same.values() if len(masks) >= 2) >= 8
  # 32 alts and bit 31; a candidate without support; ghosts
  wide = [i for i, c in enumerate(b.cands) if len(c.alts) == 32]
  assert len(wide) == 1 and any(int(d['combo_mask']) >> 31 for d in b.draws if int(d['cand']) == wide[0])
  assert sum(1 for c in b.cands if not c.support) == 1
  assert sum(1 for c in b.cands for key, _ in c.support if key == DC.GHOST) >= 10 and (b.support_key == DC.NO_KEY).sum() >= 10
  # reads under two alts, the larger alt first in list order: first_alt != group, seen in the output
  larger_first = 0
  for c in b.cands:
    seen = {}
    for key, alt in c.support:
      if key in seen and alt < seen[key]:
        larger_first += 1
      seen.setdefault(key, alt)
  assert larger_first >= 5
  assert (want['list_code'] > 0).sum() > 1000
  off = want['item_list_off'].astype(np.int64)
  both = 0
  for d, draw in enumerate(b.draws):
    c = int(draw['cand'])
    lo, n = int(b.first_support[c]), int(b.n_support[c])
    by_key = {}
    for key, alt in zip(b.support_key[lo:lo + n].tolist(), b.support_alt[lo:lo + n].tolist()):
      by_key.setdefault(key, set()).add(alt)
    rows = want['list_read'][off[d]:off[d + 1]]
    both += sum(1 for r in rows.tolist() if len(by_key.get(int(b.rows_key[r]), ())) >= 2)
  assert both >= 50
  # the same name in two regions, supporting alt 0 in one and alt 1 in the other, and drawn in both
  where = [(k, keys.index(DC.SHARED)) for k, keys in enumerate(b.region_keys) if DC.SHARED in keys]
  assert [k for k, _ in where] == [0, 1]
  shared_alts = {c.region: alt for c in b.cands for key, alt in c.support if key == DC.SHARED}
  assert shared_alts == {0: 0, 1: 1}
  # alt draws: rows of the alt segment, keys through two hops
  alt_draws = [d for d in b.draws if int(d['row_first']) >= b.n_trimmed and int(d['n_rows'])]
  assert len(alt_draws) >= 10 and len(b.draws) - b.n_examples == len(alt_draws)
  assert all(int(d['out_off']) >= b.n_examples * DC.EXAMPLE_BYTES for d in alt_draws)
  for d in alt_draws[:3]:
    row = int(d['row_first'])
    assert b.rows_key[row] == b.rows_key[int(b.alt_src[row - b.n_trimmed])]


def test_a_key_that_leaks_across_regions_changes_a_code():
  """Row keys left unshifted while the support keys are shifted (or the other way round): the shared read's code
  changes in the region behind the first, so the cases tell a region offset applied on one side only."""
  b, want = DC.batch(), DC.expected()
  leaky = DC.build(shift_rows=False)
  np.testing.assert_array_equal(leaky.support_key, b.support_key)
  got = DC.transcription(leaky.rows_key, leaky.draws, leaky.n_alts, leaky.first_support, leaky.n_support,
                         leaky.support_key, leaky.support_alt)
  changed = np.nonzero(got['list_code'] != want['list_code'])[0]
  assert len(changed) > 100
  regions = {DC.key_string(b, int(want['list_read'][i]))[1] for i in changed.tolist()}
  assert regions == {1, 2}                          # region 0's offset is 0
  shared_rows = [i for i in changed.tolist() if DC.key_string(b, int(want['list_read'][i]))[0] == DC.SHARED]
  assert shared_rows


def _table(keys, positions, lengths):
  n = len(keys)
  z = np.zeros(n, np.int32)
  seq_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
  ranks = np.argsort(np.argsort(keys)).astype(np.uint32)
  pos = np.asarray(positions, np.int32)
  return packing.ReadTable(
      n_reads=n, read_pos=pos, read_sort_pos=None, read_seq_off=seq_off,
      read_cigar_off=np.arange(n + 1, dtype=np.uint32), read_mapq=np.full(n, 60, np.uint8), read_flags=z.astype(np.uint8),
      read_frag_len=z, read_hp=z, read_name_rank=ranks, read_aux=None, bases=np.full(int(seq_off[-1]), 65, np.uint8),
      quals=np.full(int(seq_off[-1]), 30, np.uint8), mod_5mc=None, mod_6ma=None,
      cigar=(np.asarray(lengths, np.uint32) << 4) | 1, keys=list(keys), read_end=pos.astype(np.int64) + np.asarray(lengths))


def test_trim_table_remembers_the_source_rows():
  """src_row of trim_table(device=False) names the rows whose keys the trimmed rows carry; the integer keys copied
  through it group the trimmed rows as their key strings do; a table of any other origin remembers nothing."""
  from deepvariant_amd import alt_aligned_pileup_lib as A
  rng = np.random.default_rng(4)
  n = 60
  keys = ['f%d/%d' % (i // 2, i % 2) for i in range(n)]
  keys[31] = keys[5]                                # two rows, one key
  positions = np.sort(rng.integers(0, 400, size=n))
  table = _table(keys, positions, rng.integers(40, 120, size=n))
  assert packing.table_src_rows(table) is None
  windows = [(95, 106, 70, 131, 15), (205, 212, 175, 236, 15), (95, 106, 70, 131, 61)]
  trimmed, ranges = A.trim_table(table, windows, device=False)
  src = packing.table_src_rows(trimmed)
  assert src is not None and src.dtype == np.int32 and len(src) == trimmed.n_reads > 20
  assert [keys[r] for r in src.tolist()] == trimmed.keys
  assert ranges[0][1] > ranges[0][0] and ranges[2][1] - ranges[2][0] < ranges[0][1] - ranges[0][0]
  for lo, hi in ranges:
    assert np.all(np.diff(src[lo:hi]) > 0)          # a window's copies keep the table's order
  copied = packing.copy_row_keys(trimmed, packing._row_keys(table))           # pylint: disable=protected-access
  ids = {}
  by_name = np.array([ids.setdefault(k, len(ids)) for k in keys], np.int32)
  np.testing.assert_array_equal(copied, by_name[src])
  assert 'src_row' not in {f.name for f in __import__('dataclasses').fields(trimmed)}
  with pytest.raises(ValueError, match='source rows'):
    packing.copy_row_keys(table, by_name)


def test_the_wrapper_refuses_arrays_that_do_not_fit():
  b = DC.batch()
  with pytest.raises(ValueError, match='one entry per row'):
    DC.call(b, rows_key=b.rows_key[:-1])
  with pytest.raises(ValueError, match='differ in length'):
    DC.call(b, support_alt=b.support_alt[:-1])
  assert packing.DRAW_DTYPE.itemsize == C.sizeof(_lib.DvPackDraw) == 48
  for name in packing.DRAW_DTYPE.names:
    assert packing.DRAW_DTYPE.fields[name][1] == getattr(_lib.DvPackDraw, name).offset, name
