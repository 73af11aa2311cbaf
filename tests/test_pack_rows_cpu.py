"""The device packer's host side (dv_pack_regions_device's argument checks, packing.table_key_ids,
packing.support_arrays, DeepVariantCall.support_rows) and the cases its GPU tests run (tests/pack_cases.py).
No GPU needed: every argument error comes back before any device work."""
import ctypes as C

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from tests import pack_cases as PC


def _small():
  return PC.DeviceInputs([PC.pile_region(), PC.no_candidates_region()])


def _refused(inputs, out=True):
  handle = C.c_void_p(1)
  status = _lib.lib().dv_pack_regions_device(
      inputs.n_regions, inputs.slices, C.byref(inputs.rows) if inputs.rows is not None else None,
      C.byref(inputs.opt) if inputs.opt is not None else None, inputs.cands, inputs.masks.ctypes.data,
      inputs.support_key.ctypes.data, inputs.support_alt.ctypes.data, None, C.byref(handle) if out else None)
  assert status == _lib.DV_ERR_INVALID_ARGUMENT, (status, _lib.last_error())
  if out:
    assert handle.value is None          # *out is NULL


def _set(obj, name, value):
  setattr(obj, name, value)


@pytest.mark.parametrize('name,edit', [
    ('null rows', lambda i: _set(i, 'rows', None)),
    ('null options', lambda i: _set(i, 'opt', None)),
    ('negative n_regions', lambda i: _set(i, 'n_regions', -1)),
    ('negative n_reads', lambda i: _set(i.rows, 'n_reads', -1)),
    ('negative n_candidates', lambda i: _set(i.opt, 'n_candidates', -1)),
    ('null read_pos', lambda i: _set(i.rows, 'read_pos', None)),
    ('null read_end', lambda i: _set(i.rows, 'read_end', None)),
    ('rows outside the table', lambda i: _set(i.slices[1], 'n_reads', i.slices[1].n_reads + 1)),
    ('negative first row', lambda i: _set(i.slices[0], 'read_first', -1)),
    ('candidates outside cands', lambda i: _set(i.slices[1], 'n_cands', 1)),
    ('candidate slices with a gap', lambda i: _set(i.slices[1], 'cand_first', i.slices[1].cand_first + 1)),
    ('candidates not covered', lambda i: _set(i.opt, 'n_candidates', i.opt.n_candidates + 1)),
    ('combinations outside combo_masks', lambda i: _set(i.cands[1], 'n_combos', 1000)),
    ('support outside its arrays', lambda i: _set(i.cands[2], 'first_support', i.opt.n_support)),
    ('n_alts > 32', lambda i: _set(i.cands[0], 'n_alts', 33)),
    ('negative n_alts', lambda i: _set(i.cands[0], 'n_alts', -1)),
    ('support_alt >= n_alts', lambda i: i.support_alt.__setitem__(0, 9)),
    ('width < 3', lambda i: _set(i.opt, 'width', 2)),
    ('pileup_height <= 0', lambda i: _set(i.opt, 'pileup_height', 0)),
])
def test_argument_errors_come_back_before_device_work(name, edit):
  inputs = _small()
  edit(inputs)
  _refused(inputs)


def test_null_out_and_null_arrays_are_refused():
  _refused(_small(), out=False)
  handle = C.c_void_p(1)
  i = _small()
  for missing in ('cands', 'masks', 'support_key', 'support_alt'):
    args = dict(cands=i.cands, masks=i.masks.ctypes.data, support_key=i.support_key.ctypes.data,
                support_alt=i.support_alt.ctypes.data)
    args[missing] = None
    status = _lib.lib().dv_pack_regions_device(i.n_regions, i.slices, C.byref(i.rows), C.byref(i.opt), args['cands'],
                                               args['masks'], args['support_key'], args['support_alt'], None,
                                               C.byref(handle))
    assert status == _lib.DV_ERR_INVALID_ARGUMENT and handle.value is None, missing
  assert _lib.lib().dv_packed_regions_fill_batch(None, 0, None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert _lib.lib().dv_packed_regions_download(None, None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert _lib.lib().dv_pack_regions_device_last_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT


def test_nothing_to_draw_needs_no_device_and_the_rest_does():
  """No candidate with a reference window: DV_OK and an empty handle whatever the machine; otherwise a machine
  without a device answers DV_ERR_NO_DEVICE (there is no host fallback)."""
  lib = _lib.lib()
  region = PC.pile_region()
  for cand in region.candidates:
    cand.window = False
  inputs = PC.DeviceInputs([region, PC.no_candidates_region()])
  status, handle = inputs.call()
  assert status == _lib.DV_OK, _lib.last_error()
  try:
    view = _lib.DvPackedRegionsView()
    _lib.check(lib.dv_packed_regions_download(handle, C.byref(view)))
    assert (view.n_items, view.n_list, view.max_list_len) == (0, 0, 0)
    assert C.cast(view.item_list_off, C.POINTER(C.c_uint32))[0] == 0
    assert lib.dv_packed_regions_items(handle, None, None) == 0
    b = _lib.DvBatch()
    b.memory = _lib.DV_MEM_HOST
    assert lib.dv_packed_regions_fill_batch(handle, 0, C.byref(b)) == _lib.DV_ERR_INVALID_ARGUMENT   # device batches only
    b.memory = _lib.DV_MEM_DEVICE
    _lib.check(lib.dv_packed_regions_fill_batch(handle, 0, C.byref(b)))
    assert (b.n_items, b.n_list, b.max_list_len) == (0, 0, 0)
    stats = packing.pack_device_stats()
    assert stats == dict(regions=2, candidates=4, items=0, list_entries=0, regions_unsorted=0, launches=0)
  finally:
    lib.dv_packed_regions_free(handle)
  if lib.dv_device_count() == 0:
    status, handle = _small().call()
    assert status == _lib.DV_ERR_NO_DEVICE and handle.value is None


def _table(keys):
  n = len(keys)
  z = np.zeros(n, np.int32)
  return packing.ReadTable(
      n_reads=n, read_pos=z, read_sort_pos=None, read_seq_off=np.zeros(n + 1, np.uint32),
      read_cigar_off=np.zeros(n + 1, np.uint32), read_mapq=z.astype(np.uint8), read_flags=z.astype(np.uint8),
      read_frag_len=z, read_hp=z, read_name_rank=z.astype(np.uint32), read_aux=None, bases=np.zeros(0, np.uint8),
      quals=np.zeros(0, np.uint8), mod_5mc=None, mod_6ma=None, cigar=np.zeros(0, np.uint32), keys=list(keys),
      read_end=z.astype(np.int64))


def test_table_key_ids_group_rows_as_their_key_strings_do():
  from deepvariant_amd import allelecounter
  region = PC.generator_region(5, shuffle=True)
  table = _table(region.keys)
  ids = packing.table_key_ids(table)
  assert ids.dtype == np.int32 and len(ids) == table.n_reads
  keys = table.keys
  same_id = ids[:, None] == ids[None, :]
  same_key = np.array(keys)[:, None] == np.array(keys)[None, :]
  assert np.array_equal(same_id, same_key) and same_key.sum() > table.n_reads       # keys are shared
  assert np.array_equal(ids, allelecounter.AlleleCounter._read_key_ids(keys))       # pylint: disable=protected-access
  assert packing.table_key_ids(table) is ids                                          # cached on the table
  distinct = _table(PC.pile_region().keys)
  assert packing.table_key_ids(distinct) is None
  assert allelecounter.AlleleCounter._read_key_ids(distinct.keys) is None            # pylint: disable=protected-access


def _calls(region):
  calls = []
  for cand in region.candidates:
    alts = ['ACGTACGTACGTACGTACGTACGTACGTACGT'[:k + 1] + 'T' for k in range(cand.n_alts)]
    support = {}
    for key, alt in cand.support:
      support.setdefault(alts[alt], T.SupportingReads()).read_names.append(key)
    support['NOT_AN_ALT'] = T.SupportingReads([PC.GHOST])
    calls.append(T.DeepVariantCall(variant=T.Variant('chr1', cand.start, cand.end, 'A', alts), allele_support=support))
  return calls


@pytest.mark.parametrize('make', [lambda: PC.generator_region(5, shuffle=False), PC.pile_region, PC.edges_region])
def test_support_arrays_from_names_keep_each_keys_alts(make):
  """Per candidate and key the same (min alt, max alt) -- first_alt and group -- as the name lists give."""
  region = make()
  table = _table(region.keys)
  calls = _calls(region)
  first, count, support_key, support_alt = packing.support_arrays(table, calls)
  assert first.dtype == np.uint32 and support_key.dtype == np.int32 and support_alt.dtype == np.uint8
  row_key = packing.table_key_ids(table)
  if row_key is None:
    row_key = np.arange(table.n_reads)
  key_of = dict(zip(table.keys, row_key.tolist()))
  n_multi = 0
  for cand, f, n in zip(region.candidates, first.tolist(), count.tolist()):
    want, got = {}, {}
    for key, alt in cand.support:
      if key in key_of:                       # a ghost matches no row
        lo, hi = want.get(key_of[key], (alt, alt))
        want[key_of[key]] = (min(lo, alt), max(hi, alt))
    for key, alt in zip(support_key[f:f + n].tolist(), support_alt[f:f + n].tolist()):
      if key == packing.NO_SUCH_KEY:
        continue
      lo, hi = got.get(key, (alt, alt))
      got[key] = (min(lo, alt), max(hi, alt))
    assert n == len(cand.support) and got == want
    n_multi += sum(lo != hi for lo, hi in want.values())
  assert n_multi > 10
  # ... and rows instead of names give the same entries
  a_row = {key: row for row, key in reversed(list(enumerate(table.keys)))}
  for call in calls:
    call.support_rows = {allele: np.array([a_row.get(name, 0) for name in s.read_names], np.int64)
                         for allele, s in call.allele_support.items()}
  by_rows = packing.support_arrays(table, calls)
  known = support_key != packing.NO_SUCH_KEY
  assert np.array_equal(by_rows[2][known], support_key[known]) and np.array_equal(by_rows[3], support_alt)


def test_support_rows_is_no_part_of_a_calls_value():
  a = T.DeepVariantCall(variant=T.Variant('chr1', 1, 2, 'A', ['C']))
  b = T.DeepVariantCall(variant=T.Variant('chr1', 1, 2, 'A', ['C']), support_rows={'C': np.array([1])})
  assert a.support_rows is None and a == b and 'support_rows' not in repr(b)


def test_the_cases_contain_what_they_promise():
  regions = PC.batch()
  by_name = {r.name: r for r in regions}
  assert [r.name for r in regions] == ['generator-sorted', 'empty', 'generator-shuffled', 'no-candidates', 'pile', 'edges']
  gen = by_name['generator-sorted']
  assert gen.sorted and not by_name['generator-shuffled'].sorted
  for r in (gen, by_name['generator-shuffled']):
    assert r.n_reads == 700 and len(set(r.names)) <= 300 and len(set(r.keys)) < 700 and len(r.candidates) == 60
    starts = [c.start for c in r.candidates]
    assert len(set(starts)) < 60                                       # duplicates
    assert 2 <= sum(not c.window for c in r.candidates) <= 12          # candidates without a reference window
    assert {c.n_alts for c in r.candidates} == {1, 2, 3}
    assert all(any(k == PC.GHOST for k, _ in c.support) for c in r.candidates)
    # reads listed under several alts that the candidate picks: first_alt != group
    keys = r.keys
    multi = 0
    for c in r.candidates:
      alts_of = {}
      for k, a in c.support:
        alts_of.setdefault(k, set()).add(a)
      multi += sum(len(alts_of.get(keys[row], ())) > 1 for row in r.picked(c).tolist())
    assert multi > 200
  # the sorted region's long read: picked by candidates whose bound, without the largest span, starts behind it
  far = [c for c in gen.candidates if 1000 < c.start < 2900]
  assert len(far) > 20 and all(0 in gen.picked(c).tolist() for c in far)
  assert int((gen.read_end - gen.read_pos)[1:].max()) < 400
  pile = by_name['pile']
  assert pile.n_reads == 1100 and len(set(pile.read_pos.tolist())) == 1
  assert sorted(len(pile.picked(c)) for c in pile.candidates)[-1] == 1100
  edges = by_name['edges']
  sizes = sorted(len(edges.picked(c)) for c in edges.candidates)
  assert sizes == sorted(PC.EDGE_SIZES + (65,))
  wide = [c for c in edges.candidates if c.n_alts == 32]
  assert len(wide) == 1 and any(m >> 31 for m in wide[0].masks) and any(a == 31 for _, a in wide[0].support)
  assert by_name['empty'].n_reads == 0 and len(by_name['empty'].candidates) == 1
  assert by_name['no-candidates'].n_reads == 50 and not by_name['no-candidates'].candidates
  # the checker agrees with the contract's predicate on list lengths, and sees a candidate with an empty list
  host = PC.host_pack(edges, use_groups=True)
  lengths = np.diff(host['item_list_off'].astype(np.int64))
  assert set(lengths.tolist()) == set(PC.EDGE_SIZES) and host['max_list_len'] == 1025
  assert len(PC.host_pack(by_name['empty'], use_groups=False)['item_height']) == 1


def test_the_switch_is_read_at_each_call(monkeypatch):
  monkeypatch.delenv('DV_PACK_DEVICE', raising=False)
  assert not packing.pack_device_enabled()
  monkeypatch.setenv('DV_PACK_DEVICE', '0')
  assert not packing.pack_device_enabled()
  monkeypatch.setenv('DV_PACK_DEVICE', '1')
  assert packing.pack_device_enabled()
