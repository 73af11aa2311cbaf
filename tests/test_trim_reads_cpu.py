"""Window trimming on a packed read table, host side (no GPU): the closed form csrc/trim_reads.hip states, the
host entry point dv_trim_reads_batch and alt_aligned_pileup_lib.trim_table(device=False) against
alt_aligned_pileup_lib.trim_reads on Read objects -- the restatement of TrimReads
(deepvariant/alt_aligned_pileup_lib.cc:231-248) that the reference's own vectors pin in
tests/test_alt_aligned_pileup_lib_cpu.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import alt_aligned_pileup_lib as A
from deepvariant_amd import packing
from tests import trim_cases as TC


@pytest.mark.parametrize('name', TC.CASE_NAMES)
def test_closed_form_equals_trim_reads(name):
  want, objects, _ = TC.reference(name)
  TC.assert_same_arrays(TC.closed_form(name), want, name)
  assert len(objects) == len(want['src_row'])


def test_cases_cover_what_they_claim():
  """The hand-made windows do produce the situations they are there for."""
  t = TC.table('hand')
  want, _, _ = TC.reference('hand')
  cigars = [want['cigar'][want['cigar_off'][k]:want['cigar_off'][k + 1]].tolist() for k in range(len(want['src_row']))]
  rows = lambda w: range(want['window_row_off'][w], want['window_row_off'][w + 1])   # noqa: E731
  word = lambda op, ln: (ln << 4) | op                                               # noqa: E731
  # window 7 = [990, 1020): 20M 3I 20M ends at the boundary: the I stays and a zero-length M closes the CIGAR
  ins = [k for k in rows(7) if want['src_row'][k] == 1]
  assert [cigars[k] for k in ins] == [[word(TC.M, 20), word(TC.I, 3), word(TC.M, 0)]]
  # window 3 = [1020, 1081) starts where that I sits: it is kept whole, after 20 trimmed read bases
  ins = [k for k in rows(3) if want['src_row'][k] == 1]
  assert [cigars[k] for k in ins] == [[word(TC.I, 3), word(TC.M, 20)]] and want['read_trim'][ins[0]] == 20
  # overlap 14 is dropped, 15 kept ('plain' is row 0), from either side
  for narrow, wide in ((10, 11), (12, 13)):
    assert 0 not in want['src_row'][list(rows(narrow))] and 0 in want['src_row'][list(rows(wide))]
  # only I / S in the window: queried but dropped; a window without reads; min_overlap = width drops partial reads
  assert 5 in t.query(*TC.case('hand').windows[14][:2]) and 5 not in want['src_row'][list(rows(14))]
  assert len(rows(19)) == 0 and len(t.query(7000, 7061)) == 0
  assert len(rows(2)) < len(rows(1))
  # both chunk boundaries are crossed by a and by b
  for name in ('ops65', 'ops130'):
    read = TC.case(name).reads[0]
    spans = [_kept_range(read, r0, r1) for _, _, r0, r1, _ in TC.case(name).windows]
    spans = [s for s in spans if s is not None]
    assert any(a < 64 <= b for a, b in spans) and any(a == 64 for a, b in spans) and any(a == 63 for a, b in spans)
    assert any(b == 63 for a, b in spans) and any(b == 64 for a, b in spans)
  assert any(64 < a < 128 for a, b in spans) and any(a >= 128 for a, b in spans)      # ops130: the third chunk too


def _kept_range(read, r0, r1):
  """(a, b): the first and last operation of `read` that trim_cigar keeps for the window, or None."""
  pos = read.alignment.position.position
  trim, cover = max(r0 - pos, 0), r1 - max(r0, pos)
  if cover <= 0:
    return None
  kept = []
  for k, u in enumerate(read.alignment.cigar):
    step = u.operation_length if u.operation in TC.REF_OPS else 0
    if trim > 0:
      if step <= trim:
        trim -= step
        continue
      step -= trim
      trim = 0
    kept.append(k)
    if step > cover:
      break
    cover -= step
  return (kept[0], kept[-1]) if kept else None


def _call(entry, table, windows, device=False, read_end='table'):
  lib = _lib.lib()
  b = _lib.DvBatch()
  keep = [np.ascontiguousarray(table.read_pos, np.int32), np.ascontiguousarray(table.read_seq_off, np.uint32),
          np.ascontiguousarray(table.read_cigar_off, np.uint32), np.ascontiguousarray(table.cigar, np.uint32),
          np.ascontiguousarray(table.read_end, np.int64)]
  b.memory, b.n_reads = _lib.DV_MEM_HOST, table.n_reads
  b.read_pos, b.read_seq_off, b.read_cigar_off, b.cigar = (a.ctypes.data for a in keep[:4])
  b.n_bases, b.n_cigar = int(keep[1][-1]), int(keep[2][-1])
  wins = (_lib.DvTrimWindow * max(len(windows), 1))(*[_lib.DvTrimWindow(*w, 0) for w in windows])
  handle = C.c_void_p(0xdead)
  args = [C.byref(b), keep[4].ctypes.data if read_end == 'table' else read_end, len(windows), wins, C.byref(handle)]
  rc = getattr(lib, entry)(*(args + ([None] if device else [])))
  return rc, handle


@pytest.mark.parametrize('name', TC.CASE_NAMES)
def test_host_entry_equals_trim_reads(name):
  want, _, _ = TC.reference(name)
  got = A.trim_arrays(TC.table(name), TC.case(name).windows, device=False)
  TC.assert_same_arrays(got, want, name)
  assert 'stats' not in got


def _assert_same_table(got, want, what):
  for f in dataclasses.fields(packing.ReadTable):
    g, w = getattr(got, f.name), getattr(want, f.name)
    if w is None or g is None:
      assert g is None and w is None, (what, f.name)
    elif isinstance(w, np.ndarray):
      assert g.dtype == w.dtype and g.shape == w.shape, (what, f.name, g.dtype, w.dtype, g.shape, w.shape)
      np.testing.assert_array_equal(g, w, err_msg='%s: %s' % (what, f.name))
    else:
      assert g == w, (what, f.name)


@pytest.mark.parametrize('name', TC.CASE_NAMES)
def test_trim_table_equals_from_reads_of_the_trimmed_objects(name):
  want_arrays, objects, starts = TC.reference(name)
  want = packing.ReadTable.from_reads(objects, alignment_positions=starts)
  got, ranges = A.trim_table(TC.table(name), TC.case(name).windows, device=False)
  _assert_same_table(got, want, name)
  off = want_arrays['window_row_off'].tolist()
  assert ranges == list(zip(off[:-1], off[1:]))


def test_trim_table_keeps_base_modifications_and_haplotype_tags():
  """Per-base planes are sliced with the bases, per-read fields come from the source row."""
  from deepvariant_amd import dv_types as T
  rng = np.random.default_rng(9)
  reads = [dataclasses.replace(r) for r in TC.case('hand').reads]
  for k, r in enumerate(reads):
    n = len(r.aligned_sequence)
    if k % 2 == 0:
      r.base_modifications = {T.K5MC: bytes(rng.integers(0, 255, size=n).astype(np.uint8))}
    if k % 3 == 0:
      r.base_modifications = dict(r.base_modifications, **{T.K6MA: bytes(rng.integers(0, 255, size=n).astype(np.uint8))})
    if k % 4 != 1:
      r.info = {'HP': T.ListValue(values=[T.Value(int_value=int(rng.integers(0, 3)))])}
  windows = TC.case('hand').windows
  table = packing.ReadTable.from_reads(reads)
  objects, starts = [], []
  for q0, q1, r0, r1, min_overlap in windows:
    kept, original = A.trim_reads([reads[int(k)] for k in table.query(q0, q1)], r0, r1, min_overlap)
    objects.extend(kept)
    starts.extend(original)
  got, _ = A.trim_table(table, windows, device=False)
  assert got.mod_5mc is not None and got.mod_6ma is not None and (got.read_hp != _lib.DV_HP_NONE).any()
  _assert_same_table(got, packing.ReadTable.from_reads(objects, alignment_positions=starts), 'mods')
  # a window set that keeps nothing: an empty table, as from_reads gives for no reads
  got, ranges = A.trim_table(table, [windows[19]], device=False)
  _assert_same_table(got, packing.ReadTable.from_reads([]), 'empty')
  assert ranges == [(0, 0)]


def test_trim_table_refuses_aux_tables():
  reads = TC.case('hand').reads
  for kw in (dict(need_aux=True), dict(need_seq_aux=True)):
    table = packing.ReadTable.from_reads([dataclasses.replace(r) for r in reads], **kw)
    with pytest.raises(ValueError, match='trimmed sequence'):
      A.trim_table(table, TC.case('hand').windows, device=False)


def test_cover_error_raises_on_both_sides():
  c = TC.cover_error_case()
  table = packing.ReadTable.from_reads(c.reads)
  q0, q1, r0, r1, min_overlap = c.windows[0]
  rows = table.query(q0, q1).tolist()
  assert rows == [0, 1]
  with pytest.raises(ValueError, match='ref_length > 0'):
    A.trim_reads([c.reads[k] for k in rows], r0, r1, min_overlap)
  with pytest.raises(ValueError, match='ref_length > 0'):
    TC.closed_form_pair(table.cigar[1:2], 1090, 50, r0, r1, min_overlap)
  with pytest.raises(ValueError, match=r'window 0 \[1010, 1071\), row 1: Check failed: ref_length > 0'):
    A.trim_arrays(table, c.windows, device=False)
  rc, handle = _call('dv_trim_reads_batch', table, c.windows)
  assert rc == _lib.DV_ERR_BAD_INPUT and handle.value is None          # nothing stays allocated


def test_length_error_raises_on_both_sides():
  c, table = TC.length_error_case()
  q0, q1, r0, r1, min_overlap = c.windows[0]
  with pytest.raises(ValueError, match='read_trim \\+ new_read_length'):
    A.trim_reads(c.reads, r0, r1, min_overlap)
  with pytest.raises(ValueError, match='read_trim \\+ new_read_length'):
    TC.closed_form_pair(table.cigar[1:2], 1000, 50, r0, r1, min_overlap)
  with pytest.raises(ValueError, match=r'window 0 \[990, 1100\), row 1: Check failed: read_trim \+ new_read_length'):
    A.trim_arrays(table, c.windows, device=False)
  rc, handle = _call('dv_trim_reads_batch', table, c.windows)
  assert rc == _lib.DV_ERR_BAD_INPUT and handle.value is None
  # a window that ends before the missing bases are needed is fine
  got = A.trim_arrays(table, [(990, 1040, 990, 1040, 15)], device=False)
  assert got['new_len'].tolist() == [40, 40]


@pytest.mark.parametrize('entry,device', [('dv_trim_reads_batch', False), ('dv_trim_reads_batch_device', True)])
def test_argument_errors_come_first(entry, device):
  """Null pointers and negative counts are DV_ERR_INVALID_ARGUMENT on both entry points, with or without a GPU,
  and leave no result behind."""
  lib = _lib.lib()
  table = TC.table('hand')
  windows = TC.case('hand').windows
  extra = [None] if device else []
  fn = getattr(lib, entry)
  rc, handle = _call(entry, table, windows, device, read_end=None)
  assert rc == _lib.DV_ERR_INVALID_ARGUMENT and handle.value is None and entry in _lib.last_error()
  b = _lib.DvBatch()
  b.memory = _lib.DV_MEM_HOST
  handle = C.c_void_p(0xdead)
  wins = (_lib.DvTrimWindow * 1)()
  assert fn(None, None, 0, wins, C.byref(handle), *extra) == _lib.DV_ERR_INVALID_ARGUMENT and handle.value is None
  assert fn(C.byref(b), None, 0, wins, None, *extra) == _lib.DV_ERR_INVALID_ARGUMENT
  handle = C.c_void_p(0xdead)
  assert fn(C.byref(b), None, -1, wins, C.byref(handle), *extra) == _lib.DV_ERR_INVALID_ARGUMENT and handle.value is None
  assert fn(C.byref(b), None, 1, None, C.byref(handle), *extra) == _lib.DV_ERR_INVALID_ARGUMENT
  b.n_reads = -1
  assert fn(C.byref(b), None, 0, wins, C.byref(handle), *extra) == _lib.DV_ERR_INVALID_ARGUMENT
  b.n_reads, b.memory = 0, _lib.DV_MEM_DEVICE
  assert fn(C.byref(b), None, 0, wins, C.byref(handle), *extra) == _lib.DV_ERR_INVALID_ARGUMENT
  # descending offsets
  bad = dataclasses.replace(table, read_cigar_off=table.read_cigar_off[::-1].copy())
  rc, handle = _call(entry, bad, windows, device)
  assert rc == _lib.DV_ERR_INVALID_ARGUMENT and handle.value is None
  # an empty batch is fine on both, without a device too
  b.memory = _lib.DV_MEM_HOST
  handle = C.c_void_p()
  assert fn(C.byref(b), None, 0, None, C.byref(handle), *extra) == _lib.DV_OK and handle.value
  view = _lib.DvTrimmedReadsView()
  assert lib.dv_trimmed_reads_arrays(handle, C.byref(view)) == _lib.DV_OK
  assert (view.n_windows, view.n_rows, view.n_words) == (0, 0, 0)
  lib.dv_trimmed_reads_free(handle)
  assert lib.dv_trimmed_reads_arrays(None, C.byref(view)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert lib.dv_trim_device_last_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT


def test_device_entry_needs_a_device():
  if _lib.device_count() > 0:
    pytest.skip('GPU present')
  rc, handle = _call('dv_trim_reads_batch_device', TC.table('hand'), TC.case('hand').windows, device=True)
  assert rc == _lib.DV_ERR_NO_DEVICE and handle.value is None
