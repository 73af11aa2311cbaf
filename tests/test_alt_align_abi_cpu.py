"""dv_alt_align_batch (host code) and alt_align_table(device=False) against the object route
(fast_pass_aligner.realign_reads_to_haplotype on Read objects), the argument checks of both entry points, and the
proof that tests/alt_align_cases.py holds every kind of pair it promises.  No GPU."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import alt_aligned_pileup_lib as A
from deepvariant_amd import fast_pass_aligner as fpa
from deepvariant_amd import packing
from tests import alt_align_cases as cases

_BATCHES = {b['name']: b for b in cases.batches()}


def _pairs(d, item):
  lo, hi = int(d['item_pair_off'][item]), int(d['item_pair_off'][item + 1])
  out = []
  for k in range(lo, hi):
    words = d['cigar'][int(d['cigar_off'][k]):int(d['cigar_off'][k + 1])]
    out.append((int(d['status'][k]), int(d['position'][k]), [(int(w) & 15, int(w) >> 4) for w in words]))
  return out


def _host(batch, **cfg):
  return A.alt_align_arrays(cases.table_of(batch), batch['items'], batch['targets'], dict(batch['cfg'], **cfg),
                            device=False)


def test_header_and_bindings_agree():
  header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'dvhip.h')).read()
  assert re.search(r'#define DV_ABI_VERSION 8\b', header) and _lib.lib().dv_abi_version() == 8

  def fields(name):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    out = []
    for decl in body.split(';'):
      names = re.findall(r'[\w]+', decl)
      if names:
        first = [w for w in re.split(r',', decl)]
        out += [re.findall(r'\w+', piece)[-1] for piece in first]
    return out

  for struct, binding in (('dv_alt_align_item', _lib.DvAltAlignItem), ('dv_alt_aligned_view', _lib.DvAltAlignedView),
                          ('dv_alt_align_stats', _lib.DvAltAlignStats)):
    assert fields(struct) == [n for n, _ in binding._fields_], struct   # pylint: disable=protected-access
  assert C.sizeof(_lib.DvAltAlignItem) == 32 and C.sizeof(_lib.DvAltAlignStats) == 12 * 8
  for symbol in ('dv_alt_align_batch', 'dv_alt_align_batch_device', 'dv_alt_aligned_arrays', 'dv_alt_aligned_free',
                 'dv_alt_align_device_last_stats'):
    assert symbol in _lib.ABI_SYMBOLS and re.search(r'\b%s\s*\(' % symbol, header) and getattr(_lib.lib(), symbol)


@pytest.mark.parametrize('name', sorted(_BATCHES))
@pytest.mark.parametrize('normalize_reads', [False, True])
def test_host_entry_equals_the_object_route(name, normalize_reads):
  batch = _BATCHES[name]
  d = _host(batch, normalize_reads=int(normalize_reads))
  want = cases.object_route(batch, normalize_reads)
  assert int(d['item_pair_off'][-1]) == sum(it[1] for it in batch['items']) == len(d['status'])
  assert d['cigar_off'][0] == 0 and d['cigar_off'][-1] == len(d['cigar'])
  moved = 0
  for item, (first, n_rows, _, _, _) in enumerate(batch['items']):
    got = _pairs(d, item)
    assert len(got) == n_rows == len(want[item])
    for row, ((status, position, cigar), read) in enumerate(zip(got, want[item])):
      source = batch['reads'][first + row]
      if read is None:
        assert (status, position, cigar) == (2, 0, []), (item, row)
      elif read is source:
        assert (status, position, cigar) == (0, 0, []), (item, row)
      else:
        moved += 1
        assert status == 1 and position == read.alignment.position.position, (item, row)
        assert cigar == [(u.operation, u.operation_length) for u in read.alignment.cigar], (item, row)
  assert moved > 0


def test_the_cases_hold_every_kind_of_pair():
  batch = _BATCHES['kinds']
  cfg, kinds, t = batch['cfg'], batch['kinds'], batch['targets'][0]
  n = len(t)
  d = _host(batch)
  seq = lambda kind: batch['reads'][batch['items'][kinds[kind][0]][0] + kinds[kind][1]].aligned_sequence   # noqa: E731
  pair = lambda kind: _pairs(d, kinds[kind][0])[kinds[kind][1]]                                               # noqa: E731
  main = [r.aligned_sequence for r in batch['reads'][:batch['items'][0][1]]]
  fast = fpa.fast_pass_batch([dict(reads=main, haplotypes=[t], reference=t)], cfg)[0]['read_position'][0]
  row = lambda kind: kinds[kind][1]                                                                             # noqa: E731
  # placed by the fast pass at both ends of the target, with exactly max_num_of_mismatches mismatches, in lower case
  assert fast[row('fast_p0')] == 0 and pair('fast_p0') == (1, cases.REF_START, [(1, 60)])
  assert fast[row('fast_pend')] == n - 50 and pair('fast_pend') == (1, cases.REF_START + n - 50, [(1, 50)])
  mism = lambda kind, at: sum(a != b for a, b in zip(seq(kind).upper(), t[at:]))                                # noqa: E731
  assert mism('fast_max_mismatches', 40) == cfg['max_num_of_mismatches'] and fast[row('fast_max_mismatches')] == 40
  assert pair('fast_max_mismatches') == (1, cases.REF_START + 40, [(1, 80)])
  assert seq('lower_case').islower() and fast[row('lower_case')] == 70 and pair('lower_case')[0] == 1
  # left to Smith-Waterman: one mismatch more, and a read no longer than a k-mer
  assert mism('one_more_mismatch', 40) == cfg['max_num_of_mismatches'] + 1 and fast[row('one_more_mismatch')] == -1
  assert pair('one_more_mismatch')[0] == 1
  assert len(seq('short')) <= cfg['kmer_size'] and fast[row('short')] == -1 and pair('short')[0] == 1
  # clean indels
  assert fast[row('insertion3')] == -1 and pair('insertion3') == (1, cases.REF_START + 20, [(1, 40), (2, 3), (1, 40)])
  status, position, cigar = pair('deletion5')      # the aligner places the gap as far left as the repeat allows
  assert fast[row('deletion5')] == -1 and (status, position) == (1, cases.REF_START + 100)
  assert [op for op, _ in cigar] == [1, 3, 1] and cigar[1] == (3, 5) and cigar[0][1] + cigar[2][1] == 65
  # nothing of a poly-A read aligns to a target without A
  assert 'A' not in t and pair('unrelated') == (2, 0, [])
  # a 40-base insertion: its band is past what the device traces back
  band, _ = fpa.local_align_band(t, seq('insertion40'), cfg['match'], cfg['mismatch'], cfg['gap_open'], cfg['gap_extend'])
  assert band > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND and (2, 40) in pair('insertion40')[2]
  # a read longer than its target: soft clips on both sides
  short_target = batch['targets'][1]
  assert len(seq('longer_than_target')) > len(short_target)
  assert pair('longer_than_target') == (1, cases.REF_START, [(5, 30), (1, 60), (5, 40)])
  # an insertion inside the C run in front of two N: the aligner writes a deletion run beside an insertion run, the
  # merged CIGAR could shift left, so the original alignment is kept unless normalize_reads
  odd = batch['targets'][2]
  text = fpa.local_align(odd, seq('unnormalised'), cfg['match'], cfg['mismatch'], cfg['gap_open'],
                         cfg['gap_extend']).cigar.decode()
  assert re.search(r'\d+D\d+I|\d+I\d+D', text), text
  assert pair('unnormalised') == (0, 0, [])
  normalised = _pairs(_host(batch, normalize_reads=1), kinds['unnormalised'][0])[kinds['unnormalised'][1]]
  assert normalised[0] == 1 and any(op == 2 for op, _ in normalised[2])
  # an item without reads; items over the same rows; a large batch with a wordless item in its middle
  assert batch['items'][kinds['empty_item'][0]][1] == 0
  shared = _BATCHES['shared_rows']
  assert shared['items'][0][:2] == shared['items'][1][:2] and shared['items'][0][2] != shared['items'][1][2]
  a, b = (_pairs(_host(shared), k) for k in (0, 1))
  assert a != b
  large = _BATCHES['large']
  dl = _host(large)
  assert len(dl['status']) >= 300 and len(large['items']) >= 5
  lo, hi = int(dl['item_pair_off'][2]), int(dl['item_pair_off'][3])
  assert hi - lo >= 64 and dl['cigar_off'][lo] == dl['cigar_off'][hi] and 0 < dl['cigar_off'][lo] < len(dl['cigar'])
  assert set(dl['status'].tolist()) == {0, 1, 2} or set(dl['status'].tolist()) == {1, 2}
  for batch_ in _BATCHES.values():
    assert all(60 <= len(x) <= 260 for x in batch_['targets'])
    assert all(8 <= len(r.aligned_sequence) <= 230 for r in batch_['reads'])


@pytest.mark.parametrize('name', sorted(_BATCHES))
def test_alt_align_table_equals_from_reads_of_the_kept_objects(name):
  batch = _BATCHES[name]
  table, ranges = A.alt_align_table(cases.table_of(batch), batch['items'], batch['targets'], batch['cfg'], device=False)
  kept, starts, want_ranges = [], [], []
  for (first, n_rows, _, _, _), realigned in zip(batch['items'], cases.object_route(batch)):
    lo = len(kept)
    for read, start in zip(realigned, batch['starts'][first:first + n_rows]):
      if read is not None and read.aligned_sequence:
        kept.append(read)
        starts.append(start)
    want_ranges.append((lo, len(kept)))
  want = packing.ReadTable.from_reads(kept, alignment_positions=starts)
  assert ranges == want_ranges
  for field in dataclasses.fields(packing.ReadTable):
    got, exp = getattr(table, field.name), getattr(want, field.name)
    if exp is None or got is None:
      assert got is None and exp is None, field.name
    elif isinstance(exp, np.ndarray):
      assert got.dtype == exp.dtype and np.array_equal(got, exp), field.name
    else:
      assert got == exp, field.name
  assert (table.read_pos != table.read_sort_pos).any()     # the untrimmed starts came through


def test_alt_align_table_refuses_aux_tables():
  batch = _BATCHES['shared_rows']
  table = packing.ReadTable.from_reads(batch['reads'], need_aux=True)
  with pytest.raises(ValueError, match='aux'):
    A.alt_align_table(table, batch['items'], batch['targets'], batch['cfg'], device=False)


def _raw_call(device, reads=None, n_items=1, items=None, n_targets=1, target_bytes=b'CGTCGTCGTT', target_off=None,
              options=None, out=True):
  """One call with every argument overridable; -> (status, handle value)."""
  keep = [np.array([0, 4, 8], np.uint32), np.frombuffer(b'CGTCCGTC', np.uint8).copy()]
  b = _lib.DvBatch()
  b.memory, b.n_reads, b.n_bases = _lib.DV_MEM_HOST, 2, 8
  b.read_seq_off, b.bases = keep[0].ctypes.data, keep[1].ctypes.data
  if callable(reads):
    reads(b, keep)
  item = (_lib.DvAltAlignItem * 1)(_lib.DvAltAlignItem(0, 2, 0, 200, 100, 0))
  if callable(items):
    items(item[0])
  off = np.array([0, 10] if target_off is None or isinstance(target_off, str) else target_off, np.int64)
  opt = _lib.DvAlignerOptions(force_alignment=1)
  if callable(options):
    options(opt)
  handle = C.c_void_p(0xdead)
  args = [C.byref(b) if reads != 'null' else None, n_items, None if items == 'null' else item, n_targets,
          target_bytes, None if isinstance(target_off, str) else off.ctypes.data,
          None if options == 'null' else C.byref(opt), C.byref(handle) if out else None]
  lib = _lib.lib()
  rc = lib.dv_alt_align_batch_device(*args, None) if device else lib.dv_alt_align_batch(*args)
  return rc, handle.value


@pytest.mark.parametrize('device', [False, True])
def test_argument_errors_are_invalid_argument_and_leave_nothing(device):
  def bad(**kw):
    rc, handle = _raw_call(device, **kw)
    assert rc == _lib.DV_ERR_INVALID_ARGUMENT and handle is None, kw

  bad(reads='null')
  bad(items='null')
  bad(target_off='null')
  bad(options='null')
  bad(target_bytes=None)
  assert _raw_call(device, out=False)[0] == _lib.DV_ERR_INVALID_ARGUMENT
  bad(n_items=-1)
  bad(n_targets=-1)
  bad(reads=lambda b, keep: setattr(b, 'n_reads', -1))
  bad(reads=lambda b, keep: setattr(b, 'memory', _lib.DV_MEM_DEVICE))
  bad(reads=lambda b, keep: setattr(b, 'read_seq_off', None))
  bad(reads=lambda b, keep: setattr(b, 'bases', None))
  bad(reads=lambda b, keep: keep[0].__setitem__(1, 9))        # descending read offsets
  bad(reads=lambda b, keep: setattr(b, 'n_bases', 7))         # offsets past n_bases
  bad(target_off=[4, 2])                                       # descending target offsets
  bad(target_off=[-1, 10])
  bad(items=lambda it: setattr(it, 'first_row', -1))
  bad(items=lambda it: setattr(it, 'n_rows', 3))               # the row range leaves the table
  bad(items=lambda it: setattr(it, 'n_rows', -1))
  bad(items=lambda it: setattr(it, 'target', 1))
  bad(items=lambda it: setattr(it, 'target', -1))
  bad(items=lambda it: setattr(it, 'ref_start', -5))
  bad(options=lambda o: setattr(o, 'force_alignment', 0))
  bad(options=lambda o: setattr(o, 'ref_prefix_len', 3))
  bad(options=lambda o: setattr(o, 'ref_suffix_len', 3))
  bad(options=lambda o: setattr(o, 'kmer_size', 40))            # the class refuses it


def test_the_host_entry_runs_the_small_call():
  rc, handle = _raw_call(False)
  assert rc == 0 and handle
  _lib.lib().dv_alt_aligned_free(handle)


def test_device_entry_without_pairs_needs_no_device():
  rc, handle = _raw_call(True, items=lambda it: setattr(it, 'n_rows', 0))
  assert rc == 0 and handle
  view = _lib.DvAltAlignedView()
  _lib.check(_lib.lib().dv_alt_aligned_arrays(handle, C.byref(view)))
  assert (view.n_items, view.n_pairs, view.n_words) == (1, 0, 0)
  _lib.lib().dv_alt_aligned_free(handle)
  rc, handle = _raw_call(True, n_items=0, n_targets=0)
  assert rc == 0 and handle
  _lib.lib().dv_alt_aligned_free(handle)


def test_device_entry_with_pairs_and_no_gpu_is_no_device():
  if _lib.device_count() > 0:
    pytest.skip('a GPU is present: tests/test_hip_alt_align.py runs the device entry')
  rc, handle = _raw_call(True)
  assert rc == _lib.DV_ERR_NO_DEVICE and handle is None
