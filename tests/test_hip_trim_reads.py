"""dv_trim_reads_batch_device (csrc/trim_reads.hip: one wave per (window, read) pair, count / scan / emit) against
the host entry point and alt_aligned_pileup_lib.trim_reads, on the cases of tests/trim_cases.py (GPU)."""
import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import alt_aligned_pileup_lib as A
from tests import trim_cases as TC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', TC.CASE_NAMES)
def test_device_arrays_equal_the_host_entry_and_trim_reads(name):
  table, windows = TC.table(name), TC.case(name).windows
  host = A.trim_arrays(table, windows, device=False)
  got = A.trim_arrays(table, windows, device=True)
  TC.assert_same_arrays(got, host, name + ' (device vs host entry)')
  TC.assert_same_arrays(got, TC.reference(name)[0], name + ' (device vs trim_reads)')
  # the stats: one wave per overlapping pair, three launches, and the words the pairs could write at most
  pairs = sum(len(table.query(q0, q1)) for q0, q1, _, _, _ in windows)
  ops = np.diff(table.read_cigar_off.astype(np.int64))
  st = got['stats']
  assert st['pairs_tested'] == pairs and st['pairs_kept'] == len(got['src_row'])
  assert st['words_read'] == sum(int(ops[table.query(q0, q1)].sum()) for q0, q1, _, _, _ in windows)
  assert st['words_written'] == len(got['cigar']) <= st['words_read']
  assert 1 <= st['launches'] <= 3
  # placement is a pure function of the input: a second call gives the same arrays
  TC.assert_same_arrays(A.trim_arrays(table, windows, device=True), got, name + ' (second call)')


def test_trim_table_on_the_device_equals_the_host_route():
  from tests.test_trim_reads_cpu import _assert_same_table
  table, windows = TC.table('random'), TC.case('random').windows
  want, want_ranges = A.trim_table(table, windows, device=False)
  got, ranges, stats = A.trim_table(table, windows, device=True, with_stats=True)
  _assert_same_table(got, want, 'random')
  assert ranges == want_ranges and stats['launches'] == 3


def test_caller_stream_and_empty_batches():
  import torch
  table, windows = TC.table('hand'), TC.case('hand').windows
  want = A.trim_arrays(table, windows, device=False)
  stream = torch.cuda.Stream()
  TC.assert_same_arrays(A.trim_arrays(table, windows, device=True, stream=stream.cuda_stream), want, 'caller stream')
  # no windows, and a window without reads: nothing is launched
  for wins in ([], [windows[19]]):
    got = A.trim_arrays(table, wins, device=True)
    assert got['window_row_off'].tolist() == [0] * (len(wins) + 1) and len(got['src_row']) == 0
    assert got['cigar_off'].tolist() == [0] and got['stats']['launches'] == 0
  # a table without reads
  from deepvariant_amd import packing
  got = A.trim_arrays(packing.ReadTable.from_reads([]), windows, device=True)
  assert got['window_row_off'].tolist() == [0] * (len(windows) + 1)


def test_errors_name_the_smallest_window_and_row():
  """Both error kinds come back from the kernels' flag word as the host entry reports them, and leave no result."""
  from tests.test_trim_reads_cpu import _call
  from deepvariant_amd import packing
  c = TC.cover_error_case()
  table = packing.ReadTable.from_reads(c.reads)
  # the offending window second, and twice: the smallest (window, row) is named
  fine = (1000, 1061, 1000, 1061, 15)
  with pytest.raises(ValueError, match=r'window 1 \[1010, 1071\), row 1: Check failed: ref_length > 0'):
    A.trim_arrays(table, [fine, c.windows[0], c.windows[0]], device=True)
  rc, handle = _call('dv_trim_reads_batch_device', table, c.windows, device=True)
  assert rc == _lib.DV_ERR_BAD_INPUT and handle.value is None
  c, table = TC.length_error_case()
  with pytest.raises(ValueError, match=r'window 0 \[990, 1100\), row 1: Check failed: read_trim \+ new_read_length'):
    A.trim_arrays(table, c.windows, device=True)
  # the next call on the same thread is unaffected
  TC.assert_same_arrays(A.trim_arrays(TC.table('hand'), TC.case('hand').windows, device=True),
                        TC.reference('hand')[0], 'after an error')
