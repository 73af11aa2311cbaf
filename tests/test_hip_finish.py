"""dv_align_windows_batch_device (GPU): the fast pass, the sweeps with their trace-back and the finish kernels of
csrc/realign_finish.hip return the arrays of the host entry point (FastPassAligner::align_reads window by window;
tests/test_finish_cpu.py pins that one to dv_aligner_align_reads) on every case of tests/finish_cases.py.  `==` only.
The stats keep a run that never reached the device from passing."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepvariant_amd import _lib
from deepvariant_amd import fast_pass_aligner as F
from tests import finish_cases as K

pytestmark = pytest.mark.gpu
NAMES = ('window_read_off', 'status', 'position', 'cigar_off', 'cigar')


def _same(got, want, what):
  for name in NAMES:
    assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name)
    assert np.array_equal(got[name], want[name]), (what, name)


def _compare(c, stream=0):
  """windows_on_host must equal the number worked out from the host's band and run counts."""
  want = K.host_answer(c)
  got, stats = F.align_windows_batch_device(c['windows'], c['options'], stream=stream, with_stats=True)
  _same(got, want, c['name'])
  with_reads = [w for w in c['windows'] if w['reads']]
  over = K.windows_past_the_limits(c)
  assert stats.windows == len(with_reads) and stats.windows_on_host == len(over)
  if len(with_reads) > len(over):
    assert stats.launches == 4 and stats.bytes_down > 0
  assert stats.reads == sum(len(w['reads']) for w in with_reads) - sum(len(c['windows'][w]['reads']) for w in over)
  return got, stats


@pytest.mark.parametrize('c', K.hand_made() + K.seeded_cases() + K.read_counts(), ids=lambda c: c['name'])
def test_case_equals_the_host_entry_point(c):
  got, stats = _compare(c)
  if stats.windows_on_host == 0:
    assert stats.cigar_words == len(got['cigar'])


@pytest.mark.parametrize('total', [1023, 1024, 1025, 2049])
def test_call_whose_reads_cross_the_scans_carry(total):
  got, stats = _compare(K.total_reads(total))
  assert stats.reads == total and stats.cigar_words == len(got['cigar']) > total // 2


def test_handed_back_windows_sit_between_device_windows():
  c, pairs = K.past_the_limits()
  over = []
  for w, p in enumerate(pairs):
    if p is None:
      continue
    band, runs = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().dv_local_align_band(p[0].encode(), p[1].encode(), 4, 6, 8, 1, C.byref(band), C.byref(runs)))
    if band.value > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND or runs.value > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_RUNS:
      over.append(w)
  assert over == [1, 3] == K.windows_past_the_limits(c)      # worked out from the host's band and run counts
  got, stats = _compare(c)
  assert stats.windows == 5 and stats.windows_on_host == 2 and stats.reads == sum(len(c['windows'][w]['reads']) for w in (0, 2, 4))


def test_words_past_the_first_download_are_fetched():
  c = [c for c in K.hand_made() if c['name'] == 'cigar_longer_than_the_first_download'][0]
  got, stats = _compare(c)
  assert stats.reads == 1 and stats.cigar_words == len(got['cigar']) == 5 > 4 * stats.reads


def test_words_past_the_room_on_the_device_run_the_write_pass_again(monkeypatch):
  """DV_REALIGN_FINISH_ROOM=1: room for one word per read, so the 5-word CIGAR of the one read does not fit; the call
  runs its launches again with the exact room and returns the same arrays."""
  c = [c for c in K.hand_made() if c['name'] == 'cigar_longer_than_the_first_download'][0]
  monkeypatch.setenv('DV_REALIGN_FINISH_ROOM', '1')
  got, stats = F.align_windows_batch_device(c['windows'], c['options'], with_stats=True)
  _same(got, K.host_answer(c), c['name'])
  assert stats.launches == 8 and stats.cigar_words == 5 and stats.reads == 1
  big = K.total_reads(1025)
  got, stats = F.align_windows_batch_device(big['windows'], big['options'], with_stats=True)
  _same(got, K.host_answer(big), big['name'])
  assert stats.launches == 8 and stats.cigar_words == len(got['cigar']) > 1025


def test_second_call_gives_identical_bytes():
  c = K.seeded(5, 5)
  first = F.align_windows_batch_device(c['windows'], c['options'])
  second = F.align_windows_batch_device(c['windows'], c['options'])
  for name in NAMES:
    assert first[name].tobytes() == second[name].tobytes(), name
  _same(first, K.host_answer(c), c['name'])


def test_callers_stream_with_work_queued_in_front():
  c = K.seeded(7, 5)
  stream = torch.cuda.Stream()
  with torch.cuda.stream(stream):
    x = torch.ones(1 << 22, device='cuda')
    for _ in range(8):
      x = x * 1.0001 + 1.0
    _compare(c, stream=stream.cuda_stream)
  stream.synchronize()
  assert float(x[0]) > 1.0


def test_300_windows_then_3_in_one_process():
  _compare(K.tiny_windows())
  small = K.seeded(2, 3)
  got, stats = _compare(small)
  assert stats.windows == 3 and stats.reads == len(got['status'])


def test_windows_without_reads_between_windows_with_reads():
  c = K.seeded(9, 4)
  empty = dict(c['windows'][0], reads=[], name='empty')
  c = dict(c, name='with_empty_windows', windows=[empty, c['windows'][0], empty, c['windows'][1], empty])
  got, stats = _compare(c)
  assert got['window_read_off'][1] == 0 and stats.windows == 2
