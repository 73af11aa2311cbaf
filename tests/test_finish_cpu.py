"""The finish step of the realigner's alignments without a GPU: the new symbols and struct layouts, the argument checks
of dv_align_windows_batch / _device, the host entry point against dv_aligner_align_reads window by window, the
permutation helper against std::sort over real HaplotypeAlignment objects, what each named case of
tests/finish_cases.py holds (proven from the host answer), and tools/realign_finish_check.cpp built and run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import fast_pass_aligner as F
from tests import finish_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(res, i):
  a, b = int(res['cigar_off'][i]), int(res['cigar_off'][i + 1])
  return ''.join('%d%s' % (w >> 4, '?MID?S'[w & 15]) for w in res['cigar'][a:b])


def rows(res):
  return [(int(res['status'][i]), int(res['position'][i]), text(res, i)) for i in range(len(res['status']))]


def test_symbols_and_layouts():
  lib = _lib.lib()
  for name in ('dv_align_windows_batch', 'dv_align_windows_batch_device', 'dv_aligned_windows_arrays',
               'dv_aligned_windows_free', 'dv_realign_finish_last_stats', 'dv_realign_finish_sorted_order'):
    assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS
  assert C.sizeof(_lib.DvAlignWindow) == 40 and _lib.DvAlignWindow.ref_start.offset == 32
  assert C.sizeof(_lib.DvRealignFinishStats) == 48
  assert [n for n, _ in _lib.DvRealignFinishStats._fields_] == ['windows', 'windows_on_host', 'reads', 'cigar_words',
                                                                 'launches', 'bytes_down']
  assert C.sizeof(_lib.DvAlignedWindowsView) == 56
  assert lib.dv_abi_version() == 8


def _raw_call(entry, n_seqs, table, off, n_windows, descs, opt, device):
  handle = C.c_void_p(1)
  args = [n_seqs, table, off.ctypes.data if off is not None else None, n_windows, descs,
          C.byref(opt) if opt is not None else None, C.byref(handle)]
  if device:
    args.append(None)
  return entry(*args), handle


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
def test_argument_errors_come_before_any_device_work(device):
  lib = _lib.lib()
  entry = lib.dv_align_windows_batch_device if device else lib.dv_align_windows_batch
  table = b'ACGTACGTACGTACGTACGT'
  off = np.array([0, 10, 20], np.int64)
  opt = _lib.DvAlignerOptions()

  def window(**kw):
    d = (_lib.DvAlignWindow * 1)()
    d[0].first_read, d[0].n_reads, d[0].first_haplotype, d[0].n_haplotypes, d[0].reference = 0, 1, 1, 1, 1
    for k, v in kw.items():
      setattr(d[0], k, v)
    return d
  bad = [
      (2, table, off, 1, window(), None),                       # null options
      (2, table, off, -1, window(), opt),                       # negative count
      (2, table, off, 1, None, opt),                            # null windows
      (2, table, None, 1, window(), opt),                       # null offsets
      (2, None, off, 1, window(), opt),                         # null bytes
      (2, table, np.array([0, 12, 10], np.int64), 1, window(), opt),   # descending offsets
      (2, table, off, 1, window(n_reads=3), opt),               # reads past the table
      (2, table, off, 1, window(first_haplotype=2), opt),       # haplotypes past the table
      (2, table, off, 1, window(reference=-1), opt),            # the reference is required
      (2, table, off, 1, window(reference=2), opt),
      (2, table, off, 1, window(ref_prefix_len=-1), opt),
      (2, table, off, 1, window(ref_start=-5), opt),
  ]
  for args in bad:
    rc, handle = _raw_call(entry, *args, device)
    assert rc == _lib.DV_ERR_INVALID_ARGUMENT, args
    assert handle.value is None
  refused = _lib.DvAlignerOptions()
  refused.kmer_size = 2
  rc, handle = _raw_call(entry, 2, table, off, 1, window(), refused, device)
  assert rc == _lib.DV_ERR_INVALID_ARGUMENT and handle.value is None
  refused = _lib.DvAlignerOptions()
  refused.match = 128
  rc, handle = _raw_call(entry, 2, table, off, 1, window(), refused, device)
  assert rc == _lib.DV_ERR_INVALID_ARGUMENT and handle.value is None


@pytest.mark.parametrize('entry', [F.align_windows_batch, F.align_windows_batch_device], ids=['host', 'device'])
def test_zero_windows_and_windows_without_reads_need_no_device(entry):
  res = entry([], {})
  assert res['window_read_off'].tolist() == [0] and len(res['status']) == 0 and res['cigar_off'].tolist() == [0]
  res = entry([dict(reads=[], haplotypes=['ACGT' * 10], reference='ACGT' * 10)] * 2, {})
  assert res['window_read_off'].tolist() == [0, 0, 0] and len(res['status']) == 0


def test_finish_stats_are_zero_before_any_device_call():
  stats = _lib.DvRealignFinishStats()
  F.align_windows_batch_device([], {})
  _lib.check(_lib.lib().dv_realign_finish_last_stats(C.byref(stats)))
  assert [getattr(stats, n) for n, _ in stats._fields_] == [0] * 6


def _object_route(w, options):
  opts = {k: v for k, v in options.items() if k != 'normalize_reads'}
  a = F.FastPassAligner(normalize_reads=bool(options.get('normalize_reads', 0)),
                        ref_prefix_len=w.get('ref_prefix_len', 0), ref_suffix_len=w.get('ref_suffix_len', 0), **opts)
  a.set_reference(w['reference'], w['ref_start'])
  a.set_haplotypes(w['haplotypes'])
  return a.align_reads(w['reads'])


@pytest.mark.parametrize('c', K.hand_made() + K.seeded_cases()[:8] + [K.past_the_limits()[0]], ids=lambda c: c['name'])
def test_host_entry_point_equals_dv_aligner_align_reads_window_by_window(c):
  res = K.host_answer(c)
  got = rows(res)
  at = 0
  for w in c['windows']:
    want = _object_route(w, c['options'])
    assert len(want) == len(w['reads'])
    for r in want:
      status, position, cigar = r[0], r[1], ''.join('%d%s' % (n, '?MID?S'[op]) for op, n in r[2])
      assert got[at][0] == status, (w['name'], at)
      if status == 1:
        assert got[at][1:] == (position, cigar), (w['name'], at)
      else:
        assert got[at][1:] == (0, '')
      at += 1
  assert at == len(got) and res['window_read_off'].tolist() == list(np.cumsum([0] + [len(w['reads']) for w in c['windows']]))


@pytest.mark.parametrize('n', [1, 16, 17, 40, 96])
def test_permutation_helper_equals_the_real_sort(n):
  rng = np.random.RandomState(n)
  for trial in range(20):
    scores = (rng.randint(0, 4, n) * 240).astype(np.int32)      # many ties
    records, objects = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _lib.check(_lib.lib().dv_realign_finish_sorted_order(n, scores.ctypes.data, records.ctypes.data, objects.ctypes.data))
    assert records.tolist() == objects.tolist()
    assert sorted(records.tolist()) == list(range(n)) and (np.diff(scores[records]) >= 0).all()
  if n > 16:   # what a stable sort would give is not what std::sort gives: the helper has something to get right
    unstable = 0
    for trial in range(20):
      scores = (rng.randint(0, 3, n) * 240).astype(np.int32)
      records, objects = np.zeros(n, np.int32), np.zeros(n, np.int32)
      _lib.check(_lib.lib().dv_realign_finish_sorted_order(n, scores.ctypes.data, records.ctypes.data, objects.ctypes.data))
      unstable += records.tolist() != np.argsort(scores, kind='stable').tolist()
    assert unstable > 0


EXPECT = {
    'fast_pass_read_on_haplotype_with_insertion': [(1, 5090, '29M6I25M'), (1, 5010, '60M')],
    'fast_pass_read_on_haplotype_with_deletion': [(1, 5090, '30M7D30M'), (1, 5010, '60M')],
    'fast_pass_read_on_haplotype_with_both': [(1, 5060, '20M5I70M4D25M'), (1, 5010, '60M')],
    'cigar_longer_than_the_first_download': [(1, 5060, '20M5I70M4D25M')],
    'read_starts_inside_the_haplotypes_insertion': [(1, 5090, '29M6I25M'), (1, 5119, '2I58M')],
    'read_starts_right_behind_the_deletion': [(1, 5090, '30M7D30M'), (1, 5127, '60M')],   # 5127: the front D is dropped
    'read_i3_on_haplotype_d2': [(1, 5090, '30M2D30M'), (1, 5080, '40M1I42M')],             # 1I, then the pushed matches
    'read_i1_on_haplotype_d3': [(1, 5090, '30M3D30M'), (1, 5080, '40M2D41M')],
    'read_d2_on_haplotype_i3': [(1, 5090, '30M3I27M'), (1, 5080, '40M1I42M')],
    'read_d3_on_haplotype_i1': [(1, 5090, '30M1I29M'), (1, 5080, '39M2D43M')],
    'leading_soft_clip': [(1, 5090, '29M6I25M'), (1, 5100, '8S19M6I35M')],
    'soft_clipped_tail_past_the_haplotype_end': [(1, 5090, '29M6I25M'), (1, 5190, '50M10S')],
    'read_runs_past_the_haplotype_is_cleared': [(1, 5090, '29M6I25M'), (0, 0, '')],
    'haplotype_with_soft_clips_offset_negative': [(1, 5000, '10S50M'), (1, 5002, '8S52M'), (1, 5090, '29M6I25M')],
    'haplotype_all_n_cannot_be_aligned': [(1, 5010, '60M'), (0, 0, ''), (1, 5100, '60M')],
    'non_normalized_indel_normalize_reads_0': [(1, 5090, '30M2D30M'), (0, 0, '')],
    'non_normalized_indel_normalize_reads_1': [(1, 5090, '30M2D30M'), (1, 5080, '40M1I42M')],
    'force_alignment_haplotype_not_the_reference': [(1, 5090, '29M6I25M'), (2, 0, ''), (1, 5010, '60M')],
    'force_alignment_only_the_reference': [(1, 5090, '60M'), (2, 0, ''), (1, 5010, '60M')],
    'every_haplotype_is_the_reference': [(1, 5010, '60M'), (1, 5100, '60M')],
    'equal_scores_on_reference_and_non_reference': [(1, 5010, '60M'), (1, 5090, '29M6I25M'), (1, 5130, '60M')],
    'equal_scores_on_two_non_reference_haplotypes': [(1, 5090, '29M6I25M'), (1, 5100, '19M6I35M'), (1, 5010, '60M')],
    # read 0 fits all tied haplotypes: std::sort leaves one with the insertion last, index order one without (another CIGAR)
    'tied_scores_17_haplotypes': [(1, 5070, '49M5I'), (1, 5010, '60M')],
    'tied_scores_40_haplotypes': [(1, 5070, '49M5I'), (1, 5010, '60M')],
    'lower_case_and_n_in_reference_and_reads': [(1, 5090, '29M6I25M'), (1, 5010, '60M')],
    'no_unplaced_read': [(1, 5010, '60M'), (1, 5090, '29M6I25M'), (1, 5150, '60M')],
}


@pytest.mark.parametrize('c', K.hand_made(), ids=lambda c: c['name'])
def test_named_case_holds_what_its_name_says(c):
  got = rows(K.host_answer(c))
  assert got == EXPECT[c['name']]


def test_tied_haplotypes_are_taken_in_the_sorts_order():
  """17 and 40 haplotypes: all but the reference tie, std::sort leaves them in another order than their indices, and
  the haplotype it leaves last is of the other kind than the one index order leaves last, so read 0's CIGAR (pinned in
  EXPECT) tells the two orders apart."""
  for c in K.hand_made():
    if not c['name'].startswith('tied_scores_'):
      continue
    w = c['windows'][0]
    n = len(w['haplotypes'])
    fast = F.fast_pass_batch([w], c['options'])[0]
    scores = np.where(fast['haplotype_discarded'] != 0, 0, fast['haplotype_score']).astype(np.int32)
    assert len(set(scores[:-1].tolist())) == 1 and scores[-1] < scores[0]
    assert fast['read_score'][:-1, 0].tolist() == [4 * len(w['reads'][0])] * (n - 1)     # read 0 fits each without a mismatch
    records, objects = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _lib.check(_lib.lib().dv_realign_finish_sorted_order(n, scores.ctypes.data, records.ctypes.data, objects.ctypes.data))
    stable = np.argsort(scores, kind='stable')
    assert records.tolist() == objects.tolist() != stable.tolist()
    with_insertion = lambda h: h < n // 2                                                 # noqa: E731
    assert with_insertion(int(records[-1])) and not with_insertion(int(stable[-1]))
    # the haplotype index order would end on, alone with the reference, gives the other CIGAR
    alone = K.case('alone', K.window('alone', [w['haplotypes'][int(stable[-1])], K.REF], w['reads']))
    other = rows(F.align_windows_batch(alone['windows'], alone['options']))[0]
    assert other[0] == 1 and other[2] != EXPECT[c['name']][0][2]


def test_past_the_limits_case_is_past_the_limits():
  c, pairs = K.past_the_limits()
  over = []
  for p in pairs:
    if p is None:
      over.append(False)
      continue
    band, runs = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().dv_local_align_band(p[0].encode(), p[1].encode(), 4, 6, 8, 1, C.byref(band), C.byref(runs)))
    over.append(band.value > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND or runs.value > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_RUNS)
  assert over == [False, True, False, True, False]
  band, runs = C.c_int32(), C.c_int32()
  _lib.check(_lib.lib().dv_local_align_band(pairs[1][0].encode(), pairs[1][1].encode(), 4, 6, 8, 1, C.byref(band), C.byref(runs)))
  assert band.value > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND and runs.value <= _lib.DV_LOCAL_ALIGN_DEVICE_MAX_RUNS
  _lib.check(_lib.lib().dv_local_align_band(pairs[3][0].encode(), pairs[3][1].encode(), 4, 6, 8, 1, C.byref(band), C.byref(runs)))
  assert runs.value > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_RUNS


def test_case_sizes():
  names = [c['name'] for c in K.all_cases()]
  assert len(names) == len(set(names))
  assert [len(c['windows'][0]['reads']) for c in K.read_counts()] == [1, 63, 64, 65, 257]
  for total in (1023, 1024, 1025, 2049):
    assert sum(len(w['reads']) for w in K.total_reads(total)['windows']) == total
  assert len(K.tiny_windows()['windows']) == 300
  for c in K.all_cases():
    for w in c['windows']:
      assert len(w['reference']) <= 400 and len(w['haplotypes']) <= 40 and all(30 <= len(r) <= 250 for r in w['reads'])


def test_check_tool_builds_and_reports_no_difference(tmp_path):
  # local_align.cpp needs clang's vector builtins: the compiler the library itself is built with, as plain C++
  cxx = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
  exe = str(tmp_path / 'realign_finish_check')
  csrc = os.path.join(ROOT, 'deepvariant_amd', 'csrc')
  subprocess.check_call([cxx, '-O2', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), '-I' + csrc,
                         os.path.join(ROOT, 'tools', 'realign_finish_check.cpp'), os.path.join(csrc, 'fast_pass_aligner.cpp'),
                         os.path.join(csrc, 'local_align.cpp'), '-lpthread', '-o', exe])
  out = subprocess.run([exe, '3000', '4', '11'], stdout=subprocess.PIPE, universal_newlines=True)
  line = out.stdout.strip().splitlines()[-1]
  assert out.returncode == 0, out.stdout[-2000:]
  fields = line.split()
  value = lambda key: int(fields[fields.index(key) + 1])      # noqa: E731
  assert value('windows') == 3000 and value('differences') == 0 and value('failed') == 0
  assert value('reads') > 20000 and value('status0') > 0 and value('status1') > 0 and value('status2') > 0
  assert value('reads_with_id_cancellation') > 0
