"""dv_fast_pass_batch (include/dvhip.h, "the fast pass over many windows in one call"), host code, against
dv_aligner_fast_align haplotype by haplotype and against a transcription of the closed form the device kernel
implements (tests/fast_pass_cases.py); its argument checks; the device entry point without a device; and
FastPassAligner::AlignReads through the split steps with the batch's arrays installed.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import fast_pass_aligner as F
from tests import fast_pass_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dv_fast_pass_batch', 'dv_fast_pass_batch_device', 'dv_fast_pass_device_last_stats')


def _lists(result):
  return {name: a.tolist() for name, a in result.items()}


def _one_by_one(w):
  """The window through dv_aligner_fast_align, one haplotype at a time, in dv_fast_pass_batch's terms: the rows of
  a haplotype with score 0 are reset, as FastAlignReadsToHaplotypes does after each haplotype."""
  o = dict(w['options'])
  a = F.FastPassAligner(ref_prefix_len=w['ref_prefix_len'], ref_suffix_len=w['ref_suffix_len'], **o)
  if w['reference'] is not None:
    a.set_reference(w['reference'])
  a.set_reads([r.upper() for r in w['reads']])
  a.stage(F.BUILD_INDEX)
  out = dict(haplotype_score=[], read_position=[], read_score=[])
  for h in w['haplotypes']:
    score, rows = a.fast_align_reads_to_haplotype(h)
    out['haplotype_score'].append(score)
    for read, ra in zip(w['reads'], rows):
      assert ra.cigar == ('' if ra.position is None else '%d=' % len(read))
    out['read_position'].append([-1 if score == 0 or ra.position is None else ra.position for ra in rows])
    out['read_score'].append([0 if score == 0 or ra.position is None else ra.score for ra in rows])
  return out


def _check(windows, options):
  got = [_lists(g) for g in F.fast_pass_batch(windows, options)]
  assert len(got) == len(windows)
  for w, g in zip(windows, got):
    want = _one_by_one(w)
    for name in want:
      assert g[name] == want[name], (w['name'], name)
    assert g == K.window_model(w), w['name']           # the closed form, discarded flags included
    assert all(s == 0 for s, d in zip(g['haplotype_score'], g['haplotype_discarded']) if d), w['name']
    if w['expect_discarded'] is not None:
      assert g['haplotype_discarded'] == w['expect_discarded'], w['name']
  return got


def test_abi_is_still_8_and_declares_the_new_symbols():
  l = _lib.lib()
  assert l.dv_abi_version() == 8
  text = open(os.path.join(ROOT, 'include', 'dvhip.h')).read()
  assert re.search(r'#define DV_ABI_VERSION 8\b', text)
  for sym in NEW_SYMBOLS:
    assert hasattr(l, sym) and sym in _lib.ABI_SYMBOLS and re.search(r'\bint %s\(' % sym, text), sym
  for name in ('DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE', 'DV_FAST_PASS_DEVICE_MAX_SCORING'):
    assert int(re.search(r'#define %s (\d+)' % name, text).group(1)) == getattr(_lib, name)
  assert C.sizeof(_lib.DvFastPassStats) == 40 and C.sizeof(_lib.DvFastPassWindow) == 32


@pytest.mark.parametrize('w', K.hand_made(), ids=lambda w: w['name'])
def test_hand_made_case_equals_fast_align(w):
  _check([w], w['options'])


def test_the_hand_made_cases_are_what_their_names_say():
  cases = {w['name']: w for w in K.hand_made()}

  def accepted(name):
    w = cases[name]
    o = w['options']
    return K.closed_form(w['reads'], w['haplotypes'][0], w['reference'], 0, 0, o['kmer_size'],
                         o.get('max_num_of_mismatches') or K.DEFAULT_M, o.get('match') or K.MATCH,
                         o.get('mismatch') or K.MISMATCH)
  _, _, rows, acc = accepted('negative diagonal accepted at 0')
  assert rows == [(0, 12)] and acc[0] == [((0, 3), 0, 2, 12)]          # the seed lies on diagonal -3
  _, _, rows, acc = accepted('negative diagonal rejected at 0, later start accepted')
  assert rows == [(12, 32)] and [a[1] for a in acc[0]] == [12]
  _, _, rows, acc = accepted('tandem repeat tie')
  assert rows[0] == (0, 36) and [a[3] for a in acc[0]] == [36] * 4
  _, _, rows, acc = accepted('tie reached through a negative diagonal')
  assert rows == [(0, 50)] and sorted(acc[0]) == [((0, 6), 0, 1, 50), ((11, 5), 6, 1, 50)]
  _, discarded, rows, acc = accepted('accepted with score <= 0')
  assert not discarded and rows[1] == (-1, 0) and [a[3] <= 0 for a in acc[1]] == [True]
  _, _, rows, acc = accepted('a second-best alignment closes the hole')
  assert rows[3] == (0, 48) and sorted(a[1] for a in acc[3]) == [0, 24]
  for m in (1, 2):
    _, _, rows, acc = accepted('M = %d: M and M + 1 mismatches' % m)
    assert [p for p, _ in rows] == [0, 11, 30, -1, -1, -1] and [a[0][2] for a in acc[:3]] == [m] * 3
  for count in (63, 64, 65, 127, 128, 129):
    w = cases['%d diagonals' % count]
    assert len(w['haplotypes'][0]) - len(w['reads'][0]) + 1 == count
    assert K.window_model(w)['read_position'][0][-2:] == [count - 1, count - 1]      # the last diagonal is reached


@pytest.mark.parametrize('seed', [1, 2, 3, 4])
def test_seeded_windows_equal_fast_align(seed):
  windows = K.seeded(seed, 6)
  got = _check(windows, windows[0]['options'])
  assert sum(p >= 0 for g in got for row in g['read_position'] for p in row) > 50      # reads are placed
  assert all(2 <= len(w['haplotypes']) <= 5 and 20 <= len(w['reads']) <= 70 for w in windows)


def test_many_small_windows_in_one_call():
  windows = K.seeded(9, 200, small=True)
  got = _check(windows, windows[0]['options'])
  flags = [d for g in got for d in g['haplotype_discarded']]
  assert 0 < sum(flags) < len(flags)


def test_one_byte_over_the_device_cap_on_the_host():
  w = K.over_the_cap(_lib.DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE)
  got = _lists(F.fast_pass_batch([w], w['options'])[0])
  want = _one_by_one(w)
  for name in want:
    assert got[name] == want[name], name
  assert got['read_position'][0] == [0, 8153, 8152, 4000, 100] and got['haplotype_discarded'] == [0, 1]


def _raw_call(entry, n_seqs=3, table=b'ACGTACGTACGTACGTACGTAC', off=(0, 8, 14, 22), windows=((0, 2, 2, 1, 2, 0, 0),),
              options=(0, 0, 0, 0, 4, 0, 0), outputs=True, n_windows=None):
  off = np.ascontiguousarray(off, np.int64)
  descs = (_lib.DvFastPassWindow * max(len(windows), 1))()
  for d, w in zip(descs, windows):
    d.first_read, d.n_reads, d.first_haplotype, d.n_haplotypes, d.reference, d.ref_prefix_len, d.ref_suffix_len = w
  opt = _lib.DvAlignerOptions(*options) if options is not None else None
  out = [np.zeros(16, np.int32) for _ in range(4)]
  ptrs = [a.ctypes.data if outputs else None for a in out]
  return entry(n_seqs, table, off.ctypes.data, len(windows) if n_windows is None else n_windows, descs,
               C.byref(opt) if opt is not None else None, None, *ptrs)


@pytest.mark.parametrize('entry_name', ['dv_fast_pass_batch', 'dv_fast_pass_batch_device'])
def test_argument_errors_come_before_any_device_work(entry_name):
  entry = getattr(_lib.lib(), entry_name)
  bad = [dict(n_seqs=-1), dict(n_windows=-1), dict(off=(0, 8, 6, 22)), dict(off=(-1, 8, 14, 22)), dict(table=None),
         dict(outputs=False), dict(options=(0, 0, 0, 0, 2, 0, 0)), dict(options=(0, 0, 0, 0, 33, 0, 0)),
         dict(windows=((0, 3, 2, 1, 2, 0, 0), (2, 1, 0, 4, -1, 0, 0))), dict(windows=((0, -1, 2, 1, 2, 0, 0),)),
         dict(windows=((0, 2, 2, 2, 2, 0, 0),)), dict(windows=((0, 2, 2, 1, 3, 0, 0),)),
         dict(windows=((0, 2, 2, 1, -2, 0, 0),)), dict(windows=((0, 2, 2, 1, 2, -1, 0),)),
         dict(windows=((0, 2, 2, 1, 2, 0, -1),)), dict(windows=((-1, 2, 2, 1, 2, 0, 0),))]
  for kw in bad:
    assert _raw_call(entry, **kw) == _lib.DV_ERR_INVALID_ARGUMENT, kw
    assert _lib.last_error()
  assert _lib.lib().dv_fast_pass_device_last_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize('entry_name', ['dv_fast_pass_batch', 'dv_fast_pass_batch_device'])
def test_the_empty_call_needs_no_device(entry_name):
  entry = getattr(_lib.lib(), entry_name)
  assert _raw_call(entry, n_seqs=0, table=None, off=(0,), windows=()) == _lib.DV_OK
  assert _raw_call(entry, windows=((0, 2, 2, 0, -1, 0, 0),), outputs=False) == _lib.DV_OK      # reads, no haplotypes
  assert _raw_call(entry, options=None, windows=((0, 2, 2, 0, -1, 0, 0),)) == _lib.DV_OK       # NULL options: defaults
  stats = _lib.DvFastPassStats(1, 1, 1, 1, 1)
  assert _lib.lib().dv_fast_pass_device_last_stats(C.byref(stats)) == _lib.DV_OK
  if entry_name.endswith('device'):
    assert (stats.haplotypes, stats.haplotypes_on_host, stats.pairs, stats.cells, stats.launches) == (0, 0, 0, 0, 0)


def test_no_device_is_an_error_not_a_fallback():
  if _lib.lib().dv_device_count() > 0:
    pytest.skip('a GPU is present')
  assert _raw_call(_lib.lib().dv_fast_pass_batch_device) == _lib.DV_ERR_NO_DEVICE
  assert 'dv_fast_pass_batch' in _lib.last_error()
  assert _raw_call(_lib.lib().dv_fast_pass_batch) == _lib.DV_OK


def _align(w, sequences, preset, in_phases=0):
  o = dict(w['options'])
  a = F.FastPassAligner(ref_prefix_len=w['ref_prefix_len'], ref_suffix_len=w['ref_suffix_len'],
                        read_size=len(sequences[0]), realignment_similarity_threshold=0.5, **o)
  a.set_reference(w['reference'], 1000)
  a.set_haplotypes(w['haplotypes'])
  if preset:
    a.set_reads(preset)
  if in_phases:
    a.stage(F.ALIGN_IN_PHASES, in_phases)
  res = a.align_reads(sequences)
  state = [(a.haplotype_alignment(k), [a.read_alignment(k, r) for r in range(len(preset) + len(sequences))])
           for k in range(len(w['haplotypes']))]
  return res, state


@pytest.mark.parametrize('seed', [5, 6, 7])
def test_align_reads_through_the_split_steps(seed):
  """begin_alignments + the batch's host fast pass + install_fast_pass + collect_alignments leave what
  prepare_alignments leaves: align_reads' results and the aligner's state, field for field."""
  moved = 0
  for w in K.seeded(seed, 4):
    if w['reference'] not in w['haplotypes']:
      continue
    for preset in ([], w['reads'][:2]):
      sequences = w['reads'][len(preset):]
      want = _align(w, sequences, preset)
      assert _align(w, sequences, preset, 1) == want
      assert _align(w, sequences, preset, 2) == want, w['name']
      moved += sum(1 for status, _, _ in want[0] if status == 1)
      assert any('=' in ra.cigar and ra.cigar.count('=') == 1 and ra.cigar[:-1].isdigit()
                 for _, rows in want[1] for ra in rows)                 # "<L>=" rows of the fast pass are compared
  assert moved > 20
