"""The device trace-back of the local aligner, as far as a machine without a GPU can check it
(include/dvhip.h: dv_realign_traceback_stats, dv_local_align_device_last_traceback_stats, dv_local_align_band):

  * the new symbols are declared, exported and mirrored, the stats struct and the two limits agree with _lib;
  * a null argument is DV_ERR_INVALID_ARGUMENT, and an empty pair list leaves all-zero trace-back stats;
  * dv_local_align_band -- the band LocalAligner::banded_cigar ends with and the number of M/I/D runs, the two
    figures that decide whether the kernel traces a pair back itself -- on hand-made pairs.
"""
import ctypes as C
import os
import re

import numpy as np

from deepvariant_amd import _lib
from deepvariant_amd import fast_pass_aligner as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dv_local_align_device_last_traceback_stats', 'dv_local_align_band')
REALIGNER = (4, 6, 8, 1)
LETTERS = np.array(list('ACGT'))


def _random(rng, n):
  return ''.join(rng.choice(LETTERS, size=n))


def test_symbols_are_declared_exported_and_mirrored():
  text = open(os.path.join(ROOT, 'include', 'dvhip.h')).read()
  l = _lib.lib()
  for name in NEW_SYMBOLS:
    assert re.search(r'\b%s\s*\(' % name, text), name
    assert name in _lib.ABI_SYMBOLS and hasattr(l, name), name
  assert 'dv_realign_traceback_stats' in text
  assert re.search(r'#define DV_ABI_VERSION 8\b', text) and l.dv_abi_version() == 8
  for name in ('DV_LOCAL_ALIGN_DEVICE_MAX_BAND', 'DV_LOCAL_ALIGN_DEVICE_MAX_RUNS'):
    assert int(re.search(r'#define %s (\d+)' % name, text).group(1)) == getattr(_lib, name)
  assert 2 * _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND + 1 <= 64       # one band diagonal per lane of a wave


def test_traceback_stats_layout():
  assert C.sizeof(_lib.DvRealignTracebackStats) == 32
  assert [f[0] for f in _lib.DvRealignTracebackStats._fields_] == ['traced_on_device', 'traced_on_host', 'band_cells',
                                                                   'widest_band']
  text = open(os.path.join(ROOT, 'include', 'dvhip.h')).read()
  body = re.search(r'typedef struct dv_realign_traceback_stats \{(.*?)\} dv_realign_traceback_stats;', text, re.S).group(1)
  assert re.findall(r'int64_t (\w+);', body) == ['traced_on_device', 'traced_on_host', 'band_cells', 'widest_band']


def test_null_arguments():
  l = _lib.lib()
  band, runs = C.c_int32(7), C.c_int32(7)
  assert l.dv_local_align_device_last_traceback_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert 'dv_local_align_device_last_traceback_stats' in _lib.last_error()
  assert l.dv_local_align_band(None, b'ACGT', *REALIGNER, C.byref(band), C.byref(runs)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_local_align_band(b'ACGT', None, *REALIGNER, C.byref(band), C.byref(runs)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_local_align_band(b'ACGT', b'ACGT', *REALIGNER, None, C.byref(runs)) == _lib.DV_ERR_INVALID_ARGUMENT
  assert l.dv_local_align_band(b'ACGT', b'ACGT', *REALIGNER, C.byref(band), None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert 'dv_local_align_band' in _lib.last_error()
  assert (band.value, runs.value) == (7, 7)


def test_stats_are_zero_after_an_empty_pair_list():
  stats = _lib.DvRealignTracebackStats(1, 2, 3, 4)
  got = F.local_align_pairs_device(['ACGT'], [], with_traceback_stats=True)
  assert got[0] == []
  assert _lib.lib().dv_local_align_device_last_traceback_stats(C.byref(stats)) == _lib.DV_OK
  for s in (stats, got[1]):
    assert (s.traced_on_device, s.traced_on_host, s.band_cells, s.widest_band) == (0, 0, 0, 0)
  # the return value without the new keyword is what it was
  assert F.local_align_pairs_device(['ACGT'], []) == []
  res, device_stats = F.local_align_pairs_device(['ACGT'], [], with_stats=True)
  assert res == [] and isinstance(device_stats, _lib.DvRealignDeviceStats)
  res, device_stats, traceback = F.local_align_pairs_device(['ACGT'], [], with_stats=True, with_traceback_stats=True)
  assert isinstance(device_stats, _lib.DvRealignDeviceStats) and isinstance(traceback, _lib.DvRealignTracebackStats)


def test_band_and_runs_of_hand_made_pairs():
  rng = np.random.default_rng(23)
  reference = _random(rng, 400)
  # an exact copy: equal lengths, band |0| + 1, one M run
  copy = reference[100:250]
  assert F.local_align_band(reference, copy, *REALIGNER) == (1, 1)
  assert F.local_align(reference, copy, *REALIGNER).cigar == b'150='
  # one 5-base deletion: the reference side is 5 longer, band 5 + 1, M D M
  deletion = reference[100:175] + reference[180:255]
  assert F.local_align_band(reference, deletion, *REALIGNER) == (6, 3)
  assert re.fullmatch(rb'\d+=5D\d+=', F.local_align(reference, deletion, *REALIGNER).cigar)
  # a 5-base insertion and a 5-base deletion 60 bases apart in a 200-base read: equal lengths, so the band
  # starts at 1 and has to double past the 5-base shift between the two edits: 1 -> 2 -> 4 -> 8; M I M D M
  both = reference[100:170] + 'ACCAT' + reference[170:230] + reference[235:300]
  assert len(both) == 200
  assert re.fullmatch(rb'\d+=5I\d+=5D\d+=', F.local_align(reference, both, *REALIGNER).cigar)   # a gap may shift by a base
  assert F.local_align_band(reference, both, *REALIGNER) == (8, 5)
  # nothing aligns: no CIGAR
  assert F.local_align_band(reference, 'N' * 30, *REALIGNER) == (0, 0)
  # and where dv_local_align itself fails (an empty query)
  assert F.local_align_band(reference, '', *REALIGNER) == (0, 0)
