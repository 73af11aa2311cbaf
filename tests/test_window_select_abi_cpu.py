"""The window pass' C ABI without a GPU (dv_select_windows_batch, include/dvhip.h): the symbols exist, the option
struct's layout matches the ctypes mirror, argument errors are reported before any device work, DV_ABI_VERSION is
still 8, and the batch plan's new sections hold against tools/count_batch_layout_check.cpp."""
import ctypes as C
import os
import re
import subprocess

import pytest

from deepvariant_amd import _lib
from deepvariant_amd import allelecounter as A
from deepvariant_amd.realigner import realigner as R
from deepvariant_amd.realigner import window_selector as ws

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(ROOT, 'include', 'dvhip.h')
LINEAR, THRESHOLD = 2, 1


def test_symbols_and_version():
  lib = _lib.lib()
  for name in ('dv_select_windows_batch', 'dv_windows_arrays', 'dv_windows_free'):
    assert getattr(lib, name) is not None and name in _lib.ABI_SYMBOLS
  assert lib.dv_abi_version() == 8
  with open(HEADER) as f:
    header = f.read()
  assert re.search(r'#define DV_ABI_VERSION 8\b', header)
  for name in ('dv_window_options', 'dv_windows', 'dv_select_windows_batch', 'dv_windows_arrays', 'dv_windows_free',
               'DV_WINDOW_MODEL_VARIANT_READS 1', 'DV_WINDOW_MODEL_ALLELE_COUNT_LINEAR 2'):
    assert name in header
  assert (ws.VARIANT_READS, ws.ALLELE_COUNT_LINEAR) == (THRESHOLD, LINEAR)


def test_struct_layout():
  # the static_assert of csrc/window_select.hip holds the C side to the same size
  o = _lib.DvWindowOptions
  assert C.sizeof(o) == 64
  assert (o.bias.offset, o.coeff_reference.offset, o.min_windows_distance.offset) == (20, 40, 44)
  assert (o.decision_boundary.offset, o.decision_boundary.size, o.want_debug.offset) == (48, 8, 56)
  assert o.coeff_insertion.size == 4                      # C floats: the proto fields' precision


def _options(model=LINEAR, lo=0, hi=0, distance=80):
  return _lib.DvWindowOptions(model, lo, hi, 2, 0, -0.68, 3.0, -0.09, 2.5, 1.8, -0.06, distance, 3.0, 0, 0)


def _status(options, n=1, windows=True, reads=True):
  lib = _lib.lib()
  slots = (C.c_void_p * 1)()
  out, win = (C.c_void_p * 1)(), (C.c_void_p * 1)()
  rc = lib.dv_select_windows_batch(n, slots if reads else None, slots, None,
                                   C.byref(options) if options is not None else None, out, win if windows else None, None)
  assert not out[0] and not win[0]                        # nothing is left allocated
  return rc, lib.dv_last_error().decode()


@pytest.mark.parametrize('options,message', [
    (_options(model=0), 'unknown window selector model type'), (_options(model=3), 'unknown window selector model type'),
    (_options(model=THRESHOLD, lo=5, hi=4), 'max_num_supporting_reads'), (_options(lo=1, hi=0), 'max_num_supporting_reads'),
    (_options(distance=-1), 'min_windows_distance')])
def test_bad_options_are_invalid_arguments(options, message):
  rc, text = _status(options)
  assert rc == -1 and message in text and 'dv_select_windows_batch' in text      # DV_ERR_INVALID_ARGUMENT
  with pytest.raises(_lib.DvError):
    _lib.check(rc)


def test_null_arguments():
  good = _options()
  assert _status(None)[0] == -1
  assert _status(good, windows=False)[0] == -1
  assert _status(good, reads=False)[0] == -1
  assert _status(good)[0] == -1                           # a null read table, found before any device call
  rc, message = _status(good, n=-1)
  assert rc == -1 and 'dv_select_windows_batch' in message
  lib = _lib.lib()
  # an empty batch is not an error and needs no device; counts_out may be NULL
  assert lib.dv_select_windows_batch(0, None, None, None, C.byref(good), None, None, None) == 0
  assert lib.dv_windows_arrays(None, None, None, None, None) == -1
  lib.dv_windows_free(None)


def test_options_mirror_the_selector_config():
  config = R.realigner_config(ws_use_window_selector_model=True).ws_config
  o = A._window_options_struct(config, True)              # pylint: disable=protected-access
  m = config.window_selector_model.allele_count_linear_model
  assert (o.model_type, o.min_allele_support, o.min_windows_distance, o.want_debug) == (LINEAR, 2, 80, 1)
  assert o.coeff_insertion == C.c_float(m.coeff_insertion).value and o.decision_boundary == 3.0
  config = R.realigner_config(enable_strict_insertion_filter=True).ws_config
  o = A._window_options_struct(config, False)             # pylint: disable=protected-access
  assert (o.model_type, o.min_num_supporting_reads, o.max_num_supporting_reads) == (THRESHOLD, 2, 300)
  assert o.enable_strict_insertion_filter == 1 and o.want_debug == 0
  assert A._window_key(config, False) != A._window_key(config, True)              # pylint: disable=protected-access


def test_the_switch_is_off_by_default(monkeypatch):
  monkeypatch.delenv('DV_WINDOWS_DEVICE', raising=False)
  assert not ws.windows_on_device()
  monkeypatch.setenv('DV_WINDOWS_DEVICE', '1')
  assert ws.windows_on_device()


def test_batch_layout_with_the_window_sections(tmp_path):
  """plan_batch and second_image with the window pass on, against the tool's own statement of every offset."""
  hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
  exe = str(tmp_path / 'count_batch_layout_check')
  subprocess.check_call([hipcc, '-std=c++17', '-O1', '-I' + os.path.join(ROOT, 'include'),
                         '-I' + os.path.join(ROOT, 'deepvariant_amd', 'csrc'),
                         os.path.join(ROOT, 'tools', 'count_batch_layout_check.cpp'), '-o', exe])
  out = subprocess.check_output([exe]).decode()
  assert re.search(r'^\d+ cases, 0 mismatches$', out.strip().splitlines()[-1]) and int(out.split()[0]) > 400000
