"""HIP encoder vs oracle on BOTH routes of the kernel's phase D (GPU), bit-exact.

encode_items_kernel renders an item's read rows either as a two-stage pipeline (window of at most 256 columns and every
kept read's CIGAR inside the LDS cache) or row by row, one pass per 256 columns, CIGARs beyond the cache read from
global memory 64 operations at a time.  The random inputs of the other encoder tests take the first route almost
everywhere; the inputs here (tests/encoder_cases.py, proven by tests/test_encoder_cases_cpu.py) sit on every boundary
between the two: CIGARs of exactly 7 ... 200 operations, windows of 1-3 column passes, both routes inside one launch,
every source of the cache geometry, pixels padded up to 64 channels, and the shape the encoder refuses.

Why a wrong kernel fails here (the conditions are tests/test_encoder_cases_cpu.py's): with the two routes' condition
swapped, items wider than 256 columns would run the single-pass pipeline, whose walk resolves columns 0-255 only, while
the oracle's images have pixels, indel anchors and boundary-spanning reads in columns >= 256 and >= 512, and items with
CIGARs beyond the cache would read them from a cache that holds their first 8 / 16 words; with the chunk offset of the
global CIGAR load dropped, operations 0-63 would be walked again in place of 64-127 and 128-191, while the oracle's
image of the same reads cut after operation 64 (128) differs from the full one, i.e. those operations draw inside the
window.  With the padding fix of store_pixel reverted, channels 16 and up hold whatever the registers behind the pixel
held, where the test demands zeros over a 0xAB prefill."""
import os
import subprocess
import sys

import numpy as np
import pytest

from deepvariant_amd import dv_types as T
from tests import encoder_cases as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(cases):
  from deepvariant_amd.pileup_image_native import PileupImageEncoderNative
  from oracle import oracle as O
  encoders = {}
  for case in cases:
    opts = case.options()
    key = (tuple(case.channels), case.width, case.height, tuple(sorted(case.okw.items())))
    enc = encoders.setdefault(key, PileupImageEncoderNative(opts))
    call, ref, reads, start, combo = case.build()
    got = enc.build_pileup_for_one_sample(call, ref, reads, start, combo, T.SampleOptions(pileup_height=case.height),
                                          mean_coverage=case.mean_coverage, channels_to_blank=case.blank_enums())
    want = O.build_pileup(opts, call, ref, reads, start, combo, pileup_height=case.height,
                          mean_coverage=case.mean_coverage, channels_to_blank=case.blank_enums())
    np.testing.assert_array_equal(got, want, err_msg=case.name)


@pytest.mark.parametrize('width', E.BOUNDARY_WIDTHS)
def test_operation_count_boundaries(width):
  """(a) Every read of an item with exactly n operations, n around the cache sizes (8, 16) and the chunk ends (64, 128);
  one long read among short ones; deeper than the image, a blanked channel, mean_coverage below the reads."""
  cases = E.boundary_cases(width)
  assert {c.max_ops for c in cases} >= set(E.OP_COUNTS)
  _compare(cases)


@pytest.fixture(scope='module')
def mixed():
  from oracle import oracle as O
  opts, batch = E.mixed_batch()
  want, want_rows = O.encode_packed(opts, batch, 7)
  want.setflags(write=False)
  want_rows.setflags(write=False)
  return opts, batch, want, want_rows


def test_both_routes_in_one_launch(mixed):
  """(b) Items of the pipelined and of the plain route alternate inside one dv_encode_batch call and share reads."""
  from deepvariant_amd.pileup_image_native import _Encoder
  opts, batch, want, want_rows = mixed
  out, rows = _Encoder(opts, opts.width).encode(batch, 7)
  np.testing.assert_array_equal(rows, want_rows)
  np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize('width', E.PASS_WIDTHS)
def test_column_passes(width):
  """(c) 1, 2 and 3 passes of 256 columns, short CIGARs only and long ones, reference bands of 5 and of 2."""
  _compare(E.pass_cases(width))


@pytest.mark.parametrize('name,channels,out_channels', E.PADDED, ids=['%s_to_%d' % (n, oc) for n, _, oc in E.PADDED])
def test_padded_channels(name, channels, out_channels):
  """(d) out_channels > n_channels: the oracle's pixels, then zeros -- written into a tensor that held 0xAB before, and
  through the host-output path."""
  import torch
  from deepvariant_amd.device_batch import DeviceBatch
  from deepvariant_amd.pileup_image_native import PileupImageEncoderNative
  from oracle import oracle as O
  c = len(channels)
  for width in E.padded_widths(out_channels):
    case = E.padded_case(name, channels, width)
    opts = case.options()
    call, ref, reads, start, combo = case.build()
    want = np.zeros((case.height, width, out_channels), np.uint8)
    want[..., :c] = O.build_pileup(opts, call, ref, reads, start, combo, pileup_height=case.height)
    native = PileupImageEncoderNative(opts)
    batch = native.pack_one_item(call, ref, reads, start, combo, case.height)
    enc = native._encoder(width)   # pylint: disable=protected-access
    out, rows = enc.encode(batch, out_channels)
    np.testing.assert_array_equal(out.reshape(want.shape), want, err_msg='host output, width %d' % width)
    assert 0 < rows[0] < len(reads)
    out_t = torch.full((batch.out_bytes(out_channels),), 0xAB, dtype=torch.uint8, device='cuda:0')
    rows_t = torch.full((1,), -1, dtype=torch.int32, device='cuda:0')
    DeviceBatch(batch, torch.device('cuda:0')).encode(enc, out_channels, out_t, rows_t)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_t.cpu().numpy().reshape(want.shape), want,
                                  err_msg='device output, width %d' % width)
    assert int(rows_t.cpu()[0]) == rows[0]


def test_cache_geometry_sources(mixed):
  """(e) The CIGAR cache sized from the host batch, from a device batch's hints, and without a hint (max_cigar_ops = 0:
  8 words, so reads of 9-16 operations move their items to the plain route): the same bytes every time."""
  import torch
  from deepvariant_amd.device_batch import DeviceBatch
  from deepvariant_amd.pileup_image_native import _Encoder
  opts, batch, want, want_rows = mixed
  enc = _Encoder(opts, opts.width)
  dev = torch.device('cuda:0')
  hinted, unknown = DeviceBatch(batch, dev), DeviceBatch(batch, dev)
  assert (hinted.c.max_cigar_ops, hinted.c.max_item_height) == (200, E.MIXED_HEIGHT)
  unknown.c.max_cigar_ops = 0
  results = [enc.encode(batch, 7)]
  for db in (hinted, unknown):
    out = torch.full((batch.out_bytes(7),), 0xAB, dtype=torch.uint8, device=dev)
    rows = torch.full((batch.n_items,), -1, dtype=torch.int32, device=dev)
    db.encode(enc, 7, out, rows)
    torch.cuda.synchronize()
    results.append((out.cpu().numpy(), rows.cpu().numpy()))
  for (out, rows), source in zip(results, ('host batch', 'device batch with hints', 'device batch without hints')):
    np.testing.assert_array_equal(rows, want_rows, err_msg=source)
    np.testing.assert_array_equal(out, want, err_msg=source)


def _child(**env):
  done = subprocess.run([sys.executable, '-m', 'tests.encoder_cache_child'], cwd=ROOT, env=dict(os.environ, **env),
                        capture_output=True, text=True, timeout=300)
  assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
  return done.stdout


@pytest.mark.parametrize('env', [dict(DV_CIG_CACHE='32'), dict(DV_CIG_CACHE='64'),
                                 dict(DV_CIG_CACHE='32', DV_CIG_KEPT_MAX='1')],
                         ids=['cache32', 'cache64', 'cache32_kept_max'])
def test_cig_cache_knob_in_a_child_process(env):
  """(f) DV_CIG_CACHE (read once per process) changes the cache's indexing and the LDS layout, not a byte of output."""
  n = E.mixed_batch()[1].n_items
  assert 'items equal to the oracle: %d/%d' % (n, n) in _child(**env)


def test_cig_cache_64_with_kept_max_is_refused_in_a_child_process():
  """(f) DV_CIG_CACHE=64 together with DV_CIG_KEPT_MAX sizes the cache for 64 words x 256 reads = 64 KiB, more than a
  launch of this kernel may ask for with the other tables next to it: the encoder refuses the geometry (test (g)'s
  check) instead of failing in the launch.  The layout with 256 kept rows is covered by cache32_kept_max above."""
  out = _child(DV_CIG_CACHE='64', DV_CIG_KEPT_MAX='1')
  assert 'refused: status -1' in out and 'width 221' in out and 'out_channels 7' in out
  assert 'items equal to the oracle' not in out


def test_oversized_lds_request_is_refused(mixed):
  """(g) width 2049 with 64 output channels needs 4 x 131 KB of row buffers: DV_ERR_INVALID_ARGUMENT naming both, before
  anything is staged or launched; the process goes on encoding."""
  from deepvariant_amd import _lib
  from deepvariant_amd.pileup_image_native import PileupImageEncoderNative, _Encoder
  case = E.Case('refused_w2049', T.PILEUP_CHANNELS_WITH_INSERT_SIZE, 2049, 20, [8] * 8)
  call, ref, reads, start, combo = case.build()
  native = PileupImageEncoderNative(case.options())
  batch = native.pack_one_item(call, ref, reads, start, combo, case.height)
  with pytest.raises(_lib.DvError) as err:
    native._encoder(2049).encode(batch, 64)   # pylint: disable=protected-access
  assert err.value.status == _lib.DV_ERR_INVALID_ARGUMENT
  assert 'width 2049' in _lib.last_error() and 'out_channels 64' in _lib.last_error()
  assert E.lds_bytes(2049, 64, 7, 20, 5, 8) > 64 * 1024
  opts, mixed_batch, want, want_rows = mixed
  out, rows = _Encoder(opts, opts.width).encode(mixed_batch, 7)
  np.testing.assert_array_equal(rows, want_rows)
  np.testing.assert_array_equal(out, want)
