"""mixed3.hip (the double-3x3 branch of the reduction block mixed3 -- 1x1 288->64, 3x3 64->96, 3x3 / 2 96->96 -- as
ONE launch on tiles of one whole map, both intermediates in LDS) against the three per-layer launches (GPU):
same K order, same fp16 rounding of both intermediates -- the mixed3 output, the 2048 features and the
probabilities must be BIT-identical to DV_NO_MIXED3_FUSE=1 (conv_mfma 1x1, imgconv 3x3, conv_mfma 3x3 / 2) and
to DV_NO_CHAIN=1 (no fused kernel of this family at all).  Shapes: WGS 221-wide (10x25 maps -> 4x12, two output
fragments), 6-channel WGS, PacBio 147-wide (10x16 -> 4x7, one partial fragment, precise mode), ONT 199-wide
(10x22 -> 4x10, second fragment partial); batches smaller than the grid, larger than it (every workgroup takes
2-3 tiles, the input ring wraps across tiles), and below the model's max_batch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


_KNOBS = ('DV_NO_MIXED3_FUSE', 'DV_NO_BLOCK35', 'DV_NO_CHAIN')


def _model(shape, weights, max_batch, env):
  from deepvariant_amd.inception_v3 import InceptionV3
  old = {k: os.environ.pop(k, None) for k in _KNOBS}
  os.environ.update(env)
  try:
    m = InceptionV3(shape, max_batch=max_batch)
    m.load_flat_weights(weights)
  finally:
    for k in _KNOBS:
      os.environ.pop(k, None)
      if old[k] is not None:
        os.environ[k] = old[k]
  return m


def _run(m, x):
  probs, outs = m.forward_outputs(x, ['mixed3'])
  return probs.cpu().numpy(), m.debug_tensor(-1, x.shape[0]), outs['mixed3'].cpu().numpy()


def _forward(shape, weights, x, env, max_batch=None):
  return _run(_model(shape, weights, max_batch or x.shape[0], env), x)


def _images(n, shape, seed):
  h, w, c = shape
  rng = np.random.default_rng(seed)
  x = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
  x[: n // 2, 40:] = 0                     # pileup-like: zero rows below the reads
  return x


def _same(a, b, what):
  np.testing.assert_array_equal(a[2], b[2], err_msg='mixed3: ' + what)
  np.testing.assert_array_equal(a[1], b[1], err_msg='features: ' + what)
  np.testing.assert_array_equal(a[0], b[0], err_msg='probabilities: ' + what)


def _branch_is_fused(m):
  """Whether the plan keeps the two tensors inside mixed3's double-3x3 branch in LDS only (dv_model_op_label)."""
  from deepvariant_amd import _lib
  lib = _lib.lib()
  labels = []
  for i in range(lib.dv_model_num_ops(m._handle)):
    buf = C.create_string_buffer(256)
    _lib.check(lib.dv_model_op_label(m._handle, i, buf, 256))
    labels.append(buf.value.decode())
  last = [i for i, l in enumerate(labels) if ' k=3x3 s=2 cin=96 cout=96 ' in l]
  assert len(last) == 1, labels
  i = last[0]
  assert ' k=1x1 s=1 ' in labels[i - 2] and ' cout=64 ' in labels[i - 2], labels[i - 2]
  assert ' k=3x3 s=1 cin=64 cout=96 ' in labels[i - 1], labels[i - 1]
  lds = [l.endswith('lds_only=1') for l in labels[i - 2:i + 1]]
  assert lds in ([True, True, False], [False, False, False]), labels[i - 2:i + 1]
  return lds[0]


@pytest.mark.parametrize('shape,n', [((100, 221, 7), 3), ((100, 221, 7), 601), ((100, 147, 10), 5),
                                     ((100, 199, 9), 130), ((100, 221, 6), 64)])
def test_mixed3_is_bit_identical_to_the_per_layer_launches(shape, n):
  from oracle import inception_ref as R
  weights = R.make_random_model(shape[2], seed=41).export_flat()
  xd = torch.from_numpy(_images(n, shape, 19)).cuda()
  m = _model(shape, weights, n, {})
  assert _branch_is_fused(m)
  fused = _run(m, xd)
  assert np.isfinite(fused[0]).all() and np.abs(fused[2]).max() > 0
  unfused = _model(shape, weights, n, {'DV_NO_MIXED3_FUSE': '1'})
  assert not _branch_is_fused(unfused)
  _same(fused, _run(unfused, xd), 'DV_NO_MIXED3_FUSE')
  _same(fused, _forward(shape, weights, xd, {'DV_NO_CHAIN': '1'}), 'DV_NO_CHAIN')


def test_mixed3_with_a_batch_smaller_than_the_model():
  """max_batch above the batch: tiles past the batch are never touched."""
  from oracle import inception_ref as R
  shape = (100, 221, 7)
  weights = R.make_random_model(shape[2], seed=7).export_flat()
  xd = torch.from_numpy(_images(37, shape, 3)).cuda()
  _same(_forward(shape, weights, xd, {}, max_batch=300),
        _forward(shape, weights, xd, {'DV_NO_MIXED3_FUSE': '1'}, max_batch=300), 'max_batch 300, batch 37')


def test_mixed3_with_blank_row_skipping_on_and_off_and_without_block35():
  """...and DV_NO_BLOCK35=1 (the 35x35 blocks per layer) still fuses mixed3's branch and agrees."""
  from oracle import inception_ref as R
  shape = (100, 221, 7)
  weights = R.make_random_model(shape[2], seed=9).export_flat()
  xd = torch.from_numpy(_images(96, shape, 5)).cuda()
  want = _forward(shape, weights, xd, {'DV_NO_MIXED3_FUSE': '1'})
  m = _model(shape, weights, 96, {})
  for on in (False, True):
    m.set_blank_skip(on)
    _same(_run(m, xd), want, 'blank skip %s' % on)
  m = _model(shape, weights, 96, {'DV_NO_BLOCK35': '1'})
  assert _branch_is_fused(m)
  _same(_run(m, xd), want, 'DV_NO_BLOCK35')


def test_mixed3_after_calibration():
  """The branch reads the shifts dv_model_calibrate rewrites: calibrated models agree bit for bit too."""
  from oracle import inception_ref as R
  shape = (100, 221, 7)
  weights = R.make_random_model(shape[2], seed=23).export_flat()
  cal = torch.from_numpy(_images(48, shape, 515)).cuda()
  xd = torch.from_numpy(_images(40, shape, 77)).cuda()
  got = []
  for env in ({}, {'DV_NO_MIXED3_FUSE': '1'}):
    m = _model(shape, weights, 64, env)
    corr = m.calibrate(cal)
    assert np.abs(corr).max() > 0
    got.append(_run(m, xd))
  _same(got[0], got[1], 'calibrated')


def test_mixed3_against_the_oracle():
  """...and within the 1e-3 bar of the fp32 restatement (oracle/inception_ref.py)."""
  from oracle import inception_ref as R
  shape = (100, 221, 7)
  ref = R.make_random_model(shape[2], seed=13)
  x = _images(24, shape, 17)
  p = _forward(shape, ref.export_flat(), torch.from_numpy(x).cuda(), {})[0]
  with torch.no_grad():
    want = ref(torch.from_numpy(x)).numpy()
  assert np.abs(p - want).max() <= 1e-3
