"""block35.hip (each Inception-A block of the 35x35 stage, mixed0..mixed2, as ONE launch: the 1x1 heads, the
average pool, the 5x5 and the 3x3 -> 3x3 pair on tiles of one whole map, reducers and intermediates in LDS)
against the per-layer launches (GPU): same K order, same fp16 rounding of every intermediate, same pooling
sums -- the 2048 features and the probabilities must be BIT-identical to DV_NO_BLOCK35=1 (grouped heads,
imgconv 5x5, chain 3x3 -> 3x3) and to DV_NO_CHAIN=1 (every layer on its own).  Shapes: WGS 221-wide (10x25
maps), 6-channel WGS, PacBio 147-wide (10x16 maps), ONT 199-wide (10x22 maps); batches smaller than the grid,
larger than it, and below the model's max_batch."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


_KNOBS = ('DV_NO_BLOCK35', 'DV_NO_CHAIN', 'DV_NO_AVG_EPI')


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
  probs = m(x).cpu().numpy()
  return probs, m.debug_tensor(-1, x.shape[0])


def _forward(shape, weights, x, env, max_batch=None):
  return _run(_model(shape, weights, max_batch or x.shape[0], env), x)


def _images(n, shape, seed):
  h, w, c = shape
  rng = np.random.default_rng(seed)
  x = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
  x[: n // 2, 40:] = 0                     # pileup-like: zero rows below the reads
  return x


def _same(a, b, what):
  np.testing.assert_array_equal(a[1], b[1], err_msg='features: ' + what)
  np.testing.assert_array_equal(a[0], b[0], err_msg='probabilities: ' + what)


@pytest.mark.parametrize('shape,n', [((100, 221, 7), 1203), ((100, 221, 7), 3), ((100, 221, 6), 64),
                                     ((100, 147, 10), 601), ((100, 147, 10), 5), ((100, 199, 9), 130)])
def test_block35_is_bit_identical_to_the_per_layer_launches(shape, n):
  from oracle import inception_ref as R
  weights = R.make_random_model(shape[2], seed=41).export_flat()
  xd = torch.from_numpy(_images(n, shape, 19)).cuda()
  fused = _forward(shape, weights, xd, {})
  assert np.isfinite(fused[0]).all()
  _same(fused, _forward(shape, weights, xd, {'DV_NO_BLOCK35': '1'}), 'DV_NO_BLOCK35')
  _same(fused, _forward(shape, weights, xd, {'DV_NO_CHAIN': '1'}), 'DV_NO_CHAIN')


def test_block35_with_a_batch_smaller_than_the_model():
  """max_batch above the batch: tiles past the batch are never touched."""
  from oracle import inception_ref as R
  shape = (100, 221, 7)
  weights = R.make_random_model(shape[2], seed=7).export_flat()
  xd = torch.from_numpy(_images(37, shape, 3)).cuda()
  _same(_forward(shape, weights, xd, {}, max_batch=300),
        _forward(shape, weights, xd, {'DV_NO_BLOCK35': '1'}, max_batch=300), 'max_batch 300, batch 37')


def test_block35_with_blank_row_skipping_on_and_off():
  from oracle import inception_ref as R
  shape = (100, 221, 7)
  weights = R.make_random_model(shape[2], seed=9).export_flat()
  xd = torch.from_numpy(_images(96, shape, 5)).cuda()
  want = _forward(shape, weights, xd, {'DV_NO_BLOCK35': '1'})
  m = _model(shape, weights, 96, {})
  for on in (False, True):
    m.set_blank_skip(on)
    _same(_run(m, xd), want, 'blank skip %s' % on)


def test_block35_without_the_pooling_epilogue():
  """DV_NO_AVG_EPI=1: the per-layer path pools in avgpool3s1_kernel; block35 still pools in LDS -- same bits."""
  from oracle import inception_ref as R
  shape = (100, 199, 9)
  weights = R.make_random_model(shape[2], seed=12).export_flat()
  xd = torch.from_numpy(_images(50, shape, 8)).cuda()
  _same(_forward(shape, weights, xd, {'DV_NO_AVG_EPI': '1'}),
        _forward(shape, weights, xd, {'DV_NO_AVG_EPI': '1', 'DV_NO_BLOCK35': '1'}), 'DV_NO_AVG_EPI')


def test_block35_after_calibration():
  """The block reads the shifts dv_model_calibrate rewrites: calibrated models agree bit for bit too."""
  from oracle import inception_ref as R
  shape = (100, 221, 7)
  weights = R.make_random_model(shape[2], seed=23).export_flat()
  cal = torch.from_numpy(_images(48, shape, 515)).cuda()
  xd = torch.from_numpy(_images(40, shape, 77)).cuda()
  got = []
  for env in ({}, {'DV_NO_BLOCK35': '1'}):
    m = _model(shape, weights, 64, env)
    corr = m.calibrate(cal)
    assert np.abs(corr).max() > 0
    got.append(_run(m, xd))
  _same(got[0], got[1], 'calibrated')


def test_block35_against_the_oracle():
  """...and within the 1e-3 bar of the fp32 restatement (oracle/inception_ref.py)."""
  from oracle import inception_ref as R
  shape = (100, 221, 7)
  ref = R.make_random_model(shape[2], seed=13)
  x = _images(24, shape, 17)
  p, _ = _forward(shape, ref.export_flat(), torch.from_numpy(x).cuda(), {})
  with torch.no_grad():
    want = ref(torch.from_numpy(x)).numpy()
  assert np.abs(p - want).max() <= 1e-3
