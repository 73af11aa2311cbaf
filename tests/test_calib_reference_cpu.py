"""The float64 reference the calibration's exact pipeline R is pinned to (tests/calib_reference.py), checked on the
CPU: two independent float64 restatements of the classifier agree to rounding, another float32 evaluation is
within 1e-5 of them, and two single-pixel geometry errors move a logit by far more than the GPU bar
(tests/test_hip_calib_pipelines.py: 16 x d32) -- which is what makes that bar worth having."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import calib_emulation as E
from tests import calib_reference as CR


def _walk64(ref64, images_u8, walk=E._Walk):
  with torch.no_grad():
    return walk(ref64, False).logits(torch.from_numpy(images_u8)).numpy()


@pytest.mark.parametrize('shape', [s for s, _ in CR.CASES])
def test_two_float64_restatements_agree_and_float32_is_close(shape):
  """The oracle runs avg-pool -> conv -> BatchNorm as Keras states them; the emulation's walk folds BatchNorm into the
  weights and commutes the pooled projection (1x1 conv, then the average) as the product does."""
  ref = CR.reference(shape)
  l64 = ref['l64']
  w64 = _walk64(ref['ref64'], ref['images'])
  assert w64.dtype == np.float64
  scale = float(np.abs(l64).max())
  diff = float(np.abs(w64 - l64).max())
  print('%s: max|l64| %.3g, float64 walk - float64 oracle %.2e, d32 %.2e' % (shape, scale, diff, ref['d32']))
  assert diff <= 1e-12 * scale
  assert 0.0 < ref['d32'] <= 1e-5     # keeps the GPU bar of 16 x d32 meaningful (the reference alone: <= 2.2e-6)


class _PoolDivisor(E._Walk):
  """mixed0's pooled projection divides its top-left output by 9 (every cell of the window) where 4 cells are
  inside the map."""

  def pooled_projection(self, cb, x, keep_f32=False):
    if cb is not self.ref.mixed_a[0]['bp'][0]:
      return super().pooled_projection(cb, x, keep_f32)
    w, shift = E._folded(cb)
    avg = F.avg_pool2d(F.conv2d(x, w), 3, stride=1, padding=1, count_include_pad=False)
    avg[:, :, 0, 0] *= 4.0 / 9.0
    return self._act(self.index[id(cb)], avg + shift[None, :, None, None], keep_f32)


class _DroppedTap(E._Walk):
  """mixed0's 5x5 leaves out its bottom-right tap (kh = kw = 4: the input pixel (2, 2)) at the top-left output."""

  def conv(self, cb, x, keep_f32=False):
    if cb is not self.ref.mixed_a[0]['b5'][1]:
      return super().conv(cb, x, keep_f32)
    w, shift = E._folded(cb)
    z = F.conv2d(x, w, None, cb.conv.stride, cb.conv.padding) + shift[None, :, None, None]
    z[:, :, 0, 0] -= torch.einsum('oi,ni->no', w[:, :, 4, 4], x[:, :, 2, 2])
    return self._act(self.index[id(cb)], z, keep_f32)


@pytest.mark.parametrize('walk', [_PoolDivisor, _DroppedTap])
def test_a_single_pixel_geometry_error_is_far_above_the_bar(walk):
  shape = (100, 221, 7)
  ref = CR.reference(shape)
  bar = CR.FACTOR * ref['d32']
  moved = float(np.abs(_walk64(ref['ref64'], ref['images'], walk) - ref['l64']).max())
  print('%s at %s: a logit moves by %.2e = %.0f bars of %.2e' % (walk.__name__, shape, moved, moved / bar, bar))
  assert moved >= CR.INJECTED_MARGIN * bar
