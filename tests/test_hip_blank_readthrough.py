"""Where the stem's consumers get their blank rows from against the dense kernels (GPU).

By default stem_b takes the conv2 rows below stem_a's last computed tile row straight from the all-blank image's response
(stem_a copies no tile), and copies of its own blank rows only the strip the 3x3 80->192 reads, once per image.
DV_BLANK_COPY_TILES=1 keeps the earlier scheme: both producers copy every blank tile a computed tile of the consumer
touches.  Neither may be visible: the probabilities and the stem's output are compared BIT FOR BIT with the dense model
and with the copying model, on images whose rows used sit on every side of the tile boundaries of both links, next to
deeper neighbours (whose pile-up decides how far the 3x3 80->192's walk reads), after forwards that left other rows in
the same buffers, at a batch that does not fill the persistent grids, after calibration, with the rows hinted and with
the run-time switch.  The thresholds that make each case what it is are asserted from the rows used alone, with the
arithmetic of tests/test_hip_blank_skip.py's _expected_thresholds, before anything runs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS_USED = (0, 1, 13, 14, 26, 27, 28, 29, 37, 41, 42, 43, 47, 48, 55, 56, 99, 100)
STEM_A_TH, STEM_B_PH = 7, 6   # rows of a conv2 tile (stem_a) and of a pooled tile (stem_b)


def _model(shape, weights, max_batch, skip=True, copy_tiles=False):
  from deepvariant_amd.inception_v3 import InceptionV3
  old = {k: os.environ.pop(k, None) for k in ('DV_BLANK_SKIP', 'DV_BLANK_COPY_TILES')}
  if not skip:
    os.environ['DV_BLANK_SKIP'] = '0'
  if copy_tiles:
    os.environ['DV_BLANK_COPY_TILES'] = '1'
  try:
    m = InceptionV3(shape, max_batch=max_batch)
  finally:
    for k, v in old.items():
      os.environ.pop(k, None)
      if v is not None:
        os.environ[k] = v
  m.load_flat_weights(weights)
  return m


def _image(shape, r, rng, col=None):
  """Rows [0, r) used: random bytes, except that with `col` the last used row holds a single nonzero byte there."""
  h, w, c = shape
  im = np.zeros((h, w, c), np.uint8)
  if r > 0:
    im[:r] = rng.integers(0, 256, (r, w, c), dtype=np.uint8)
    if col is not None:
      im[r - 1] = 0
      im[r - 1, col, 0 if col == 0 else c - 1] = 1
  return im


def _mixed_batch(shape, seed):
  """(images, rows used): the hand-placed rows, a run of r = 37, r = 27 / r = 55 alternating, then encoded pileups."""
  rng = np.random.default_rng(seed)
  w = shape[1]
  imgs, rows = [], []
  for r in ROWS_USED:
    for col in (0, w - 1):
      imgs.append(_image(shape, r, rng, col))
      rows.append(r)
  for r in (37,) * 5 + (27, 55) * 4:
    imgs.append(_image(shape, r, rng))
    rows.append(r)
  from deepvariant_amd import calibration_set
  drawn = calibration_set.draw(shape, 64, seed=seed) if calibration_set.supported(shape) else None
  if drawn is not None:
    imgs.extend(drawn.cpu().numpy())
  x = np.stack(imgs)
  assert x.shape[0] <= 192
  return x, np.array(rows)


def _thresholds(x):
  """tests/test_hip_blank_skip.py's _expected_thresholds, and from them what each link reads and what is computed."""
  n, h, w = x.shape[0], x.shape[1], x.shape[2]
  nz = x.reshape(n, h, -1).any(axis=2)
  r = np.where(nz.any(axis=1), h - np.argmax(nz[:, ::-1], axis=1), 0)
  t2 = (r + 1) // 2
  t4 = (t2 + 2) // 2
  thr = np.stack([r, t2, t4, t4, (t4 + 1) // 2]).astype(np.int32)
  oh2 = (h - 3) // 2 + 1 - 2                 # conv 3x3/2 valid, conv 3x3 valid
  ph = (oh2 - 3) // 2 + 1                    # conv 3x3 same, max-pool 3x3/2 (the 1x1 keeps it)
  ow2 = (w - 3) // 2 + 1 - 2
  p4 = ((ph - 2) - 3) // 2 + 1               # the 3x3 80->192 valid, max-pooled 3x3/2 in its kernel
  pw4 = ((((ow2 - 3) // 2 + 1) - 2) - 3) // 2 + 1
  cut2 = np.minimum(oh2, STEM_A_TH * -(-t2 // STEM_A_TH))          # first conv2 row stem_a does not compute
  kb = -(-np.minimum(t4, ph) // STEM_B_PH)
  need2 = np.where(kb > 0, np.minimum(oh2, 2 * STEM_B_PH * kb + 2), 0)   # conv2 rows under stem_b's computed tiles
  cutb = np.minimum(ph, STEM_B_PH * -(-t4 // STEM_B_PH))           # first pooled row stem_b does not compute
  span = 31 // pw4 + 1                       # images a 32-position fragment of the 3x3 80->192's walk can touch
  m5 = np.minimum(thr[4], p4)
  deepest = np.array([m5[max(0, i - span):i + span + 1].max() for i in range(n)])
  need4 = np.where(deepest > 0, np.minimum(ph, 2 * deepest + 3), 0)       # stem_b rows under that walk
  return thr, dict(cut2=cut2, need2=need2, cutb=cutb, need4=need4)


def _check_preconditions(x, rows):
  thr, t = _thresholds(x)
  k = len(rows)
  np.testing.assert_array_equal(thr[0][:k], rows)
  cut2, need2, cutb, need4 = t['cut2'], t['need2'], t['cutb'], t['need4']

  def through(r):   # conv2 rows stem_b reads from the blank response, for the images of `r` rows used
    i = int(np.flatnonzero(rows == r)[0])
    return int(cut2[i]), int(need2[i])
  assert through(37) == (21, 26)             # rows 21-25
  assert through(27) == (14, 26)             # more than one tile row
  assert through(0) == (0, 14)               # everything a computed tile of stem_b reads
  assert through(47) == (28, 38)
  for r in (43, 100):                        # nothing read through
    c, nd = through(r)
    assert c >= nd
  assert (cut2 < need2).any() and (cut2 >= need2).any()
  # the strip stem_b copies: a run of r = 37 reads row 12 alone; the shallow image between two deep ones rows 12-18
  run37 = np.flatnonzero(rows == 37)[-3]     # the middle of the five: its neighbours are r = 37 too
  assert (cutb[run37], need4[run37]) == (12, 13)
  alt = np.flatnonzero(rows == 27)[-2]
  assert rows[alt - 1] == 55 and rows[alt + 1] == 55
  assert (cutb[alt], need4[alt]) == (12, 19)
  assert (cutb < need4).any() and (cutb >= need4).any()
  return thr


@pytest.mark.parametrize('shape', [(100, 221, 7), (100, 221, 6), (100, 199, 9), (100, 147, 10)])
def test_blank_rows_read_through_is_bit_identical(shape):
  from oracle import inception_ref as R
  x, rows = _mixed_batch(shape, seed=11)
  thr = _check_preconditions(x, rows)
  n = x.shape[0]
  w = R.make_random_model(shape[2], seed=29).export_flat()
  dense = _model(shape, w, n, skip=False)
  skip = _model(shape, w, n)
  copy = _model(shape, w, n, copy_tiles=True)
  xd = torch.from_numpy(x).cuda()

  def same(images, **kw):
    want = dense(images).cpu().numpy()
    k = images.shape[0]
    want_stem = dense.debug_tensor(-2, k)
    for m in (skip, copy):
      np.testing.assert_array_equal(m(images, **kw).cpu().numpy(), want)
      np.testing.assert_array_equal(m.debug_tensor(-2, k), want_stem)
    return want

  # stale rows: every row of the inter-kernel tensors computed, then none, then the mixed batch -- same buffers, same graph
  rng = np.random.default_rng(3)
  full = torch.from_numpy(rng.integers(1, 256, x.shape, dtype=np.uint8)).cuda()
  same(full)
  same(torch.zeros_like(xd))
  want = same(xd)
  np.testing.assert_array_equal(skip.blank_thresholds(n), thr)
  np.testing.assert_array_equal(copy.blank_thresholds(n), thr)
  # the rows hinted: exactly, and generous by 3
  exact = torch.from_numpy(thr[0].copy()).cuda()
  same(xd, rows_used=exact)
  same(xd, rows_used=exact, rows_add=3)
  # the run-time switch off and on
  skip.set_blank_skip(False)
  np.testing.assert_array_equal(skip(xd).cpu().numpy(), want)
  skip.set_blank_skip(True)
  same(xd)
  # a batch that does not fill the persistent grids (the run of r = 37 and the first deep neighbour)
  at = int(np.flatnonzero(rows == 37)[-5])
  same(xd[at:at + 7])
  # calibration moves the shifts: the blank responses are recomputed, the graphs captured again
  from deepvariant_amd import calibration_set
  if calibration_set.supported(shape):
    for m in (dense, skip, copy):
      m.calibrate_for_checkpoint(64)
    same(xd)
