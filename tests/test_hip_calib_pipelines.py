"""The calibration's two float32 pipelines (deepvariant_amd/csrc/calib.hip, through dv_model_probe_rounding) on the GPU.

R, the exact pipeline, is the whole classifier in plain float32: it is held to a float64 restatement
(tests/calib_reference.py) within 16 x d32, d32 being what torch's own float32 evaluation is off by -- two orders
below a single-pixel geometry error (tests/test_calib_reference_cpu.py) and three below the fp16 product's own logit
error.  E, the pipeline with the MFMA kernels' rounding points, is tied to R where nothing is rounded (bit for bit).
Around that: batch independence, determinism, the measure path against dv_model_calibrate, the op table and the
argument checks.  No test here compares E with the product's kernels: E is nearer to them than R in three of the
four cases measured but not in calibrated fast mode, and no rounding point that E leaves out was found
(tools/calib_e_vs_product.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_KNOBS = ('DV_NO_POOL_FUSE', 'DV_NO_POOL2_IN_CONV', 'DV_NO_STEM_FUSE', 'DV_PRECISE')
# R / float64 in units of d32, per shape on one MI355X ("What pins the calibration"): the largest over
# every plan of the shape.  Kept for the record; the assertion below is the fixed factor CR.FACTOR.
MEASURED_R_OVER_D32 = {(75, 75, 1): 1.10, (100, 221, 7): 1.49, (100, 147, 10): 4.28, (100, 199, 9): 5.95,
                       (120, 301, 16): 0.84, (300, 221, 6): 0.86}


def _model(shape, flat=None, env=None):
  """InceptionV3(shape, max_batch=8) whose plan is built under `env` (the knobs not named are unset meanwhile)."""
  from deepvariant_amd.inception_v3 import InceptionV3
  old = {k: os.environ.pop(k, None) for k in _KNOBS}
  os.environ.update(env or {})
  try:
    m = InceptionV3(shape, max_batch=8)
  finally:
    for k in _KNOBS:
      os.environ.pop(k, None)
      if old[k] is not None:
        os.environ[k] = old[k]
  if flat is not None:
    m.load_flat_weights(flat)
  return m


def _random_images(shape, n, seed):
  x = np.random.default_rng(seed).integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)
  x[: n // 2, 40:] = 0
  return torch.from_numpy(x).cuda()


def _probs(m, x):
  return np.concatenate([m(x[i:i + 8]).cpu().numpy() for i in range(0, x.shape[0], 8)])


# ------------------------------------------------------------------------------------------------ R against float64
def _cases():
  from tests import calib_reference as CR
  out = [(s, {}) for s, _ in CR.CASES]
  for s in ((100, 221, 7), (100, 147, 10)):
    out += [(s, {k: '1'}) for k in ('DV_NO_POOL_FUSE', 'DV_NO_POOL2_IN_CONV', 'DV_NO_STEM_FUSE')]
  return out + [((100, 147, 10), {'DV_PRECISE': '0'})]


@pytest.mark.parametrize('shape,env', _cases(), ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else
                         '-'.join(v) or 'default')
def test_exact_pipeline_equals_the_float64_reference(shape, env):
  """max |logits_r - l64| <= 16 x d32 under every plan: the default one and the ones with explicit max-pool ops
  (DV_NO_POOL_FUSE), pool_in on mixed0's heads and its raw projection (DV_NO_POOL2_IN_CONV), per-layer stem buffers
  (DV_NO_STEM_FUSE) and fp16 instead of hi + lo tensors (DV_PRECISE=0) -- R is the same function under all of them."""
  from tests import calib_probe as P
  from tests import calib_reference as CR
  ref = CR.reference(shape)
  m = _model(shape, ref['flat'], env)
  labels = P.op_labels(m)
  if 'DV_NO_POOL_FUSE' in env:
    assert sum(l['kind'] == 'maxpool' for l in labels) == 4      # both stem pools are ops of their own
  if 'DV_PRECISE' in env:
    assert not m.precise
  lr, le, _ = P.probe(m, ref['flat'], torch.from_numpy(ref['images']).cuda())
  err = float(np.abs(lr.astype(np.float64) - ref['l64']).max())
  scale = float(np.abs(ref['l64']).max())
  bar = CR.FACTOR * ref['d32']
  print('calib-R %s %s: max|l64| %.3g d32 %.3e max|R - l64| %.3e ratio %.2f (bar %d); E - R max %.3e' % (
      shape, '-'.join(env) or 'default', scale, ref['d32'], err, err / ref['d32'], CR.FACTOR,
      float(np.abs(le - lr).max())))
  assert np.isfinite(lr).all() and np.isfinite(le).all()
  assert bar < 1e-4 * scale          # the bar stays two orders under a geometry error, or it is not worth having
  assert err <= bar, (err, bar)


# ------------------------------------------------------------------------------------------- E where nothing is rounded
@pytest.mark.parametrize('shape', [(100, 221, 7), (100, 147, 10)])
def test_e_with_nothing_rounded_is_r(shape):
  from tests import calib_probe as P
  from tests import calib_reference as CR
  flat = CR.reference(shape)['flat']
  m = _model(shape, flat)
  x = _random_images(shape, 5, seed=21)
  keep = np.ones(len(P.op_labels(m)), np.uint8)
  lr, le, _ = P.probe(m, flat, x, keep=keep, weights_f32=True)
  assert lr.tobytes() == le.tobytes()
  lr2, le2, corr = P.probe(m, flat, x, keep=keep, weights_f32=True, measure=True)
  assert corr.shape == (P.num_corrections(m),) and not np.any(corr)        # every correction is exactly 0.0
  assert lr2.tobytes() == lr.tobytes() and le2.tobytes() == lr.tobytes()
  _, le3, _ = P.probe(m, flat, x)                                           # and the product's roundings do move E
  assert le3.tobytes() != lr.tobytes()


# ------------------------------------------------------------------------------------------------ batch independence
def test_an_images_logits_do_not_depend_on_the_batch():
  """(100, 221, 7): the 8x8 stage is a 1 x 5 map, m_total = 5 n -- n = 1, 3, 8, 9 end conv_direct's last 8-pixel
  group after 5, 7, 8 and 5 pixels, so the clamp of the pixels past the batch is crossed both ways."""
  from tests import calib_probe as P
  from tests import calib_reference as CR
  shape = (100, 221, 7)
  flat = CR.reference(shape)['flat']
  m = _model(shape, flat)
  x = _random_images(shape, 9, seed=22)
  lr9, _, corr = P.probe(m, flat, x, measure=True)
  _, le9, _ = P.probe(m, flat, x, corrections=corr)
  for n in (1, 3, 8, 9):
    lr, le, _ = P.probe(m, flat, x[:n], corrections=corr)
    assert lr.tobytes() == lr9[:n].tobytes(), n
    assert le.tobytes() == le9[:n].tobytes(), n
  lr, le, _ = P.probe(m, flat, x[4:7], corrections=corr)      # ... nor on where in the batch the image stands
  assert lr.tobytes() == lr9[4:7].tobytes() and le.tobytes() == le9[4:7].tobytes()


# --------------------------------------------------------------------------------------------------- the measure path
@pytest.mark.parametrize('shape', [(100, 221, 7), (100, 147, 10)])
def test_measuring_probe_is_the_calibration(shape):
  from tests import calib_probe as P
  from tests import calib_reference as CR
  flat = CR.reference(shape)['flat']
  m = _model(shape, flat)
  x = _random_images(shape, 6, seed=23)
  lr, le, corr = P.probe(m, flat, x, measure=True)
  assert np.isfinite(corr).all() and np.any(corr[:32]) and np.any(corr[-3:])
  lr2, le2, corr2 = P.probe(m, flat, x, measure=True)
  assert (lr2.tobytes(), le2.tobytes(), corr2.tobytes()) == (lr.tobytes(), le.tobytes(), corr.tobytes())
  lr3, le3, _ = P.probe(m, flat, x, corrections=corr)         # fed back as fixed corrections: the same E
  assert lr3.tobytes() == lr.tobytes() and le3.tobytes() == le.tobytes()
  assert m.calibrate(x).tobytes() == corr.tobytes()           # dv_model_calibrate on the same images, bit for bit


@pytest.mark.parametrize('n', [1, 65, 130])
def test_measured_corrections_remove_the_mean_logit_error(n):
  """One, two and three segments of channel_partials over the n logits -- and, on this shape's 1 x 1 last map, over the
  n pixels of every layer of the 8x8 stage.  The returned logits_e has the Dense correction subtracted, so its mean
  error against R is what float32 leaves of a mean computed in float64."""
  from tests import calib_probe as P
  from tests import calib_reference as CR
  shape = (75, 75, 1)
  flat = CR.reference(shape)['flat']
  m = _model(shape, flat)
  x = _random_images(shape, n, seed=24)
  lr, le, corr = P.probe(m, flat, x, measure=True)
  scale = max(1.0, float(np.abs(lr).max()), float(np.abs(le).max()))
  mean = np.abs((le.astype(np.float64) - lr.astype(np.float64)).mean(0))
  print('calib-mean n %d: |mean(E - R)| %s, Dense corrections %s, max|logit| %.3g' % (n, mean, corr[-3:], scale))
  # (n = 1 on a 1 x 1 map: each layer's correction is its whole error, E's features are R's and the Dense
  # corrections are 0.0; from two images on they are not)
  assert np.isfinite(corr).all() and np.any(corr[:32]) and (n == 1 or np.any(corr[-3:]))
  assert (mean <= 1e-6 * scale).all(), (mean, scale)


# ------------------------------------------------------------------------------------------------ the model is untouched
def test_probing_leaves_the_model_alone_and_r_ignores_the_probe_arguments():
  from tests import calib_probe as P
  from tests import calib_reference as CR
  shape = (100, 147, 10)
  flat = CR.reference(shape)['flat']
  m = _model(shape, flat)
  x = _random_images(shape, 5, seed=25)
  m.calibrate(_random_images(shape, 4, seed=26))              # a calibrated model: its corrections stay applied
  before = _probs(m, x)
  stats = m.graph_stats()
  n_ops = len(P.op_labels(m))
  lr0, le0, corr = P.probe(m, flat, x, measure=True)
  keep = (np.arange(n_ops) % 2).astype(np.uint8)
  fixed = (0.01 * np.random.default_rng(3).standard_normal(corr.size)).astype(np.float32)
  seen = [le0.tobytes()]
  for kw in (dict(), dict(weights_f32=True), dict(keep=keep), dict(keep=keep, measure=True),
             dict(corrections=fixed), dict(keep=np.ones(n_ops, np.uint8), corrections=fixed, weights_f32=True)):
    lr, le, _ = P.probe(m, flat, x, **kw)
    assert lr.tobytes() == lr0.tobytes(), kw
    seen.append(le.tobytes())
  assert len(set(seen)) == len(seen)                          # every one of them did change E
  _, le, _ = P.probe(m, flat, x, corrections=fixed, want_r=False)         # R skipped: E is the same
  assert le.tobytes() == seen[-2]
  assert m.graph_stats() == stats
  assert np.array_equal(_probs(m, x), before)
  assert m.graph_stats()[0] == stats[0]                       # and the forward's graph was still there to replay


# ------------------------------------------------------------------------------------------------------------ op table
def test_op_table():
  from deepvariant_amd import _lib
  from tests import calib_probe as P
  lib = _lib.lib()
  m = _model((100, 221, 7))                                   # the op table needs no weights
  n_ops = lib.dv_model_num_ops(m._handle)
  labels = P.op_labels(m)
  assert len(labels) == n_ops and lib.dv_model_num_ops(None) == 0
  convs = [l for l in labels if l['kind'] == 'conv']
  table = m.layer_table()
  assert {l['kind'] for l in labels} == {'conv', 'maxpool', 'avgpool'}
  assert sorted(l['layer'] for l in convs) == list(range(len(table) - 1))          # every conv layer is one op
  for l in convs:
    kh, kw, _, co, _ = table[l['layer']]
    assert (l['k'], l['cout']) == ((kh, kw), co)
  # one correction per conv output channel, then one per logit: dv_model_calibrate's layout
  assert sum(l['cout'] for l in convs) + m.num_classes == P.num_corrections(m)
  assert all(0 <= l['in_buf'] and 0 <= l['out_buf'] and l['lds_only'] in (0, 1) and l['raw'] in (0, 1) for l in labels)
  assert sum(l['raw'] for l in convs) == sum(l['kind'] == 'avgpool' for l in labels) == 9   # the pooled projections
  # an index out of range and a buffer of no bytes are refused; a short buffer gets a truncated, terminated label
  buf = C.create_string_buffer(b'\xaa' * 256, 256)
  for bad in (-1, n_ops):
    assert lib.dv_model_op_label(m._handle, bad, buf, 256) == _lib.DV_ERR_INVALID_ARGUMENT
  assert lib.dv_model_op_label(m._handle, 0, buf, 0) == _lib.DV_ERR_INVALID_ARGUMENT
  assert lib.dv_model_op_label(m._handle, 0, None, 256) == _lib.DV_ERR_INVALID_ARGUMENT
  assert buf.raw == b'\xaa' * 256
  full = C.create_string_buffer(256)
  _lib.check(lib.dv_model_op_label(m._handle, 0, full, 256))
  assert lib.dv_model_op_label(m._handle, 0, buf, 8) == _lib.DV_OK
  assert buf.raw[:8] == full.value[:7] + b'\0' and buf.raw[8:] == b'\xaa' * 248


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing():
  from deepvariant_amd import _lib
  from tests import calib_probe as P
  from tests import calib_reference as CR
  shape = (75, 75, 1)
  flat = CR.reference(shape)['flat']
  x = _random_images(shape, 2, seed=27)
  le = np.zeros((2, 3), np.float32)
  bad = _lib.DV_ERR_INVALID_ARGUMENT
  empty = _model(shape)
  assert P.probe_raw(empty, flat, x, logits_e=le) == bad and b'load weights first' in _lib.lib().dv_last_error()
  m = _model(shape, flat)
  n_corr = P.num_corrections(m)
  lr0, le0, corr = P.probe(m, flat, x, measure=True)
  before = _probs(m, x)
  sentinel = np.full((2, 3), 7.0, np.float32)
  le[:] = sentinel
  lr = sentinel.copy()
  out = np.full(n_corr, 7.0, np.float32)
  assert P.probe_raw(m, flat, x, logits_r=lr, logits_e=None, corrections_out=out) == bad
  for kw in (dict(n_weights=flat.size - 1), dict(n_images=0), dict(n_images=4097),
             dict(corrections=corr[:-1]), dict(corrections=corr, n_corrections=n_corr + 1),
             dict(corrections=corr, flags=P.MEASURE)):
    assert P.probe_raw(m, flat, x, logits_r=lr, logits_e=le, corrections_out=out, **kw) == bad, kw
    assert _lib.lib().dv_last_error()
  assert np.array_equal(lr, sentinel) and np.array_equal(le, sentinel) and np.all(out == 7.0)   # nothing was written
  lr1, le1, corr1 = P.probe(m, flat, x, measure=True)
  assert (lr1.tobytes(), le1.tobytes(), corr1.tobytes()) == (lr0.tobytes(), le0.tobytes(), corr.tobytes())
  assert np.array_equal(_probs(m, x), before)
