"""Named intermediate outputs of the classifier (dv_model_infer_outputs, dv_model_output_info,
InceptionV3.forward_outputs) on the GPU.

1. The forward is unchanged: the probabilities of an export call equal the plain forward's bit for bit, at every input
   shape (fast and precise mode), with blank-row skipping on and off, uncalibrated and calibrated, at 1, 37 and 512
   examples, with every output requested at once and each alone; export calls between plain calls never make the
   plain forward capture again.
2. The outputs agree with each other: softmax(logits) = probs, prelogits @ W + b = logits within fp32 summation error,
   mixed10 = what dv_model_debug_tensor(-1) reads from the same buffer, prelogits = the spatial mean of mixed10.
3. Against the fp32 oracle (tests/layer_ref.py) block by block, with bounds set from measurements.
4. Errors and shapes: unknown names, null outputs and n > max_batch are refused; the shapes follow the Keras graph.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import layer_ref

pytestmark = pytest.mark.gpu

NAMES = layer_ref.NAMES
# every input shape the product emits with a distinct plan: short reads (fast mode), the two long-read shapes
# (precise mode: wide buffers from mixed4 on), the alt-aligned row stack
SHAPES = [(100, 221, 7), (100, 147, 10), (100, 199, 9), (300, 221, 6)]


def _model(shape, weights, max_batch):
  from deepvariant_amd.inception_v3 import InceptionV3
  m = InceptionV3(shape, max_batch=max_batch)
  m.load_flat_weights(weights)
  return m


@pytest.mark.parametrize('shape', SHAPES)
def test_probabilities_are_the_plain_forwards_bit_for_bit(shape):
  from deepvariant_amd import calibration_set
  from oracle import inception_ref as R
  model = _model(shape, R.make_random_model(shape[2], seed=23).export_flat(), 512)
  assert model.precise == (shape[2] > 8)
  x = calibration_set.draw(shape, 512, seed=4242)
  s = torch.cuda.Stream()
  with torch.cuda.stream(s):            # the plain forward replays its hipGraph here; the export forward never does
    for calibrated in (False, True):
      if calibrated:
        model.calibrate_for_checkpoint(64)
      for blank in (True, False):
        model.set_blank_skip(blank)
        for n in (1, 37, 512):
          xs = x[:n]
          want = model(xs)
          probs, outs = model.forward_outputs(xs, NAMES)
          assert torch.equal(probs, want), (calibrated, blank, n)
          for name in NAMES:
            assert torch.isfinite(outs[name]).all(), name
            p1, o1 = model.forward_outputs(xs, [name])
            assert torch.equal(p1, want), (calibrated, blank, n, name)
            assert torch.equal(o1[name], outs[name]), (calibrated, blank, n, name)
  s.synchronize()


def test_export_calls_leave_the_plain_forwards_graph_alone():
  from deepvariant_amd.inception_v3 import InceptionV3
  model = InceptionV3((100, 221, 7), max_batch=64)
  model.init_random(seed=3)
  rng = np.random.default_rng(5)
  x = torch.from_numpy(rng.integers(0, 256, (64, 100, 221, 7), dtype=np.uint8)).cuda()
  s = torch.cuda.Stream()
  with torch.cuda.stream(s):
    want = model(x)
    captures, replays = model.graph_stats()
    for k in range(3):
      probs, _ = model.forward_outputs(x, NAMES if k != 1 else ['mixed4', 'logits'])
      assert torch.equal(probs, want)
      assert torch.equal(model(x), want)
    assert model.graph_stats() == (captures, replays + 3)
  s.synchronize()
  assert captures == 1


@pytest.mark.parametrize('shape', [(100, 221, 7), (100, 147, 10)])
def test_outputs_agree_with_each_other(shape):
  from deepvariant_amd import calibration_set
  from oracle import inception_ref as R
  flat = R.make_random_model(shape[2], seed=31).export_flat()
  model = _model(shape, flat, 64)       # uncalibrated: the Dense bias is the loaded one
  x = calibration_set.draw(shape, 64, seed=777)
  probs, outs = model.forward_outputs(x, ['prelogits', 'logits', 'mixed10'])
  p = probs.cpu().double().numpy()
  logits = outs['logits'].cpu().double().numpy()
  pre = outs['prelogits'].cpu().double().numpy()
  e = np.exp(logits - logits.max(axis=1, keepdims=True))
  assert np.abs(e / e.sum(axis=1, keepdims=True) - p).max() <= 1e-6
  assert (logits.argmax(axis=1) == p.argmax(axis=1)).all()
  k = model.num_classes
  w = flat[-(2048 * k + k):-k].astype(np.float64).reshape(2048, k)
  b = flat[-k:].astype(np.float64)
  bound = 2048 * 2.0 ** -24 * (np.abs(pre) @ np.abs(w) + np.abs(b))
  assert (np.abs(pre @ w + b - logits) <= bound).all()
  # mixed10 is the buffer dv_model_debug_tensor(-1) reads (as fp16, padded, NHWC)
  h, wd, c = model.output_info('mixed10')
  m10 = outs['mixed10'].cpu().numpy()
  assert m10.shape == (64, h, wd, c)
  dbg = model.debug_tensor(-1, 64)
  halo = (dbg.shape[1] - h) // 2
  np.testing.assert_array_equal(m10.astype(np.float16), dbg[:, halo:halo + h, halo:halo + wd, :])
  np.testing.assert_allclose(m10.astype(np.float64).mean(axis=(1, 2)), pre, rtol=1e-5, atol=1e-6)


# --------------------------------------------------------------------------------------------- against the oracle
HELD_OUT_SEEDS = (101, 202, 303)
N_ORACLE = 256
IMAGE_SEED = 6060001           # synthetic pile-ups of neither the calibration set nor any other test
# (max|d| / max|ref|, RMS(d) / RMS(ref)) per output: the largest of the three seeds, measured on one MI355X with
# N_ORACLE images and rounded to three digits.  The test allows twice these.
MEASURED = {
    'illumina': {'mixed0': (9.47e-4, 5.13e-4), 'mixed1': (1.14e-3, 5.85e-4), 'mixed2': (9.95e-4, 6.30e-4),
                 'mixed3': (1.03e-3, 6.23e-4), 'mixed4': (1.02e-3, 6.43e-4), 'mixed5': (8.66e-4, 6.21e-4),
                 'mixed6': (9.24e-4, 6.47e-4), 'mixed7': (1.13e-3, 6.74e-4), 'mixed8': (9.40e-4, 6.34e-4),
                 'mixed9': (9.96e-4, 6.81e-4), 'mixed10': (1.12e-3, 6.91e-4), 'mixed9_0': (1.02e-3, 7.34e-4),
                 'mixed9_1': (1.27e-3, 7.27e-4), 'prelogits': (4.97e-4, 3.74e-4), 'logits': (8.96e-4, 3.66e-4)},
    'hifi': {'mixed0': (1.12e-3, 6.12e-4), 'mixed1': (1.24e-3, 6.79e-4), 'mixed2': (1.35e-3, 7.10e-4),
             'mixed3': (1.14e-3, 7.23e-4), 'mixed4': (1.17e-3, 5.98e-4), 'mixed5': (9.86e-4, 5.40e-4),
             'mixed6': (8.91e-4, 4.92e-4), 'mixed7': (7.10e-4, 4.57e-4), 'mixed8': (5.92e-4, 3.95e-4),
             'mixed9': (6.55e-4, 3.78e-4), 'mixed10': (6.26e-4, 3.63e-4), 'mixed9_0': (7.06e-4, 4.03e-4),
             'mixed9_1': (6.52e-4, 4.10e-4), 'prelogits': (3.75e-4, 2.42e-4), 'logits': (9.98e-4, 3.62e-4)},
    'ont': {'mixed0': (1.10e-3, 5.78e-4), 'mixed1': (1.20e-3, 6.38e-4), 'mixed2': (1.24e-3, 7.08e-4),
            'mixed3': (1.20e-3, 6.90e-4), 'mixed4': (1.00e-3, 5.72e-4), 'mixed5': (8.50e-4, 5.23e-4),
            'mixed6': (7.69e-4, 4.48e-4), 'mixed7': (7.49e-4, 4.40e-4), 'mixed8': (6.80e-4, 3.81e-4),
            'mixed9': (4.92e-4, 3.77e-4), 'mixed10': (5.21e-4, 3.65e-4), 'mixed9_0': (4.91e-4, 4.14e-4),
            'mixed9_1': (5.42e-4, 3.69e-4), 'prelogits': (2.95e-4, 2.22e-4), 'logits': (4.27e-4, 2.17e-4)},
}
MARGIN = 2.0


def _oracle_outputs(ref_gpu, x, batch=64):
  from oracle import inception_ref as R
  parts = []
  R.ConvBN.as_gemm = True      # rocBLAS / ATen only (oracle/inception_gpu.py)
  try:
    for i in range(0, x.shape[0], batch):
      parts.append(layer_ref.named_outputs(ref_gpu, x[i:i + batch]))
  finally:
    R.ConvBN.as_gemm = False
  return {k: torch.cat([p[k] for p in parts]) for k in NAMES}


@pytest.mark.parametrize('seed', HELD_OUT_SEEDS)
@pytest.mark.parametrize('kind', ['illumina', 'hifi', 'ont'])
def test_outputs_against_the_fp32_oracle(kind, seed):
  from tests import cnn_tail as T
  from oracle import inception_ref as R
  if kind == 'illumina':
    x = T.illumina_pileups_gpu(N_ORACLE, IMAGE_SEED)
  else:
    x = T.longread_images_gpu(kind, N_ORACLE, seed=IMAGE_SEED)
  shape = tuple(x.shape[1:])
  ref = R.make_random_model(shape[2], seed=seed)
  model = T.product_model(shape, ref.export_flat(), N_ORACLE)    # the shape's default mode, calibrated
  want = _oracle_outputs(R.make_random_model(shape[2], seed=seed).cuda(), x)
  _, got = model.forward_outputs(x, NAMES)
  for name in NAMES:
    g, r = got[name].double(), want[name].double()
    assert g.shape == r.shape, (name, g.shape, r.shape)
    d = g - r
    rel_max = float(d.abs().max() / r.abs().max())
    rel_rms = float(d.pow(2).mean().sqrt() / r.pow(2).mean().sqrt())
    print('layer-outputs %s %s seed %d (%s) %-9s max|d|/max|ref| %.3e  rms(d)/rms(ref) %.3e' % (
        kind, shape, seed, 'precise' if model.precise else 'fast', name, rel_max, rel_rms))
    max_seen, rms_seen = MEASURED[kind][name]
    assert rel_max <= MARGIN * max_seen and rel_rms <= MARGIN * rms_seen, (name, rel_max, rel_rms)


# -------------------------------------------------------------------------------------------------- errors, shapes
def _keras_concat_channels():
  """{name: channels} of the named concats of the graph deepvariant_amd/keras_layout.py restates (construction
  order; the unnamed 3x3dbl concats inside mixed9 / mixed10 are skipped)."""
  from deepvariant_amd import keras_layout
  g, _ = keras_layout.build_graph(7)
  ch = {}
  for l in g.layers:
    if l.kind == 'input':
      ch[l] = 7
    elif l.kind == 'conv':
      ch[l] = g.conv_shapes[l.conv_index][3]
    elif l.kind == 'concat':
      ch[l] = sum(ch[i] for i in l.inputs)
    elif l.inputs:
      ch[l] = ch[l.inputs[0]]
  concats = [ch[l] for l in g.layers if l.kind == 'concat']
  order = ['mixed%d' % i for i in range(9)] + ['mixed9_0', None, 'mixed9', 'mixed9_1', None, 'mixed10']
  assert len(concats) == len(order)
  return {name: c for name, c in zip(order, concats) if name}


def test_output_shapes_follow_the_keras_graph():
  from deepvariant_amd.inception_v3 import InceptionV3
  from oracle import inception_ref as R
  table = {'mixed0': (10, 25, 256), 'mixed1': (10, 25, 288), 'mixed2': (10, 25, 288), 'mixed8': (1, 5, 1280),
           'mixed9': (1, 5, 2048), 'mixed10': (1, 5, 2048), 'mixed9_0': (1, 5, 768), 'mixed9_1': (1, 5, 768),
           'prelogits': (1, 1, 2048), 'logits': (1, 1, 3)}
  table.update({'mixed%d' % i: (4, 12, 768) for i in range(3, 8)})
  m = InceptionV3((100, 221, 7), max_batch=4)
  assert {name: m.output_info(name) for name in NAMES} == table
  keras = _keras_concat_channels()
  assert sorted(keras) == sorted(n for n in NAMES if n.startswith('mixed'))
  for name, c in keras.items():
    assert m.output_info(name)[2] == c, name
  for shape in [(100, 147, 10), (100, 199, 9), (300, 221, 6)]:
    m = InceptionV3(shape, max_batch=4)
    ref = R.make_random_model(shape[2], seed=1)
    want = layer_ref.named_outputs(ref, torch.zeros((1,) + shape, dtype=torch.uint8))
    for name in NAMES:
      ref_shape = tuple(want[name].shape[1:])
      assert m.output_info(name) == (ref_shape if len(ref_shape) == 3 else (1, 1) + ref_shape), (shape, name)


def test_errors():
  from deepvariant_amd import _lib
  from deepvariant_amd.inception_v3 import InceptionV3
  m = InceptionV3((100, 221, 7), max_batch=8)
  m.init_random(seed=1)
  x = torch.zeros((9, 100, 221, 7), dtype=torch.uint8, device='cuda')
  for bad in ['conv2d_5', 'activation_3', 'global_average_pooling2d', 'mixed11', 'Mixed0', 'mixed9_2', '',
              'mixed0 ', 'classification']:
    with pytest.raises(_lib.DvError) as e:
      m.output_info(bad)
    assert e.value.status == _lib.DV_ERR_INVALID_ARGUMENT
    assert 'mixed9_0' in str(e.value) and 'prelogits' in str(e.value), str(e.value)
    with pytest.raises(_lib.DvError) as e:
      m.forward_outputs(x[:2], ['mixed0', bad])
    assert e.value.status == _lib.DV_ERR_INVALID_ARGUMENT
  with pytest.raises(_lib.DvError) as e:
    m.forward_outputs(x, ['logits'])                        # n = 9 > max_batch = 8
  assert e.value.status == _lib.DV_ERR_INVALID_ARGUMENT and 'max_batch' in str(e.value)
  with pytest.raises(_lib.DvError):
    m.forward_outputs(x[:2], ['mixed0', 'mixed0'])
  lib = _lib.lib()
  probs = torch.empty((2, 3), dtype=torch.float32, device='cuda')
  out = torch.empty((2, 10, 25, 256), dtype=torch.float32, device='cuda')
  stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

  def call(n_out, names, outs, images=x.data_ptr(), p=probs.data_ptr(), n=2):
    return lib.dv_model_infer_outputs(m._handle, images, n, p, n_out, names, outs, stream)

  names = (C.c_char_p * 1)(b'mixed0')
  assert call(1, names, (C.c_void_p * 1)(out.data_ptr())) == _lib.DV_OK
  assert call(1, names, (C.c_void_p * 1)(None)) == _lib.DV_ERR_INVALID_ARGUMENT           # null output
  assert call(1, names, (C.c_void_p * 1)(out.data_ptr() + 4)) == _lib.DV_ERR_INVALID_ARGUMENT   # misaligned
  assert call(1, (C.c_char_p * 1)(None), (C.c_void_p * 1)(out.data_ptr())) == _lib.DV_ERR_INVALID_ARGUMENT
  for bad in (b'conv2d_5', b''):
    assert call(1, (C.c_char_p * 1)(bad), (C.c_void_p * 1)(out.data_ptr())) == _lib.DV_ERR_INVALID_ARGUMENT
    assert 'accepted: mixed0, ' in _lib.last_error()
  assert call(1, None, (C.c_void_p * 1)(out.data_ptr())) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(1, names, None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(1, names, (C.c_void_p * 1)(out.data_ptr()), images=None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(1, names, (C.c_void_p * 1)(out.data_ptr()), p=None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(-1, names, (C.c_void_p * 1)(out.data_ptr())) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(0, None, None, n=9) == _lib.DV_ERR_INVALID_ARGUMENT
  assert call(0, None, None) == _lib.DV_OK                  # no output requested: dv_model_infer
  assert lib.dv_model_output_info(None, b'mixed0', None, None, None) == _lib.DV_ERR_INVALID_ARGUMENT
  torch.cuda.synchronize()
