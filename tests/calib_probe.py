"""ctypes wrapper of dv_model_probe_rounding / dv_model_num_ops / dv_model_op_label (include/dvhip.h, ABI v8) -- test
infrastructure.  The calibration's two float32 pipelines (deepvariant_amd/csrc/calib.hip: R exact, E with the MFMA
kernels' rounding points) on a loaded model, without changing it."""
import ctypes as C

import numpy as np
import torch

from deepvariant_amd import _lib

WEIGHTS_F32 = 1    # flags bit 0: E multiplies the float32 weights
MEASURE = 2        # flags bit 1: measure the corrections on these images under this plan


def op_labels(model):
  """dv_model_op_label of every graph op, parsed: {'kind': 'conv' | 'maxpool' | 'avgpool', 'layer': int, 'k': (kh, kw),
  'out': (oh, ow), and every other key=value as int}."""
  lib = _lib.lib()
  buf = C.create_string_buffer(256)
  labels = []
  for i in range(lib.dv_model_num_ops(model._handle)):
    _lib.check(lib.dv_model_op_label(model._handle, i, buf, 256))
    words = buf.value.decode().split()
    d = {'kind': words[0]}
    for kv in words[1:]:
      k, v = kv.split('=')
      d[k] = tuple(int(t) for t in v.split('x')) if 'x' in v else int(v)
    labels.append(d)
  return labels


def num_corrections(model):
  return sum(co for _, _, _, co, _ in model.layer_table())


def probe_raw(model, flat, images, keep=None, flags=0, corrections=None, logits_r=None, logits_e=None,
              corrections_out=None, n_weights=None, n_images=None, n_corrections=None):
  """The bare call, every argument as given (None = NULL): -> the return code."""
  arr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
  torch.cuda.synchronize()
  return _lib.lib().dv_model_probe_rounding(
      model._handle, arr(flat), flat.size if n_weights is None else n_weights, images.data_ptr(),
      images.shape[0] if n_images is None else n_images, arr(keep), flags, arr(corrections),
      (0 if corrections is None else corrections.size) if n_corrections is None else n_corrections,
      arr(logits_r), arr(logits_e), arr(corrections_out))


def probe(model, flat, images, keep=None, corrections=None, weights_f32=False, measure=False, want_r=True):
  """images: CUDA uint8 [n, h, w, c]; keep: uint8 per graph op or None (the product's rounding points); corrections:
  float32 in dv_model_calibrate's layout or None.  -> (logits_r [n, 3] or None, logits_e [n, 3], corrections measured
  or None)."""
  images = images.contiguous()
  n = images.shape[0]
  flat = np.ascontiguousarray(flat, np.float32)
  keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
  if keep is not None:
    assert keep.size == _lib.lib().dv_model_num_ops(model._handle)
  corrections = None if corrections is None else np.ascontiguousarray(corrections, np.float32)
  lr = np.full((n, model.num_classes), np.nan, np.float32) if want_r else None
  le = np.full((n, model.num_classes), np.nan, np.float32)
  out = np.full(num_corrections(model), np.nan, np.float32) if measure else None
  _lib.check(probe_raw(model, flat, images, keep, (WEIGHTS_F32 if weights_f32 else 0) | (MEASURE if measure else 0),
                       corrections, lr, le, out))
  return lr, le, out
