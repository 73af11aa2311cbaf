"""The float64 reference of the calibration's exact pipeline R (deepvariant_amd/csrc/calib.hip) -- test infrastructure.

`logits_r` of dv_model_probe_rounding is the classifier in plain float32, so it must equal a float64 restatement to
float32 summation error.  Per (shape, seed) case this module computes, once per process (the results are shared and
must be left unchanged):
  l64   the logits of a .double() copy of the oracle (oracle/inception_ref.py), float64 end to end;
  d32   max |torch float32 oracle - l64|: what ANOTHER float32 evaluation of the same network is off by -- the unit of
        the GPU bar (tests/test_hip_calib_pipelines.py), taken from the reference alone.
Used by tests/test_calib_reference_cpu.py (CPU) and tests/test_hip_calib_pipelines.py (GPU).
"""
import functools
import os

import numpy as np
import torch

from oracle import inception_ref as R

# (shape, model seed); images: default_rng(channels), image 0 zero from row 40 (pile-up-like: nothing below the reads)
CASES = (((75, 75, 1), 5), ((100, 221, 7), 101), ((100, 147, 10), 202), ((100, 199, 9), 303), ((120, 301, 16), 5),
         ((300, 221, 6), 7))
N_IMAGES = 3
FACTOR = 16          # the GPU bar is FACTOR x d32: sequential fmaf over K <= 4032 against a blocked GEMM, one order
INJECTED_MARGIN = 20  # each injected geometry error moves a float64 logit by at least this many bars


def seed_of(shape):
  return dict(CASES)[tuple(shape)]


def images(shape, n=N_IMAGES):
  h, w, c = shape
  x = np.random.default_rng(c).integers(0, 256, (n, h, w, c), dtype=np.uint8)
  x[0, 40:] = 0
  return x


def _threads():
  torch.set_num_threads(min(16, os.cpu_count() or 1))


def oracle_logits(ref, images_u8):
  """The oracle's logits in the dtype of its parameters (forward() without the softmax)."""
  dtype = ref.classification.weight.dtype
  with torch.no_grad():
    x = ((torch.from_numpy(images_u8).to(dtype) - 128.0) / 128.0).permute(0, 3, 1, 2).contiguous()
    return ref.classification(ref.features(x))


@functools.lru_cache(maxsize=None)
def reference(shape):
  """-> dict(images uint8 [3,h,w,c], flat float32 weights, l64 float64 [3,3], d32 float, ref64 the float64 oracle)."""
  _threads()
  shape = tuple(shape)
  seed = seed_of(shape)
  ref32 = R.make_random_model(shape[2], seed=seed)
  ref64 = R.make_random_model(shape[2], seed=seed).double()
  x = images(shape)
  l64 = oracle_logits(ref64, x).numpy()
  l32 = oracle_logits(ref32, x).numpy()
  assert l64.dtype == np.float64 and l32.dtype == np.float32
  out = dict(images=x, flat=ref32.export_flat(), l64=l64, d32=float(np.abs(l32.astype(np.float64) - l64).max()),
             ref64=ref64)
  out['l64'].setflags(write=False)
  return out
