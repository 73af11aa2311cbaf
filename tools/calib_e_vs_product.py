"""How close is the calibration's E pipeline to the HIP kernels, and where do the two part (GPU box; test
infrastructure)?

  python tools/calib_e_vs_product.py [--shape 100 221 7] > profile.txt

E (deepvariant_amd/csrc/calib.hip through dv_model_probe_rounding) rounds where the MFMA kernels round.  On 64 held-out
synthetic pile-ups, with the model calibrated on 64 others and E given the same corrections, this prints
  1. rms of product - R, E - R and product - E over the logits, and the correlation of the two errors;
  2. keep-one-op probes: rms(product - E_i) with the rounding of op i alone flipped against the plan -- an op whose
     rounding E has and the product has not (or the other way round) would stand out;
  3. E with every op from op c on kept in float32, c = 0, 8, 16, ...: whether each further stretch of E's roundings
     brings it nearer to the product (the roundings are the same draws) or takes it away (independent draws);
  4. E against E with conv1's corrections moved by 1e-7 and 1e-6: how far a last-bit difference of a float32 sum
     carries through these rounding points -- the distance two correct pipelines keep from each other.
It first prints the uncalibrated ratio (E without corrections).
The figures of DESIGN.md 6, "What pins the calibration".
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import calib_probe as P   # noqa: E402
from tests import calib_reference as CR   # noqa: E402
from tests import cnn_tail as T   # noqa: E402
from deepvariant_amd.inception_v3 import InceptionV3   # noqa: E402


def rms(a):
  return float(np.sqrt((a.astype(np.float64) ** 2).mean()))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shape', type=int, nargs=3, default=(100, 221, 7), help='(100, 221, 7) or (100, 147, 10)')
  shape = tuple(ap.parse_args().shape)
  flat = CR.reference(shape)['flat']
  if shape[2] == 7:
    x, xc = T.illumina_pileups_gpu(64, seed=7070001), T.illumina_pileups_gpu(64, seed=7070002)
  else:
    x, xc = T.longread_images_gpu('hifi', 64, seed=7070001), T.longread_images_gpu('hifi', 64, seed=7070002)
  m = InceptionV3(shape, max_batch=8)
  m.load_flat_weights(flat)

  def product_logits():
    return np.concatenate([m.forward_outputs(x[i:i + 8], ['logits'])[1]['logits'].cpu().numpy() for i in range(0, 64, 8)])
  got = product_logits()
  lr, le, _ = P.probe(m, flat, x)
  print('# %s %s, uncalibrated (E without corrections), 64 held-out pile-ups' % (shape, 'precise' if m.precise else 'fast'))
  print('rms product - R %.3e  product - E %.3e  ratio %.3f' % (rms(got - lr), rms(got - le), rms(got - le) / rms(got - lr)),
        flush=True)
  corr = m.calibrate(xc)
  got = product_logits()
  labels = P.op_labels(m)
  feat = labels[-1]['out_buf']
  # the plan's own keep_f32 (calib_plan_of): float32 tensors -- raw pooled projections, the global pool's inputs
  base = np.array([1 if (l['kind'] == 'conv' and l['raw'] == 1) or (l['kind'] != 'maxpool' and l['out_buf'] == feat)
                   else 0 for l in labels], np.uint8)
  lr, le, _ = P.probe(m, flat, x, corrections=corr)
  if not m.precise:
    _, le_b, _ = P.probe(m, flat, x, keep=base, corrections=corr, want_r=False)
    assert le_b.tobytes() == le.tobytes(), 'the reconstructed keep_f32 is not the plan\'s'
  else:
    base = None   # hi + lo tensors are kept too and the labels do not say which: only part 1
  dp, de = (got - lr).astype(np.float64), (le - lr).astype(np.float64)
  print('# %s %s, calibrated on 64 other pile-ups, 64 held-out pile-ups' % (shape, 'precise' if m.precise else 'fast'))
  print('rms product - R %.3e  E - R %.3e  product - E %.3e  ratio %.3f  correlation(product - R, E - R) %.3f' % (
      rms(dp), rms(de), rms(got - le), rms(got - le) / rms(dp),
      float((dp * de).sum() / np.sqrt((dp ** 2).sum() * (de ** 2).sum()))), flush=True)
  # 4. how far a perturbation of one float32 ulp carries: E with conv1's corrections moved by 1e-7 (its pre-activations
  # are of order 1).  Two correct pipelines with these rounding points whose float32 sums differ in the last bit are
  # this far apart at the logits.
  for eps in (1e-7, 1e-6):
    moved = corr.copy()
    moved[:32] += np.float32(eps)
    _, le_p, _ = P.probe(m, flat, x, corrections=moved, want_r=False)
    print('conv1 corrections + %.0e: rms(E\' - E) %.3e (rms E - R %.3e, product - E %.3e)' % (
        eps, rms(le_p - le), rms(de), rms(got - le)), flush=True)
  if base is None:
    return
  rows = []
  for i, l in enumerate(labels):
    if l['kind'] == 'maxpool':
      continue
    keep = base.copy()
    keep[i] ^= 1
    _, le_i, _ = P.probe(m, flat, x, keep=keep, corrections=corr, want_r=False)
    rows.append((rms(got - le_i), i))
    print('op %3d %-7s layer %3d out %s raw %d keep_f32 %d -> %d: rms(product - E_i) %.4e' % (
        i, l['kind'], l['layer'], l['out'], l['raw'], base[i], keep[i], rows[-1][0]), flush=True)
  rows.sort()
  print('# nearest 5 (rms, op): %s' % rows[:5])
  print('# farthest 5 (rms, op): %s' % rows[-5:])
  for cut in range(0, len(labels), 8):
    keep = base.copy()
    keep[cut:] = 1
    _, le_c, _ = P.probe(m, flat, x, keep=keep, corrections=corr, want_r=False)
    print('ops >= %3d kept in float32: rms(E_c - R) %.3e  rms(product - E_c) %.3e' % (cut, rms(le_c - lr), rms(got - le_c)),
          flush=True)


if __name__ == '__main__':
  main()
