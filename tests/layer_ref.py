"""The fp32 oracle's named intermediate tensors (test infrastructure, never imported by the product).

Walks oracle.inception_ref.InceptionV3's own modules block by block, as its features() does, and keeps each concat
under the name Keras InceptionV3 gives it -- the names dv_model_infer_outputs accepts (include/dvhip.h):
mixed0 .. mixed10, mixed9_0 / mixed9_1 (the 3x3-split concats inside mixed9 and mixed10), prelogits (the pooled
vector that features() returns) and logits (the Dense output forward() puts through softmax).
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from oracle.inception_ref import _avgpool, _maxpool   # noqa: E402

NAMES = ['mixed%d' % i for i in range(11)] + ['mixed9_0', 'mixed9_1', 'prelogits', 'logits']


def named_outputs(ref, images_u8_nhwc):
  """{name: float32 tensor} for uint8 NHWC images on ref's device: the mixed blocks NHWC [N, h, w, c], prelogits
  [N, 2048], logits [N, num_classes]."""
  out = {}
  with torch.no_grad():
    x = images_u8_nhwc.to(torch.float32)
    x = ((x - 128.0) / 128.0).permute(0, 3, 1, 2).contiguous()   # forward()'s preprocessing
    s = ref.stem
    x = s[2](s[1](s[0](x)))
    x = _maxpool(x)
    x = s[4](s[3](x))
    x = _maxpool(x)
    names = iter('mixed%d' % i for i in range(11))
    for blk in ref.mixed_a:
      x = torch.cat([ref._seq(blk['b1'], x), ref._seq(blk['b5'], x), ref._seq(blk['b3'], x),
                     ref._seq(blk['bp'], _avgpool(x))], 1)
      out[next(names)] = x
    x = torch.cat([ref._seq(ref.mixed3['b3'], x), ref._seq(ref.mixed3['b3d'], x), _maxpool(x)], 1)
    out[next(names)] = x
    for blk in ref.mixed_b:
      x = torch.cat([ref._seq(blk['b1'], x), ref._seq(blk['b7'], x), ref._seq(blk['b7d'], x),
                     ref._seq(blk['bp'], _avgpool(x))], 1)
      out[next(names)] = x
    x = torch.cat([ref._seq(ref.mixed8['b3'], x), ref._seq(ref.mixed8['b7'], x), _maxpool(x)], 1)
    out[next(names)] = x
    for i, blk in enumerate(ref.mixed_c):
      b3 = blk['b3'][0](x)
      b3 = torch.cat([blk['b3'][1](b3), blk['b3'][2](b3)], 1)
      out['mixed9_%d' % i] = b3
      b3d = blk['b3d'][1](blk['b3d'][0](x))
      b3d = torch.cat([blk['b3d'][2](b3d), blk['b3d'][3](b3d)], 1)
      x = torch.cat([ref._seq(blk['b1'], x), b3, b3d, ref._seq(blk['bp'], _avgpool(x))], 1)
      out[next(names)] = x
    out['prelogits'] = x.mean(dim=(2, 3))
    out['logits'] = ref.classification(out['prelogits'])
  return {k: (v.permute(0, 2, 3, 1).contiguous() if v.dim() == 4 else v) for k, v in out.items()}
