"""The mixed-route batch of tests/encoder_cases.py through dv_encode_batch in a process of its own (python -m
tests.encoder_cache_child), so that DV_CIG_CACHE / DV_CIG_KEPT_MAX -- read once per process -- are read the way a
tuning run reads them.  Host batch and device-resident batch against the oracle; prints "items equal to the oracle:
N/N", or "refused: ..." with the encoder's message when it declines the geometry.  Exit status 0 in both cases."""
import numpy as np


def main():
  import torch
  from deepvariant_amd import _lib
  from deepvariant_amd.device_batch import DeviceBatch
  from deepvariant_amd.pileup_image_native import _Encoder
  from oracle import oracle as O
  from tests import encoder_cases as E
  torch.cuda.init()
  opts, batch = E.mixed_batch()
  want, want_rows = O.encode_packed(opts, batch, 7)
  enc = _Encoder(opts, opts.width)
  try:
    out, rows = enc.encode(batch, 7)
  except _lib.DvError as e:
    print('refused: status %d: %s' % (e.status, e))
    return 0
  dev = torch.device('cuda:0')
  out_t = torch.full((batch.out_bytes(7),), 0xAB, dtype=torch.uint8, device=dev)
  rows_t = torch.full((batch.n_items,), -1, dtype=torch.int32, device=dev)
  DeviceBatch(batch, dev).encode(enc, 7, out_t, rows_t)
  torch.cuda.synchronize()
  n = batch.n_items
  shape = (n, -1)
  same = (out.reshape(shape) == want.reshape(shape)).all(axis=1) & (rows == want_rows) & \
         (out_t.cpu().numpy().reshape(shape) == want.reshape(shape)).all(axis=1) & (rows_t.cpu().numpy() == want_rows)
  print('DV_CIG_CACHE geometry: items equal to the oracle: %d/%d' % (int(same.sum()), n))
  return 0 if same.all() else 1


if __name__ == '__main__':
  raise SystemExit(main())
