"""A .g.vcf.gz as BGZF: the parent's gzip write against the BGZF compressor on the host
(dv_bgzf_compress), on the device (dv_bgzf_compress_device) and behind the rows (dv_gvcf_rows_bgzf_device), alternating
in one process, on the layouts of tools/gvcf_rows_ab.py.

Stretches, each the median, minimum and maximum wall time over --repeats runs after a warm-up, after the outputs were
compared with == (the device's file with the host's, every file decompressed with the text):
  gzip             the baseline: the rows' device call (section 23's route c, its download included), then
                   gzip.GzipFile(mtime=0) over the text, as _write_bytes does without DV_BGZF
  gzip_alone       the gzip pass alone, the text ready
  host             bgzf_compress over the ready text
  device           bgzf_compress(device=True) over the ready text in host memory: upload, five launches, download
  rows_then_host   the rows' device call, then bgzf_compress on the host
  rows_bgzf        gvcf_rows_bgzf_native(device=True): the rows and the compressor in one call, the text never downloaded
Sizes: the text, the gzip stream, the BGZF file, zlib level 1 and level 6 over the same blocks (payloads alone + 26
bytes a member), the stored blocks, bytes_down of rows_bgzf (rows + compressor) and of the rows' call alone.
Prints one JSON line per layout.  Fails without a GPU.

  python tools/bgzf_ab.py --layout fixture [--repeats 7] [--out result.json]
  python tools/bgzf_ab.py --layout synthetic --blocks 8000000 --variants 400000 [--gzip_repeats 1]
  python tools/bgzf_ab.py --kernels_only --blocks 8000000 --variants 400000     # rows_bgzf three times and nothing
                                                    # else: run under rocprofv3 --kernel-trace --stats
"""
import argparse
import gc
import gzip
import io
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gvcf_merge_ab as AB                                          # noqa: E402
import gvcf_rows_ab as RAB                                          # noqa: E402
from deepvariant_amd import _lib                                    # noqa: E402
from deepvariant_amd import postprocess_variants as pp              # noqa: E402


def parent_gzip(text):
  stream = io.BytesIO()
  with gzip.GzipFile(filename='', fileobj=stream, mode='wb', mtime=0) as z:
    z.write(text)
  return stream.getvalue()


def zlib_per_block(text, level, block):
  total = 28
  for at in range(0, len(text), block):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    total += len(c.compress(text[at:at + block])) + len(c.flush()) + 26
  return total


def measure(records, blocks, ref_reader, contigs, repeats, gzip_repeats):
  import torch
  _, kwargs = RAB.native_arguments(records, blocks, ref_reader, contigs)
  kwargs = {k: v for k, v in kwargs.items() if k != 'want_row_off'}
  med_dp = int(bool((kwargs['blocks']['med_dp'] >= 0).any()))
  text = pp.gvcf_rows_native(device=True, **kwargs).text
  rows_down = pp.last_rows_stats()['bytes_down']
  routes = {
      'gzip': lambda: parent_gzip(pp.gvcf_rows_native(device=True, **kwargs).text),
      'gzip_alone': lambda: parent_gzip(text),
      'host': lambda: pp.bgzf_compress(text),
      'device': lambda: pp.bgzf_compress(text, device=True),
      'rows_then_host': lambda: pp.bgzf_compress(pp.gvcf_rows_native(device=True, **kwargs).text),
      'rows_bgzf': lambda: pp.gvcf_rows_bgzf_native(b'', med_dp=med_dp, device=True, **kwargs).file.data,
  }
  # the outputs first
  file = routes['host']()
  stream = routes['gzip']()
  if gzip.decompress(file) != text or gzip.decompress(stream) != text:
    raise SystemExit('bgzf_ab: a file does not decompress to the text')
  gzip_bytes = len(stream)
  del stream
  for route in ('device', 'rows_then_host', 'rows_bgzf'):
    if routes[route]() != file:
      raise SystemExit('bgzf_ab: route %s writes other bytes than the host code' % route)
  fused_down = pp.last_rows_stats()['bytes_down'] + pp.last_bgzf_stats()['bytes_down']
  stats = pp.last_bgzf_stats()
  block = pp.bgzf_params()['block']
  sizes = {'text_bytes': len(text), 'gzip_bytes': gzip_bytes, 'bgzf_bytes': len(file),
           'zlib1_per_block_bytes': zlib_per_block(text, 1, block), 'zlib6_per_block_bytes': zlib_per_block(text, 6, block),
           'stored_blocks': stats['stored_blocks'], 'blocks_of_text': stats['blocks'],
           'bytes_down_rows_bgzf': fused_down, 'bytes_down_rows_alone': rows_down}
  del file
  times = {route: [] for route in routes}
  for i in range(repeats + 1):            # the routes alternate, one warm-up run each
    for route, fn in routes.items():
      if route.startswith('gzip') and i > gzip_repeats:
        continue                          # a level-9 pass over a contig's text takes tens of seconds
      gc.collect()
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      out = fn()
      seconds = time.perf_counter() - t0
      del out
      if i:
        times[route].append(seconds)
  result = {route: AB._summary(t) for route, t in times.items()}
  result.update(sizes)
  result['gzip_repeats'] = min(repeats, gzip_repeats)
  result['device_stats'] = stats
  return result


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--layout', choices=('fixture', 'synthetic'), default='fixture')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--gzip_repeats', type=int, default=7, help='runs of the two gzip stretches after the warm-up')
  ap.add_argument('--contig_kb', type=float, default=230000.0)
  ap.add_argument('--blocks', type=int, default=8_000_000)
  ap.add_argument('--variants', type=int, default=400_000)
  ap.add_argument('--kernels_only', action='store_true')
  ap.add_argument('--out', default='')
  args = ap.parse_args(argv)
  if _lib.device_count() == 0:
    raise SystemExit('bgzf_ab: no GPU')
  import torch
  torch.cuda.init()
  if args.kernels_only:
    _, kwargs = RAB.native_arguments(*RAB.synthetic_layout(args.blocks, args.variants, args.contig_kb))
    kwargs = {k: v for k, v in kwargs.items() if k != 'want_row_off'}
    for _ in range(3):
      pp.gvcf_rows_bgzf_native(b'', med_dp=0, device=True, **kwargs)
    print(json.dumps({'kernels_only': {'rows': pp.last_rows_stats(), 'bgzf': pp.last_bgzf_stats()}}))
    return
  if args.layout == 'fixture':
    records, blocks, ref_reader, contigs, kb = AB.fixture_run()
    result = {'layout': 'fixture', 'kb': kb}
  else:
    records, blocks, ref_reader, contigs = RAB.synthetic_layout(args.blocks, args.variants, args.contig_kb)
    result = {'layout': 'synthetic', 'contig_kb': args.contig_kb}
  result.update(blocks=sum(len(b) for b in blocks.values()), variants=len(records), repeats=args.repeats)
  result.update(measure(records, blocks, ref_reader, contigs, args.repeats, args.gzip_repeats))
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'a') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
