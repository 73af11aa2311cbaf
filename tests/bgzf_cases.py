"""The BGZF rule of DESIGN.md section 24 restated in plain Python, and the texts the BGZF tests share
(tests/test_bgzf_cpu.py, tests/test_hip_bgzf.py).

The restatement loops over bytes and keeps a list of bits; it shares no code with the library.  The fixed Huffman codes
come from RFC 1951's code lengths by its canonical-code algorithm, the length and distance symbols from the RFC's tables
of bases and extra bits, written out here.  The parameters are read from the library (pp.bgzf_params()), so another
block, tile, segment or hash size changes nothing here.
"""
import functools
import zlib

import numpy as np

from deepvariant_amd import postprocess_variants as pp

PARAMS = pp.bgzf_params()
B, TILE, SEG, HASH_BITS = PARAMS['block'], PARAMS['tile'], PARAMS['seg'], PARAMS['hash_bits']
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
               258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in range(2)]


def _canonical(lengths):
  """RFC 1951 section 3.2.2: code lengths -> [(code, length)], a code's bits from its most significant."""
  count = [0] * (max(lengths) + 1)
  for n in lengths:
    count[n] += 1
  count[0] = 0
  code, first = 0, [0] * (max(lengths) + 1)
  for n in range(1, max(lengths) + 1):
    code = (code + count[n - 1]) << 1
    first[n] = code
  out = []
  for n in lengths:
    out.append((first[n], n))
    first[n] += 1
  return out


def _msb_first(code, n):
  return [(code >> (n - 1 - k)) & 1 for k in range(n)]


def _lsb_first(value, n):
  return [(value >> k) & 1 for k in range(n)]


LITERAL_BITS = [_msb_first(c, n) for c, n in _canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)]
DISTANCE_BITS = [_msb_first(c, n) for c, n in _canonical([5] * 30)]


def tokens_of_block(data):
  """One block's tokens in order: an int is a literal, (length, distance) a match."""
  n = len(data)
  head = [-1] * (1 << HASH_BITS)
  cand = [-1] * n
  for base in range(0, n, TILE):
    seen = []
    for i in range(base, min(base + TILE, n)):
      if i + 4 <= n:
        w = data[i] | data[i + 1] << 8 | data[i + 2] << 16 | data[i + 3] << 24
        h = ((w * 2654435761) & 0xffffffff) >> (32 - HASH_BITS)
        cand[i] = head[h]
        seen.append((h, i))
    for h, i in seen:
      head[h] = max(head[h], i)
  tokens = []
  for begin in range(0, n, SEG):
    end = min(begin + SEG, n)
    i = begin
    while i < end:
      c, length = cand[i], 0
      if c >= 0:
        cap = min(258, end - i)
        while length < cap and data[c + length] == data[i + length]:
          length += 1
      if c >= 0 and i - c <= 32768 and length >= 4:
        tokens.append((length, i - c))
        i += length
      else:
        tokens.append(data[i])
        i += 1
  return tokens


def bits_of_tokens(tokens):
  bits = [1, 1, 0]                      # BFINAL = 1, BTYPE = 01 from its least significant bit
  for token in tokens:
    if isinstance(token, int):
      bits.extend(LITERAL_BITS[token])
      continue
    length, distance = token
    k = max(j for j in range(29) if LENGTH_BASE[j] <= length)
    bits.extend(LITERAL_BITS[257 + k])
    bits.extend(_lsb_first(length - LENGTH_BASE[k], LENGTH_EXTRA[k]))
    k = max(j for j in range(30) if DIST_BASE[j] <= distance)
    bits.extend(DISTANCE_BITS[k])
    bits.extend(_lsb_first(distance - DIST_BASE[k], DIST_EXTRA[k]))
  bits.extend(LITERAL_BITS[256])
  return bits


def member_of_block(data):
  """-> (the member's bytes, stored)."""
  n = len(data)
  bits = bits_of_tokens(tokens_of_block(data))
  bits.extend([0] * (-len(bits) % 8))
  payload = bytes(sum(bit << k for k, bit in enumerate(bits[at:at + 8])) for at in range(0, len(bits), 8))
  stored = len(payload) > n + 5
  if stored:
    payload = b'\x01' + n.to_bytes(2, 'little') + (n ^ 0xffff).to_bytes(2, 'little') + data
  size = 18 + len(payload) + 8
  head = b'\x1f\x8b\x08\x04' + b'\0' * 4 + b'\x00\xff' + b'\x06\x00' + b'BC' + b'\x02\x00' + (size - 1).to_bytes(2, 'little')
  return head + payload + zlib.crc32(data).to_bytes(4, 'little') + n.to_bytes(4, 'little'), stored


def restated(text):
  """-> (the file, block_coff, the number of stored blocks)."""
  out, coff, stored = [], [0], 0
  for at in range(0, len(text), B):
    member, kept = member_of_block(text[at:at + B])
    out.append(member)
    coff.append(coff[-1] + len(member))
    stored += kept
  return b''.join(out) + EOF, coff, stored


def members(file):
  """The file walked by BSIZE -> [(offset, member bytes)], the end-of-file member last."""
  out, at = [], 0
  while at < len(file):
    assert file[at:at + 4] == b'\x1f\x8b\x08\x04' and file[at + 10:at + 16] == b'\x06\x00BC\x02\x00'
    size = int.from_bytes(file[at + 16:at + 18], 'little') + 1
    out.append((at, file[at:at + size]))
    at += size
  assert at == len(file)
  return out


# ---- the texts
ROW = b'chr20\t10000001\t.\tA\t<*>\t0\t.\tEND=10000042\tGT:GQ:MIN_DP:PL\t0/0:50:31:0,90,899'.ljust(79, b'x') + b'\n'
assert len(ROW) == 80
EDGE = TILE * SEG // np.gcd(TILE, SEG)          # a position where a tile and a segment both begin


def noise(n, seed, values=144):
  """Seeded bytes below `values`.  Below 144 every literal takes eight bits, so a block with one match is shorter
  deflated than stored and its tokens show in the file; with all 256 values a block of noise is stored."""
  return np.random.default_rng(seed).integers(0, values, n, dtype=np.uint8).tobytes()


def repeat_at_distance(distance, length=40, at=None, seed=5):
  """Noise with one stretch of `length` bytes standing twice, `distance` apart; the second starts at `at`, where a tile
  and a segment begin, so that the first lies in an earlier tile whatever the distance.  A distance below the length
  gives a stretch that overlaps itself."""
  at = at if at is not None else (distance // EDGE + 1) * EDGE
  assert at % EDGE == 0 and at >= distance
  if distance < length:
    unit = noise(distance, seed + 1)
    body = (unit * (length // distance + 2))[:distance + length]
  else:
    # one letter between them: noise would enter thousands of positions into the 2^HASH_BITS heads and push the first
    # stretch out of its own
    stretch = noise(length, seed + 1)
    body = stretch + b'z' * (distance - length) + stretch
  return noise(at - distance, seed) + body + noise(50, seed + 3)


@functools.lru_cache(maxsize=None)
def named_texts():
  from tests import gvcf_rows_cases as R
  from tests import test_gvcf_text_cpu as G
  texts = {}
  for n in (0, 1, 3, 4, 5, SEG - 1, SEG, SEG + 1, B - 1, B, B + 1, 2 * B + 1):
    texts['length_%d' % n] = (ROW * (n // len(ROW) + 1))[:n]
  texts['one_letter'] = b'A' * (B + 1)
  texts['row_400_times'] = ROW * 400
  texts['noise_2000'] = noise(2000, 11, 256)
  texts['every_byte_twice'] = bytes(range(256)) * 2
  texts['repeat_of_3'] = noise(EDGE - 100, 21) + b'abcQ' + noise(96, 22) + b'abcR' + noise(30, 23)
  texts['repeat_of_4'] = noise(EDGE - 100, 21) + b'abcdQ' + noise(95, 22) + b'abcdR' + noise(30, 23)
  texts['stretch_of_300_twice'] = noise(300, 31) + noise(EDGE * (300 // EDGE + 1) - 300, 32) + noise(300, 31) + noise(9, 33)
  for distance in (4, 5, 256, 257, 24576, 24577, B - 300):
    if distance + 100 <= B:
      texts['distance_%d' % distance] = repeat_at_distance(distance)
  texts['same_tile'] = noise(3 * TILE + 2, 41) + noise(20, 42) * 2 + noise(100, 43)
  texts['gvcf_by_hand'] = (G.HEADER % G.MED_DP_LINE + G.ROWS_WITH_MED_DP).encode()
  layout = R.fill(R.split_blocks(2049 - 200, range(0, 500, 5)))
  texts['gvcf_2049_rows'] = R.reference(*layout)[0]
  return texts


def seeded_text(seed):
  """A mixture of repeated rows and noise, 0 to 3 B bytes.  The length is 3 B u^4 for a uniform u: every length up to
  3 B can come, most texts are short (the restatement is a Python loop over bytes), and about one in four passes a
  block's end."""
  rng = np.random.default_rng(1000 + seed)
  n = int(3 * B * rng.random() ** 4)
  parts, have = [], 0
  while have < n:
    kind = rng.integers(0, 3)
    if kind == 0:
      part = noise(int(rng.integers(1, 200)), int(rng.integers(0, 1 << 30)), (144, 256)[int(rng.integers(0, 2))])
    elif kind == 1:
      part = ROW[int(rng.integers(0, 40)):] * int(rng.integers(1, 30))
    else:
      row = b'chr%d\t%d\t.\tN\t<*>\t0\t.\tEND=%d\n' % (seed % 23, int(rng.integers(0, 10 ** 8)), int(rng.integers(0, 10 ** 8)))
      part = row * int(rng.integers(1, 12))
    parts.append(part)
    have += len(part)
  return b''.join(parts)[:n]


def block_counts_text(blocks):
  """A repeated row cut to exactly `blocks` blocks, the last of them one byte."""
  n = (blocks - 1) * B + 1
  return (ROW * (n // len(ROW) + 1))[:n]
