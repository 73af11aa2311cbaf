// The rule by which a text becomes BGZF members, written once and compiled for both sides:
// dv_bgzf_compress walks a block with it on the host, deflate_blocks_kernel (bgzf.hip) gives every block a workgroup.
// Integer arithmetic in a fixed order, so both sides write the same bytes.
//
//   the text is cut every kBlock bytes; a block of n bytes becomes one member:
//   candidates  h(i) = (the four bytes at i, little-endian, * 2654435761 mod 2^32) >> (32 - kHashBits), i <= n - 4;
//               head[] starts empty; the positions go in tiles of kTile: every i of a tile reads cand(i) = head[h(i)],
//               then head[h] becomes the largest i of the tile with that hash -- a candidate lies in an earlier tile
//   parse       segments of kSeg bytes, each from its start, greedy: len = the common prefix of cand(i) and i, at most
//               min(258, segment end - i); a match (len, i - cand(i)) when len >= 4, else the literal
//   bits        one deflate block, BFINAL = 1, fixed Huffman, the tokens, symbol 256; when that takes more than n + 5
//               bytes the block is stored (BTYPE = 00) instead
//   member      the 18-byte BGZF header, the payload, CRC-32 and ISIZE
#ifndef DV_BGZF_DEFLATE_H_
#define DV_BGZF_DEFLATE_H_

#include <cstdint>

#if defined(__HIPCC__)
#define DV_BZ_HD __host__ __device__ inline
#define DV_BZ_CX __host__ __device__ constexpr
#else
#define DV_BZ_HD inline
#define DV_BZ_CX constexpr
#endif

namespace dv {
namespace bz {

constexpr int32_t kBlock = 32640;       // input bytes per member: the block, its candidates and head share the LDS
constexpr int32_t kTile = 64;           // one wave
constexpr int32_t kSeg = 128;           // a block has at most 255 segments: one per lane of a 256-lane workgroup
constexpr int32_t kHashBits = 12;
constexpr int32_t kHeads = 1 << kHashBits;
constexpr int32_t kNoCand = 0xffff;     // in the uint16 candidate array; positions stay below kBlock
constexpr int32_t kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr int32_t kHeadBytes = 18, kTailBytes = 8, kStoredBytes = 5, kEofBytes = 28;
constexpr int32_t kSlot = (kBlock + kStoredBytes + kHeadBytes + kTailBytes + 3) / 4 * 4;   // no member is longer
constexpr int32_t kBlockBits = 3, kEndBits = 7;         // BFINAL and BTYPE in front, symbol 256 behind

static_assert(kBlock < kNoCand && kBlock % 4 == 0, "a position fits the candidate array");
static_assert(kSlot <= 65536, "a BGZF member is at most 64 KiB");

DV_BZ_HD uint32_t hash4(const uint8_t* p) {
  const uint32_t w = static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 |
                     static_cast<uint32_t>(p[3]) << 24;
  return (w * 2654435761u) >> (32 - kHashBits);
}

// The low `bits` bits of v in reverse order: a Huffman code goes out from its most significant bit.
DV_BZ_CX uint32_t reversed(uint32_t v, int32_t bits) {
  uint32_t r = 0;
  for (int32_t k = 0; k < bits; ++k) r |= ((v >> k) & 1u) << (bits - 1 - k);
  return r;
}

DV_BZ_CX int32_t floor_log2(uint32_t v) {       // v > 0
  int32_t n = 0;
  while (v >>= 1) ++n;
  return n;
}

struct Code {                   // a symbol of the fixed trees with its extra bits
  uint32_t code;                // already reversed
  int32_t bits;
  uint32_t extra;
  int32_t extra_bits;
};

DV_BZ_CX Code literal_code(uint32_t symbol) {           // 0..287 of the literal/length tree
  if (symbol < 144) return Code{reversed(0x30 + symbol, 8), 8, 0, 0};
  if (symbol < 256) return Code{reversed(0x190 + symbol - 144, 9), 9, 0, 0};
  if (symbol < 280) return Code{reversed(symbol - 256, 7), 7, 0, 0};
  return Code{reversed(0xc0 + symbol - 280, 8), 8, 0, 0};
}

DV_BZ_CX Code length_code(int32_t len) {                // 3..258
  if (len == 258) return literal_code(285);
  const uint32_t l = static_cast<uint32_t>(len - 3);
  if (l < 8) return literal_code(257 + l);
  const int32_t eb = floor_log2(l) - 2;
  Code c = literal_code(261 + 4 * static_cast<uint32_t>(eb) + ((l >> eb) & 3u));
  c.extra = l & ((1u << eb) - 1);
  c.extra_bits = eb;
  return c;
}

DV_BZ_CX Code distance_code(int32_t dist) {             // 1..32768, five bits a code
  const uint32_t d = static_cast<uint32_t>(dist - 1);
  if (d < 4) return Code{reversed(d, 5), 5, 0, 0};
  const int32_t eb = floor_log2(d) - 1;
  return Code{reversed(2 * static_cast<uint32_t>(eb) + 2 + ((d >> eb) & 1u), 5), 5, d & ((1u << eb) - 1), eb};
}

// ---- the symbols above against RFC 1951's tables of bases and extra bits, at every build: with kSeg = 128 no text
// reaches a length above 128, so nothing else would see symbols 281 to 285 before someone changes kSeg.
// (tools/bgzf_check.cpp walks every distance up to 32,768 as well.)
namespace rfc {
constexpr int32_t kLengthBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                     31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr int32_t kLengthExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr int32_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                   193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr int32_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

constexpr bool length_is(int32_t len) {
  int32_t k = 28;
  while (kLengthBase[k] > len) --k;
  if (len == 258) k = 28;
  const Code want = literal_code(static_cast<uint32_t>(257 + k)), got = length_code(len);
  return got.code == want.code && got.bits == want.bits && got.extra_bits == kLengthExtra[k] &&
         got.extra == static_cast<uint32_t>(len - kLengthBase[k]);
}
constexpr bool distance_is(int32_t dist) {
  int32_t k = 29;
  while (kDistBase[k] > dist) --k;
  const Code got = distance_code(dist);
  return got.code == reversed(static_cast<uint32_t>(k), 5) && got.bits == 5 && got.extra_bits == kDistExtra[k] &&
         got.extra == static_cast<uint32_t>(dist - kDistBase[k]);
}
constexpr bool symbols_agree() {
  for (int32_t len = 3; len <= 258; ++len) {
    if (!length_is(len)) return false;
  }
  for (int32_t k = 0; k < 30; ++k) {            // both sides of every edge between two distance symbols
    if (!distance_is(kDistBase[k]) || !distance_is(k < 29 ? kDistBase[k + 1] - 1 : 32768)) return false;
  }
  return true;
}
static_assert(symbols_agree(), "length_code and distance_code give RFC 1951's symbols and extra bits");
}  // namespace rfc

// A segment's tokens in order: sink.literal(byte) and sink.match(len, dist).  cand: kNoCand or a position before i.
template <class Sink>
DV_BZ_HD void walk_segment(const uint8_t* data, const uint16_t* cand, int32_t begin, int32_t end, Sink& sink) {
  int32_t i = begin;
  while (i < end) {
    const int32_t c = cand[i];
    const int32_t cap = end - i < kMaxMatch ? end - i : kMaxMatch;
    int32_t len = 0;
    if (c != kNoCand && i - c <= kMaxDist && cap >= kMinMatch) {
      while (len < cap && data[c + len] == data[i + len]) ++len;
    }
    if (len >= kMinMatch) {
      sink.match(len, i - c);
      i += len;
    } else {
      sink.literal(data[i]);
      ++i;
    }
  }
}

struct CountSink {              // the bits a segment takes
  int32_t bits = 0;
  DV_BZ_HD void literal(uint8_t b) { bits += b < 144 ? 8 : 9; }
  DV_BZ_HD void match(int32_t len, int32_t dist) {
    const Code l = length_code(len), d = distance_code(dist);
    bits += l.bits + l.extra_bits + d.bits + d.extra_bits;
  }
};

// Out: put(value, bits) appends the low `bits` (<= 16) bits of value to an LSB-first stream.
template <class Out>
struct BitSink {
  Out* out;
  DV_BZ_HD void symbol(const Code& c) {
    out->put(c.code, c.bits);
    if (c.extra_bits > 0) out->put(c.extra, c.extra_bits);
  }
  DV_BZ_HD void literal(uint8_t b) { symbol(literal_code(b)); }
  DV_BZ_HD void match(int32_t len, int32_t dist) {
    symbol(length_code(len));
    symbol(distance_code(dist));
  }
};

// The payload's length for `bits` token bits of an n-byte block, and whether the block is stored instead.
DV_BZ_HD int32_t fixed_payload_bytes(int64_t token_bits) {
  return static_cast<int32_t>((kBlockBits + token_bits + kEndBits + 7) / 8);
}
DV_BZ_HD bool keeps_bytes(int64_t token_bits, int32_t n) { return fixed_payload_bytes(token_bits) > n + kStoredBytes; }

// Byte k of a member's 18-byte header; member_bytes is the whole member's length.
DV_BZ_HD uint8_t head_byte(int32_t k, int32_t member_bytes) {
  switch (k) {
    case 0: return 0x1f;
    case 1: return 0x8b;
    case 2: return 8;
    case 3: return 4;
    case 9: return 0xff;
    case 10: return 6;
    case 12: return 'B';
    case 13: return 'C';
    case 14: return 2;
    case 16: return static_cast<uint8_t>((member_bytes - 1) & 0xff);
    case 17: return static_cast<uint8_t>((member_bytes - 1) >> 8);
    default: return 0;          // mtime, XFL, the high bytes of XLEN and of the subfield's length
  }
}

// Byte k of the end-of-file member: an empty fixed-Huffman block.
DV_BZ_HD uint8_t eof_byte(int32_t k) {
  if (k < kHeadBytes) return head_byte(k, kEofBytes);
  return k == kHeadBytes ? 3 : 0;
}

// ---- CRC-32 (gzip's polynomial, reflected) and the operator that joins two slices' CRCs
constexpr uint32_t kCrcPoly = 0xedb88320u;

// a(x) * b(x) mod P, both in the reflected representation (bit 31 is x^0).
DV_BZ_HD uint32_t crc_multiply(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int32_t k = 31; k >= 0; --k) {
    if ((a >> k) & 1u) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

DV_BZ_HD uint32_t crc_bytes(const uint32_t* table, const uint8_t* data, int32_t from, int32_t to) {
  uint32_t crc = 0xffffffffu;
  for (int32_t i = from; i < to; ++i) crc = table[(crc ^ data[i]) & 0xffu] ^ (crc >> 8);
  return ~crc;
}

}  // namespace bz
}  // namespace dv

#endif  // DV_BGZF_DEFLATE_H_
