// The text of a gVCF reference-block row, written once and compiled for both sides: dv_gvcf_rows
// formats with it on the host, the kernels of gvcf_rows.hip give every piece a lane.  Integers and one double multiply
// per likelihood, so both sides agree byte for byte with the Python formatter (postprocess_variants._piece_rows):
//
//   NAME \t START+1 \t . \t BASE \t <*> \t 0 \t . \t END=<end> \t GT:GQ:MIN_DP[:MED_DP]:PL \t
//   <0/0|./.>:gq:min_dp[:<med_dp|.>]:p0,p1,p2 \n
//
// No array is indexed by a run-time value here: the digit count comes from comparisons, the digits go straight to
// their bytes from the last to the first, and the fixed parts are literals copied by unrolled loops.
#ifndef DV_GVCF_ROWS_H_
#define DV_GVCF_ROWS_H_

#include <cmath>
#include <cstdint>

#include "dvhip.h"
#include "gvcf_merge.h"

namespace dv {
namespace gr {

// |v| as an unsigned number, INT64_MIN included.
DV_GM_HD uint64_t magnitude(int64_t v) { return v < 0 ? 0 - static_cast<uint64_t>(v) : static_cast<uint64_t>(v); }

// The number of bytes '%d' % v takes: the digits, and the sign of a negative number.
DV_GM_HD int32_t decimal_length(int64_t v) {
  const uint64_t m = magnitude(v);
  int32_t n = 1;
  uint64_t power = 10;                          // 10^n; 10^19 still fits, and n stops at 20
  while (n < 20 && m >= power) {
    power *= 10;
    ++n;
  }
  return n + (v < 0 ? 1 : 0);
}

// '%d' % v at `at` -> its length.
DV_GM_HD int32_t write_decimal(char* at, int64_t v) {
  const int32_t n = decimal_length(v);
  uint64_t m = magnitude(v);
  if (v < 0) at[0] = '-';
  int32_t i = n - 1;
  while (m > 0xffffffffull) {                   // 64-bit divisions only while they are needed
    at[i--] = static_cast<char>('0' + static_cast<int32_t>(m % 10));
    m /= 10;
  }
  uint32_t small = static_cast<uint32_t>(m);
  do {
    at[i--] = static_cast<char>('0' + static_cast<int32_t>(small % 10));
    small /= 10;
  } while (small != 0);
  return n;
}

// A likelihood the rule can print: finite, and |10 GL| below 2^53 (np.rint(...).astype(int64) is garbage past it).
DV_GM_HD bool likelihood_ok(double gl) {
  const double x = -10.0 * gl;
  return x == x && x > -9007199254740992.0 && x < 9007199254740992.0;
}

// int(np.rint(-10 GL)): half to even.
DV_GM_HD int64_t phred(double gl) { return static_cast<int64_t>(rint(-10.0 * gl)); }

// The block's three PLs, less the smallest.
DV_GM_HD void block_pls(const dv_gvcf_block& b, int64_t* p0, int64_t* p1, int64_t* p2) {
  const int64_t a = phred(b.likelihoods[0]), c = phred(b.likelihoods[1]), d = phred(b.likelihoods[2]);
  int64_t low = a < c ? a : c;
  if (d < low) low = d;
  *p0 = a - low;
  *p1 = c - low;
  *p2 = d - low;
}

// Where a row goes: Count adds the lengths up, Write stores the bytes.  One template over both states the format once.
struct Count {
  int64_t n = 0;
  template <int N>
  DV_GM_HD void literal(const char (&)[N]) { n += N - 1; }
  DV_GM_HD void bytes(const char*, int64_t len) { n += len; }
  DV_GM_HD void byte(char) { ++n; }
  DV_GM_HD void decimal(int64_t v) { n += decimal_length(v); }
};
struct Write {
  char* at;
  template <int N>
  DV_GM_HD void literal(const char (&text)[N]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < N - 1; ++i) at[i] = text[i];
    at += N - 1;
  }
  DV_GM_HD void bytes(const char* from, int64_t len) {
    for (int64_t i = 0; i < len; ++i) at[i] = from[i];
    at += len;
  }
  DV_GM_HD void byte(char c) { *at++ = c; }
  DV_GM_HD void decimal(int64_t v) { at += write_decimal(at, v); }
};

// One piece [start, end) of block `b` on the contig `name`; `base`: the reference base at `start`; med_dp: the call
// carries MED_DP.
template <class Sink>
DV_GM_HD void piece_row(Sink& out, const char* name, int64_t name_len, int64_t start, int64_t end, uint8_t base,
                        const dv_gvcf_block& b, bool med_dp) {
  int64_t p0, p1, p2;
  block_pls(b, &p0, &p1, &p2);
  out.bytes(name, name_len);
  out.byte('\t');
  out.decimal(start + 1);
  out.literal("\t.\t");
  out.byte(static_cast<char>(base));
  out.literal("\t<*>\t0\t.\tEND=");
  out.decimal(end);
  if (med_dp) {
    out.literal("\tGT:GQ:MIN_DP:MED_DP:PL\t");
  } else {
    out.literal("\tGT:GQ:MIN_DP:PL\t");
  }
  if (b.has_valid_gl) {
    out.literal("0/0:");
  } else {
    out.literal("./.:");
  }
  out.decimal(b.gq);
  out.byte(':');
  out.decimal(b.min_dp);
  out.byte(':');
  if (med_dp) {
    if (b.med_dp < 0) {
      out.byte('.');
    } else {
      out.decimal(b.med_dp);
    }
    out.byte(':');
  }
  out.decimal(p0);
  out.byte(',');
  out.decimal(p1);
  out.byte(',');
  out.decimal(p2);
  out.byte('\n');
}

DV_GM_HD int64_t piece_row_length(int64_t name_len, int64_t start, int64_t end, const dv_gvcf_block& b, bool med_dp) {
  Count out;
  piece_row(out, nullptr, name_len, start, end, 'N', b, med_dp);
  return out.n;
}

// The row at `at` -> its length, which is piece_row_length's.
DV_GM_HD int64_t write_piece_row(char* at, const char* name, int64_t name_len, int64_t start, int64_t end, uint8_t base,
                                 const dv_gvcf_block& b, bool med_dp) {
  Write out{at};
  piece_row(out, name, name_len, start, end, base, b, med_dp);
  return out.at - at;
}

// No piece of the block is longer than this: a piece's start + 1 and its end lie in [block start + 1, block end], so
// neither prints longer than the longer of those two.
DV_GM_HD int64_t longest_piece_row(int64_t name_len, const dv_gvcf_block& b, bool med_dp) {
  const int32_t first = decimal_length(b.start + 1), last = decimal_length(b.end);
  return piece_row_length(name_len, b.start, b.end, b, med_dp) - first - last + 2 * (first > last ? first : last);
}

// gm::walk_range, which also reports where each piece's start came from: emit(k, piece_start, piece_end, src) with
// src = the variant whose end last moved the cursor, so that piece_start == var_end[src], or -1 for a piece that starts
// at the block's start.
template <class Emit>
DV_GM_HD int32_t walk_range_src(int64_t s, int64_t e, const int64_t* var_start, const int64_t* var_end, int64_t lo,
                                int64_t hi, Emit&& emit) {
  int64_t cursor = s, src = -1;
  int32_t n = 0;
  for (int64_t j = lo; j < hi && cursor < e; ++j) {
    if (cursor < var_start[j]) {
      emit(n, cursor, var_start[j], src);
      ++n;
    }
    if (var_end[j] > cursor) {
      cursor = var_end[j];
      src = j;
    }
  }
  if (cursor < e) {
    emit(n, cursor, e, src);
    ++n;
  }
  return n;
}

// gm::walk_block likewise.
template <class Emit>
DV_GM_HD int32_t walk_block_src(int64_t s, int64_t e, const int64_t* var_start, const int64_t* var_end,
                                const int64_t* cm, int64_t v0, int64_t v1, Emit&& emit) {
  return walk_range_src(s, e, var_start, var_end, gm::first_above(cm, v0, v1, s), gm::first_at_least(var_start, v0, v1, e),
                        emit);
}

// A byte that survives Python's latin-1 decode and UTF-8 encode as itself and shows in a row.
DV_GM_HD bool printable(uint8_t c) { return c >= 0x21 && c <= 0x7e; }

}  // namespace gr
}  // namespace dv

#endif  // DV_GVCF_ROWS_H_
