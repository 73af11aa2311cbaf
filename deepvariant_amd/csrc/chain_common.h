// Device pieces shared by the kernels that keep whole feature maps of a tile resident in LDS
// and feed both MFMA operands from there (chain.hip, block35.hip): barriers, the LDS-DMA
// descriptor helper, one 16-channel chunk of MFMAs over the filter taps, the shift + ReLU +
// fp16 epilogue into C8 pieces, and the filter-tap masks at the map border.
#ifndef DV_CHAIN_COMMON_H_
#define DV_CHAIN_COMMON_H_

#include "conv_common.h"

namespace dv {
namespace chaink {

using namespace convk;

typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __forceinline__ void barrier_after_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
__device__ __forceinline__ void barrier_after_dma() {
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
}
__device__ __forceinline__ void barrier_only() { asm volatile("s_barrier" ::: "memory"); }

__device__ __forceinline__ const char* uniform_ptr(const char* q) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(q);
  const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v));
  const unsigned up = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v >> 32));
  return reinterpret_cast<const char*>((static_cast<unsigned long long>(up) << 32) | lo);
}

// Which of a wave's NB x 3 (cout subtile, pixel fragment) MFMA tiles exist.  A layer of five
// subtiles (160 channels) cannot be halved: 3 + 2 subtiles leaves two SIMDs idle a third of the
// time.  Instead the pixel half's 15 tiles go 8 + 7: the first wave takes subtiles 0-2 WITHOUT
// (subtile 2, fragment 2), the second subtiles 2-4 with ONLY fragment 2 of subtile 2.
//   SKIP 0: all NB x 3     SKIP 1: without (nb 2, pt 2)     SKIP 2: without (nb 0, pt 0) and (nb 0, pt 1)
template <int SKIP>
__device__ __forceinline__ constexpr bool chain_tile(int nb, int pt) {
  return SKIP == 1 ? !(nb == 2 && pt == 2) : SKIP == 2 ? !(nb == 0 && pt < 2) : true;
}

// One 16-channel chunk: NT filter taps x the wave's MFMA tiles.  The fragments of tap i + 1 are
// requested between the MFMAs of tap i (two static register sets, one request per MFMA slot).
// PRE: the first tap's pixel fragments were requested by the caller BEFORE the chunk barrier (the
// activation tile does not change inside a layer; only the weight slab waits for the barrier).
// KW: 0 = one-dimensional filter, tap i sits i * b_tap_stride bytes from the first (b_tap_stride =
// one pixel or one tile row); > 0 = KW-wide two-dimensional filter, tap i = (i / KW) tile rows
// (b_tap_stride bytes each) + (i % KW) pixels.
template <int NB, int PT, int NT, int KW, int SKIP, bool PRE>
__device__ __forceinline__ void chain_step(const char* smem, unsigned a_addr, unsigned a_tap_stride,
                                           const unsigned (&b_addr)[PT], unsigned b_tap_stride,
                                           const unsigned (&mask)[PT], unsigned zero_addr,
                                           const half8_t (&b_pre)[PT], float16_t (&acc)[NB][PT]) {
  half8_t A[2][NB], B[2][PT];
  auto load_a = [&](int i, int s) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      A[s][nb] = *reinterpret_cast<const half8_t*>(smem + a_addr + i * a_tap_stride + nb * 512);
    }
  };
  auto load_b = [&](int i, int s) {
    const unsigned off = KW == 0 ? i * b_tap_stride : (i / (KW ? KW : 1)) * b_tap_stride + (i % (KW ? KW : 1)) * 16u;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const unsigned ad = (mask[pt] >> i) & 1u ? b_addr[pt] + off : zero_addr;
      B[s][pt] = *reinterpret_cast<const half8_t*>(smem + ad);
    }
  };
  auto load = [&](int i, int s) {
    load_a(i, s);
    load_b(i, s);
  };
  load_a(0, 0);
  if (PRE) {
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) B[0][pt] = b_pre[pt];
  } else {
    load_b(0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (i + 1 < NT) load(i + 1, (i + 1) & 1);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        if (chain_tile<SKIP>(nb, pt)) {
          acc[nb][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[i & 1][nb], B[i & 1][pt], acc[nb][pt], 0, 0, 0);
        }
      }
    }
    if (i + 1 < NT) {
      // the next tap's NB + PT requests (and their address selects) ride in the issue slots
      // between this tap's MFMAs, one request per MFMA, instead of in a gap after them
#pragma unroll
      for (int k = 0; k < NB + PT; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);     // MFMA
        __builtin_amdgcn_sched_group_barrier(0x2, 2, 0);     // VALU
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

typedef float float4_t __attribute__((ext_vector_type(4)));

// shift + ReLU + fp16 of one 32-cout accumulator, lanes l / l+32 paired into standard C8 pieces:
// piece[t] = output channels cbase + 8 * (2t + hi) .. +7 of this lane's pixel (conv_common.h's
// epilogue arithmetic, so that values match the per-layer kernels bit for bit).  sh[q] = the
// shifts of couts cbase + 8q + 4hi .. +3, loaded by the caller (one 16-byte load per quad, all in
// flight together -- scalar loads here cost a round trip each: 7 k cycles per layer, measured).
__device__ __forceinline__ void chain_pieces(const float16_t& a, const float4_t (&sh)[4], uint4_t (&piece)[2]) {
  const half2_t zero2 = {static_cast<_Float16>(0.f), static_cast<_Float16>(0.f)};
  unsigned pk[4][2];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float2_t v0 = float2_t{a[4 * q], a[4 * q + 1]} + float2_t{sh[q][0], sh[q][1]};
    const float2_t v1 = float2_t{a[4 * q + 2], a[4 * q + 3]} + float2_t{sh[q][2], sh[q][3]};
    half2_t h0 = __builtin_convertvector(v0, half2_t), h1 = __builtin_convertvector(v1, half2_t);
    h0 = __builtin_elementwise_max(h0, zero2);
    h1 = __builtin_elementwise_max(h1, zero2);
    pk[q][0] = __builtin_bit_cast(unsigned, h0);
    pk[q][1] = __builtin_bit_cast(unsigned, h1);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const auto d0 = __builtin_amdgcn_permlane32_swap(pk[2 * t][0], pk[2 * t + 1][0], false, false);
    const auto d1 = __builtin_amdgcn_permlane32_swap(pk[2 * t][1], pk[2 * t + 1][1], false, false);
    piece[t] = uint4_t{d0[0], d1[0], d0[1], d1[1]};
  }
}

// Positions t of a `taps`-long filter axis that meet the map for a pixel at `pos` of `lim`:
// t + pos - pad in [0, lim).
__device__ __forceinline__ unsigned chain_axis_mask(int pos, int lim, int taps, int pad) {
  const int lo = max(0, pad - pos), hi = min(taps - 1, lim - 1 + pad - pos);
  return hi >= lo ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

// Taps (row-major kh x kw) of the filter that meet an h x w map for the pixel at (row, col).
__device__ __forceinline__ unsigned chain_tap_mask_hw(int h, int w, int kh, int kw, int row, int col, bool valid) {
  if (!valid) return 0u;
  const unsigned rows = chain_axis_mask(row, h, kh, (kh - 1) >> 1);
  const unsigned cols = chain_axis_mask(col, w, kw, (kw - 1) >> 1);
  unsigned m = 0;
  for (int ty = 0; ty < kh; ++ty) {
    if ((rows >> ty) & 1u) m |= cols << (ty * kw);
  }
  return m;
}

}  // namespace chaink
}  // namespace dv

#endif  // DV_CHAIN_COMMON_H_
