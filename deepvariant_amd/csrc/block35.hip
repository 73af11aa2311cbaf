// block35.hip -- one Inception-A block of the 35x35 stage (tf_keras InceptionV3 mixed0..mixed2,
// deepvariant/keras_modeling.py:268-274) as ONE persistent launch.
//
// Per-layer, a block is three launches: the grouped 1x1 heads (b1, 5x5 reducer, 3x3dbl reducer,
// pooled projection), the 5x5 48->64 (imgconv.hip) and the 3x3 64->96 -> 3x3 96->96 chain
// (chain.hip).  The heads are bandwidth-bound, and most of what they write -- the 48- and 64-
// channel reducer tensors -- is read straight back by the next two launches and never again.
// Here a workgroup owns a tile of ONE whole map (<= 256 pixels) and walks the whole block on it:
//   * phase 1, the four 1x1 heads in two K passes over the block input (5x5 reducer + 3x3
//     reducer, then b1 + pooled projection: 128 couts each, 8 accumulators per computing wave).
//     Each 16-channel chunk of the input (8 KB) and its weights (4 KB) arrive by LDS-DMA in a
//     ring of seven slots, six chunks ahead of the MFMAs.  The reducers go to LDS as fp16, b1
//     to the concat buffer; the raw float32 projection is staged in LDS and averaged there with
//     conv_epilogue_avg's arithmetic (avg_pool_group);
//   * phase 2, the 5x5 48->64 from the LDS-resident 5x5 reducer into the concat buffer.  A 5x5
//     weight slab of one chunk (51 KB) is split over two slots: filter rows 0-2, then rows 3-4;
//   * phase 3, 3x3 64->96 in place in LDS, then 3x3 96->96 into the concat buffer (chain.hip).
// The block input is read from HBM once per pass (the second pass mostly hits the caches) and
// its output is written once; no other tensor of the block reaches HBM.  As in chain.hip, waves
// 0-3 only compute and waves 4-7 only move data, and they meet at one s_barrier per chunk.  The
// next tile's first six input chunks are in flight while the last layer stores its output.
// K order (chunk major, tap minor), fp32 accumulation, the fp16 rounding of every intermediate,
// shift + ReLU and the pooling sums are those of the per-layer kernels: results are bit-identical
// to them (tests/test_hip_block35.py).
#include <cstdlib>

#include "block35.h"
#include "chain_common.h"

namespace dv {
namespace {

using namespace convk;
using namespace chaink;

constexpr int B35_THREADS = 512;
constexpr int TPX = kBlock35TilePx;
// LDS layout (bytes)
constexpr unsigned ACT_OFF = 0;                          // 3x3 branch activations: [group][256 px][8], <= 96 channels
constexpr unsigned R5_OFF = ACT_OFF + 12 * TPX * 16;     // 5x5 reducer: 6 groups
constexpr unsigned RING_OFF = R5_OFF + 6 * TPX * 16;     // DMA ring (phase 1 slots, or two big slots, or pool staging)
constexpr unsigned P1_ACT = 2 * TPX * 16;                // one input chunk of the tile: [k-group][256 px][8]
constexpr unsigned P1_W = 2 * 128 * 16;                  // its weights: [k-group][128 couts][8]
constexpr unsigned P1_SLOT = P1_ACT + P1_W;
constexpr int R1 = 7;                                    // phase 1 ring depth (DMAs run R1 - 1 chunks ahead)
constexpr int P1_PIECES = static_cast<int>(P1_SLOT / 1024);   // 1 KB DMA pieces per chunk: 3 per moving wave
constexpr unsigned W5_HALF0 = 15 * 2 * kBlock35Out5 * 16;     // 5x5 filter rows 0-2 (taps 0-14)
constexpr unsigned W5_HALF1 = 10 * 2 * kBlock35Out5 * 16;     // rows 3-4 (taps 15-24)
constexpr unsigned W5_CHUNK = W5_HALF0 + W5_HALF1;
constexpr unsigned W3_CHUNK = 9 * 2 * kBlock35Out3 * 16;
constexpr unsigned BIG_SLOT = W5_HALF0 > W3_CHUNK ? W5_HALF0 : W3_CHUNK;
constexpr unsigned STAGE_OFF = RING_OFF + BIG_SLOT;     // raw projection of one 32-cout subtile, float32 (beside big slot 0)
constexpr unsigned STAGE_BYTES = 4 * 2 * TPX * 16;
constexpr unsigned RING_BYTES = R1 * P1_SLOT;
constexpr unsigned ZERO_OFF = RING_OFF + RING_BYTES;
// every shift of the block, copied once per launch (float offsets; each branch padded to whole 32-cout subtiles)
constexpr unsigned SH_OFF = ZERO_OFF + 16;
constexpr int SH_RED5 = 0, SH_RED3 = 64, SH_B1 = 128, SH_POOL = 192, SH_5 = 256, SH_3A = 320, SH_3B = 416, SH_N = 512;
constexpr unsigned LDS_BYTES = SH_OFF + SH_N * 4;
constexpr int N5 = kBlock35Red5 / 16, N3A = kBlock35Red3 / 16, N3B = kBlock35Out3 / 16;   // K chunks of phases 2-3
constexpr int BIG_STEPS = 2 * N5 + N3A + N3B;            // weight slabs of phases 2-3 per tile
static_assert(P1_SLOT % 4096 == 0 && P1_PIECES == 12, "three 1 KB pieces per moving wave and chunk");
static_assert(2 * BIG_SLOT <= RING_BYTES && STAGE_OFF + STAGE_BYTES <= RING_OFF + RING_BYTES, "phase 2-3 slots / pool staging fit the ring");
static_assert(LDS_BYTES <= 160 * 1024, "the CU's LDS");

// s_waitcnt needs an immediate: at most n of this wave's DMAs may still fly (they land in issue order)
__device__ __forceinline__ void wait_dma_barrier(int n) {
  switch (n) {
    case 3: asm volatile("s_waitcnt vmcnt(3)\n\ts_barrier" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)\n\ts_barrier" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)\n\ts_barrier" ::: "memory"); break;
    case 15: asm volatile("s_waitcnt vmcnt(15)\n\ts_barrier" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); break;
  }
}

template <int NB>
__device__ __forceinline__ void zero_acc(float16_t (&acc)[NB][2]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][pt][i] = 0.f;
}

// the shifts of couts cbase + 8q + 4hi .. +3 (chain_pieces' operand) from the LDS copy
__device__ __forceinline__ void load_sh(const char* smem, int shift, int cbase, int hi, float4_t (&sh)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    sh[q] = *reinterpret_cast<const float4_t*>(smem + SH_OFF + (shift + cbase + 4 * hi + 8 * q) * 4);
  }
}

struct Lane {
  int px[2], row[2], col[2];
  bool val[2];
  unsigned act[2];   // (hi * 256 + px) * 16: this lane's piece of a [2 groups][256 px] chunk image
  int l31, hi;
};

// subtiles [nb0, nb0 + n) of acc (couts cbase0 + 32 * k) -> fp16 pieces into an LDS activation region
template <int NB>
__device__ __forceinline__ void store_lds(char* smem, unsigned region, const float16_t (&acc)[NB][2], int nb0, int n,
                                          int shift, int cout, const Lane& c) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (nb < nb0 || nb >= nb0 + n) continue;
    const int cbase = (nb - nb0) * 32;
    float4_t sh[4];
    load_sh(smem, shift, cbase, c.hi, sh);
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      uint4_t piece[2];
      chain_pieces(acc[nb][pt], sh, piece);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int group = cbase / 8 + 2 * t + c.hi;
        if (group * 8 < cout) {
          *reinterpret_cast<uint4_t*>(smem + region + static_cast<unsigned>(group * TPX + c.px[pt]) * 16u) = piece[t];
        }
      }
    }
  }
}

// subtiles [nb0, nb0 + n) of acc -> fp16 pieces into the concat buffer at channel group goff
template <int NB>
__device__ __forceinline__ void store_hbm(const Block35Args& p, const char* smem, const float16_t (&acc)[NB][2], int nb0,
                                          int n, int shift, int cout, int goff, int img, const Lane& c) {
  const unsigned gstride = static_cast<unsigned>(p.og.hp * p.og.wp);
  uint4_t* outp = reinterpret_cast<uint4_t*>(p.out);
  unsigned obase[2];
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    obase[pt] = static_cast<unsigned>(((img * p.og.groups + goff) * p.og.hp + c.row[pt] + p.og.halo) * p.og.wp +
                                      c.col[pt] + p.og.halo);
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (nb < nb0 || nb >= nb0 + n) continue;
    const int cbase = (nb - nb0) * 32;
    float4_t sh[4];
    load_sh(smem, shift, cbase, c.hi, sh);
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      uint4_t piece[2];
      chain_pieces(acc[nb][pt], sh, piece);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int group = cbase / 8 + 2 * t + c.hi;
        if (c.val[pt] && group * 8 < cout) outp[obase[pt] + static_cast<unsigned>(group) * gstride] = piece[t];
      }
    }
  }
}

// ------------------------------------------------------------------ computing waves (0-3)
// wave = pixel quarter: fragments 2 wave, 2 wave + 1 of the tile, every cout subtile of the layer.
template <int NP>
__device__ __forceinline__ void b35_compute(const Block35Args& p, char* smem, int wave, int lane) {
  constexpr int NBB = 2 + NP;   // pass 1: b1 (2 subtiles) + pooled projection (NP)
  Lane c;
  c.l31 = lane & 31;
  c.hi = lane >> 5;
  const int P = p.h * p.w;
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    const int px = (wave * 2 + pt) * 32 + c.l31;
    c.px[pt] = px;
    c.val[pt] = px < P;
    const int q = c.val[pt] ? px : 0;
    c.row[pt] = q / p.w;
    c.col[pt] = q - c.row[pt] * p.w;
    c.act[pt] = static_cast<unsigned>(c.hi * TPX + px) * 16u;
  }
  if (wave == 0 && lane < 4) *reinterpret_cast<unsigned*>(smem + ZERO_OFF + lane * 4) = 0u;
  // the shifts (as dv_model_apply_corrections left them) -> LDS, visible after the first barrier
  for (int j = wave * 64 + lane; j < SH_N; j += 256) {
    const float* src = j < SH_RED3 ? p.sh_red5 + (j - SH_RED5) : j < SH_B1 ? p.sh_red3 + (j - SH_RED3)
                     : j < SH_POOL ? p.sh_b1 + (j - SH_B1) : j < SH_5 ? p.sh_pool + (j - SH_POOL)
                     : j < SH_3A ? p.sh5 + (j - SH_5) : j < SH_3B ? p.sh3a + (j - SH_3A) : p.sh3b + (j - SH_3B);
    // every shift array is padded past its couts (model_graph.cpp dv_model::conv: cout + 128 floats)
    reinterpret_cast<float*>(smem + SH_OFF)[j] = *src;
  }
  const unsigned one[2] = {1u, 1u};
  const half8_t nopre[2] = {};
  const int K = p.n_chunks;
  const unsigned a_lane1 = static_cast<unsigned>((c.hi * 128 + c.l31) * 16);
  const unsigned a_lane5 = static_cast<unsigned>((c.hi * kBlock35Out5 + c.l31) * 16);
  const unsigned a_lane3 = static_cast<unsigned>((c.hi * kBlock35Out3 + c.l31) * 16);
  const unsigned row16 = static_cast<unsigned>(p.w * 16);
  const unsigned chunk_lds = static_cast<unsigned>(2 * TPX * 16);

  for (int img = blockIdx.x; img < p.N; img += gridDim.x) {
    // ---- phase 1, pass 0: 5x5 reducer (subtiles 0-1) + 3x3 reducer (2-3) ----------------------
    {
      float16_t acc[4][2];
      zero_acc(acc);
      for (int s = 0; s < K; ++s) {
        barrier_after_lds();   // B1(s): chunk s landed
        const unsigned slot = RING_OFF + static_cast<unsigned>(s % R1) * P1_SLOT;
        const unsigned b[2] = {slot + c.act[0], slot + c.act[1]};
        chain_step<4, 2, 1, 0, 0, false>(smem, slot + P1_ACT + a_lane1, 0u, b, 0u, one, ZERO_OFF, nopre, acc);
      }
      barrier_after_lds();     // E_A: (nothing reads the reducer regions any more)
      store_lds<4>(smem, R5_OFF, acc, 0, 2, SH_RED5, kBlock35Red5, c);
      store_lds<4>(smem, ACT_OFF, acc, 2, 2, SH_RED3, kBlock35Red3, c);
    }
    // ---- phase 1, pass 1: b1 (subtiles 0-1) + raw pooled projection ---------------------------
    {
      float16_t acc[NBB][2];
      zero_acc(acc);
      for (int s = K; s < 2 * K; ++s) {
        barrier_after_lds();
        const unsigned slot = RING_OFF + static_cast<unsigned>(s % R1) * P1_SLOT;
        const unsigned b[2] = {slot + c.act[0], slot + c.act[1]};
        chain_step<NBB, 2, 1, 0, 0, false>(smem, slot + P1_ACT + a_lane1, 0u, b, 0u, one, ZERO_OFF, nopre, acc);
      }
      barrier_after_lds();     // E_B: every wave is done reading the ring (the first 5x5 slab may come)
      store_hbm<NBB>(p, smem, acc, 0, 2, SH_B1, kBlock35B1, p.goff_b1, img, c);
      // the pooled projection, one 32-cout subtile at a time: raw float32 accumulators -> staging [group q][half hi]
      // [slot][4 floats] (conv_epilogue_avg's image), then thread = pixel slot averages the window (avg_pool_group)
      int my_slot = wave * 64 + lane;
      // (opaque per tile: its loop-invariant address arithmetic, hoisted out of the tile loop, spilled to scratch)
      asm volatile("" : "+v"(my_slot));
      const int py = my_slot / p.w, pxx = my_slot - py * p.w;
      const bool plive = my_slot < P;
      const float pinv = 1.0f / static_cast<float>(((py > 0) + (py < p.h - 1) + 1) * ((pxx > 0) + (pxx < p.w - 1) + 1));
      const unsigned gstride = static_cast<unsigned>(p.og.hp * p.og.wp);
      const unsigned obase = static_cast<unsigned>(((img * p.og.groups + p.goff_pool) * p.og.hp + py + p.og.halo) * p.og.wp +
                                                   pxx + p.og.halo);
      float4* tile = reinterpret_cast<float4*>(smem + STAGE_OFF);
#pragma unroll
      for (int k = 0; k < NP; ++k) {
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
          const float16_t a = acc[2 + k][pt];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            tile[(q * 2 + c.hi) * TPX + c.px[pt]] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
          }
        }
        barrier_after_lds();   // P1(k): the staging is complete
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int group = 4 * k + q;
          float o[8];
          avg_pool_group(tile + q * 2 * TPX, py, pxx, p.h, p.w, lane, pinv,
                         reinterpret_cast<const float*>(smem + SH_OFF) + SH_POOL + group * 8, o);
          half8_t hv;
#pragma unroll
          for (int j = 0; j < 8; ++j) hv[j] = static_cast<_Float16>(o[j]);
          if (plive) reinterpret_cast<uint4_t*>(p.out)[obase + static_cast<unsigned>(group) * gstride] = __builtin_bit_cast(uint4_t, hv);
        }
        barrier_after_lds();   // P2(k): the staging is free again
      }
    }
    // ---- phase 2: 5x5 48->64 from the 5x5 reducer; filter rows 0-2 and 3-4 in consecutive slots --
    int q = 0;
    {
      unsigned m5[2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        m5[pt] = chain_tap_mask_hw(p.h, p.w, 5, 5, c.row[pt], c.col[pt], c.val[pt]);
        asm volatile("" : "+v"(m5[pt]));   // (computed per tile, not kept live across it)
      }
      float16_t acc[2][2];
      zero_acc(acc);
      const unsigned first = static_cast<unsigned>(-(2 * p.w + 2) * 16);
      for (int cc = 0; cc < N5; ++cc, q += 2) {
        const unsigned b[2] = {R5_OFF + c.act[0] + first + cc * chunk_lds, R5_OFF + c.act[1] + first + cc * chunk_lds};
        barrier_after_lds();
        chain_step<2, 2, 15, 5, 0, false>(smem, RING_OFF + (q & 1) * BIG_SLOT + a_lane5, 2 * kBlock35Out5 * 16, b, row16,
                                          m5, ZERO_OFF, nopre, acc);
        const unsigned b2[2] = {b[0] + 3 * row16, b[1] + 3 * row16};
        const unsigned m5b[2] = {m5[0] >> 15, m5[1] >> 15};
        barrier_after_lds();
        chain_step<2, 2, 10, 5, 0, false>(smem, RING_OFF + ((q + 1) & 1) * BIG_SLOT + a_lane5, 2 * kBlock35Out5 * 16, b2,
                                          row16, m5b, ZERO_OFF, nopre, acc);
      }
      store_hbm<2>(p, smem, acc, 0, 2, SH_5, kBlock35Out5, p.goff_5, img, c);
    }
    // ---- phase 3: 3x3 64->96 in place, 3x3 96->96 into the concat buffer ------------------------
    const unsigned first3 = static_cast<unsigned>(-(p.w + 1) * 16);
    const unsigned b3[2] = {ACT_OFF + c.act[0] + first3, ACT_OFF + c.act[1] + first3};
    unsigned m3[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      m3[pt] = chain_tap_mask_hw(p.h, p.w, 3, 3, c.row[pt], c.col[pt], c.val[pt]);
      asm volatile("" : "+v"(m3[pt]));
    }
    {
      float16_t acc[3][2];
      zero_acc(acc);
      for (int cc = 0; cc < N3A; ++cc, ++q) {
        const unsigned b[2] = {b3[0] + cc * chunk_lds, b3[1] + cc * chunk_lds};
        barrier_after_lds();
        chain_step<3, 2, 9, 3, 0, false>(smem, RING_OFF + (q & 1) * BIG_SLOT + a_lane3, 2 * kBlock35Out3 * 16, b, row16,
                                         m3, ZERO_OFF, nopre, acc);
      }
      barrier_after_lds();     // E3a: every wave is done reading the 3x3 reducer
      store_lds<3>(smem, ACT_OFF, acc, 0, 3, SH_3A, kBlock35Out3, c);
    }
    {
      float16_t acc[3][2];
      zero_acc(acc);
      for (int cc = 0; cc < N3B; ++cc, ++q) {
        const unsigned b[2] = {b3[0] + cc * chunk_lds, b3[1] + cc * chunk_lds};
        barrier_after_lds();
        chain_step<3, 2, 9, 3, 0, false>(smem, RING_OFF + (q & 1) * BIG_SLOT + a_lane3, 2 * kBlock35Out3 * 16, b, row16,
                                         m3, ZERO_OFF, nopre, acc);
      }
      barrier_after_lds();     // E3b: every wave is done reading the slots (the next tile's input may come)
      store_hbm<3>(p, smem, acc, 0, 3, SH_3B, kBlock35Out3, p.goff_3, img, c);
    }
  }
}

// ------------------------------------------------------------------ moving waves (4-7)
template <int NP>
__device__ __forceinline__ void b35_move(const Block35Args& p, char* smem, int lw, int lane) {
  const int P = p.h * p.w;
  // this wave moves pixels lw * 64 .. + 63 of every input chunk: the lane's source offset relative to (the tile's
  // image, group 0)
  unsigned src;
  {
    const int px = lw * 64 + lane;
    const int q = px < P ? px : 0;
    const int row = q / p.w, col = q - row * p.w;
    src = static_cast<unsigned>(((row + p.ig.halo) * p.ig.wp + col + p.ig.halo) * 16);
  }
  const unsigned plane_bytes = static_cast<unsigned>(p.ig.hp * p.ig.wp * 16);
  const int K = p.n_chunks;
  // phase 1 chunk s of image img: pieces lw (k-group 0) and lw + 4 (k-group 1) of the input, 1 KB lw of the weights
  auto issue_p1 = [&](int img, int s) {
    const int pass = s >= K ? 1 : 0, cc = s - pass * K;
    const unsigned slot = RING_OFF + static_cast<unsigned>(s % R1) * P1_SLOT;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(uniform_ptr(reinterpret_cast<const char*>(p.in) + static_cast<size_t>(img) * p.in_img_bytes)), 0,
        0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(uniform_ptr(reinterpret_cast<const char*>(p.w1) + static_cast<size_t>(pass * K + cc) * P1_W)), 0,
        P1_W, 0x00020000);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(smem + slot + (g * TPX + lw * 64) * 16), 16, src,
                                               (2 * cc + g) * plane_bytes, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(smem + slot + P1_ACT + lw * 1024), 16, lane * 16, lw * 1024, 0, 0);
  };
  // weight slab q of phases 2-3 into big slot q & 1
  auto issue_big = [&](int q) {
    const char* base;
    unsigned bytes;
    if (q < 2 * N5) {
      base = reinterpret_cast<const char*>(p.w5) + static_cast<size_t>(q >> 1) * W5_CHUNK + (q & 1) * W5_HALF0;
      bytes = (q & 1) ? W5_HALF1 : W5_HALF0;
    } else if (q < 2 * N5 + N3A) {
      base = reinterpret_cast<const char*>(p.w3a) + static_cast<size_t>(q - 2 * N5) * W3_CHUNK;
      bytes = W3_CHUNK;
    } else {
      base = reinterpret_cast<const char*>(p.w3b) + static_cast<size_t>(q - 2 * N5 - N3A) * W3_CHUNK;
      bytes = W3_CHUNK;
    }
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(uniform_ptr(base)), 0, bytes, 0x00020000);
    const unsigned slot = RING_OFF + static_cast<unsigned>(q & 1) * BIG_SLOT;
    const int pieces = static_cast<int>(bytes >> 10);
    for (int j = lw; j < pieces; j += 4) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(smem + slot + j * 1024), 16, lane * 16, j * 1024, 0, 0);
    }
  };

  int img = blockIdx.x;
  if (img >= p.N) return;
  for (int s = 0; s < R1 - 1; ++s) issue_p1(img, s);
  for (; img < p.N; img += gridDim.x) {
    for (int s = 0; s < 2 * K; ++s) {
      wait_dma_barrier(3 * min(R1 - 2, 2 * K - 1 - s));   // B1(s)
      if (s + R1 - 1 < 2 * K) issue_p1(img, s + R1 - 1);
      if (s == K - 1) barrier_only();                     // E_A
    }
    barrier_only();   // E_B
    issue_big(0);     // big slot 0 lies below the pool staging
    for (int k = 0; k < 2 * NP; ++k) barrier_only();   // P1(k), P2(k)
    for (int q = 0; q < BIG_STEPS; ++q) {
      barrier_after_dma();                                // slab q landed
      if (q + 1 < BIG_STEPS) issue_big(q + 1);
      if (q == 2 * N5 + N3A - 1) barrier_only();          // E3a
    }
    barrier_only();   // E3b
    const int next = img + static_cast<int>(gridDim.x);
    if (next < p.N) {
      for (int s = 0; s < R1 - 1; ++s) issue_p1(next, s);
    }
  }
}

template <int NP>
__global__ __launch_bounds__(B35_THREADS, 1) void block35_kernel(Block35Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (static_cast<int>(blockIdx.x) >= p.N) return;
  if (wave < 4) {
    b35_compute<NP>(p, smem, wave, lane);
  } else {
    b35_move<NP>(p, smem, wave - 4, lane);
  }
}

template <int NP>
void launch_as(const Block35Args& a, int grid, hipStream_t stream) {
  static const bool attr = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(block35_kernel<NP>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL((block35_kernel<NP>), dim3(grid), dim3(B35_THREADS), LDS_BYTES, stream, a);
}

}  // namespace

size_t block35_lds_bytes() { return LDS_BYTES; }

void launch_block35(const Block35Args& a, int blocks, hipStream_t stream) {
  int grid = a.N < blocks ? a.N : blocks;
  if (grid < 1) grid = 1;
  if (a.pool_c > 32) {
    launch_as<2>(a, grid, stream);
  } else {
    launch_as<1>(a, grid, stream);
  }
}

}  // namespace dv
