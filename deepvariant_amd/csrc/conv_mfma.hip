// conv_mfma.hip -- the MFMA implicit-GEMM convolution kernels of the classifier (interface: conv_mfma.h; launch
// arguments, C8 layout and epilogues: conv_common.h).
//
// Kernels (HISTORY.md 4.2 has the measurements behind each choice)
//   conv_mfma_kernel<NB,PT>   implicit-GEMM conv + shift + ReLU on v_mfma_f32_32x32x16_f16:
//                             D[cout][pixel] = sum_k W[cout][k] X[k][pixel]; a wave owns
//                             PT*32 pixels x NB*32 couts; weights stream through LDS in
//                             slabs of 8 K-chunks, pixel fragments go global -> VGPR;
//                             sibling 1x1 heads share one launch over their concatenated
//                             couts
//   conv_resident_kernel<NB,PT>      the same with the whole cout tile's weights resident in LDS (persistent blocks)
//   conv_pool_resident_kernel<NB>    resident weights, output max-pooled (3x3/2) before it is stored
//   conv_pool1x1_kernel<NB>   1x1 conv whose input is max-pooled (3x3/2) on the fly
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "conv_mfma.h"

using namespace dv::convk;

namespace {

// Pixel-operand prefetch depth, in chunks, per tile shape.  Measured on MI355X: 8 or 16
// instead of 4 changes nothing (+-1 %) for thin, mid or big tiles -- the queue is not what
// the waves wait for (HISTORY.md 7) -- so every shape uses 4.
constexpr int prefetch_depth(int /*nb*/, int /*pt*/) { return 4; }

// Wave-uniform walk over the K chunks kept in SGPRs and advanced with selects
// only -- no memory, no branches.  K order is channel-chunk major, filter tap
// minor: the KH*KW taps of one 16-channel chunk are consecutive, so a block
// re-reads the same two channel-group planes (a few KB incl. halo) KH*KW times
// back to back and the vector L1 serves all but the first pass.
// off = byte offset of (group 2*cc, kh, kw) relative to (group 0, ih0, iw0).
struct ChunkWalk {
  int kh, kw;
  unsigned tap_off;    // (kh*wp + kw) * 16
  unsigned chunk_off;  // cc * chunk_stride
  __device__ __forceinline__ unsigned off() const { return chunk_off + tap_off; }
  __device__ __forceinline__ void advance(const ConvArgs& p) {
    const bool row_end = ++kw == p.KW;
    kw = row_end ? 0 : kw;
    tap_off += row_end ? static_cast<unsigned>((p.ig.wp - p.KW + 1) * 16) : 16u;
    kh += row_end ? 1 : 0;
    const bool taps_end = kh == p.KH;
    kh = taps_end ? 0 : kh;
    tap_off = taps_end ? 0u : tap_off;
    chunk_off += taps_end ? p.chunk_stride : 0u;
  }
};

// One weight slab of R (<= 8) K-chunks: straight-line code, no branches, so the
// compiler's s_waitcnt insertion keeps the kPrefetch-deep load pipeline intact.
// Pixel fragments: voffset = per-lane base (VGPR, fixed for the whole kernel),
// soffset = chunk offset (SGPR): ZERO vector ALU work per load.  Chunks past the
// end of K simply read the next bytes of the (larger) input tensor or hit the
// descriptor's range check; their values are never used.
// SPLIT (ConvArgs::split): weight chunks come in (hi, lo) pairs -- W = W_hi + W_lo, both fp16 --
// that multiply the SAME pixel fragment: chunk j of the slab uses pixel slot (S0 + j) / 2 and
// the slot is refilled after the lo half.  The products are exact and the accumulator is fp32,
// so the layer sees 22-bit weights for one extra MFMA and one extra ds_read per fragment.
// State of the side max-pool (ConvArgs::side_pool_out) of one wave: the running maximum of the
// current 16-channel chunk's window pieces and where the finished ones go.
template <int PT>
struct SidePool {
  half8_t best[PT];
  int tap, cc;          // position in the K walk (wave-uniform): tap of the chunk, channel chunk
  int cc_mod;           // cc % n_tiles: the cout tiles of a pixel block load the same fragments and share
  int n_tiles, my_tile; // the pool's chunks round robin (tile t stores the chunks with cc % n_tiles == t)
  int taps, n_cc;
  unsigned at[PT];      // piece index of (n, group side_pool_goff + hi, oh, ow) in the pooled tensor
  bool ok[PT];
  unsigned gstride2;    // two channel groups (one chunk) further
  uint4_t* out;
};

template <int NB, int PT, int R, int S0 = 0, bool SPLIT = false, bool POOL = false>
__device__ __forceinline__ void conv_slab(const ConvArgs& p, const __amdgpu_buffer_rsrc_t rsrc,
                                          const _Float16* wslab, ChunkWalk& walk,
                                          const unsigned (&base)[PT],
                                          uint4_t (&xf)[prefetch_depth(NB, PT)][PT],
                                          float16_t (&acc)[NB][PT], SidePool<PT>* sp = nullptr) {
  constexpr int BN = NB * 32;
  constexpr int kPrefetch = prefetch_depth(NB, PT);
  // Weight fragments are double buffered in registers: the ds_reads of chunk
  // j+1 are issued before the MFMAs of chunk j, whose 32*NB*PT cycles cover the
  // LDS latency.
  half8_t wf[2][NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    wf[0][nb] = *reinterpret_cast<const half8_t*>(wslab + (nb * 32) * 8);
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    // DV_ABLATE_* (tools/ablate_conv.sh): timing ablations, results are WRONG by construction --
    // _W reuses the first chunk's weight fragments, _X never refills the pixel fragments,
    // _LOOP skips the K loop, _EPI (conv_common.h) suppresses the output stores.
#ifndef DV_ABLATE_W
    if (j + 1 < R) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        wf[(j + 1) & 1][nb] = *reinterpret_cast<const half8_t*>(
            wslab + (j + 1) * BN * kChunk + (nb * 32) * 8);
      }
    }
#else
    if (j + 1 < R) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wf[(j + 1) & 1][nb] = wf[j & 1][nb];
    }
#endif
    __builtin_amdgcn_sched_barrier(0);
    constexpr int kDiv = SPLIT ? 2 : 1;
    const int slot = ((S0 + j) / kDiv) % kPrefetch;
    half8_t xh[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) xh[pt] = __builtin_bit_cast(half8_t, xf[slot][pt]);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        acc[nb][pt] =
            __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j & 1][nb], xh[pt], acc[nb][pt], 0, 0, 0);
      }
    }
    if constexpr (POOL) {
      // this step's fragments ARE window pieces of the sibling max-pool (K order: channel chunk
      // major, tap minor); exact, so the result equals the separate max-pool kernel's bit for bit.
      // The cout tiles of a pixel block see the same fragments: tile t keeps the chunks with
      // cc % n_tiles == t (wave-uniform), the running maximum restarts from the lowest fp16 number.
      if (sp->cc_mod == sp->my_tile) {
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) sp->best[pt] = __builtin_elementwise_max(sp->best[pt], xh[pt]);
      }
      if (sp->tap == sp->taps - 1) {   // wave-uniform
        if (sp->cc < sp->n_cc && sp->cc_mod == sp->my_tile) {
          const _Float16 lowest = static_cast<_Float16>(-65504.f);
#pragma unroll
          for (int pt = 0; pt < PT; ++pt) {
            if (sp->ok[pt]) sp->out[sp->at[pt]] = __builtin_bit_cast(uint4_t, sp->best[pt]);
            sp->best[pt] = half8_t{lowest, lowest, lowest, lowest, lowest, lowest, lowest, lowest};
          }
        }
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) sp->at[pt] += sp->gstride2;
        sp->tap = 0;
        ++sp->cc;
        sp->cc_mod = sp->cc_mod + 1 == sp->n_tiles ? 0 : sp->cc_mod + 1;
      } else {
        ++sp->tap;
      }
    }
    // refill the slot just consumed with chunk (current + kPrefetch)
    if (!SPLIT || ((S0 + j) & 1)) {
#ifndef DV_ABLATE_X
      const unsigned soff = walk.off();
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        xf[slot][pt] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, base[pt], soff, 0);
      }
#endif
      walk.advance(p);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// conv_slab for a WIDE input (ConvArgs::wide_in): R K-chunks, each multiplied against the hi and then the lo pixel
// fragment with the same weight fragments.  The prefetch ring of four fragments holds two chunks' (hi, lo) pairs; the
// fragment consumed is replaced by the same part of the chunk two further on.  R is even (slabs of 8 or 4 chunks), so the
// ring position is 0 at every call.
template <int NB, int PT, int R>
__device__ __forceinline__ void conv_slab_wide(const ConvArgs& p, const __amdgpu_buffer_rsrc_t rsrc,
                                               const _Float16* wslab, ChunkWalk& walk, const unsigned (&base)[PT],
                                               uint4_t (&xf)[prefetch_depth(NB, PT)][PT], float16_t (&acc)[NB][PT]) {
  constexpr int BN = NB * 32;
  static_assert(prefetch_depth(NB, PT) == 4 && R % 2 == 0, "two (hi, lo) pairs in flight");
  half8_t wf[2][NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) wf[0][nb] = *reinterpret_cast<const half8_t*>(wslab + (nb * 32) * 8);
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (j + 1 < R) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        wf[(j + 1) & 1][nb] = *reinterpret_cast<const half8_t*>(wslab + (j + 1) * BN * kChunk + (nb * 32) * 8);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int part = 0; part < 2; ++part) {
      const int slot = (2 * j + part) & 3;
      half8_t xh[PT];
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) xh[pt] = __builtin_bit_cast(half8_t, xf[slot][pt]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          acc[nb][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j & 1][nb], xh[pt], acc[nb][pt], 0, 0, 0);
        }
      }
      const unsigned soff = walk.off() + (part ? p.lo_off : 0u);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) xf[slot][pt] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, base[pt], soff, 0);
      if (part) walk.advance(p);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Blank-row skipping (ConvArgs::blank_row): the wave's PT*32 pixels x NB*32 couts copied from the
// all-blank image's response instead of computed.  Lanes l / l+32 take alternate 8-cout
// groups; all loads are issued before the first store.
template <int NB, int PT>
__device__ __forceinline__ void copy_blank_wave(const ConvArgs& p, int n_tile, const int (&pn)[PT],
                                                const int (&poh)[PT], const int (&pow_)[PT],
                                                const bool (&mvalid)[PT], int lane) {
  const ConvBranch& b = p.br[0];
  const unsigned gstride = static_cast<unsigned>(b.og.hp * b.og.wp);
  const int hi = lane >> 5;
  const uint4_t* src = reinterpret_cast<const uint4_t*>(p.blank_src);
  uint4_t* dst = reinterpret_cast<uint4_t*>(b.out);
  uint4_t v[PT][NB * 2];
  unsigned at[PT][NB * 2];
  bool ok[PT][NB * 2];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const unsigned rel = static_cast<unsigned>((poh[pt] + b.og.halo) * b.og.wp + pow_[pt] + b.og.halo);
#pragma unroll
    for (int j = 0; j < NB * 2; ++j) {
      const int g = n_tile * NB * 4 + 2 * j + hi;
      ok[pt][j] = mvalid[pt] && g * 8 < b.Cout;
      at[pt][j] = static_cast<unsigned>(b.out_goff + g) * gstride + rel;
      v[pt][j] = ok[pt][j] ? src[at[pt][j]] : uint4_t{0u, 0u, 0u, 0u};
    }
  }
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const unsigned img = static_cast<unsigned>(pn[pt] * b.og.groups) * gstride;
#pragma unroll
    for (int j = 0; j < NB * 2; ++j) {
      if (ok[pt][j]) dst[img + at[pt][j]] = v[pt][j];
    }
  }
}

// Implicit-GEMM convolution, D[cout][pixel] = sum_k W[cout][k] * X[k][pixel].
//
//  * The block's weight tile (NB*32 couts) streams through LDS in slabs of 8
//    K-chunks (128 K values), double buffered: ONE barrier per 8*NB*PT MFMAs.
//  * The pixel operand never touches LDS: an MFMA B fragment is 8 consecutive
//    channels of one pixel = one 16-byte piece of the C8 layout, loaded
//    kPrefetch chunks ahead straight into VGPRs; 32 consecutive pixels are one
//    contiguous 512-byte run.
//  * Each wave owns PT*32 pixels x all NB*32 couts of the tile: NB*PT
//    independent 32x32 accumulators keep the matrix pipe busy back to back.
//  * Epilogue: shift + ReLU, lanes l / l+32 pair their halves into 16-byte
//    pieces, stored as contiguous 512-byte runs (no LDS).
template <int NB, int PT, int MINB = (NB * PT >= 8 ? 1 : 2), int SLAB = kSlabChunks, int WAVES = 4,
          bool SPLIT = false, bool SIDE_POOL = false, bool AVG = false, bool WIDE = false>
__global__ __launch_bounds__(WAVES * 64, MINB) void conv_mfma_kernel(ConvArgs p) {
  constexpr int BN = NB * 32;
  constexpr int kThreads = WAVES * 64;   // (WAVES = 8: tuning experiment DV_CONV_W8, HISTORY.md 7)
  constexpr int SLAB_HALFS = SLAB * BN * kChunk;
  constexpr int SLAB_PIECES = SLAB_HALFS / 8;            // 16-byte pieces
  constexpr int W_PER_THREAD = SLAB_PIECES / kThreads;   // = 2 * NB with four waves
  static_assert(SLAB_PIECES % kThreads == 0, "slab does not split evenly over the block");
  constexpr int kPrefetch = prefetch_depth(NB, PT);
  extern __shared__ __attribute__((aligned(16))) _Float16 smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // 1-D grid.  Blocks are dispatched round-robin over the 8 XCDs (block b ->
  // XCD b % 8); remap so that logically consecutive blocks -- the cout tiles of
  // the same pixel tile, which re-read the same input -- share an XCD's L2.
  const int nwg = gridDim.x;
  const int xq = nwg >> 3, xr = nwg & 7;
  const int xcd = blockIdx.x & 7;
  int xi = blockIdx.x >> 3;
  if (p.cu_pair) {
    // An XCD hands its blocks to its 32 CUs in turn: block xi runs on CU xi % 32, and with two
    // blocks per CU the ones 32 apart share a CU.  Give those two consecutive logical numbers.
    const int cnt = xcd < xr ? xq + 1 : xq;
    if (xi < cnt / 64 * 64) {
      const int w = xi & 63;
      xi = (xi & ~63) + (w & 31) * 2 + (w >> 5);
    }
  }
  const int logical = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + xi;
  const int n_tile = logical % p.n_tiles;
  int pix_block = logical / p.n_tiles;
  int band_r = 0;  // row-band mode: the output row of every pixel of this block
  if (p.band) {
    band_r = pix_block % p.band;   // rows minor: the H blocks reading the same images are neighbours
    pix_block /= p.band;
  }
  const int m_block = pix_block * (32 * PT * WAVES);

  // Buffer offsets are 32 bit, tensors are not (8 K examples x 1.4 MB): every wave
  // addresses the input relative to the first example it touches (n0), through its
  // own descriptor -- a wave's 64 pixels never span more than a few hundred KB.
  int n0 = 0;
  unsigned base[PT];   // byte offset of (n - n0, group lane>>5, ih0, iw0) in the input
  int pn[PT], poh[PT], pow_[PT];  // output coordinates, turned into addresses per branch
  bool mvalid[PT];
  const int ohow = p.OH * p.OW;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int m = m_block + (wave * PT + pt) * 32 + (lane & 31);
    int n, pix, oh, ow, iy;
    if constexpr (AVG) {   // image-aligned tiles (ConvArgs::tile_g): slot -> (map of the block, pixel of the map)
      int il;
      divmod_small((wave * PT + pt) * 32 + (lane & 31), p.tile_p, p.rcp_tile_p, il, pix);
      n = pix_block * p.tile_g + il;
      mvalid[pt] = il < p.tile_g && n < p.N;
      n = min(n, p.N - 1);
      divmod_small(pix, p.OW, p.rcp_ow, oh, ow);
      iy = oh * p.stride - p.pad_h + p.ig.halo;
    } else if (p.band) {  // m runs over (example, column) of row band_r; taps start at map row 0
      mvalid[pt] = m < p.N * p.OW;
      divmod_small(mvalid[pt] ? m : 0, p.OW, p.rcp_ow, n, ow);
      oh = band_r;
      iy = p.ig.halo;
    } else {
      mvalid[pt] = m < p.M;
      divmod_small(mvalid[pt] ? m : 0, ohow, p.rcp_ohow, n, pix);
      divmod_small(pix, p.OW, p.rcp_ow, oh, ow);
      iy = oh * p.stride - p.pad_h + p.ig.halo;
    }
    const int ix = ow * p.stride - p.pad_w + p.ig.halo;
    if (pt == 0) n0 = __builtin_amdgcn_readfirstlane(n);  // lane 0 holds the wave's first pixel
    base[pt] = mvalid[pt]
                   ? static_cast<unsigned>(((((n - n0) * p.ig.groups + (lane >> 5)) * p.ig.hp + iy) *
                                                p.ig.wp + ix) * 16)
                   : 0x80000000u;  // beyond the descriptor's range: reads as zero
    pn[pt] = n;
    poh[pt] = oh;
    pow_[pt] = ow;
  }

  // Blank-row skipping (opt-in): a pixel range that lies in ONE example, from a row at or past
  // that example's first blank-determined row, is copied instead of computed.  Decided for the
  // whole block (no slab traffic, no barriers) and per wave (the wave keeps its share of the
  // weight-slab copies and the barriers, but issues no pixel loads and no MFMAs).
  bool wave_blank = false;
  if (p.blank_row != nullptr) {
    auto range_blank = [&](int m_lo, int m_hi) -> bool {  // pixels [m_lo, m_hi), uniform arguments
      m_hi = min(m_hi, p.M);
      if (m_lo >= m_hi) return false;
      int nf, pf, nl, pl, ohf, owf;
      divmod_small(m_lo, ohow, p.rcp_ohow, nf, pf);
      divmod_small(m_hi - 1, ohow, p.rcp_ohow, nl, pl);
      divmod_small(pf, p.OW, p.rcp_ow, ohf, owf);
      return nf == nl && ohf >= p.blank_row[nf];
    };
    if (range_blank(m_block, m_block + 32 * PT * WAVES)) {   // block-uniform, before any barrier
      bool wanted = true;   // rows nobody reads are not even copied (ConvArgs::blank_need)
      if (p.blank_need != nullptr) {
        int nf, pf, ohf, owf;
        divmod_small(m_block, ohow, p.rcp_ohow, nf, pf);
        divmod_small(pf, p.OW, p.rcp_ow, ohf, owf);
        wanted = ohf < p.blank_need[nf];
      }
      if (wanted) copy_blank_wave<NB, PT>(p, n_tile, pn, poh, pow_, mvalid, lane);
      return;
    }
    const int m_wave = m_block + wave * (32 * PT);
    wave_blank = __builtin_amdgcn_readfirstlane(range_blank(m_wave, m_wave + 32 * PT) ? 1 : 0) != 0;
  }

  const size_t in_off = static_cast<size_t>(n0) * p.img_bytes;
  const size_t in_left = p.in_bytes - in_off;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.in) + in_off), 0,
      static_cast<unsigned>(in_left < 0x7fffffffu ? in_left : 0x7fffffffu), 0x00020000);

  // ---- weight slabs: global -> registers -> LDS ---------------------------
  const uint4* wsrc = reinterpret_cast<const uint4*>(p.w) +
                      static_cast<size_t>(band_r * p.n_tiles + n_tile) * p.n_slabs * (kSlabChunks * BN * 2);
  uint4_t wreg[W_PER_THREAD];
#define DV_LOAD_SLAB(s_)                                                                   \
  {                                                                                        \
    const uint4_t* src_ = reinterpret_cast<const uint4_t*>(wsrc) +                         \
                          static_cast<size_t>(s_) * SLAB_PIECES + tid;                     \
    _Pragma("unroll") for (int j_ = 0; j_ < W_PER_THREAD; ++j_) wreg[j_] =                \
        src_[j_ * kThreads];                                                           \
  }
#define DV_STORE_SLAB(buf_)                                                                \
  {                                                                                        \
    uint4_t* dst_ = reinterpret_cast<uint4_t*>(smem + (buf_) * SLAB_HALFS) + tid;          \
    _Pragma("unroll") for (int j_ = 0; j_ < W_PER_THREAD; ++j_) dst_[j_ * kThreads] = \
        wreg[j_];                                                                          \
  }

  uint4_t xf[kPrefetch][PT];
  float16_t acc[NB][PT];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][pt][i] = 0.f;

  ChunkWalk walk{0, 0, 0u, 0u};
  DV_LOAD_SLAB(0)
#pragma unroll
  for (int d = 0; d < kPrefetch; ++d) {  // chunks 0 .. kPrefetch-1 (wide input: the (hi, lo) pairs of chunks 0 and 1)
    const unsigned soff = walk.off() + (WIDE && (d & 1) ? p.lo_off : 0u);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      xf[d][pt] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, base[pt], soff, 0);
    }
    if (!WIDE || (d & 1)) walk.advance(p);
  }
  DV_STORE_SLAB(0)
  __syncthreads();

  // LDS image of a chunk: [k-group g = lane>>5][cout][8 halfs] -> each half-wave
  // reads 512 contiguous bytes: conflict-free for ds_read_b128 (a [cout][16]
  // image is 2-way conflicted: measured SQ_LDS_BANK_CONFLICT ~ LDS active).
  const int frag_off = (lane >> 5) * (BN * 8) + (lane & 31) * 8;  // halfs
  if (wave_blank) {   // wave-uniform: same slab copies and barriers as the computing waves
    const int n_full_b = p.n_chunks / SLAB;
    for (int s = 0; s < n_full_b; ++s) {
      const int next = s + 1 < (p.n_chunks + SLAB - 1) / SLAB ? s + 1 : s;
      DV_LOAD_SLAB(next)
      DV_STORE_SLAB((s + 1) & 1)
      __syncthreads();
    }
    copy_blank_wave<NB, PT>(p, n_tile, pn, poh, pow_, mvalid, lane);
    return;
  }
  // The K loop of one cout tile over `n_chunks` weight chunks, with (S = true) or without the
  // (hi, lo) pairing of split weights.  A split launch may mix both kinds of tile: the leading
  // ConvArgs::split_tiles cout tiles carry W_hi + W_lo (2 K chunks), the others plain weights
  // (K chunks, the first half of their slot in the packed image) -- block-uniform choice.
  SidePool<PT> side;
  auto k_loop = [&](auto split_tag, auto pool_tag, const int n_chunks) {
    constexpr bool S = decltype(split_tag)::value;
    constexpr bool P = decltype(pool_tag)::value;
    SidePool<PT>* const sp = P ? &side : nullptr;
    const int tile_slabs = (n_chunks + SLAB - 1) / SLAB;
#ifdef DV_ABLATE_LOOP
    const int n_full = n_chunks < 0 ? 1 : 0;
    const int rem = 0;
#else
    const int n_full = n_chunks / SLAB;
    const int rem = n_chunks - n_full * SLAB;
#endif
    for (int s = 0; s < n_full; ++s) {
      // The next slab's global loads are UNCONDITIONAL (the last trip re-reads its own slab
      // into the idle buffer): behind an `if` the compiler has to assume at the first
      // pixel-fragment wait that they were not issued and emits vmcnt(7) -- which, when they
      // were, drains the whole four-chunk prefetch queue at every slab start.
      const int next = s + 1 < tile_slabs ? s + 1 : s;
      DV_LOAD_SLAB(next)
      if constexpr (WIDE) {
        conv_slab_wide<NB, PT, SLAB>(p, rsrc, smem + (s & 1) * SLAB_HALFS + frag_off, walk, base, xf, acc);
      } else {
        conv_slab<NB, PT, SLAB, 0, S, P>(p, rsrc, smem + (s & 1) * SLAB_HALFS + frag_off, walk, base, xf, acc, sp);
      }
      DV_STORE_SLAB((s + 1) & 1)
      __syncthreads();
    }
    // Tail slab (n_chunks % 8 chunks), in straight-line groups of 4: K is padded
    // to a multiple of 4 chunks with zero weights (the slab image is zero there),
    // so no chunk count ever needs a branch or a register rotation inside the
    // load pipeline.  (A rolled one-chunk loop had to rotate the prefetch slots and
    // drained vmcnt(0) every chunk; per-count unrolled variants behind a switch
    // made the register allocator clone the accumulators.)
    if (rem) {
      const _Float16* wslab = smem + (n_full & 1) * SLAB_HALFS + frag_off;
      if constexpr (WIDE) {
        conv_slab_wide<NB, PT, 4>(p, rsrc, wslab, walk, base, xf, acc);
        if constexpr (SLAB > 4) {
          if (rem > 4) conv_slab_wide<NB, PT, 4>(p, rsrc, wslab + 4 * BN * kChunk, walk, base, xf, acc);
        }
      } else {
      conv_slab<NB, PT, 4, 0, S, P>(p, rsrc, wslab, walk, base, xf, acc, sp);
      if constexpr (SLAB > 4) {
        if (rem > 4) conv_slab<NB, PT, 4, 4, S, P>(p, rsrc, wslab + 4 * BN * kChunk, walk, base, xf, acc, sp);
      }
      }
    }
  };
  if constexpr (SPLIT) {
    if (n_tile < p.split_tiles) {
      k_loop(std::true_type{}, std::false_type{}, p.n_chunks);
    } else {
      k_loop(std::false_type{}, std::false_type{}, p.n_chunks >> 1);
    }
  } else if constexpr (SIDE_POOL) {   // the reduction block's 3x3 / 2 with its sibling max-pool on the side
    side.tap = 0;
    side.cc = 0;
    side.cc_mod = 0;
    side.n_tiles = p.n_tiles;
    side.my_tile = n_tile;
    side.taps = p.KH * p.KW;
    side.n_cc = p.Cin / kChunk;
    side.gstride2 = 2u * static_cast<unsigned>(p.side_pool_og.hp * p.side_pool_og.wp);
    side.out = reinterpret_cast<uint4_t*>(p.side_pool_out);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const _Float16 lowest = static_cast<_Float16>(-65504.f);
      side.best[pt] = half8_t{lowest, lowest, lowest, lowest, lowest, lowest, lowest, lowest};
      side.ok[pt] = mvalid[pt];
      side.at[pt] = static_cast<unsigned>(
          ((pn[pt] * p.side_pool_og.groups + p.side_pool_goff + (lane >> 5)) * p.side_pool_og.hp + poh[pt] +
           p.side_pool_og.halo) * p.side_pool_og.wp + pow_[pt] + p.side_pool_og.halo);
    }
    k_loop(std::false_type{}, std::true_type{}, p.n_chunks);
  } else {
    k_loop(std::false_type{}, std::false_type{}, p.n_chunks);
  }
#undef DV_LOAD_SLAB
#undef DV_STORE_SLAB

  if constexpr (AVG) {
    conv_epilogue_avg<NB, PT>(acc, p, n_tile, pix_block, pn, poh, pow_, mvalid, lane, wave, smem);
  } else {
    conv_epilogue<NB, PT>(acc, p, n_tile, pn, poh, pow_, mvalid, lane);
  }
}

// Resident-weight variant of conv_mfma_kernel for layers whose whole cout tile fits the CU's LDS
// (K * NB*32 halfs <= ~150 KB: the 3x3 80->192, short-K 1x1 heads).  HISTORY.md 7: halving a
// launch's MFMA work and pixel traffic moved it by 10 %, so what a block of the streaming
// kernel waits for is its weight slabs (global -> registers -> LDS behind a barrier per slab,
// 138 KB per 256-pixel block on the 3x3 80->192).  Here a PERSISTENT block of eight waves
// copies its cout tile's packed weights into LDS once; after that there is no barrier and no
// weight traffic at all: every wave walks its own sequence of PT*32-pixel tiles with the same
// straight-line slab code (conv_slab), the same K order and the same epilogue, so results are
// bit-identical to conv_mfma_kernel's.  Blocks b and b + 8 (same XCD, same L2) take the
// cout tiles of the same pixels.
template <int NB, int PT>
__global__ __launch_bounds__(512, 1) void conv_resident_kernel(ConvArgs p) {
  constexpr int BN = NB * 32;
  constexpr int WAVES = 8, kThreads = WAVES * 64;
  constexpr int SLAB_HALFS = kSlabChunks * BN * kChunk;
  constexpr int kPrefetch = prefetch_depth(NB, PT);
  extern __shared__ __attribute__((aligned(16))) _Float16 smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x;
  const int n_tile = (blk >> 3) % p.n_tiles;
  const int seq = (blk & 7) + 8 * ((blk >> 3) / p.n_tiles);
  const int n_seq = 8 * ((static_cast<int>(gridDim.x) >> 3) / p.n_tiles);
  {  // the cout tile's weights: [slab][chunk][2 k-groups][cout][8], contiguous in the packed image
    const uint4_t* wsrc = reinterpret_cast<const uint4_t*>(p.w) +
                          static_cast<size_t>(n_tile) * p.n_slabs * (kSlabChunks * BN * 2);
    uint4_t* wdst = reinterpret_cast<uint4_t*>(smem);
    const int pieces = p.n_slabs * (kSlabChunks * BN * 2);
    for (int i = tid; i < pieces; i += kThreads) wdst[i] = wsrc[i];
  }
  __syncthreads();
  const int frag_off = (lane >> 5) * (BN * 8) + (lane & 31) * 8;  // halfs
  const int ohow = p.OH * p.OW;
  const int n_full = p.n_chunks / kSlabChunks;
  const int rem = p.n_chunks - n_full * kSlabChunks;
  const int n_wave_tiles = (p.M + 32 * PT - 1) / (32 * PT);
  for (int wt = seq * WAVES + wave; wt < n_wave_tiles; wt += n_seq * WAVES) {
    int n0 = 0;
    unsigned base[PT];
    int pn[PT], poh[PT], pow_[PT];
    bool mvalid[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int m = (wt * PT + pt) * 32 + (lane & 31);
      int n, pix, oh, ow;
      mvalid[pt] = m < p.M;
      divmod_small(mvalid[pt] ? m : 0, ohow, p.rcp_ohow, n, pix);
      divmod_small(pix, p.OW, p.rcp_ow, oh, ow);
      const int iy = oh * p.stride - p.pad_h + p.ig.halo;
      const int ix = ow * p.stride - p.pad_w + p.ig.halo;
      if (pt == 0) n0 = __builtin_amdgcn_readfirstlane(n);
      base[pt] = mvalid[pt]
                     ? static_cast<unsigned>(((((n - n0) * p.ig.groups + (lane >> 5)) * p.ig.hp + iy) *
                                                  p.ig.wp + ix) * 16)
                     : 0x80000000u;
      pn[pt] = n;
      poh[pt] = oh;
      pow_[pt] = ow;
    }
    const size_t in_off = static_cast<size_t>(n0) * p.img_bytes;
    const size_t in_left = p.in_bytes - in_off;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.in) + in_off), 0,
        static_cast<unsigned>(in_left < 0x7fffffffu ? in_left : 0x7fffffffu), 0x00020000);
    uint4_t xf[kPrefetch][PT];
    float16_t acc[NB][PT];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[nb][pt][i] = 0.f;
    ChunkWalk walk{0, 0, 0u, 0u};
#pragma unroll
    for (int d = 0; d < kPrefetch; ++d) {
      const unsigned soff = walk.off();
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        xf[d][pt] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, base[pt], soff, 0);
      }
      walk.advance(p);
    }
    for (int s = 0; s < n_full; ++s) {
      conv_slab<NB, PT, kSlabChunks>(p, rsrc, smem + s * SLAB_HALFS + frag_off, walk, base, xf, acc);
    }
    if (rem) {
      const _Float16* wslab = smem + n_full * SLAB_HALFS + frag_off;
      conv_slab<NB, PT, 4>(p, rsrc, wslab, walk, base, xf, acc);
      if (rem > 4) conv_slab<NB, PT, 4, 4>(p, rsrc, wslab + 4 * BN * kChunk, walk, base, xf, acc);
    }
    conv_epilogue<NB, PT>(acc, p, n_tile, pn, poh, pow_, mvalid, lane);
  }
}

// conv_resident_kernel with the 3x3 / stride-2 max-pool that follows the convolution taken INSIDE
// (stem: 3x3 80->192 -> max-pool -> mixed0).  The conv tensor (21 x 51 x 192 per example, 0.4 MB
// written and read back: the worst launch of round 3 was the pooled re-read) never exists; only
// the pooled tensor (10 x 25 x 192) is stored, and mixed0's heads become an ordinary grouped 1x1.
//
// Max-pooling commutes with every monotone map, so pooling the fp16 results of shift + ReLU is the
// same as Keras' order -- results are bit-identical to the separate max-pool.
//
//  * A wave owns 32 POSITIONS of the flattened (example, conv column) index -- fragment f covers
//    positions 30 f .. 30 f + 31, an overlap of two so that every 3-wide window that starts in
//    the first 30 lies inside the wave (6 % of the MFMA work is recomputed) -- and walks DOWN the
//    map two conv rows per step (the two pixel fragments of conv_slab<NB,2>: same K order, same
//    weights resident in LDS, same straight-line slab code as conv_resident_kernel).
//  * Vertical maximum: rows 2i, 2i+1, 2i+2 of one position sit in the same lane of three
//    accumulator sets, so it is register-wise (v_pk_max_f16); max(row 2i+2, row 2i+3) is carried
//    into the next step as 8 packed dwords per 32-cout subtile.
//  * Horizontal maximum: positions +1 / +2 are lanes +1 / +2 of the same register
//    (ds_bpermute_b32, no LDS memory); lanes on even columns then hold pooled pixels and store
//    16-byte pieces after the usual permlane32_swap pairing.
//  * The last step has one conv row only (row 2 PH) and runs conv_slab<NB,1>.
template <int NB, int PT>
__device__ __forceinline__ void resident_rows(const ConvArgs& p, const __amdgpu_buffer_rsrc_t rsrc,
                                              const _Float16* wfrag, const unsigned (&base)[PT],
                                              float16_t (&acc)[NB][PT]) {
  constexpr int BN = NB * 32;
  constexpr int SLAB_HALFS = kSlabChunks * BN * kChunk;
  constexpr int kPrefetch = prefetch_depth(NB, PT);
  const int n_full = p.n_chunks / kSlabChunks;
  const int rem = p.n_chunks - n_full * kSlabChunks;
  uint4_t xf[kPrefetch][PT];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][pt][i] = 0.f;
  ChunkWalk walk{0, 0, 0u, 0u};
#pragma unroll
  for (int d = 0; d < kPrefetch; ++d) {
    const unsigned soff = walk.off();
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) xf[d][pt] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, base[pt], soff, 0);
    walk.advance(p);
  }
  for (int s = 0; s < n_full; ++s) {
    conv_slab<NB, PT, kSlabChunks>(p, rsrc, wfrag + s * SLAB_HALFS, walk, base, xf, acc);
  }
  if (rem) {
    const _Float16* wslab = wfrag + n_full * SLAB_HALFS;
    conv_slab<NB, PT, 4>(p, rsrc, wslab, walk, base, xf, acc);
    if (rem > 4) conv_slab<NB, PT, 4, 4>(p, rsrc, wslab + 4 * BN * kChunk, walk, base, xf, acc);
  }
}

// shift + ReLU + fp16 of one conv row held in accumulators: pk[nb][q][hq] = couts
// nb*32 + 8q + 4*(lane>>5) + 2hq + {0,1} of the lane's position (conv_epilogue's packing)
template <int NB>
__device__ __forceinline__ void pack_row(const float16_t (&acc)[NB], const ConvArgs& p, int n_tile, int hi,
                                         unsigned (&pk)[NB][4][2]) {
  const ConvBranch& b = p.br[0];
  const half2_t zero2 = {static_cast<_Float16>(0.f), static_cast<_Float16>(0.f)};
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int cbase = (n_tile * NB + nb) * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      typedef float f4_t __attribute__((ext_vector_type(4)));
      typedef const f4_t __attribute__((address_space(4))) * const_f4_ptr;
      const_f4_ptr sp = (const_f4_ptr)(reinterpret_cast<uintptr_t>(b.shift + (cbase + 8 * q)));
      const f4_t l4 = sp[0], u4 = sp[1];   // the shift array is padded past Cout
      const float2_t s0 = hi ? float2_t{u4[0], u4[1]} : float2_t{l4[0], l4[1]};
      const float2_t s1 = hi ? float2_t{u4[2], u4[3]} : float2_t{l4[2], l4[3]};
      const float2_t v0 = float2_t{acc[nb][4 * q], acc[nb][4 * q + 1]} + s0;
      const float2_t v1 = float2_t{acc[nb][4 * q + 2], acc[nb][4 * q + 3]} + s1;
      pk[nb][q][0] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_convertvector(v0, half2_t), zero2));
      pk[nb][q][1] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_convertvector(v1, half2_t), zero2));
    }
  }
}

__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(half2_t, a),
                                                                __builtin_bit_cast(half2_t, b)));
}

template <int NB>
__global__ __launch_bounds__(512, 1) void conv_pool_resident_kernel(ConvArgs p) {
  constexpr int BN = NB * 32;
  constexpr int WAVES = 8, kThreads = WAVES * 64;
  constexpr int kNew = 30;   // positions a fragment owns (the last two belong to the next one)
  extern __shared__ __attribute__((aligned(16))) _Float16 smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x;
  const int n_tile = (blk >> 3) % p.n_tiles;
  const int seq = (blk & 7) + 8 * ((blk >> 3) / p.n_tiles);
  const int n_seq = 8 * ((static_cast<int>(gridDim.x) >> 3) / p.n_tiles);
  {
    const uint4_t* wsrc = reinterpret_cast<const uint4_t*>(p.w) +
                          static_cast<size_t>(n_tile) * p.n_slabs * (kSlabChunks * BN * 2);
    uint4_t* wdst = reinterpret_cast<uint4_t*>(smem);
    const int pieces = p.n_slabs * (kSlabChunks * BN * 2);
    for (int i = tid; i < pieces; i += kThreads) wdst[i] = wsrc[i];
  }
  __syncthreads();
  const _Float16* wfrag = smem + (lane >> 5) * (BN * 8) + (lane & 31) * 8;
  const ConvBranch& b = p.br[0];
  const int PH = b.og.h, PW = b.og.w;          // pooled map
  const int n_pos = p.N * p.OW;
  const int n_frag = (n_pos + kNew - 1) / kNew;
  const unsigned row_b = static_cast<unsigned>(p.ig.wp) * 16u;
  const int hi = lane >> 5, l32 = lane & 31;
  const unsigned gstride = static_cast<unsigned>(b.og.hp * b.og.wp);
  uint4_t* outp = reinterpret_cast<uint4_t*>(b.out);
  for (int f = seq * WAVES + wave; f < n_frag; f += n_seq * WAVES) {
    const int pos = f * kNew + l32;
    const bool valid = pos < n_pos;
    int n, col;
    divmod_small(valid ? pos : 0, p.OW, p.rcp_ow, n, col);
    const int n0 = __builtin_amdgcn_readfirstlane(n);
    // (example n - n0, channel group lane>>5, input row halo, input column col + halo): 'valid' conv
    const unsigned base0 =
        valid ? static_cast<unsigned>(((((n - n0) * p.ig.groups + hi) * p.ig.hp + p.ig.halo) * p.ig.wp + col +
                                       p.ig.halo) * 16)
              : 0x80000000u;
    const size_t in_off = static_cast<size_t>(n0) * p.img_bytes;
    const size_t in_left = p.in_bytes - in_off;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.in) + in_off), 0,
        static_cast<unsigned>(in_left < 0x7fffffffu ? in_left : 0x7fffffffu), 0x00020000);
    // pooled pixel (n, s - 1, col / 2) leaves from this lane at step s
    const bool emits = valid && l32 < kNew && (col & 1) == 0 && (col >> 1) < PW;
    const unsigned obase0 = static_cast<unsigned>(
        ((n * b.og.groups + b.out_goff) * b.og.hp + b.og.halo) * b.og.wp + (col >> 1) + b.og.halo);
    const int nb_addr1 = ((lane + 1) & 63) * 4, nb_addr2 = ((lane + 2) & 63) * 4;
    unsigned carry[NB][4][2];   // max(row 2s, row 2s+1) of the previous step
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int q = 0; q < 4; ++q) carry[nb][q][0] = carry[nb][q][1] = 0u;
    // Blank-row skipping (ConvArgs::blank_row = first blank-determined POOLED row per example): the wave walks
    // down only as far as the deepest pile-up among its (at most two) examples reaches -- pooled rows
    // 0 .. s_end - 1 -- and copies the rows below from the all-blank image's response (the values the walk would
    // produce there, bit for bit).  A lane whose own example turns blank earlier computes its blank rows: same bits.
    int s_end = PH;
    if (p.blank_row != nullptr) {
      int mine = valid ? min(p.blank_row[n], PH) : 0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mine = max(mine, __shfl_xor(mine, off));
      s_end = __builtin_amdgcn_readfirstlane(mine);
    }
    for (int s = 0; s <= s_end; ++s) {
      if (s_end == 0) break;      // every pooled row of this fragment is blank-determined
      unsigned top[NB][4][2];   // conv row 2s
      if (s < s_end) {
        unsigned base[2] = {base0, base0};
        if (valid) {
          base[0] = base0 + static_cast<unsigned>(2 * s) * row_b;
          base[1] = base[0] + row_b;
        }
        float16_t acc[NB][2];
        resident_rows<NB, 2>(p, rsrc, wfrag, base, acc);
        float16_t r0[NB], r1[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          r0[nb] = acc[nb][0];
          r1[nb] = acc[nb][1];
        }
        unsigned bot[NB][4][2];
        pack_row<NB>(r0, p, n_tile, hi, top);
        pack_row<NB>(r1, p, n_tile, hi, bot);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int hq = 0; hq < 2; ++hq) {
              const unsigned t = top[nb][q][hq];
              top[nb][q][hq] = pk_max(carry[nb][q][hq], t);   // rows 2s-2, 2s-1, 2s (s = 0: row 0 alone, unused)
              carry[nb][q][hq] = pk_max(t, bot[nb][q][hq]);
            }
      } else {   // the last pooled row's third conv row
        unsigned base[1] = {valid ? base0 + static_cast<unsigned>(2 * s) * row_b : base0};
        float16_t acc[NB][1];
        resident_rows<NB, 1>(p, rsrc, wfrag, base, acc);
        float16_t r0[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) r0[nb] = acc[nb][0];
        pack_row<NB>(r0, p, n_tile, hi, top);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int hq = 0; hq < 2; ++hq) top[nb][q][hq] = pk_max(carry[nb][q][hq], top[nb][q][hq]);
      }
      if (s == 0) continue;   // wave-uniform
      const unsigned obase = obase0 + static_cast<unsigned>(s - 1) * static_cast<unsigned>(b.og.wp);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int cbase = (n_tile * NB + nb) * 32;
        unsigned hm[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int hq = 0; hq < 2; ++hq) {
            const unsigned v = top[nb][q][hq];
            const unsigned v1 = static_cast<unsigned>(__builtin_amdgcn_ds_bpermute(nb_addr1, static_cast<int>(v)));
            const unsigned v2 = static_cast<unsigned>(__builtin_amdgcn_ds_bpermute(nb_addr2, static_cast<int>(v)));
            hm[q][hq] = pk_max(pk_max(v, v1), v2);
          }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const auto d0 = __builtin_amdgcn_permlane32_swap(hm[2 * t][0], hm[2 * t + 1][0], false, false);
          const auto d1 = __builtin_amdgcn_permlane32_swap(hm[2 * t][1], hm[2 * t + 1][1], false, false);
          const uint4_t piece = {d0[0], d1[0], d0[1], d1[1]};
          const int group = cbase / 8 + 2 * t + hi;
          if (emits && group * 8 < b.Cout) outp[obase + static_cast<unsigned>(group) * gstride] = piece;
        }
      }
    }
    if (s_end < PH && emits) {   // the blank-determined pooled rows of this lane's column: copied
      const uint4_t* src = reinterpret_cast<const uint4_t*>(p.blank_src);
      const unsigned rel0 = static_cast<unsigned>(b.og.halo * b.og.wp + (col >> 1) + b.og.halo);
      const unsigned img = static_cast<unsigned>(n * b.og.groups) * gstride;
      for (int pr = s_end; pr < PH; ++pr) {
        const unsigned rel = rel0 + static_cast<unsigned>(pr * b.og.wp);
#pragma unroll
        for (int j = 0; j < NB * 2; ++j) {   // lanes l / l + 32 take alternate 8-cout groups of this tile
          const int group = n_tile * NB * 4 + 2 * j + hi;
          if (group * 8 < b.Cout) {
            const unsigned at = static_cast<unsigned>(b.out_goff + group) * gstride + rel;
            outp[img + at] = src[at];
          }
        }
      }
    }
  }
}

// MaxPooling2D(3, strides 2) fused into the 1x1 convolution that consumes it (stem:
// maxpool -> 64->80): the pooled tensor (0.16 MB / example written and read back) never
// exists.  A pixel fragment is the element-wise maximum of the nine 16-byte pieces of its
// window, taken in registers (v_pk_max_f16) -- exact, so results are bit-identical to the
// separate max-pool kernel.  K is short (Cin/16 chunks): the whole weight tile sits in LDS,
// fragments of chunk c+1 are in flight while chunk c multiplies.  One 32-pixel fragment
// per wave (PT = 1) keeps the 2 x 9 outstanding loads within the register budget.
template <int NB, int WAVES = 4>
__global__ __launch_bounds__(WAVES * 64, WAVES == 4 ? 2 : 1) void conv_pool1x1_kernel(ConvArgs p) {
  constexpr int BN = NB * 32;
  constexpr int PT = 1;
  constexpr int kThreads = WAVES * 64;
  extern __shared__ __attribute__((aligned(16))) _Float16 smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int nwg = gridDim.x;
  const int xq = nwg >> 3, xr = nwg & 7;
  const int xcd = blockIdx.x & 7, xi = blockIdx.x >> 3;
  const int logical = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + xi;
  const int n_tile = logical % p.n_tiles;
  const int m_block = (logical / p.n_tiles) * (WAVES * 32);

  {  // whole weight tile -> LDS
    const int pieces = p.n_slabs * kSlabChunks * BN * 2;
    const uint4_t* src = reinterpret_cast<const uint4_t*>(p.w) + static_cast<size_t>(n_tile) * pieces;
    uint4_t* dst = reinterpret_cast<uint4_t*>(smem);
    for (int i = tid; i < pieces; i += kThreads) dst[i] = src[i];
  }
  int pn[PT], poh[PT], pow_[PT];
  bool mvalid[PT];
  const int m = m_block + wave * 32 + (lane & 31);
  mvalid[0] = m < p.M;
  int n, pix, oh, ow;
  divmod_small(mvalid[0] ? m : 0, p.OH * p.OW, p.rcp_ohow, n, pix);
  divmod_small(pix, p.OW, p.rcp_ow, oh, ow);
  pn[0] = n;
  poh[0] = oh;
  pow_[0] = ow;
  const int n0 = __builtin_amdgcn_readfirstlane(n);
  // window origin: pooled pixel (oh, ow) covers input rows 2oh..2oh+2, cols 2ow..2ow+2
  const unsigned base =
      mvalid[0] ? static_cast<unsigned>(((((n - n0) * p.ig.groups + (lane >> 5)) * p.ig.hp + 2 * oh +
                                          p.ig.halo) * p.ig.wp + 2 * ow + p.ig.halo) * 16)
                : 0x80000000u;
  const size_t in_off = static_cast<size_t>(n0) * p.img_bytes;
  const size_t in_left = p.in_bytes - in_off;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.in) + in_off), 0,
      static_cast<unsigned>(in_left < 0x7fffffffu ? in_left : 0x7fffffffu), 0x00020000);
  const unsigned row_b = static_cast<unsigned>(p.ig.wp) * 16u;

  float16_t acc[NB][PT];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][0][i] = 0.f;

  half8_t win[2][9];
#define DV_LOAD_WINDOW(slot_, cc_)                                                          \
  {                                                                                         \
    const unsigned so_ = static_cast<unsigned>(cc_) * p.chunk_stride;                       \
    _Pragma("unroll") for (int t_ = 0; t_ < 9; ++t_) win[slot_][t_] = __builtin_bit_cast(  \
        half8_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc, base,                          \
                                                       so_ + (t_ / 3) * row_b + (t_ % 3) * 16, 0)); \
  }
  DV_LOAD_WINDOW(0, 0)
  __syncthreads();
  const _Float16* wfrag = smem + (lane >> 5) * (BN * 8) + (lane & 31) * 8;
  for (int cc = 0; cc < p.n_chunks; cc += 2) {   // two chunks per trip: static window slots
    if (cc + 1 < p.n_chunks) DV_LOAD_WINDOW(1, cc + 1)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (half == 1) {
        if (cc + 1 >= p.n_chunks) break;
        if (cc + 2 < p.n_chunks) DV_LOAD_WINDOW(0, cc + 2)
      }
      half8_t x = win[half][0];
#pragma unroll
      for (int t = 1; t < 9; ++t) x = __builtin_elementwise_max(x, win[half][t]);
      const _Float16* wc = wfrag + (cc + half) * (BN * kChunk);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const half8_t wf = *reinterpret_cast<const half8_t*>(wc + nb * 32 * 8);
        acc[nb][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, x, acc[nb][0], 0, 0, 0);
      }
    }
  }
#undef DV_LOAD_WINDOW
  conv_epilogue<NB, PT>(acc, p, n_tile, pn, poh, pow_, mvalid, lane);
}

template <int NB>
constexpr size_t conv_lds_bytes() {
  return static_cast<size_t>(2) * kSlabChunks * NB * 32 * kChunk * 2;
}

// 192-cout tiles (NB = 6), one pixel fragment per wave: the pixel operand -- the texture-
// addresser path that bounds the other shapes (HISTORY.md 7) -- is fetched once for all 192
// couts instead of once per 96-cout tile.  Weight slabs of 4 chunks keep two blocks per CU.
void launch_conv6(const ConvArgs& a, hipStream_t stream) {
  const long rows = a.band ? a.band : 1;
  const long row_px = a.band ? static_cast<long>(a.N) * a.OW : a.M;
  const long blocks = rows * ((row_px + 127) / 128) * a.n_tiles;
  constexpr size_t lds = static_cast<size_t>(2) * 4 * 192 * kChunk * 2;
  if (a.wide_in) {
    hipLaunchKernelGGL((conv_mfma_kernel<6, 1, 2, 4, 4, false, false, false, true>), dim3(static_cast<unsigned>(blocks)),
                       dim3(kConvThreads), lds, stream, a);
    return;
  }
  hipLaunchKernelGGL((conv_mfma_kernel<6, 1, 2, 4>), dim3(static_cast<unsigned>(blocks)), dim3(kConvThreads), lds,
                     stream, a);
}

template <int NB>
void launch_conv(const ConvArgs& a, hipStream_t stream) {
  const int n_tiles = a.n_tiles;
  // pixel blocks of `px` pixels: over all N*OH*OW pixels, or per output row in row-band mode
  const long rows = a.band ? a.band : 1;
  const long row_px = a.band ? static_cast<long>(a.N) * a.OW : a.M;
  auto blocks = [&](int px) { return rows * ((row_px + px - 1) / px) * n_tiles; };
  // Two pixel tiles per wave halve the LDS weight traffic per MFMA; fall back
  // to one when that would leave CUs without a block.
  const long blocks2 = blocks(256);
  if constexpr (NB == 4) {
    if (a.side_pool_out != nullptr) {   // its own instantiations: the side pool costs registers the other launches keep
      if (blocks2 >= 512) {
        hipLaunchKernelGGL((conv_mfma_kernel<NB, 2, 2, kSlabChunks, 4, false, true>), dim3(static_cast<unsigned>(blocks2)),
                           dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
      } else {
        hipLaunchKernelGGL((conv_mfma_kernel<NB, 1, 2, kSlabChunks, 4, false, true>), dim3(static_cast<unsigned>(blocks(128))),
                           dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
      }
      return;
    }
  }
  if (a.wide_in) {   // precise mode: hi + lo pixel fragments per K chunk (conv_slab_wide); the two usual tile shapes
    if constexpr (NB >= 2 && NB <= 4) {
      if constexpr (NB == 4) {
        if (a.tile_g > 0) {
          const long tiles = (static_cast<long>(a.N) + a.tile_g - 1) / a.tile_g * n_tiles;
          hipLaunchKernelGGL((conv_mfma_kernel<NB, 2, 2, kSlabChunks, 4, false, false, true, true>),
                             dim3(static_cast<unsigned>(tiles)), dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
          return;
        }
      }
      if (blocks2 >= 512) {
        hipLaunchKernelGGL((conv_mfma_kernel<NB, 2, 2, kSlabChunks, 4, false, false, false, true>),
                           dim3(static_cast<unsigned>(blocks2)), dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
      } else {
        hipLaunchKernelGGL((conv_mfma_kernel<NB, 1, 2, kSlabChunks, 4, false, false, false, true>),
                           dim3(static_cast<unsigned>(blocks(128))), dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
      }
      return;
    }
  }
  if constexpr (NB == 4) {
    if (a.tile_g > 0) {   // image-aligned 256-pixel tiles, pooled projection averaged in the epilogue
      const long tiles = (static_cast<long>(a.N) + a.tile_g - 1) / a.tile_g * n_tiles;
      hipLaunchKernelGGL((conv_mfma_kernel<NB, 2, 2, kSlabChunks, 4, false, false, true>),
                         dim3(static_cast<unsigned>(tiles)), dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
      return;
    }
  }
  if (a.split) {  // W_hi + W_lo images: the same two tile shapes, SPLIT slab code
    static const long pt2_min = getenv("DV_SPLIT_PT2_MIN") ? atol(getenv("DV_SPLIT_PT2_MIN")) : 256;  // split layers carry twice the weight bytes per pixel: two fragments per wave from 256 blocks up (1x3 / 3x1 / 3x3 of mixed9-10: -12...-15 %, tools/r4_run.sh ab:DV_SPLIT_PT2_MIN=256)
    if (blocks2 >= pt2_min) {
      hipLaunchKernelGGL((conv_mfma_kernel<NB, 2, 2, kSlabChunks, 4, true>), dim3(static_cast<unsigned>(blocks2)),
                         dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
    } else {
      hipLaunchKernelGGL((conv_mfma_kernel<NB, 1, 2, kSlabChunks, 4, true>), dim3(static_cast<unsigned>(blocks(128))),
                         dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
    }
    return;
  }
  // (Round 6, measured and removed: <4,4> -- 128 pixels x 128 couts per wave, 16 accumulators in AGPRs, one workgroup
  // per CU, half the weight-slab bytes per MFMA: 17x17 heads 455 -> 490 us, 524 -> 568; 35x35 heads 449 -> 528; the
  // step 465.6 -> 449.1 K candidates/s with the pools unfused on both sides.  profiles/r06_experiments.txt.)
  static const int force_pt = getenv("DV_CONV_PT") ? atoi(getenv("DV_CONV_PT")) : 0;  // tuning knob
  // Four pixel tiles per wave where the accumulators still leave two blocks per CU and
  // K is long enough to amortise the wider prologue: measured -6 % on the 32-cout stem
  // 3x3 and -7 % on the 5x5s; +11 % (slower) on <2,4> 3x3 and 1x1 layers.
  static const bool no_pt4 = getenv("DV_NO_PT4") != nullptr;  // tuning knob
  if constexpr (NB <= 2) {
    if (!no_pt4 && !force_pt && blocks2 >= 4096 && (NB == 1 || a.KH * a.KW >= 25)) {
      hipLaunchKernelGGL((conv_mfma_kernel<NB, 4>), dim3(static_cast<unsigned>(blocks(512))),
                         dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
      return;
    }
  }
  // tuning experiments (HISTORY.md 7): 4-chunk weight slabs; 8-wave blocks of 512 pixels
  static const bool slab4 = getenv("DV_CONV_SLAB4") != nullptr;
  static const bool w8 = getenv("DV_CONV_W8") != nullptr;
  if constexpr (NB >= 3 && NB <= 4) {
    if (slab4 && blocks2 >= 512) {
      hipLaunchKernelGGL((conv_mfma_kernel<NB, 2, 2, 4>), dim3(static_cast<unsigned>(blocks2)),
                         dim3(kConvThreads), static_cast<size_t>(2) * 4 * NB * 32 * kChunk * 2, stream, a);
      return;
    }
    if (w8 && blocks2 >= 1024) {
      hipLaunchKernelGGL((conv_mfma_kernel<NB, 2, 1, kSlabChunks, 8>), dim3(static_cast<unsigned>(blocks(512))),
                         dim3(512), conv_lds_bytes<NB>(), stream, a);
      return;
    }
  }
  if (force_pt ? force_pt == 2 : blocks2 >= 512) {
    if constexpr (NB == 4) {
      // <4,2> compiled for two blocks per CU (249 VGPRs, no spills) instead of one with
      // accumulators in AGPRs (284): a second wave per SIMD covers the other's waits --
      // measured -12...-26 % on every nb4 layer (DV_CONV42_BLOCKS=1 restores one block).
      static const bool two = getenv("DV_CONV42_BLOCKS") == nullptr || atoi(getenv("DV_CONV42_BLOCKS")) != 1;
      if (two) {
        hipLaunchKernelGGL((conv_mfma_kernel<NB, 2, 2>), dim3(static_cast<unsigned>(blocks2)),
                           dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
        return;
      }
    }
    hipLaunchKernelGGL((conv_mfma_kernel<NB, 2>), dim3(static_cast<unsigned>(blocks2)),
                       dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
  } else {
    hipLaunchKernelGGL((conv_mfma_kernel<NB, 1>), dim3(static_cast<unsigned>(blocks(128))),
                       dim3(kConvThreads), conv_lds_bytes<NB>(), stream, a);
  }
}

}  // namespace
namespace dv {
namespace convk {

// (The order of the functions below fixes the order in which the compiler instantiates the kernels, and that reaches
// the operand order of a few instructions: profiles/model_split_kernels.txt.  Keep it when the per-kernel hashes of
// tools/kasm.sh --hash are to be compared across a change.)

// One opt-in to 160 KB of dynamic LDS per kernel and process.
template <typename K>
static void allow_big_lds(K kernel) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

void launch_conv_pool_resident(const ConvArgs& a, int n_cus, hipStream_t stream) {
  static const bool attr = (allow_big_lds(conv_pool_resident_kernel<3>), true);
  (void)attr;
  // one wave per fragment of 30 new positions of the (example, conv column) index; a persistent
  // grid of up to one block per CU, in whole sets of 8 blocks per cout tile
  const long frags = (static_cast<long>(a.N) * a.OW + 29) / 30;
  const int per_set = 8 * a.n_tiles;
  const long want = (frags + 8 * 8 - 1) / (8 * 8) * per_set;   // 8 waves x 8 blocks cover 64 fragments per set
  const int grid = static_cast<int>(std::max<long>(per_set, std::min<long>(want, n_cus / per_set * per_set)));
  hipLaunchKernelGGL((conv_pool_resident_kernel<3>), dim3(grid), dim3(512), resident_lds_bytes(a), stream, a);
}

void launch_conv_pool1x1(const ConvArgs& a, int nb, hipStream_t stream) {
  const size_t lds = static_cast<size_t>(a.n_slabs) * kSlabChunks * nb * 32 * kChunk * 2;
  const dim3 grid(static_cast<unsigned>(((a.M + 127) / 128) * a.n_tiles));
  switch (nb) {
    case 7: {  // mixed0's heads: all 7 subtiles in one tile, every window pooled once
      static const bool attr = (allow_big_lds(conv_pool1x1_kernel<7, 8>), true);
      (void)attr;
      hipLaunchKernelGGL((conv_pool1x1_kernel<7, 8>), dim3(static_cast<unsigned>((a.M + 255) / 256)), dim3(512), lds, stream, a);
      break;
    }
    case 1: hipLaunchKernelGGL((conv_pool1x1_kernel<1>), grid, dim3(kConvThreads), lds, stream, a); break;
    case 2: hipLaunchKernelGGL((conv_pool1x1_kernel<2>), grid, dim3(kConvThreads), lds, stream, a); break;
    case 3: hipLaunchKernelGGL((conv_pool1x1_kernel<3>), grid, dim3(kConvThreads), lds, stream, a); break;
    default: hipLaunchKernelGGL((conv_pool1x1_kernel<4>), grid, dim3(kConvThreads), lds, stream, a); break;
  }
}

void launch_conv_resident(const ConvArgs& a, int n_cus, hipStream_t stream) {
  static const bool attr = (allow_big_lds(conv_resident_kernel<3, 2>), true);
  (void)attr;
  const int grid = n_cus / (8 * a.n_tiles) * (8 * a.n_tiles);
  hipLaunchKernelGGL((conv_resident_kernel<3, 2>), dim3(grid), dim3(512), resident_lds_bytes(a), stream, a);
}

void launch_conv(const ConvArgs& a, int nb, hipStream_t stream) {
  switch (nb) {
    case 1: ::launch_conv<1>(a, stream); break;
    case 2: ::launch_conv<2>(a, stream); break;
    case 3: ::launch_conv<3>(a, stream); break;
    case 6: launch_conv6(a, stream); break;
    default: ::launch_conv<4>(a, stream); break;
  }
}

}  // namespace convk
}  // namespace dv
