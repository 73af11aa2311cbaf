// mixed3.hip -- the double-3x3 branch of the reduction block mixed3 (tf_keras InceptionV3: 1x1 288->64, 3x3
// 64->96 'same', 3x3 96->96 stride 2 'valid') as ONE persistent launch.
//
// Per layer the branch is three launches: a 1x1 that reads the whole block input to do very little
// arithmetic, a 3x3 (imgconv.hip) and a tiny stride-2 GEMM (conv_mfma.hip); the 64- and 96-channel tensors
// between them are written and read straight back, and never again.  Here a workgroup owns a tile of ONE whole
// input map (<= 256 pixels) and walks the three layers on it, as block35.hip does for an Inception-A block:
//   * phase 1, the 1x1 Cin->64.  Each 16-channel chunk of the input (8 KB) and its weights (2 KB) arrive by
//     LDS-DMA in a ring of R1 slots, R1 - 1 chunks ahead of the MFMAs; the result goes to LDS as fp16;
//   * phase 2, the 3x3 64->96 in place in LDS (block35.hip's phase 3, first layer), one 27 KB weight slab per
//     chunk in two alternating slots;
//   * phase 3, the 3x3 / 2 96->96 from the resident tile into the concat buffer: output pixel (r, c) reads LDS
//     pixel (2r + kr, 2c + kc) -- a per-lane base plus the tap offsets of a stride-1 3x3, no masks and no halo.
//     Its 4 x 12 output is two MFMA fragments: waves 0-1 take cout subtiles 0-1 of one fragment each, waves
//     2-3 subtile 2.
// Only phase 1 touches HBM.  Waves 0-3 compute, waves 4-7 move data; they meet at one s_barrier per chunk.
// The ring overlays the two weight slots (eleven slots; the slots past them are free during phases 2-3), and
// during those phases movers 2-3 do nothing but fetch the NEXT tile's first chunks into the free slots, one chunk
// per step, while movers 0-1 bring the weight slabs: each wave's DMAs land in issue order, so the two streams
// must not share a wave if the slabs are not to wait for HBM.  (-DDV_MIXED3_SEPARATE_RING: a five-slot ring
// beside the weight slots instead, the arrangement this one was measured against -- DESIGN.md 7.)
// K order (chunk major, tap minor), one 32x32x16 MFMA per chunk and tap, fp32 accumulation, shift + ReLU and
// the fp16 rounding of both intermediates are those of the per-layer kernels: results are bit-identical to them
// (tests/test_hip_mixed3.py).
#include "mixed3.h"
#include "chain_common.h"

namespace dv {
namespace {

using namespace convk;
using namespace chaink;

constexpr int M3_THREADS = 512;
constexpr int TPX = kMixed3TilePx;
constexpr int CMID = kMixed3Mid;
static_assert(kMixed3Red == 64 && kMixed3Mid == 96 && kMixed3Out == 96, "the wave split below is written for 64 -> 96 -> 96");
// LDS layout (bytes)
constexpr unsigned ACT_OFF = 0;                          // activations: [group][256 px][8], <= 96 channels
constexpr unsigned BIG_OFF = ACT_OFF + 12 * TPX * 16;    // two 3x3 weight slabs of one chunk each
constexpr unsigned BIG_SLOT = 9 * 2 * CMID * 16;
constexpr unsigned P1_ACT = 2 * TPX * 16;                // one input chunk of the tile: [k-group][256 px][8]
constexpr unsigned P1_W = 2 * kMixed3Red * 16;           // its weights: [k-group][64 couts][8]
constexpr unsigned P1_SLOT = P1_ACT + P1_W;
#ifdef DV_MIXED3_SEPARATE_RING
constexpr unsigned RING_OFF = BIG_OFF + 2 * BIG_SLOT;
constexpr int R1 = 5;                                    // phase 1 ring depth (DMAs run R1 - 1 chunks ahead)
constexpr int OV = 0;                                    // leading ring slots that the weight slabs overlay
#else
constexpr unsigned RING_OFF = BIG_OFF;
constexpr int R1 = 11;
constexpr int OV = static_cast<int>((2 * BIG_SLOT + P1_SLOT - 1) / P1_SLOT);
#endif
// chunk s of a tile sits in slot (s + OV) % R1: the tile's first NE chunks land in slots that phases 2-3 leave alone
constexpr int NE = R1 - OV < R1 - 1 ? R1 - OV : R1 - 1;
constexpr unsigned ZERO_OFF = RING_OFF + R1 * P1_SLOT;
// every shift of the branch, copied once per launch (float offsets)
constexpr unsigned SH_OFF = ZERO_OFF + 16;
constexpr int SH_1 = 0, SH_3A = 64, SH_3B = 160, SH_N = 256;
constexpr unsigned LDS_BYTES = SH_OFF + SH_N * 4;
constexpr int N3A = kMixed3Red / 16, N3B = kMixed3Mid / 16;   // K chunks of phases 2 and 3
constexpr int BIG_STEPS = N3A + N3B;
// DMAs per chunk and moving wave: a chunk is eight 1 KB input pieces and two 1 KB weight pieces.  Chunks fetched
// during phase 1 are spread over the four movers (movers 0-1: two input pieces + one weight piece, movers 2-3: two
// input pieces); a tile's first NE chunks are fetched by movers 2-3 alone (four input pieces + one weight piece each).
constexpr int DMA_EARLY = 5, DMA_LATE_W = 3, DMA_LATE = 2;
constexpr int MAX_WAIT = 30;
static_assert(OV * P1_SLOT >= (RING_OFF == BIG_OFF ? 2 * BIG_SLOT : 0u), "the early chunks' slots lie past the weight slots");
static_assert(NE >= 1 && (NE - 1) * DMA_EARLY + (R1 - 1 - NE) * DMA_LATE <= MAX_WAIT &&
                  (R1 - 1 - NE) * DMA_LATE_W <= MAX_WAIT, "wait_dma_barrier covers every count");
static_assert(NE <= BIG_STEPS, "one early chunk per step of phases 2-3");
static_assert(LDS_BYTES <= 160 * 1024, "the CU's LDS");

// s_waitcnt needs an immediate: at most n of this wave's DMAs may still fly (they land in issue order)
__device__ __forceinline__ void wait_dma_barrier(int n) {
#define DV_M3_WAIT(k) \
  case k: asm volatile("s_waitcnt vmcnt(" #k ")\n\ts_barrier" ::: "memory"); break;
  switch (n) {
    DV_M3_WAIT(1) DV_M3_WAIT(2) DV_M3_WAIT(3) DV_M3_WAIT(4) DV_M3_WAIT(5) DV_M3_WAIT(6) DV_M3_WAIT(7) DV_M3_WAIT(8)
    DV_M3_WAIT(9) DV_M3_WAIT(10) DV_M3_WAIT(11) DV_M3_WAIT(12) DV_M3_WAIT(13) DV_M3_WAIT(14) DV_M3_WAIT(15)
    DV_M3_WAIT(16) DV_M3_WAIT(17) DV_M3_WAIT(18) DV_M3_WAIT(19) DV_M3_WAIT(20) DV_M3_WAIT(21) DV_M3_WAIT(22)
    DV_M3_WAIT(23) DV_M3_WAIT(24) DV_M3_WAIT(25) DV_M3_WAIT(26) DV_M3_WAIT(27) DV_M3_WAIT(28) DV_M3_WAIT(29)
    DV_M3_WAIT(30)
    default: asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); break;
  }
#undef DV_M3_WAIT
}

// tuning aid (DV_MIXED3_PROF): shader-clock sums per computing wave -- per phase the wait at the chunk barriers, the MFMA
// steps, and the layer's closing barrier + epilogue
struct M3Prof {
  unsigned long long wait[3] = {0, 0, 0}, mfma[3] = {0, 0, 0}, epi[3] = {0, 0, 0};
};
__device__ __forceinline__ unsigned long long m3_clock() { return __builtin_amdgcn_s_memtime(); }
// adds the clocks since t0 to `sum` once the step's MFMAs (their last accumulator: `fence`) are issued; returns now
template <bool PROF>
__device__ __forceinline__ unsigned long long m3_lap(unsigned long long& sum, unsigned long long t0, float16_t& fence) {
  if (!PROF) return 0;
  asm volatile("" : "+v"(fence));
  const unsigned long long t = m3_clock();
  sum += t - t0;
  return t;
}

template <int NB, int PT>
__device__ __forceinline__ void zero_acc(float16_t (&acc)[NB][PT]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
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

// every 32-cout subtile of acc -> fp16 pieces into the LDS activation region
template <int NB>
__device__ __forceinline__ void store_lds(char* smem, const float16_t (&acc)[NB][2], int shift, const Lane& c) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    float4_t sh[4];
    load_sh(smem, shift, nb * 32, c.hi, sh);
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      uint4_t piece[2];
      chain_pieces(acc[nb][pt], sh, piece);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int group = nb * 4 + 2 * t + c.hi;
        *reinterpret_cast<uint4_t*>(smem + ACT_OFF + static_cast<unsigned>(group * TPX + c.px[pt]) * 16u) = piece[t];
      }
    }
  }
}

// phase 3 of one wave: NB cout subtiles from `sub0` of ONE output fragment, then its store into the concat buffer
template <int NB, bool PROF>
__device__ __forceinline__ void stride2_layer(const Mixed3Args& p, char* smem, int q, int sub0, unsigned a_lane3,
                                              unsigned b_base, unsigned row16, bool oval, unsigned obase, int hi,
                                              M3Prof& prof, unsigned long long t) {
  const half8_t nopre[1] = {};
  const unsigned mask[1] = {oval ? 0x1ffu : 0u};
  float16_t acc[NB][1];
  zero_acc(acc);
  for (int cc = 0; cc < N3B; ++cc, ++q) {
    const unsigned b[1] = {b_base + static_cast<unsigned>(cc) * (2 * TPX * 16)};
    barrier_after_lds();
    t = m3_lap<PROF>(prof.wait[2], t, acc[0][0]);
    chain_step<NB, 1, 9, 3, 0, false>(smem, BIG_OFF + (q & 1) * BIG_SLOT + a_lane3 + sub0 * 512, 2 * CMID * 16, b, row16,
                                      mask, ZERO_OFF, nopre, acc);
    t = m3_lap<PROF>(prof.mfma[2], t, acc[NB - 1][0]);
  }
  barrier_after_lds();     // E3: every wave is done reading the slots and the tile (the next tile's input may come)
  const unsigned gstride = static_cast<unsigned>(p.og.hp * p.og.wp);
  uint4_t* outp = reinterpret_cast<uint4_t*>(p.out);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int cbase = (sub0 + nb) * 32;
    float4_t sh[4];
    load_sh(smem, SH_3B, cbase, hi, sh);
    uint4_t piece[2];
    chain_pieces(acc[nb][0], sh, piece);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int group = cbase / 8 + 2 * k + hi;
      if (oval) outp[obase + static_cast<unsigned>(group) * gstride] = piece[k];
    }
  }
  if (PROF) prof.epi[2] += m3_clock() - t;
}

// ------------------------------------------------------------------ computing waves (0-3)
// phases 1-2: wave = pixel quarter (fragments 2 wave, 2 wave + 1 of the tile), every cout subtile of the layer
template <bool PROF>
__device__ __forceinline__ void m3_compute(const Mixed3Args& p, char* smem, int wave, int lane) {
  M3Prof prof;
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
  {
    const int j = wave * 64 + lane;
    const float* src = j < SH_3A ? p.sh1 + (j - SH_1) : j < SH_3B ? p.sh3a + (j - SH_3A) : p.sh3b + (j - SH_3B);
    reinterpret_cast<float*>(smem + SH_OFF)[j] = *src;
  }
  const unsigned one[2] = {1u, 1u};
  const half8_t nopre[2] = {};
  const int K = p.n_chunks;
  const unsigned a_lane1 = static_cast<unsigned>((c.hi * kMixed3Red + c.l31) * 16);
  const unsigned a_lane3 = static_cast<unsigned>((c.hi * CMID + c.l31) * 16);
  const unsigned row16 = static_cast<unsigned>(p.w * 16);
  const unsigned chunk_lds = static_cast<unsigned>(2 * TPX * 16);
  // phase 3: this wave's output fragment (wave & 1) and, for its lane, the output pixel and the tile pixel of tap (0, 0)
  const int opx = (wave & 1) * 32 + c.l31;
  const bool oval = opx < p.oh * p.ow;
  const int orow = oval ? opx / p.ow : 0, ocol = oval ? opx - orow * p.ow : 0;
  const unsigned b_s2 = ACT_OFF + static_cast<unsigned>(c.hi * TPX + 2 * orow * p.w + 2 * ocol) * 16u;
  const unsigned o_lane = static_cast<unsigned>((orow + p.og.halo) * p.og.wp + ocol + p.og.halo);
  const unsigned o_img = static_cast<unsigned>(p.og.groups * p.og.hp * p.og.wp);

  for (int img = blockIdx.x; img < p.N; img += gridDim.x) {
    unsigned long long t = PROF ? m3_clock() : 0;
    // ---- phase 1: 1x1 Cin->64 ------------------------------------------------------------------
    {
      float16_t acc[2][2];
      zero_acc(acc);
      for (int s = 0; s < K; ++s) {
        barrier_after_lds();   // B1(s): chunk s landed
        t = m3_lap<PROF>(prof.wait[0], t, acc[0][0]);
        const unsigned slot = RING_OFF + static_cast<unsigned>((s + OV) % R1) * P1_SLOT;
        const unsigned b[2] = {slot + c.act[0], slot + c.act[1]};
        chain_step<2, 2, 1, 0, 0, false>(smem, slot + P1_ACT + a_lane1, 0u, b, 0u, one, ZERO_OFF, nopre, acc);
        t = m3_lap<PROF>(prof.mfma[0], t, acc[1][1]);
      }
      barrier_after_lds();     // E1: every wave is done reading the ring (the first 3x3 slab may come)
      store_lds<2>(smem, acc, SH_1, c);
      t = m3_lap<PROF>(prof.epi[0], t, acc[0][0]);
    }
    // ---- phase 2: 3x3 64->96 in place ------------------------------------------------------------
    int q = 0;
    {
      const unsigned first3 = static_cast<unsigned>(-(p.w + 1) * 16);
      const unsigned b3[2] = {ACT_OFF + c.act[0] + first3, ACT_OFF + c.act[1] + first3};
      unsigned m3[2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        m3[pt] = chain_tap_mask_hw(p.h, p.w, 3, 3, c.row[pt], c.col[pt], c.val[pt]);
        asm volatile("" : "+v"(m3[pt]));   // (computed per tile, not kept live across it)
      }
      float16_t acc[3][2];
      zero_acc(acc);
      for (int cc = 0; cc < N3A; ++cc, ++q) {
        const unsigned b[2] = {b3[0] + cc * chunk_lds, b3[1] + cc * chunk_lds};
        barrier_after_lds();
        t = m3_lap<PROF>(prof.wait[1], t, acc[0][0]);
        chain_step<3, 2, 9, 3, 0, false>(smem, BIG_OFF + (q & 1) * BIG_SLOT + a_lane3, 2 * CMID * 16, b, row16, m3,
                                         ZERO_OFF, nopre, acc);
        t = m3_lap<PROF>(prof.mfma[1], t, acc[2][1]);
      }
      barrier_after_lds();     // E2: every wave is done reading the 64-channel tile
      store_lds<3>(smem, acc, SH_3A, c);
      t = m3_lap<PROF>(prof.epi[1], t, acc[0][0]);
    }
    // ---- phase 3: 3x3 / 2 96->96 into the concat buffer --------------------------------------------
    const unsigned obase = static_cast<unsigned>(img) * o_img + static_cast<unsigned>(p.goff * p.og.hp * p.og.wp) + o_lane;
    if (wave < 2) {
      stride2_layer<2, PROF>(p, smem, q, 0, a_lane3, b_s2, row16, oval, obase, c.hi, prof, t);
    } else {
      stride2_layer<1, PROF>(p, smem, q, 2, a_lane3, b_s2, row16, oval, obase, c.hi, prof, t);
    }
  }
  if (PROF && lane == 0 && p.prof != nullptr) {
    unsigned long long* dst = p.prof + (static_cast<size_t>(blockIdx.x) * 4 + wave) * 12;
    for (int k = 0; k < 3; ++k) {
      dst[3 * k] = prof.wait[k];
      dst[3 * k + 1] = prof.mfma[k];
      dst[3 * k + 2] = prof.epi[k];
    }
  }
}

// ------------------------------------------------------------------ moving waves (4-7)
__device__ __forceinline__ void m3_move(const Mixed3Args& p, char* smem, int lw, int lane) {
  const int P = p.h * p.w;
  // quarter qd of an input chunk is pixels qd * 64 .. + 63: the lane's source offset relative to (the tile's image,
  // group 0).  Slots past the map repeat pixel 0 (nothing valid reads them).
  unsigned src[4];
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int px = qd * 64 + lane;
    const int q = px < P ? px : 0;
    const int row = q / p.w, col = q - row * p.w;
    src[qd] = static_cast<unsigned>(((row + p.ig.halo) * p.ig.wp + col + p.ig.halo) * 16);
  }
  const unsigned src_own = lw == 0 ? src[0] : lw == 1 ? src[1] : lw == 2 ? src[2] : src[3];
  const unsigned plane_bytes = static_cast<unsigned>(p.ig.hp * p.ig.wp * 16);
  const int K = p.n_chunks;
  const bool slab_wave = lw < 2;
  auto rsrc_in = [&](int img) {
    return __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(uniform_ptr(reinterpret_cast<const char*>(p.in) + static_cast<size_t>(img) * p.in_img_bytes)), 0,
        0x7fffffff, 0x00020000);
  };
  // the 1x1's weights, every chunk: one descriptor for the launch (chunk s at s * P1_W)
  const __amdgpu_buffer_rsrc_t rw1 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(uniform_ptr(reinterpret_cast<const char*>(p.w1))), 0, K * static_cast<int>(P1_W), 0x00020000);
  // chunk s >= NE of image img: input pieces (k-group 0 / 1, quarter lw) and, on movers 0-1, weight piece lw
  auto issue_late = [&](const __amdgpu_buffer_rsrc_t& ra, int s) {
    const unsigned slot = RING_OFF + static_cast<unsigned>((s + OV) % R1) * P1_SLOT;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(smem + slot + (g * TPX + lw * 64) * 16), 16, src_own,
                                               (2 * s + g) * plane_bytes, 0, 0);
    }
    if (slab_wave) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw1, (lptr_t)(smem + slot + P1_ACT + lw * 1024), 16, lane * 16,
                                               s * P1_W + lw * 1024, 0, 0);
    }
  };
  // chunk s < NE of image img, movers 2-3 only: all of k-group lw - 2 of the input and of the weights
  auto issue_early = [&](int img, int s) {
    const int g = lw - 2;
    const unsigned slot = RING_OFF + static_cast<unsigned>((s + OV) % R1) * P1_SLOT;
    const __amdgpu_buffer_rsrc_t ra = rsrc_in(img);
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(smem + slot + (g * TPX + qd * 64) * 16), 16, src[qd],
                                               (2 * s + g) * plane_bytes, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw1, (lptr_t)(smem + slot + P1_ACT + g * 1024), 16, lane * 16,
                                             s * P1_W + g * 1024, 0, 0);
  };
  // weight slab q of phases 2-3 into big slot q & 1, movers 0-1 only
  auto issue_big = [&](int q) {
    const char* base = q < N3A ? reinterpret_cast<const char*>(p.w3a) + static_cast<size_t>(q) * BIG_SLOT
                               : reinterpret_cast<const char*>(p.w3b) + static_cast<size_t>(q - N3A) * BIG_SLOT;
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(uniform_ptr(base)), 0, BIG_SLOT, 0x00020000);
    const unsigned slot = BIG_OFF + static_cast<unsigned>(q & 1) * BIG_SLOT;
    for (int j = lw; j < static_cast<int>(BIG_SLOT >> 10); j += 2) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(smem + slot + j * 1024), 16, lane * 16, j * 1024, 0, 0);
    }
  };
  const int per_early = slab_wave ? 0 : DMA_EARLY, per_late = slab_wave ? DMA_LATE_W : DMA_LATE;

  int img = blockIdx.x;
  if (img >= p.N) return;
  if (!slab_wave) {
    for (int s = 0; s < NE; ++s) issue_early(img, s);
  }
  for (; img < p.N; img += gridDim.x) {
    const __amdgpu_buffer_rsrc_t ra = rsrc_in(img);
    for (int s = NE; s < R1 - 1; ++s) issue_late(ra, s);
    for (int s = 0; s < K; ++s) {
      // B1(s): chunks s + 1 .. last (issued so far) may still fly
      const int last = min(s + R1 - 2, K - 1);
      const int early = max(0, min(last, NE - 1) - s);
      wait_dma_barrier(early * per_early + (last - s - early) * per_late);
      if (s + R1 - 1 < K) issue_late(ra, s + R1 - 1);
    }
    barrier_only();   // E1
    const int next = img + static_cast<int>(gridDim.x);
    if (slab_wave) {
      issue_big(0);
    }
    for (int q = 0; q < BIG_STEPS; ++q) {
      if (slab_wave) {
        barrier_after_dma();                              // slab q landed
        if (q + 1 < BIG_STEPS) issue_big(q + 1);
      } else {
        barrier_only();
        // the next tile's chunk q into a slot the weight slabs leave alone: one chunk per step, so that the slabs do
        // not queue behind a burst of HBM reads (measured: 524 -> 500 us per forward against all NE chunks at E1)
        if (q < NE && next < p.N) issue_early(next, q);
      }
      if (q == N3A - 1) barrier_only();                   // E2
    }
    barrier_only();   // E3
  }
}

template <bool PROF>
__global__ __launch_bounds__(M3_THREADS, 1) void mixed3_kernel(Mixed3Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (static_cast<int>(blockIdx.x) >= p.N) return;
  if (wave < 4) {
    m3_compute<PROF>(p, smem, wave, lane);
  } else {
    m3_move(p, smem, wave - 4, lane);
  }
}

}  // namespace

size_t mixed3_lds_bytes() { return LDS_BYTES; }
int mixed3_min_chunks() { return R1; }

void launch_mixed3(const Mixed3Args& a, int blocks, hipStream_t stream) {
  static const bool attr = [] {
    for (const void* f : {reinterpret_cast<const void*>(mixed3_kernel<false>), reinterpret_cast<const void*>(mixed3_kernel<true>)}) {
      (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    return true;
  }();
  (void)attr;
  int grid = a.N < blocks ? a.N : blocks;
  if (grid < 1) grid = 1;
  if (a.prof != nullptr) {
    hipLaunchKernelGGL(mixed3_kernel<true>, dim3(grid), dim3(M3_THREADS), LDS_BYTES, stream, a);
  } else {
    hipLaunchKernelGGL(mixed3_kernel<false>, dim3(grid), dim3(M3_THREADS), LDS_BYTES, stream, a);
  }
}

}  // namespace dv
