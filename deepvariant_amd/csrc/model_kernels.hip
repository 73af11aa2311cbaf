// model_kernels.hip -- the classifier's small kernels (interface: model_kernels.h).
//
// Kernels
//   conv_first_u8_kernel<PT>  first 3x3/2 conv straight from the uint8 pileup tensor
//                             ((x-128)/128 in registers)
//   preprocess_kernel         uint8 HWC -> fp16 C8, only for inputs with > 8 channels
//   maxpool3s2_kernel / avgpool3s1_kernel   (avg excludes padding, optional shift + ReLU)
//   head_kernel               global average pool + Dense(3) + softmax in fp32
//   set_ext_kernel            writes the caller's pointers into the ExtPtrs table
//   blank_rows_kernel / blank_need_kernel   blank-row skipping: the per-image row thresholds of the stem
#include <cstdlib>

#include "model_kernels.h"
#include "stem_fused.h"

using namespace dv::convk;

namespace {

constexpr int kFirstUnroll = 5;  // conv_first_u8_kernel: chunks of a 3x3 filter (2 taps per chunk)

__global__ void set_ext_kernel(ExtPtrs* ext, const uint8_t* images, float* probs, const int32_t* rows_hint, int rows_add) {
  ext->images = images;
  ext->probs = probs;
  ext->rows_hint = rows_hint;
  ext->rows_add = rows_add;
}

__device__ __forceinline__ const uint8_t* ext_images(const ExtPtrs* ext, size_t off) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(ext->images + off);
  const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v));
  const unsigned up = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v >> 32));
  return reinterpret_cast<const uint8_t*>((static_cast<unsigned long long>(up) << 32) | lo);
}

// First convolution fused with preprocess_images: reads the uint8 HWC pileup
// tensor the encoder wrote (C <= 8 channels), normalises (x-128)/128 in
// registers and multiplies on MFMA.  K layout: one 16-wide chunk = two filter
// taps x 8 "channels" (C real + zero-weight padding), so a 3x3x7 filter is 5
// chunks instead of the 9 half-empty ones of a 16-channel padded fp16 image,
// and the 0.7 MB/example fp16 staging tensor disappears (HBM: 155 KB read
// instead of 155 KB read + 707 KB written + 707 KB read).
// A lane's fragment = the 8 bytes at (pixel, tap) -- unaligned, fetched as the
// 3 aligned dwords around it and funnel-shifted; byte C..7 belong to the next
// pixel and meet zero weights.  'valid' convolutions only, Cout <= 32.
template <int PT, int UNROLL = kFirstUnroll>
__global__ __launch_bounds__(kConvThreads) void conv_first_u8_kernel(FirstConvArgs p) {
  __shared__ __attribute__((aligned(16))) _Float16 wl[kFirstMaxChunks * 32 * kChunk];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int hi = lane >> 5;
  const int m_block = blockIdx.x * (128 * PT);

  {  // all weights (<= 13 KB) -> LDS
    const uint4_t* src = reinterpret_cast<const uint4_t*>(p.w);
    uint4_t* dst = reinterpret_cast<uint4_t*>(wl);
    for (int i = tid; i < p.n_chunks * 64; i += kConvThreads) dst[i] = src[i];
  }
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(ext_images(p.ext, p.in_off)), 0, p.in_bytes, 0x00020000);

  unsigned base[PT], obase[PT];
  bool mvalid[PT];
  const int ohow = p.OH * p.OW;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int m = m_block + (wave * PT + pt) * 32 + (lane & 31);
    mvalid[pt] = m < p.M;
    int n, pix, oh, ow;
    divmod_small(mvalid[pt] ? m : 0, ohow, p.rcp_ohow, n, pix);
    divmod_small(pix, p.OW, p.rcp_ow, oh, ow);
    base[pt] = mvalid[pt] ? static_cast<unsigned>(((n * p.H + oh * p.stride) * p.W +
                                                   ow * p.stride) * p.C)
                          : 0x80000000u;
    obase[pt] = static_cast<unsigned>((n * p.og.groups * p.og.hp + oh + p.og.halo) * p.og.wp +
                                      ow + p.og.halo);
  }
  const int taps = p.KH * p.KW;
  float16_t acc[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[pt][i] = 0.f;
  __syncthreads();

  // uint8 -> fp16 without per-byte converts: 0x6400 | b is the fp16 number 1024 + b, and
  // (1024 + b) * 2^-7 - 9 = (b - 128) / 128 exactly -- one v_perm_b32 and one packed FMA
  // per two channels.
  auto normalise = [](unsigned lo, unsigned up) {
    const half2_t scale = {static_cast<_Float16>(0.0078125f), static_cast<_Float16>(0.0078125f)};
    const half2_t bias = {static_cast<_Float16>(-9.0f), static_cast<_Float16>(-9.0f)};
    const unsigned k = 0x64646464u;
    const half2_t h01 = __builtin_bit_cast(half2_t, __builtin_amdgcn_perm(lo, k, 0x00050004u));
    const half2_t h23 = __builtin_bit_cast(half2_t, __builtin_amdgcn_perm(lo, k, 0x00070006u));
    const half2_t h45 = __builtin_bit_cast(half2_t, __builtin_amdgcn_perm(up, k, 0x00050004u));
    const half2_t h67 = __builtin_bit_cast(half2_t, __builtin_amdgcn_perm(up, k, 0x00070006u));
    const half2_t a = h01 * scale + bias, b = h23 * scale + bias;
    const half2_t c = h45 * scale + bias, d = h67 * scale + bias;
    return half8_t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
  };
  typedef unsigned uint3_t __attribute__((ext_vector_type(3)));
  if (p.n_chunks <= UNROLL) {
    // every fragment of the tile is requested before the first one is used
    uint3_t d[UNROLL][PT];
    unsigned sh[UNROLL][PT];
#pragma unroll
    for (int kc = 0; kc < UNROLL; ++kc) {
      const int t = min(p.wide ? kc : 2 * kc + hi, taps - 1);
      const int kh = t / p.KW, kw = t - kh * p.KW;
      const unsigned toff = static_cast<unsigned>((kh * p.W + kw) * p.C + (p.wide ? 8 * hi : 0));
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const unsigned a = base[pt] + toff;
        sh[kc][pt] = (a & 3u) * 8u;
        d[kc][pt] = kc < p.n_chunks ? __builtin_amdgcn_raw_buffer_load_b96(rsrc, a & ~3u, 0, 0)
                                    : uint3_t{0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int kc = 0; kc < UNROLL; ++kc) {
      if (kc < p.n_chunks) {
        const half8_t wf = *reinterpret_cast<const half8_t*>(
            wl + kc * 32 * kChunk + hi * (32 * 8) + (lane & 31) * 8);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          const unsigned lo = __builtin_amdgcn_alignbit(d[kc][pt][1], d[kc][pt][0], sh[kc][pt]);
          const unsigned up = __builtin_amdgcn_alignbit(d[kc][pt][2], d[kc][pt][1], sh[kc][pt]);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, normalise(lo, up), acc[pt], 0, 0, 0);
        }
      }
    }
  } else {
    for (int kc = 0; kc < p.n_chunks; ++kc) {
      // this lane-half's tap (wide: its half of the tap's channels); past the last tap the weights are zero
      const int t = min(p.wide ? kc : 2 * kc + hi, taps - 1);
      const int kh = t / p.KW, kw = t - kh * p.KW;
      const unsigned toff = static_cast<unsigned>((kh * p.W + kw) * p.C + (p.wide ? 8 * hi : 0));
      const half8_t wf = *reinterpret_cast<const half8_t*>(
          wl + kc * 32 * kChunk + hi * (32 * 8) + (lane & 31) * 8);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const unsigned a = base[pt] + toff;
        const uint3_t dd = __builtin_amdgcn_raw_buffer_load_b96(rsrc, a & ~3u, 0, 0);
        const unsigned s8 = (a & 3u) * 8u;
        const unsigned lo = __builtin_amdgcn_alignbit(dd[1], dd[0], s8);
        const unsigned up = __builtin_amdgcn_alignbit(dd[2], dd[1], s8);
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, normalise(lo, up), acc[pt], 0, 0, 0);
      }
    }
  }

  // epilogue (same piece pairing as conv_mfma_kernel, one 32-cout tile)
  const unsigned gstride = static_cast<unsigned>(p.og.hp * p.og.wp);
  uint4_t* outp = reinterpret_cast<uint4_t*>(p.out);
  const half2_t zero2 = {static_cast<_Float16>(0.f), static_cast<_Float16>(0.f)};
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    unsigned pk[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = 8 * q + 4 * hi;
#pragma unroll
      for (int hq = 0; hq < 2; ++hq) {
        const float2_t sv = {co + 2 * hq < p.Cout ? p.shift[co + 2 * hq] : 0.f,
                             co + 2 * hq + 1 < p.Cout ? p.shift[co + 2 * hq + 1] : 0.f};
        const float2_t v = float2_t{acc[pt][4 * q + 2 * hq], acc[pt][4 * q + 2 * hq + 1]} + sv;
        half2_t h = __builtin_convertvector(v, half2_t);
        h = __builtin_elementwise_max(h, zero2);
        pk[q][hq] = __builtin_bit_cast(unsigned, h);
      }
    }
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const auto d0 = __builtin_amdgcn_permlane32_swap(pk[2 * t2][0], pk[2 * t2 + 1][0], false, false);
      const auto d1 = __builtin_amdgcn_permlane32_swap(pk[2 * t2][1], pk[2 * t2 + 1][1], false, false);
      const uint4_t piece = {d0[0], d1[0], d0[1], d1[1]};
      const int group = 2 * t2 + hi;
      if (mvalid[pt] && group * 8 < p.Cout) {
        outp[obase[pt] + static_cast<unsigned>(group) * gstride] = piece;
      }
    }
  }
}

// uint8 [N,H,W,C] -> fp16 C8 [N][2][hp][wp][8]: (x - 128) / 128, exact in fp16.
__global__ void preprocess_kernel(const ExtPtrs* ext, size_t in_off, _Float16* out, size_t n_pix, int C,
                                  int H, int W, TensorGeom og) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= n_pix) return;
  const uint8_t* in = ext->images + in_off;
  const uint8_t* px = in + i * C;
  _Float16 v[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    v[c] = c < C ? static_cast<_Float16>((static_cast<float>(px[c]) - 128.0f) / 128.0f)
                 : static_cast<_Float16>(0.f);
  }
  const size_t n = i / (static_cast<size_t>(H) * W);
  const int pix = static_cast<int>(i - n * (static_cast<size_t>(H) * W));
  const int y = pix / W, x = pix - y * W;
  uint4* dst = reinterpret_cast<uint4*>(out);
  const size_t plane = static_cast<size_t>(og.hp) * og.wp;
  const size_t at = (n * 2) * plane + static_cast<size_t>(y + og.halo) * og.wp + x + og.halo;
  dst[at] = *reinterpret_cast<uint4*>(&v[0]);
  dst[at + plane] = *reinterpret_cast<uint4*>(&v[8]);
}

// Blank-row skipping (opt-in, DV_BLANK_SKIP): one workgroup per image finds the last row that
// holds a nonzero byte, scanning from the bottom (a 30x pileup is zero below row ~40, so about
// 60 % of the image is read once), and turns it into the first blank-determined row of the
// stem's tensors: an output whose receptive field sees only zero rows equals the all-blank
// image's output at the same position.
//   conv1 3x3/2 valid: rows 2y..2y+2   -> y >= ceil(r / 2)         (= conv2, 3x3 valid on those)
//   conv3 3x3 same:    rows y-1..y+1   -> y >= t2 + 1
//   max-pool 3x3/2:    rows 2y..2y+2   -> y >= ceil(t3 / 2)        (= the 1x1 and the 3x3 valid 80->192)
// thr[k * stride + n], k = 0: rows used, 1: conv2 output, 2: stem_b output, 3: 3x3 80->192 output, 4: the same, pooled.
// What the consumers of the skipping kernels read (thr rows 5 and 6): blank tiles beyond these rows are not even
// copied.  need2 = conv2 rows under stem_b's computed tiles (pooled tiles of kStemB_PH rows starting above t4: pooled
// row py reads conv3 rows 2py..2py+2, conv3 row y conv2 rows y-1..y+1); need4 = stem_b rows under the 3x3 80->192's
// walk, which goes down to the deepest pooled threshold among the examples a 32-position fragment spans (conv row r
// reads rows r..r+2; the walk's last row is 2 s_end).
// (stem_b_fused / conv4_walks = 0: the consumer is a per-layer kernel that may read every row -- everything is wanted.)
// thr row 7: cut2 = the first conv2 row the fused stem_a did not compute (its tiles of kStemA_TH rows are computed iff
// they start above t2).  When stem_b reads the blank rows through, it takes conv2 rows >= cut2 from the blank response
// and stem_a copies nothing (model.hip enqueue_stem_a / enqueue_stem_b).
__global__ void blank_need_kernel(int* thr, int stride, int n, int oh2, int ph_b, int ow4, int p4, int stem_b_fused,
                                  int conv4_walks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t4 = min(thr[2 * stride + i], ph_b);
  const int kb = (t4 + dv::kStemB_PH - 1) / dv::kStemB_PH;
  thr[5 * stride + i] = !stem_b_fused ? oh2 : kb > 0 ? min(oh2, 2 * dv::kStemB_PH * kb + 2) : 0;
  const int span = 31 / max(ow4, 1) + 1;
  int m5 = 0;
  for (int j = max(0, i - span); j <= min(n - 1, i + span); ++j) m5 = max(m5, min(thr[4 * stride + j], p4));
  thr[6 * stride + i] = !conv4_walks ? ph_b : m5 > 0 ? min(ph_b, 2 * m5 + 3) : 0;
  const int t2 = max(thr[stride + i], 0);
  thr[7 * stride + i] = min(oh2, dv::kStemA_TH * ((t2 + dv::kStemA_TH - 1) / dv::kStemA_TH));
}

__global__ __launch_bounds__(256) void blank_rows_kernel(const ExtPtrs* ext, size_t in_off, int n_hint0, int H,
                                                         int row_bytes, int* thr, int stride) {
  __shared__ int last;
  const uint8_t* images = ext->images + in_off;
  const int n = blockIdx.x, tid = threadIdx.x;
  const unsigned img_bytes = static_cast<unsigned>(H) * row_bytes;   // multiple of 4 (checked by the host)
  const uint32_t* img = reinterpret_cast<const uint32_t*>(images + static_cast<size_t>(n) * img_bytes);
  const int n_dw = static_cast<int>(img_bytes / 4);
  if (tid == 0) last = -1;
  __syncthreads();
  constexpr int kPer = 16;   // dwords per thread and trip: 16 KB of the image per barrier
  // dv_model_infer_rows: the caller (the encoder that drew the images) states the rows used -- no scan
  const bool hinted = ext->rows_hint != nullptr;   // uniform
  const int hinted_rows = hinted ? max(0, min(H, ext->rows_hint[n_hint0 + n] + ext->rows_add)) : 0;
  for (int hi = hinted ? 0 : n_dw; hi > 0; hi -= 256 * kPer) {
    uint32_t v[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {   // all loads in flight before the first compare
      const int i = hi - 1 - (k * 256 + tid);
      v[k] = i >= 0 ? img[i] : 0u;
    }
    int mine = -1;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int i = hi - 1 - (k * 256 + tid);
      if (v[k] != 0) mine = max(mine, 4 * i + 3 - (__clz(v[k]) >> 3));   // its highest nonzero byte
    }
    if (mine >= 0) atomicMax(&last, mine);
    __syncthreads();
    const int found = last;   // uniform: read after the barrier ...
    __syncthreads();          // ... and before any wave's atomicMax of the next trip
    if (found >= 0) break;
  }
  if (tid == 0) {
    const int r = hinted ? hinted_rows : last < 0 ? 0 : last / row_bytes + 1;
    const int t2 = (r + 1) / 2, t3 = t2 + 1, t4 = (t3 + 1) / 2;
    thr[n] = r;
    thr[stride + n] = t2;
    thr[2 * stride + n] = t4;
    thr[3 * stride + n] = t4;
    thr[4 * stride + n] = (t4 + 1) / 2;   // the 3x3 80->192's output max-pooled (3x3 / 2) inside its producer: rows 2s .. 2s+2
  }
}

// MaxPooling2D(3, strides=2, 'valid'), C8 layout; one thread = one 16-byte piece.  Wide tensors (precise mode): the
// maximum of hi + lo is the lexicographic maximum of (hi, lo) -- |lo| is at most half an ulp of hi.
__global__ void maxpool3s2_kernel(PoolArgs p) {
  const int cg = p.C / 8;
  const size_t total = static_cast<size_t>(p.N) * cg * p.OH * p.OW;
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= total) return;
  const int ow = i % p.OW;
  size_t t = i / p.OW;
  const int oh = t % p.OH;
  t /= p.OH;
  const int g = t % cg;
  const int n = t / cg;
  const size_t plane = static_cast<size_t>(p.ig.hp) * p.ig.wp;
  const half8_t* src = reinterpret_cast<const half8_t*>(p.in) + (static_cast<size_t>(n) * p.ig.groups + g) * plane;
  const half8_t* src_lo = src + static_cast<size_t>(p.lo_in_groups) * plane;
  half8_t best, best_lo;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    best[j] = static_cast<_Float16>(-65504.f);
    best_lo[j] = static_cast<_Float16>(0.f);
  }
  const size_t at0 = static_cast<size_t>(oh * 2 + p.ig.halo) * p.ig.wp + ow * 2 + p.ig.halo;
  if (p.lo_in_groups > 0) {   // uniform; all eighteen pieces in flight before the first compare
    half8_t v[9], l[9];
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9) {
      const size_t at = at0 + static_cast<size_t>(t9 / 3) * p.ig.wp + t9 % 3;
      v[t9] = src[at];
      l[t9] = src_lo[at];
    }
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool take = v[t9][j] > best[j] || (v[t9][j] == best[j] && l[t9][j] > best_lo[j]);
        best[j] = take ? v[t9][j] : best[j];
        best_lo[j] = take ? l[t9][j] : best_lo[j];
      }
    }
  } else {
    for (int dh = 0; dh < 3; ++dh)
      for (int dw = 0; dw < 3; ++dw) {
        const half8_t v = src[at0 + static_cast<size_t>(dh) * p.ig.wp + dw];
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = v[j] > best[j] ? v[j] : best[j];
      }
  }
  const size_t oplane = static_cast<size_t>(p.og.hp) * p.og.wp;
  half8_t* dst = reinterpret_cast<half8_t*>(p.out) + (static_cast<size_t>(n) * p.og.groups + p.out_goff + g) * oplane +
                 static_cast<size_t>(oh + p.og.halo) * p.og.wp + ow + p.og.halo;
  *dst = best;
  if (p.lo_out_groups > 0) dst[static_cast<size_t>(p.lo_out_groups) * oplane] = best_lo;
}

// AveragePooling2D(3, strides=1, 'same'): divisor = number of valid cells.  The input is the float32 raw
// 1x1 projection of a pooled branch (pooled_projection: conv -> pool -> shift -> ReLU); its buffer carries a
// zero halo of >= 1 (build() asks for it), so the taps are unconditional loads and only the divisor depends on
// the position.  One thread produces TWO horizontally adjacent outputs from a 3x4 window (12 loads instead of
// 18): the three column sums in the middle are shared.  Same arithmetic as conv_epilogue_avg (avg_finish).
__global__ void avgpool3s1_kernel(PoolArgs p) {
  const int cg = p.C / 8;
  const int H = p.ig.h, W = p.ig.w;
  const int W2 = (W + 1) >> 1;
  const size_t total = static_cast<size_t>(p.N) * cg * H * W2;
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= total) return;
  const int ow = 2 * static_cast<int>(i % W2);
  size_t t = i / W2;
  const int oh = t % H;
  t /= H;
  const int g = t % cg;
  const int n = t / cg;
  const bool two = ow + 1 < W;
  const float4* src = reinterpret_cast<const float4*>(p.in32) +
                      (((static_cast<size_t>(n) * p.ig.groups + g) * p.ig.hp + oh + p.ig.halo - 1) *
                           p.ig.wp + ow + p.ig.halo - 1) * 2;
  const int last = two ? 3 : 2;  // never read past the row's halo
  float col[4][8];
#pragma unroll
  for (int dw = 0; dw < 4; ++dw) {
    const int c = dw < 3 ? dw : last;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float4 a = src[2 * c + hf], b = src[2 * (p.ig.wp + c) + hf], d = src[2 * (2 * p.ig.wp + c) + hf];
      col[dw][4 * hf + 0] = a.x + b.x + d.x;
      col[dw][4 * hf + 1] = a.y + b.y + d.y;
      col[dw][4 * hf + 2] = a.z + b.z + d.z;
      col[dw][4 * hf + 3] = a.w + b.w + d.w;
    }
  }
  const int rows = (oh > 0) + (oh < H - 1) + 1;
  float sh[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (p.shift != nullptr) {
    const float4 s0 = *reinterpret_cast<const float4*>(p.shift + g * 8);
    const float4 s1 = *reinterpret_cast<const float4*>(p.shift + g * 8 + 4);
    sh[0] = s0.x; sh[1] = s0.y; sh[2] = s0.z; sh[3] = s0.w;
    sh[4] = s1.x; sh[5] = s1.y; sh[6] = s1.z; sh[7] = s1.w;
  }
  const size_t at = ((static_cast<size_t>(n) * p.og.groups + p.out_goff + g) * p.og.hp + oh + p.og.halo) * p.og.wp +
                    ow + p.og.halo;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (k == 1 && !two) break;
    const int x = ow + k;
    const float inv = 1.0f / static_cast<float>(rows * ((x > 0) + (x < W - 1) + 1));
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o[j] = avg_finish(col[k][j], col[k + 1][j], col[k + 2][j], inv, sh[j], p.shift != nullptr);
    }
    if (p.out32 != nullptr) {
      float4* d = reinterpret_cast<float4*>(p.out32 + (at + k) * 8);
      d[0] = make_float4(o[0], o[1], o[2], o[3]);
      d[1] = make_float4(o[4], o[5], o[6], o[7]);
    } else {
      half8_t h;
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = static_cast<_Float16>(o[j]);
      reinterpret_cast<half8_t*>(p.out)[at + k] = h;
      if (p.lo_out_groups > 0) {
        half8_t l;
#pragma unroll
        for (int j = 0; j < 8; ++j) l[j] = static_cast<_Float16>(o[j] - static_cast<float>(h[j]));
        reinterpret_cast<half8_t*>(p.out)[at + k + static_cast<size_t>(p.lo_out_groups) * p.og.hp * p.og.wp] = l;
      }
    }
  }
}

// GlobalAveragePooling2D + Dense(num_classes) + softmax, fp32.  Round 6: the last block's outputs arrive in
// float32 (BufferDesc::f32) -- the values the convolutions' accumulators held, not an fp16 copy of them.
// OUT (head_outputs_kernel, dv_model_infer_outputs): also stores the pooled vector ([C] per example) and the logits
// ([K]) where they are computed -- the same arithmetic in the same order, so the probabilities are the plain head's.
template <bool OUT>
__device__ __forceinline__ void head_body(const float* in, const float* w, const float* b, float* probs, TensorGeom g,
                                          int K, float* pooled, float* logits) {
  __shared__ float red[8][4];
  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  const int C = g.groups * 8;
  const size_t plane = static_cast<size_t>(g.hp) * g.wp * 8;
  float part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const float* x = in + static_cast<size_t>(n) * g.groups * plane;
  const float invP = 1.0f / static_cast<float>(g.h * g.w);
  // one thread per 8-channel group: the map's pixels come in as whole 16-byte pieces
  for (int grp = tid; grp * 8 < C; grp += 256) {
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const float4* xg = reinterpret_cast<const float4*>(x + static_cast<size_t>(grp) * plane);
    for (int y = 0; y < g.h; ++y)
      for (int xx = 0; xx < g.w; ++xx) {
        const float4 lo = xg[((y + g.halo) * g.wp + xx + g.halo) * 2], up = xg[((y + g.halo) * g.wp + xx + g.halo) * 2 + 1];
        s[0] += lo.x; s[1] += lo.y; s[2] += lo.z; s[3] += lo.w;
        s[4] += up.x; s[5] += up.y; s[6] += up.z; s[7] += up.w;
      }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float m = s[j] * invP;
      if (OUT && pooled != nullptr) pooled[static_cast<size_t>(n) * C + grp * 8 + j] = m;
      for (int k = 0; k < K; ++k) part[k] += m * w[static_cast<size_t>(grp * 8 + j) * K + k];
    }
  }
  for (int k = 0; k < K; ++k) {
    float v = part[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((tid & 63) == 0) red[k][tid >> 6] = v;
  }
  __syncthreads();
  if (tid == 0) {
    float logit[8], mx = -1e30f;
    for (int k = 0; k < K; ++k) {
      logit[k] = red[k][0] + red[k][1] + red[k][2] + red[k][3] + b[k];
      if (OUT && logits != nullptr) logits[static_cast<size_t>(n) * K + k] = logit[k];
      mx = fmaxf(mx, logit[k]);
    }
    float sum = 0.f;
    for (int k = 0; k < K; ++k) {
      logit[k] = expf(logit[k] - mx);
      sum += logit[k];
    }
    for (int k = 0; k < K; ++k) probs[static_cast<size_t>(n) * K + k] = logit[k] / sum;
  }
}

__global__ __launch_bounds__(256) void head_kernel(const float* in, const float* w,
                                                   const float* b, const ExtPtrs* ext, size_t probs_off,
                                                   TensorGeom g, int K) {
  head_body<false>(in, w, b, ext->probs + probs_off, g, K, nullptr, nullptr);
}

// pooled / logits: [examples][C] / [examples][K] destinations for this launch's examples; either may be null
__global__ __launch_bounds__(256) void head_outputs_kernel(const float* in, const float* w, const float* b,
                                                           const ExtPtrs* ext, size_t probs_off, TensorGeom g, int K,
                                                           float* pooled, float* logits) {
  head_body<true>(in, w, b, ext->probs + probs_off, g, K, pooled, logits);
}

}  // namespace

namespace dv {
namespace convk {

void launch_set_ext(ExtPtrs* ext, const uint8_t* images, float* probs, const int32_t* rows_hint, int rows_add,
                    hipStream_t stream) {
  hipLaunchKernelGGL(set_ext_kernel, dim3(1), dim3(1), 0, stream, ext, images, probs, rows_hint, rows_add);
}

void launch_conv_first_u8(const FirstConvArgs& f, hipStream_t stream) {
  // four pixel fragments per wave: 20 outstanding 12-byte loads per lane (+1.7 % end to end
  // over two on MI355X); DV_FIRST_PT2 restores the smaller tile for tuning.
  static const bool first4 = getenv("DV_FIRST_PT2") == nullptr;
  // wide inputs (9..16 channels): four fragments per wave as well -- 36 outstanding 12-byte loads per lane,
  // 236 VGPRs; hifi35 504.2 -> 516.6 K, ont50 369.4 -> 376.6 K candidates/s same box (DV_FIRST_WIDE_PT2 restores <2,9>)
  static const bool wide4 = getenv("DV_FIRST_WIDE_PT2") == nullptr;
  if (f.wide && wide4) {
    hipLaunchKernelGGL((conv_first_u8_kernel<4, 9>), dim3((f.M + 511) / 512), dim3(kConvThreads), 0,
                       stream, f);
  } else if (f.wide) {   // nine one-tap chunks, all requested before the first MFMA
    hipLaunchKernelGGL((conv_first_u8_kernel<2, 9>), dim3((f.M + 255) / 256), dim3(kConvThreads), 0,
                       stream, f);
  } else if (first4) {
    hipLaunchKernelGGL((conv_first_u8_kernel<4>), dim3((f.M + 511) / 512), dim3(kConvThreads), 0,
                       stream, f);
  } else {
    hipLaunchKernelGGL((conv_first_u8_kernel<2>), dim3((f.M + 255) / 256), dim3(kConvThreads), 0,
                       stream, f);
  }
}

void launch_preprocess(const ExtPtrs* ext, size_t in_off, _Float16* out, int n, int C, int H, int W, TensorGeom og,
                       hipStream_t stream) {
  const size_t n_pix = static_cast<size_t>(n) * H * W;
  hipLaunchKernelGGL(preprocess_kernel, dim3(static_cast<unsigned>((n_pix + 255) / 256)), dim3(256), 0, stream, ext, in_off,
                     out, n_pix, C, H, W, og);
}

void launch_blank_scan(const ExtPtrs* ext, size_t in_off, int n_hint0, int n, int H, int row_bytes, int* thr, int stride,
                       int oh2, int ph_b, int ow4, int p4, int stem_b_fused, int conv4_walks, hipStream_t stream) {
  hipLaunchKernelGGL(blank_rows_kernel, dim3(n), dim3(256), 0, stream, ext, in_off, n_hint0, H, row_bytes, thr, stride);
  hipLaunchKernelGGL(blank_need_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, thr, stride, n, oh2, ph_b, ow4, p4,
                     stem_b_fused, conv4_walks);
}

// one thread per 16-byte piece of the output (maxpool3s2_kernel) / per two pieces of a row (avgpool3s1_kernel)
void launch_maxpool3s2(const PoolArgs& p, hipStream_t stream) {
  const size_t total = static_cast<size_t>(p.N) * p.OH * p.OW * (p.C / 8);
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, stream, p);
}

void launch_avgpool3s1(const PoolArgs& p, hipStream_t stream) {
  const size_t total = static_cast<size_t>(p.N) * p.OH * ((p.OW + 1) / 2) * (p.C / 8);
  hipLaunchKernelGGL(avgpool3s1_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, stream, p);
}

void launch_head(const float* in, const float* w, const float* b, const ExtPtrs* ext, size_t probs_off, TensorGeom g, int K,
                 int n, bool outputs, float* pooled, float* logits, hipStream_t stream) {
  if (outputs) {
    hipLaunchKernelGGL(head_outputs_kernel, dim3(n), dim3(256), 0, stream, in, w, b, ext, probs_off, g, K, pooled, logits);
  } else {
    hipLaunchKernelGGL(head_kernel, dim3(n), dim3(256), 0, stream, in, w, b, ext, probs_off, g, K);
  }
}

}  // namespace convk
}  // namespace dv
