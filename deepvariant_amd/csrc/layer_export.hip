// layer_export.hip -- a plan tensor to dense NHWC float32 (dv_model_infer_outputs).
//
// One thread per (example, pixel, 8-channel group of the view): it reads that group's piece of the channel-blocked
// source -- one 16-byte fp16 piece, one 32-byte float32 piece, or the hi and the lo fp16 pieces of a wide tensor --
// and stores the 8 floats at their place in the destination pixel.  Consecutive threads take consecutive groups of
// one pixel, so a wave's stores are one contiguous run (32 bytes per lane as two 16-byte stores); the loads are whole
// pieces, a map plane apart, and the neighbouring pixels' waves read the rest of each line.
#include "layer_export.h"

#include <algorithm>

#include <hip/hip_fp16.h>

namespace dv {
namespace {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(256) void layer_export_kernel(LayerExportArgs a) {
  // every index fits 32 bits: the view has no more pieces than the source tensor, which dv_model_create keeps below
  // 2^31 pieces
  const unsigned total = static_cast<unsigned>(a.n) * a.h * a.w * a.groups;
  const size_t plane = static_cast<size_t>(a.hp) * a.wp;   // pieces of one channel group
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned g = i % a.groups;
    const unsigned pix = i / a.groups;   // (e * h + y) * w + x
    const unsigned x = pix % a.w;
    const unsigned ey = pix / a.w;
    const unsigned y = ey % a.h;
    const unsigned e = ey / a.h;
    const size_t piece = (static_cast<size_t>(e) * a.src_groups + a.goff + g) * plane +
                         static_cast<size_t>(y + a.halo) * a.wp + x + a.halo;
    float v[8];
    if (a.kind == kExportF32) {
      const float4* s = reinterpret_cast<const float4*>(a.src) + piece * 2;
      const float4 lo = s[0], up = s[1];
      v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
      v[4] = up.x; v[5] = up.y; v[6] = up.z; v[7] = up.w;
    } else {
      const half8_t* s = reinterpret_cast<const half8_t*>(a.src);
      const half8_t hi = s[piece];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = static_cast<float>(hi[j]);
      if (a.kind == kExportWide) {
        const half8_t lo = s[piece + static_cast<size_t>(a.lo_groups) * plane];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += static_cast<float>(lo[j]);
      }
    }
    float4* d = reinterpret_cast<float4*>(a.dst + static_cast<size_t>(i) * 8);
    d[0] = make_float4(v[0], v[1], v[2], v[3]);
    d[1] = make_float4(v[4], v[5], v[6], v[7]);
  }
}

}  // namespace

void launch_layer_export(const LayerExportArgs& a, hipStream_t stream) {
  const long total = static_cast<long>(a.n) * a.h * a.w * a.groups;
  if (total <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long>((total + 255) / 256, 8192));
  hipLaunchKernelGGL(layer_export_kernel, dim3(blocks), dim3(256), 0, stream, a);
}

}  // namespace dv
