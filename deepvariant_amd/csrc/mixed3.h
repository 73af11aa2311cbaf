// mixed3.hip's interface: the double-3x3 branch of the reduction block mixed3 (1x1 Cin->64, 3x3 64->96 'same',
// 3x3 96->96 stride 2 'valid') as ONE persistent launch on tiles of one whole map -- the 64- and 96-channel
// tensors between the layers live in LDS only.
#ifndef DV_MIXED3_H_
#define DV_MIXED3_H_

#include "conv_common.h"

namespace dv {

constexpr int kMixed3TilePx = 256;   // one input map of up to 256 pixels per tile
constexpr int kMixed3Red = 64;       // couts of the fixed branch shapes (tf_keras InceptionV3 mixed3)
constexpr int kMixed3Mid = 96;
constexpr int kMixed3Out = 96;
constexpr int kMixed3MaxOutPx = 64;  // the stride-2 layer's output map: at most two MFMA fragments

struct Mixed3Args {
  const _Float16* in;        // block input, C8
  convk::TensorGeom ig;
  unsigned in_img_bytes;     // bytes of one example of `in`
  int N, h, w;               // one h x w map per tile, h * w <= kMixed3TilePx
  int n_chunks;              // Cin / 16, at least mixed3_min_chunks()
  const _Float16* w1;        // 1x1 Cin->64, [chunk][2 k-groups][64][8]
  const float* sh1;
  const _Float16* w3a;       // 3x3 64->96, [chunk][tap][2 k-groups][96][8]
  const float* sh3a;
  const _Float16* w3b;       // 3x3 / 2 96->96, same layout
  const float* sh3b;
  _Float16* out;             // the block's concat buffer
  convk::TensorGeom og;
  int oh, ow;                // (h - 3) / 2 + 1, (w - 3) / 2 + 1; oh * ow <= kMixed3MaxOutPx
  int goff;                  // first destination channel group
  unsigned long long* prof;  // DV_MIXED3_PROF: [workgroup][computing wave][12] shader-clock sums, or null
};

size_t mixed3_lds_bytes();
int mixed3_min_chunks();     // the input ring's depth: a shorter K would not fill it
void launch_mixed3(const Mixed3Args& a, int blocks, hipStream_t stream);

}  // namespace dv

#endif  // DV_MIXED3_H_
