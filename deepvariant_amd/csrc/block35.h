// block35.hip's interface: one Inception-A block of the 35x35 stage (mixed0..mixed2) as ONE
// persistent launch -- the four 1x1 heads, the 5x5 branch and the 3x3 -> 3x3 branch on tiles of
// one whole map, the 48- and 64-channel reducers and the 3x3 intermediate resident in LDS.
#ifndef DV_BLOCK35_H_
#define DV_BLOCK35_H_

#include "conv_common.h"

namespace dv {

constexpr int kBlock35TilePx = 256;   // one map of up to 256 pixels per tile (8 MFMA fragments)
constexpr int kBlock35Red5 = 48;      // couts of the fixed branch shapes (keras_modeling / tf_keras InceptionV3)
constexpr int kBlock35Red3 = 64;
constexpr int kBlock35B1 = 64;
constexpr int kBlock35Out5 = 64;
constexpr int kBlock35Out3 = 96;

struct Block35Args {
  const _Float16* in;        // block input, C8
  convk::TensorGeom ig;
  unsigned in_img_bytes;     // bytes of one example of `in`
  int N, h, w;               // one h x w map per tile, h * w <= kBlock35TilePx
  int n_chunks;              // Cin / 16
  // the four 1x1 heads, two K passes over the input: [pass][chunk][2 k-groups][128 couts][8];
  // pass 0 = 5x5 reducer (couts 0-47) + 3x3 reducer (64-127), pass 1 = b1 (0-63) + pooled projection (64-)
  const _Float16* w1;
  const float* sh_red5;
  const float* sh_red3;
  const float* sh_b1;
  const float* sh_pool;      // the average pool's shift (applied after the pool)
  int pool_c;                // 32 or 64
  const _Float16* w5;        // 5x5 48->64, [chunk][tap][2 k-groups][64][8]
  const float* sh5;
  const _Float16* w3a;       // 3x3 64->96, [chunk][tap][2 k-groups][96][8]
  const float* sh3a;
  const _Float16* w3b;       // 3x3 96->96
  const float* sh3b;
  _Float16* out;             // the block's concat buffer
  convk::TensorGeom og;
  int goff_b1, goff_5, goff_3, goff_pool;   // first destination channel group of each branch
};

size_t block35_lds_bytes();
void launch_block35(const Block35Args& a, int blocks, hipStream_t stream);

}  // namespace dv

#endif  // DV_BLOCK35_H_
