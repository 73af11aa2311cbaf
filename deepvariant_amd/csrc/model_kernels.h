// model_kernels.hip's interface: the classifier's kernels that are not MFMA convolutions of fp16 tensors -- the caller's
// pointer table, the uint8 front end, blank-row scan, pools and head -- one launch function each.
#ifndef DV_MODEL_KERNELS_H_
#define DV_MODEL_KERNELS_H_

#include "conv_common.h"

namespace dv {
namespace convk {

// The caller's two pointers (uint8 images in, probabilities out) are read by the kernels from
// this device-side table instead of being kernel arguments: a captured forward then depends on
// the batch size only, and a caller that hands over a fresh tensor per region replays the same
// hipGraph (dv_model_infer writes the table with a one-thread kernel ahead of every forward).
struct ExtPtrs {
  const uint8_t* images;
  float* probs;
  const int32_t* rows_hint;   // dv_model_infer_rows: per image, rows at or below rows_hint[i] + rows_add are all zero
  int rows_add;
};

struct FirstConvArgs {
  const ExtPtrs* ext;       // images = ext->images + in_off: [N][H][W][C]
  size_t in_off;
  const _Float16* w;        // packed [chunk][2 k-groups = taps][32][8]
  const float* shift;
  _Float16* out;
  TensorGeom og;
  int N, H, W, C, Cout;
  int OH, OW, KH, KW, stride;
  int M, n_chunks;
  unsigned in_bytes;
  float rcp_ow, rcp_ohow;
  // C in 9..16 (the long-read channel sets: 9 = ONT_R104, 10 = PACBIO): a K chunk is ONE tap x 16
  // "channels" -- k-group 0 = bytes 0..7 of the pixel, k-group 1 = bytes 8..15 (bytes C.. belong to the
  // next pixel and meet zero weights) -- instead of two taps x 8
  int wide;
};

constexpr int kFirstMaxChunks = 13;  // up to 5x5 taps (C <= 8) / 3x3 taps (C <= 16)

struct PoolArgs {
  const _Float16* in;     // maxpool3s2_kernel: fp16
  const float* in32;      // avgpool3s1_kernel: the float32 raw projection
  _Float16* out;
  float* out32;           // avgpool3s1_kernel: non-NULL = the pooled tensor is float32 (the last block's, read by the head)
  int lo_in_groups;       // maxpool3s2_kernel: > 0 = the input is wide (hi groups, then lo groups: precise mode)
  int lo_out_groups;      // > 0 = the output tensor is wide: the lo pieces go lo_out_groups channel groups further
  TensorGeom ig, og;
  int N, C, OH, OW;
  int out_goff;
  const float* shift;  // avgpool only: per-channel shift + ReLU after the average, or NULL
};

void launch_set_ext(ExtPtrs* ext, const uint8_t* images, float* probs, const int32_t* rows_hint, int rows_add,
                    hipStream_t stream);
void launch_conv_first_u8(const FirstConvArgs& f, hipStream_t stream);   // picks the tile shape (DV_FIRST_PT2, DV_FIRST_WIDE_PT2)
void launch_preprocess(const ExtPtrs* ext, size_t in_off, _Float16* out, int n, int C, int H, int W, TensorGeom og,
                       hipStream_t stream);
// blank_rows_kernel, then blank_need_kernel, over images [n_hint0, n_hint0 + n) of the caller's batch
void launch_blank_scan(const ExtPtrs* ext, size_t in_off, int n_hint0, int n, int H, int row_bytes, int* thr, int stride,
                       int oh2, int ph_b, int ow4, int p4, int stem_b_fused, int conv4_walks, hipStream_t stream);
void launch_maxpool3s2(const PoolArgs& p, hipStream_t stream);
void launch_avgpool3s1(const PoolArgs& p, hipStream_t stream);
// head_kernel, or (outputs) head_outputs_kernel with its two optional destinations
void launch_head(const float* in, const float* w, const float* b, const ExtPtrs* ext, size_t probs_off, TensorGeom g, int K,
                 int n, bool outputs, float* pooled, float* logits, hipStream_t stream);

}  // namespace convk
}  // namespace dv

#endif  // DV_MODEL_KERNELS_H_
