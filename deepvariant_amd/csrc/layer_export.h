// layer_export.hip's interface: one activation tensor of the plan (a channel range of a concat buffer) to dense NHWC
// float32 on the device -- what dv_model_infer_outputs hands to its caller for the named Inception blocks.
#ifndef DV_LAYER_EXPORT_H_
#define DV_LAYER_EXPORT_H_

#include <hip/hip_runtime.h>

namespace dv {

// How the source buffer stores its elements (model_graph.h BufferDesc).
enum LayerExportKind {
  kExportF16 = 0,    // fp16 pieces of 8 channels
  kExportF32 = 1,    // float32 pieces of 8 channels (BufferDesc::f32)
  kExportWide = 2,   // hi fp16 groups, then lo fp16 groups; the value is float(hi) + float(lo) (BufferDesc::wide)
};

struct LayerExportArgs {
  const void* src;   // channel-blocked [n][src_groups][hp][wp][8], zero halo of `halo` around each h x w map
  int kind;          // LayerExportKind
  int n, h, w, halo, hp, wp;
  int src_groups;    // channel groups of one example in the buffer (wide: hi and lo groups together)
  int lo_groups;     // wide: how many groups further the lo piece of a group lies (the tensor's c / 8)
  int goff;          // first channel group of the view
  int groups;        // channel groups of the view: dst has groups * 8 channels
  float* dst;        // [n][h][w][groups * 8], 16-byte aligned
};

void launch_layer_export(const LayerExportArgs& a, hipStream_t stream);

}  // namespace dv

#endif  // DV_LAYER_EXPORT_H_
