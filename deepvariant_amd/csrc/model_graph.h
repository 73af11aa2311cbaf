// model_graph.cpp's interface: the classifier as a plan -- tensors, ops in launch order and the decisions of the
// planning passes (which kernel runs what, fused with what) -- and struct dv_model, which holds the plan next to the
// device memory and the captured graphs that model.hip runs it with.  Host code only; nothing here launches.
#ifndef DV_MODEL_GRAPH_H_
#define DV_MODEL_GRAPH_H_

#include <string>
#include <vector>

#include "dv_internal.h"
#include "conv_mfma.h"
#include "imgconv.h"

namespace dv {
namespace graph {

using namespace convk;

struct TensorRef {
  int buf = -1;  // index into buffers
  int h = 0, w = 0, c = 0;
};

struct BufferDesc {
  int h, w, c;  // channels = full (concat) width
  int halo = 0; // max padding any consumer needs (zero border kept in HBM)
  int min_examples = 1;  // imgconv tiles read whole groups of images: allocate at least this many
  bool f32 = false;      // float32 elements (a piece = 8 floats): tensors that no MFMA reads -- the raw 1x1 outputs of
                         // the pooled projections (input of an average pool) and the last block's outputs (input of the
                         // global pool) -- keep the accumulators' values instead of an fp16 rounding of them
  bool wide = false;     // precise mode (dv_model::precise): the tensor holds c / 8 groups of hi = fp16(x), then c / 8 groups
                         // of lo = fp16(x - hi); its consumers run their K over both with the same weights
  TensorGeom geom() const {
    return TensorGeom{h, w, halo, h + 2 * halo, w + 2 * halo, (wide ? 2 : 1) * (c / 8)};
  }
  size_t bytes_per_example() const {
    return static_cast<size_t>(h + 2 * halo) * (w + 2 * halo) * c * (f32 ? 4 : wide ? 4 : 2);
  }
};

enum OpType { kOpConv, kOpMaxPool, kOpAvgPool };

struct Op {
  OpType type;
  int in_buf, out_buf;
  int out_coff = 0;
  // conv
  int layer = -1;
  int kh = 0, kw = 0, stride = 1, pad_h = 0, pad_w = 0;
  int cin = 0, cin_real = 0, cout = 0;
  bool in_wide = false;          // the input tensor holds hi + lo pieces (BufferDesc::wide): every K chunk is multiplied
                                 // against both (ConvArgs::wide_in, conv_slab_wide)
  int ih = 0, iw = 0, oh = 0, ow = 0;
  int nb = 4;
  int n_steps = 0, n_chunks = 0;
  size_t w_off = 0;      // halfs into packed weights
  size_t shift_off = 0;  // floats into shifts
  size_t tbl_off = 0;    // int2 entries into the chunk tables
  bool raw = false;              // conv: skip shift + ReLU (applied by a later pool)
  int group_followers = 0;       // conv: the next k ops are siblings sharing this launch
  bool first_u8 = false;         // conv: reads the uint8 image directly (fused preprocess)
  bool pool_shift_relu = false;  // avgpool: add shift[c] and ReLU after averaging
  bool pool_in = false;          // 1x1 conv that max-pools (3x3, stride 2) its input on the fly
  int side_pool_partner = -1;    // 3x3 / 2 conv <-> the sibling max-pool it computes on the side (choose_side_pool)
  int avg_partner = -1;          // raw 1x1 conv <-> the average pool behind it, taken in the launch's epilogue (choose_avg_epilogue)
  int avg_tile_g = 0;            // leader of such a launch: whole maps per 256-pixel block
  bool pool_out = false;         // conv whose output is max-pooled (3x3, stride 2) before it is stored
                                 // (conv_pool_resident_kernel; oh / ow stay the conv's, the buffer is pooled)
  // Fused stem (stem.hip): the op marked stem_a / stem_b runs together with the op that
  // follows it as ONE launch; the tensor between them is never materialised.
  // imgconv.hip: whole-map tiles, both operands through LDS (set on the launch's leader op)
  int band = 0;                  // conv_mfma_kernel's row-band mode: map rows (= taps kept), 0 = off
  bool split = false;            // the LAUNCH carries W_hi + W_lo weight images (choose_split) ...
  bool split_rows = false;       // ... and this op's couts are among them (siblings of a group may not be)
  int split_tiles = 0;           // leader: leading cout tiles of the launch that hold (hi, lo) pairs
  bool v2 = false;
  int v2_g = 0;                  // images per tile
  int v2_steps = 0;              // K steps (KC channel chunks each)
  int v2_tiles = 0;              // cout tiles of nb*32
  bool stem_a = false;           // first conv (uint8 input) + conv 3x3 32->32
  bool stem_b = false;           // conv 3x3 32->64 + maxpool 3x3/2 + conv 1x1 64->80
  // chain.hip: this op and the chain_len - 1 ops behind it (1 x k / k x 1, each reading its
  // predecessor) run as ONE launch; the tensors between them live in LDS only
  int chain_len = 0;
  int chain_g = 0;               // images per tile
  int chain_tpx = 0;             // pixels per tile (192: small maps, 1-D filters; 256: 35x35 stage, 3x3 / 5x5)
  bool in_chain = false;         // a non-leading member of a chain
  // block35.hip: an Inception-A block of the 35x35 stage as ONE launch (choose_block35), placed at its heads' leader;
  // role in the block: 1 = b1 (the leader), 2 = 5x5 reducer, 3 = 3x3dbl reducer, 4 = pooled projection (raw 1x1),
  // 5 = 5x5, 6 = 3x3 64->96, 7 = 3x3 96->96, 8 = the average pool; ops 2-8 follow the leader in this order
  int b35 = 0;
  // mixed3.hip: mixed3's double-3x3 branch as ONE launch (choose_mixed3), placed at its 1x1; role in the branch:
  // 1 = 1x1 Cin->64 (the leader), 2 = 3x3 64->96, 3 = 3x3 / 2 96->96; ops 2-3 follow the leader in this order
  int m3 = 0;
};

struct LayerInfo {
  int kh, kw, cin, cout;
  int64_t param_off;
};

}  // namespace graph
}  // namespace dv

using namespace dv::graph;   // dv_model is the C ABI's global name; its members are written in these types

struct dv_model {
  int device = 0;
  dv_model_desc desc{};
  std::vector<BufferDesc> buffers;
  std::vector<Op> ops;
  std::vector<LayerInfo> layers;  // convs then dense
  int64_t n_params = 0;
  int feat_buf = -1, feat_p = 0, feat_c = 0;
  int stem_ops_end = 0, stem_out_buf = -1;
  int stem_a_grid = 512, stem_b_grid = 256;  // persistent grids of the fused stem kernels
  int n_cus = 256;
  size_t packed_halfs = 0, shift_floats = 0, tbl_entries = 0;
  std::vector<dv::DeviceBuffer> dbuf;
  dv::DeviceBuffer d_w, d_shift, d_dense_w, d_dense_b, d_tbl;
  // Blank-row skipping through the stem (round 6: on by default, DV_BLANK_SKIP=0 / dv_model_set_blank_skip turn it
  // off): tiles of conv2 / stem_b / the 3x3 80->192 whose receptive field holds only the zero rows below
  // the pile-up are copied from the all-blank image's response instead of computed -- bit-identical.
  bool blank_skip = false;        // applicable to this model and not switched off by the environment
  bool blank_enabled = true;      // dv_model_set_blank_skip
  bool blank_ready = false;       // the blank responses have been computed (after load_weights)
  int blank_conv4_op = -1;        // op index of the stem's 3x3 80->192
  dv::DeviceBuffer d_blank_thr;   // int32 [kBlankThrRows][max_batch], blank_rows_kernel + blank_need_kernel
  static constexpr int kBlankThrRows = 8;
  dv::DeviceBuffer d_blank_conv4; // the 3x3 80->192's output (pooled when its kernel pools) for the all-blank image (one example)
  dv::DeviceBuffer d_blank_c2;    // conv2's output for the all-blank image
  dv::DeviceBuffer d_blank_b;     // stem_b's (the 1x1 64->80's) output for the all-blank image
  bool blank_on() const { return blank_ready && blank_enabled; }
  // Where the consumers of the two inter-kernel tensors get the blank rows they read.  Default: stem_b
  // reads conv2's blank rows straight from the blank response (stem_a copies nothing) and copies, of its own blank
  // rows, the strip the 3x3 80->192 reads, once per example.  DV_BLANK_COPY_TILES=1 (read when the model is created):
  // both producers copy every blank tile a consumer's computed tile touches, whole -- the earlier scheme, kept for A/B.
  bool blank_copy_tiles = false;
  bool blank_read_through() const {   // the stem_a -> stem_b link: both fused (the per-layer conv2 keeps copying)
    return blank_on() && !blank_copy_tiles && ops.size() > 3 && ops[0].stem_a && ops[2].stem_b && d_blank_c2.ptr != nullptr;
  }
  // Precise mode (round 6): every fp16 tensor of the 17x17 and 8x8 stages is stored as hi + lo fp16 pieces
  // and its consumers multiply both (K doubled, the factorised-7x7 chains run per layer) -- what it takes to hold 1e-3
  // on every long-read seed, at about +40 % of the forward.  Default: on for > 8 input channels (dv_model_create).
  bool precise = false;
  bool wide_stage = false;        // build(): buffers created now belong to the wide stages
  bool loaded = false;
  std::vector<float> h_shift, h_dense_b;   // as computed by dv_model_load_weights (before any calibration)
  dv::DeviceBuffer d_ext;         // ExtPtrs: the caller's image / probability pointers of the running forward
  struct GraphEntry {
    int n;
    hipStream_t stream;
    hipGraphExec_t exec;
  };
  std::vector<GraphEntry> graphs;  // captured forwards, see dv_model_infer
  int64_t graph_captures = 0, graph_replays = 0;
  // dv_model_infer_outputs: the concat outputs Keras InceptionV3 names (mixed0 .. mixed10, and mixed9_0 / mixed9_1 =
  // the 3x3-split concats inside mixed9 and mixed10), in Keras' construction order, as (buffer, first channel,
  // channels).  Each block's output is a buffer of its own at full batch width (only the stem's tensors are
  // sub-batched), written by its own block's ops alone: after a forward of at most max_batch examples every one of
  // them still holds that forward's values.
  struct NamedView {
    std::string name;
    int buf, coff, c;
  };
  std::vector<NamedView> named_views;

  // device pointers of the plan's tensors and parameters
  template <typename T = _Float16>
  T* buf_ptr(int buf) const { return static_cast<T*>(dbuf[buf].ptr); }
  const _Float16* w_ptr(const Op& op) const { return static_cast<const _Float16*>(d_w.ptr) + op.w_off; }
  const float* shift_ptr(const Op& op) const { return static_cast<const float*>(d_shift.ptr) + op.shift_off; }
  const int* blank_thr(int row) const { return static_cast<const int*>(d_blank_thr.ptr) + row * desc.max_batch; }

  // ---- builder and planning passes (model_graph.cpp) -------------------------
  int new_buffer(int h, int w, int c);
  static int pick_nb(int cout);
  TensorRef conv(TensorRef x, int cout, int kh, int kw, int stride = 1, bool same = true,
                 int dst_buf = -1, int dst_coff = 0, int cin_real = -1);
  TensorRef full(int buf) const;
  void pooled_projection(TensorRef x, int cout, int dst_buf, int dst_coff);
  TensorRef pool(OpType type, TensorRef x, int dst_buf = -1, int dst_coff = 0);
  void group_siblings();
  dv::ImgConvArgs imgconv_geometry(const Op& op, int g) const;
  void choose_imgconv();
  void choose_band();
  void choose_side_pool();
  void choose_split();
  void choose_avg_epilogue();
  void choose_chains();
  void choose_block35();
  void choose_mixed3();
  void build();
  // the flat corrections vector of dv_model_calibrate (layer order, cout values each, no padding): the offset into
  // the shift array of every value's channel
  std::vector<size_t> correction_shift_offsets() const;
};

#endif  // DV_MODEL_GRAPH_H_
