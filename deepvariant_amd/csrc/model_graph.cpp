// model_graph.cpp -- builds the Inception-v3 plan of struct dv_model (model_graph.h): the op list in tf_keras'
// construction order, then the planning passes that decide which kernel runs which ops.
#include <algorithm>
#include <cstdlib>

#include "model_graph.h"
#include "model_kernels.h"
#include "block35.h"
#include "mixed3.h"
#include "chain.h"
#include "stem_fused.h"

int dv_model::new_buffer(int h, int w, int c) {
  buffers.push_back({h, w, c, 0});
  buffers.back().wide = precise && wide_stage;
  return static_cast<int>(buffers.size()) - 1;
}
int dv_model::pick_nb(int cout) {
  // DV_NB6: 192-cout single tiles for 129..192-cout layers (see launch_conv6)
  static const bool nb6 = getenv("DV_NB6") != nullptr && atoi(getenv("DV_NB6")) != 0;
  if (nb6 && cout > 128 && cout <= 192) return 6;
  // Cost of a cout tiling ~ tiles x (nb MFMA columns + 1 pixel-fragment stream): a
  // 160-wide layer is cheaper as 2 x 96 (one sixth padding) than as 5 x 32, whose
  // blocks re-load every pixel fragment five times.  Ties -> less padding.
  int best = 4, best_cost = 1 << 30, best_waste = 1 << 30;
  for (int nb = 4; nb >= 1; --nb) {
    const int bn = nb * 32;
    const int tiles = (cout + bn - 1) / bn;
    const int cost = tiles * (nb + 1), waste = tiles * bn - cout;
    if (cost < best_cost || (cost == best_cost && waste < best_waste)) {
      best_cost = cost;
      best_waste = waste;
      best = nb;
    }
  }
  return best;
}
TensorRef dv_model::conv(TensorRef x, int cout, int kh, int kw, int stride, bool same, int dst_buf, int dst_coff,
                        int cin_real) {
  Op op;
  op.type = kOpConv;
  op.kh = kh;
  op.kw = kw;
  op.stride = stride;
  op.pad_h = same ? (kh - 1) / 2 : 0;
  op.pad_w = same ? (kw - 1) / 2 : 0;
  op.in_wide = buffers[x.buf].wide;
  op.cin = x.c;
  op.cin_real = cin_real < 0 ? x.c : cin_real;
  op.cout = cout;
  op.ih = x.h;
  op.iw = x.w;
  op.oh = (x.h + 2 * op.pad_h - kh) / stride + 1;
  op.ow = (x.w + 2 * op.pad_w - kw) / stride + 1;
  op.in_buf = x.buf;
  if (dst_buf < 0) {
    dst_buf = new_buffer(op.oh, op.ow, cout);
    dst_coff = 0;
  }
  op.out_buf = dst_buf;
  op.out_coff = dst_coff;
  op.nb = pick_nb(cout);
  op.n_chunks = kh * kw * (op.cin / kChunk);
  op.n_steps = (op.n_chunks + kSlabChunks - 1) / kSlabChunks;  // weight slabs
  op.shift_off = shift_floats;
  shift_floats += cout + 128;  // padded: the epilogue reads whole 32-cout tiles
  op.tbl_off = tbl_entries;
  tbl_entries += op.n_chunks;
  op.layer = static_cast<int>(layers.size());
  layers.push_back({kh, kw, op.cin_real, cout, n_params});
  n_params += static_cast<int64_t>(kh) * kw * op.cin_real * cout + 3LL * cout;
  ops.push_back(op);
  TensorRef out;
  out.buf = dst_buf;
  out.h = op.oh;
  out.w = op.ow;
  out.c = cout;  // view width; the consumer of a concat reads the full buffer
  return out;
}
TensorRef dv_model::full(int buf) const {
  TensorRef t;
  t.buf = buf;
  t.h = buffers[buf].h;
  t.w = buffers[buf].w;
  t.c = buffers[buf].c;
  return t;
}
// AveragePooling2D(3,1,'same') -> conv 1x1 -> BN -> ReLU, evaluated as
// conv 1x1 (raw) -> average pool -> +shift -> ReLU.  A 1x1 convolution is a
// per-pixel linear map, so it commutes with the (per-pixel-normalised)
// average; pooling the Cout (32..192) projected channels instead of the Cin
// (192..2048) input channels moves 4-10x fewer bytes.
void dv_model::pooled_projection(TensorRef x, int cout, int dst_buf, int dst_coff) {
  TensorRef raw = conv(x, cout, 1, 1);
  ops.back().raw = true;                   // no shift, no ReLU in the conv epilogue
  buffers[raw.buf].f32 = true;             // averaged in float32 (conv_epilogue_avg / avgpool3s1_kernel)
  buffers[raw.buf].wide = false;
  const size_t shift_off = ops.back().shift_off;
  pool(kOpAvgPool, raw, dst_buf, dst_coff);
  ops.back().shift_off = shift_off;        // applied after the pool
  ops.back().pool_shift_relu = true;
}
TensorRef dv_model::pool(OpType type, TensorRef x, int dst_buf, int dst_coff) {
  Op op;
  op.type = type;
  op.in_buf = x.buf;
  op.ih = x.h;
  op.iw = x.w;
  op.cin = x.c;
  op.cout = x.c;
  if (type == kOpMaxPool) {
    op.oh = (x.h - 3) / 2 + 1;
    op.ow = (x.w - 3) / 2 + 1;
  } else {
    op.oh = x.h;
    op.ow = x.w;
  }
  if (dst_buf < 0) {
    dst_buf = new_buffer(op.oh, op.ow, x.c);
    dst_coff = 0;
  }
  op.out_buf = dst_buf;
  op.out_coff = dst_coff;
  ops.push_back(op);
  TensorRef out;
  out.buf = dst_buf;
  out.h = op.oh;
  out.w = op.ow;
  out.c = x.c;
  return out;
}

// Sibling 1x1 convolutions of an Inception block read the same tensor.  Hoist
// them next to the first one and mark them as ONE launch (ConvArgs::br): the
// input is then fetched from HBM once and re-read from L2 by the siblings.
// Layer (= weight) order is untouched -- only the execution order changes,
// which is legal because every hoisted op depends on the shared input only.
void dv_model::group_siblings() {
  static const bool off = getenv("DV_NO_GROUPING") != nullptr;  // tuning knob
  if (off) return;
  for (size_t i = 0; i < ops.size(); ++i) {
    Op& lead = ops[i];
    if (lead.type != kOpConv || lead.kh != 1 || lead.kw != 1 || lead.stride != 1) continue;
    std::vector<size_t> sib;
    for (size_t j = i + 1; j < ops.size() && j < i + 16 && sib.size() + 1 < kMaxBranches; ++j) {
      const Op& o = ops[j];
      if (o.type == kOpConv && o.kh == 1 && o.kw == 1 && o.stride == 1 &&
          o.in_buf == lead.in_buf) {
        sib.push_back(j);
      }
    }
    if (sib.empty()) continue;
    // tile width over the concatenated cout space (32-cout subtiles), same cost model
    // as pick_nb: tiles x (nb MFMA columns + 1 pixel-fragment stream)
    int subs = (lead.cout + 31) / 32;
    for (size_t j : sib) subs += (ops[j].cout + 31) / 32;
    // 128-cout tiles (<4,2>, two blocks per CU since round 2) for every grouped head from 7
    // subtiles up: the 35x35 heads (7-8 subtiles) then take 2 tiles instead of 3 -- the input is
    // re-read twice instead of three times and no padding subtile is multiplied: 495 / 556 / 583
    // -> 448 / 522 / 567 us, +0.8 % end to end (round 4, tools/r4_run.sh ab:DV_HEADS_NB4_MIN=7;
    // round 2 had measured 96-cout tiles faster when <4,2> still ran one block per CU).
    // heads that max-pool their input on the fly (DV_NO_POOL2_IN_CONV): ONE tile of all 7 subtiles, so
    // that every 3x3 window is fetched and reduced once
    static const int nb4_min = getenv("DV_HEADS_NB4_MIN") ? atoi(getenv("DV_HEADS_NB4_MIN")) : 7;  // tuning knob
    const int nb = lead.pool_in && subs == 7 && getenv("DV_POOL2_NB3") == nullptr ? 7 : subs >= nb4_min ? 4 : 3;
    std::vector<Op> moved;
    for (size_t j : sib) moved.push_back(ops[j]);
    for (size_t k = sib.size(); k-- > 0;) ops.erase(ops.begin() + sib[k]);
    ops.insert(ops.begin() + i + 1, moved.begin(), moved.end());
    ops[i].group_followers = static_cast<int>(moved.size());
    for (size_t k = 0; k <= moved.size(); ++k) ops[i + k].nb = nb;
    i += moved.size();
  }
}

// Tile geometry of an imgconv launch for `g` images per tile.
dv::ImgConvArgs dv_model::imgconv_geometry(const Op& op, int g) const {
  dv::ImgConvArgs a{};
  const int kc = dv::imgconv_kc(op.kh, op.kw);
  a.G = g;
  a.P = op.oh * op.ow;
  a.RP = op.oh + op.kh - 1;
  a.CP = op.ow + op.kw - 1;
  a.plane_pieces = g * a.RP * a.CP;
  a.act_pieces = kc * 2 * a.plane_pieces;
  a.act_slab_bytes = (a.act_pieces * 16 + 1023) / 1024 * 1024;
  a.n_steps = (op.cin / kChunk + kc - 1) / kc;
  a.c.KH = op.kh;
  a.c.KW = op.kw;
  return a;
}
// Stride-1 convolutions on small maps run in imgconv.hip (whole-map tiles, both operands
// in LDS) when a tile of G images fills at least 3/4 of the 512-pixel tile and the double
// buffered slabs fit the CU's LDS.  DV_NO_IMGCONV keeps conv_mfma_kernel for all of them.
void dv_model::choose_imgconv() {
  if (getenv("DV_NO_IMGCONV") != nullptr) return;
  const char* only = getenv("DV_IMGCONV_TAPS");  // tuning knob: e.g. "9,25" = only 3x3 and 5x5
  for (size_t i = 0; i < ops.size(); ++i) {
    Op& op = ops[i];
    const int followers = op.type == kOpConv ? op.group_followers : 0;
    bool f32_out = false;   // float32 outputs go through conv_epilogue only
    for (int gi = 0; gi <= followers; ++gi) f32_out = f32_out || buffers[ops[i + gi].out_buf].f32;
    if (op.type == kOpConv && !f32_out && !op.in_wide && !buffers[op.out_buf].wide && !op.first_u8 && !op.pool_in && !op.pool_out && !op.stem_a && !op.stem_b &&
        op.chain_len == 0 && !op.in_chain &&
        !(i > 0 && (ops[i - 1].stem_a || ops[i - 1].stem_b)) && op.stride == 1 &&
        dv::imgconv_supported(op.kh, op.kw, op.nb) && op.oh * op.ow <= 512) {
      // 1x1 layers have no taps to share a patch between: the DMA count equals
      // conv_mfma_kernel's fragment loads and the LDS round trip only costs (measured
      // 0.75x); they stay on conv_mfma_kernel unless DV_IMGCONV_1X1 is set.
      bool wanted = op.kh * op.kw > 1 || getenv("DV_IMGCONV_1X1") != nullptr;
      // Measured at 8 K examples: +10..30 % on the 10x25 maps (3x3, 5x5), no gain on the
      // 4x12 maps (7-tap filters) and a loss on 1x5 (the patch is mostly halo): only maps
      // of at least DV_IMGCONV_MINP pixels (default 100) take this path.
      static const int min_p = getenv("DV_IMGCONV_MINP") ? atoi(getenv("DV_IMGCONV_MINP")) : 100;
      if (op.oh * op.ow < min_p) wanted = false;
      if (only != nullptr) {
        wanted = false;
        for (const char* q = only; *q;) {
          if (atoi(q) == op.kh * op.kw) wanted = true;
          while (*q && *q != ',') ++q;
          if (*q == ',') ++q;
        }
      }
      int subs = 0;
      for (int gi = 0; gi <= followers; ++gi) subs += (ops[i + gi].cout + 31) / 32;
      const int P = op.oh * op.ow;
      for (int g = 512 / P; wanted && g >= 1 && g * P >= 384; --g) {
        const dv::ImgConvArgs a = imgconv_geometry(op, g);
        if (a.act_slab_bytes > 64 * 1024 || dv::imgconv_lds_bytes(a, op.nb) > 160 * 1024) continue;
        op.v2 = true;
        op.v2_g = g;
        op.v2_steps = a.n_steps;
        op.v2_tiles = (subs + op.nb - 1) / op.nb;
        buffers[op.in_buf].min_examples = std::max(buffers[op.in_buf].min_examples, g);
        break;
      }
    }
    i += followers;
  }
}

// Filters taller than the map: conv_mfma_kernel's row-band mode (ConvArgs::band) skips the
// taps that only ever see the zero halo.  At 100 x 221 inputs these are the 7x1 layers of
// the 4 x 12 maps (4 of 7 taps remain) and the 3x3 / 3x1 layers of the 1 x 5 maps (the
// middle row only).  Needs every output row to see ALL map rows (so each row keeps exactly
// H taps): H <= min(pad, KH - 1 - pad) + 1.  DV_NO_BAND keeps the full filters.
void dv_model::choose_band() {
  if (getenv("DV_NO_BAND") != nullptr) return;
  for (Op& op : ops) {
    if (op.type != kOpConv || op.first_u8 || op.pool_in || op.pool_out || op.stem_a || op.stem_b || op.v2 ||
        op.chain_len != 0 || op.in_chain || op.group_followers != 0 || op.stride != 1 || op.kh <= 1 || op.oh != op.ih) {
      continue;
    }
    const int h = op.ih;
    if (h >= op.kh || h > std::min(op.pad_h, op.kh - 1 - op.pad_h) + 1 || op.ow < 5) continue;
    bool follower = false;  // a sibling inside another op's launch keeps that launch's geometry
    for (const Op& lead : ops) {
      if (lead.type == kOpConv && lead.group_followers > 0 && &op > &lead &&
          &op <= &lead + lead.group_followers) {
        follower = true;
      }
    }
    if (follower) continue;
    op.band = h;
    // the row-band 7x1 layers are the one shape where a single 192-cout tile (launch_conv6)
    // measured faster than two 96-cout tiles (-5...-13 %); DV_NO_BAND_NB6 keeps two tiles
    if (op.cout > 128 && op.cout <= 192 && op.nb == 3 && getenv("DV_NO_BAND_NB6") == nullptr) op.nb = 6;
    op.n_chunks = h * op.kw * (op.cin / kChunk);
    op.n_steps = (op.n_chunks + kSlabChunks - 1) / kSlabChunks;
  }
}

// The reduction block mixed3 runs MaxPooling2D(3, 2) next to a 3x3 / stride-2 'valid' convolution of the
// SAME tensor: per 16-channel chunk the convolution's nine tap fragments are exactly the pool's
// window pieces, so the workgroups of its cout tile 0 take the maximum on the side (SidePool) and the
// pool's own launch (0.27 ms, a full re-read of the block input) disappears.  mixed8's pool has no
// such sibling (its stride-2 convolutions read the 1x1 outputs).  DV_NO_SIDE_POOL keeps the launch.
void dv_model::choose_side_pool() {
  if (getenv("DV_NO_SIDE_POOL") != nullptr) return;
  for (size_t pi = 0; pi < ops.size(); ++pi) {
    Op& pl = ops[pi];
    if (pl.type != kOpMaxPool) continue;
    for (size_t ci = 0; ci < ops.size(); ++ci) {
      Op& cv = ops[ci];
      if (cv.type != kOpConv || cv.in_buf != pl.in_buf || cv.stride != 2 || cv.kh != 3 || cv.kw != 3 ||
          cv.pad_h != 0 || cv.pad_w != 0 || cv.nb != 4 || cv.group_followers != 0 || cv.first_u8 || cv.pool_in ||
          cv.pool_out || cv.stem_a || cv.stem_b || cv.v2 || cv.band || cv.split || cv.chain_len != 0 || cv.in_chain ||
          cv.raw || cv.cin != pl.cin || cv.cin % kChunk != 0 || cv.cin != buffers[cv.in_buf].c ||
          cv.oh != pl.oh || cv.ow != pl.ow || cv.side_pool_partner >= 0) {
        continue;
      }
      cv.side_pool_partner = static_cast<int>(pi);
      pl.side_pool_partner = static_cast<int>(ci);
      break;
    }
  }
}

// Split weights (HISTORY.md 15).  The fp16 rounding of the BN-folded weights is ~3/4 of the variance
// of the CNN's error against the fp32 reference (tools/r4_layer_sensitivity.py: a flat budget, no
// layer above 3.5 %), and it is the half that a kernel can remove without touching its pixel
// operand.  Selected conv_mfma_kernel launches therefore carry W as W_hi + W_lo (both fp16,
// W_lo = fp16(W - W_hi)): the packed image holds every K chunk twice and the kernel multiplies the
// same pixel fragment by both -- products are exact, the sum is fp32, so those layers compute
// with 22-bit weights.  Which: in the 17x17 blocks the two 1x1 layers whose output is block
// output (b1, pooled projection -- the leading cout tiles of the grouped heads launch), in
// mixed8..10 every 1x1 / 3-tap / 3x3 layer.  Measured on 2048 pileups x seeds 17 / 29
// (profiles/r04_precision_sweep.txt): max |dp| 1.15e-3 / 1.55e-3 without, 7.8e-4 / 8.6e-4 with.
// DV_SPLIT_FROM=<layer> (construction order; 94 = none, 0 = every conv_mfma layer) and
// DV_SPLIT_LAYERS=<list> override the set for A/B runs.
void dv_model::choose_split() {
  const int first_layer_env = getenv("DV_SPLIT_FROM") ? atoi(getenv("DV_SPLIT_FROM")) : -1;  // per model (tests)
  // mixed4 (the 17x17 stage) starts at conv layer 30 of the 94 (5 stem + 3 x 7 + 4), mixed8 at 70.
  // The default set is a property of the LAYER, not of the kernel that happens to run it: 1x1
  // layers from mixed4 on, 3-tap and 3x3 layers from mixed8 on -- never the factorised-7x7
  // layers, which run as fused chains (and must give the same bits when DV_NO_CHAIN unfuses them).
  const char* list_env = getenv("DV_SPLIT_LAYERS");   // experiments: an explicit comma list of layers
  const char* split_default_env = getenv("DV_SPLIT_DEFAULT");   // 1 = the round-4 default set below
  auto wanted = [&](const Op& o) {
    if (list_env != nullptr) {
      for (const char* q = list_env; *q;) {
        if (atoi(q) == o.layer) return true;
        while (*q && *q != ',') ++q;
        if (*q == ',') ++q;
      }
      return false;
    }
    if (first_layer_env >= 0) return o.layer >= first_layer_env;
    // Round 5: OFF unless DV_SPLIT_DEFAULT=1.  The shift calibration (dv_model_calibrate, calib.hip) removes
    // the per-channel mean of the weight AND activation rounding at no run-time cost and measures better on
    // every held-out seed at N = 65,536 than this set did (profiles/r05_cnn_tail.txt: max |dp| 8.6e-4 /
    // 2.9e-4 / 7.2e-4 calibrated without split weights against 1.01e-3 / 4.2e-4 / 9.1e-4 with them).
    if (split_default_env == nullptr || atoi(split_default_env) == 0) return false;
    // 17x17 stage: the two 1x1 layers of a block whose output IS block output -- the b1 branch
    // (written into the concat buffer) and the pooled projection (raw) -- not the heads of the
    // factorised-7x7 branches (measured: profiles/r04_precision_sweep.txt)
    if (o.kh * o.kw == 1 && o.layer >= 30 && o.layer < 70) return o.raw || buffers[o.out_buf].c > o.cout;
    return o.layer >= 70 && std::max(o.kh, o.kw) <= 3;
  };
  for (size_t i = 0; i < ops.size(); ++i) {
    Op& op = ops[i];
    if (op.type != kOpConv) continue;
    const int followers = op.group_followers;
    const bool eligible = !op.first_u8 && !op.pool_in && !op.pool_out && !op.stem_a && !op.stem_b && !op.v2 &&
                          op.chain_len == 0 && !op.in_chain && !(i > 0 && (ops[i - 1].stem_a || ops[i - 1].stem_b)) &&
                          op.nb <= 4 && static_cast<int>(i) != blank_conv4_op && !op.in_wide;
    int n_wanted = 0;
    for (int gi = 0; gi <= followers; ++gi) n_wanted += wanted(ops[i + gi]) ? 1 : 0;
    if (eligible && n_wanted > 0) {
      // Siblings of which only some are wanted: the wanted ones go to the front of the launch's
      // cout space, and if they fill whole cout tiles only those tiles carry (hi, lo) pairs
      // (ConvArgs::split_tiles); otherwise -- or when the leader itself is not wanted -- the whole
      // launch is split.
      int split_subs = 0, all_subs = 0;
      bool partial = n_wanted <= followers && wanted(op);
      if (partial) {
        std::stable_partition(ops.begin() + i + 1, ops.begin() + i + 1 + followers,
                              [&](const Op& o) { return wanted(o); });
        for (int gi = 0; gi <= followers; ++gi) {
          if (wanted(ops[i + gi])) split_subs += (ops[i + gi].cout + 31) / 32;
        }
        partial = split_subs % ops[i].nb == 0;
      }
      for (int gi = 0; gi <= followers; ++gi) all_subs += (ops[i + gi].cout + 31) / 32;
      Op& lead = ops[i];   // (stable_partition leaves the leader in place)
      lead.split_tiles = partial ? split_subs / lead.nb : (all_subs + lead.nb - 1) / lead.nb;
      for (int gi = 0; gi <= followers; ++gi) {
        Op& o = ops[i + gi];
        o.split = true;
        o.split_rows = !partial || wanted(o);
        o.n_chunks *= 2;
        o.n_steps = (o.n_chunks + kSlabChunks - 1) / kSlabChunks;
      }
    }
    i += followers;
  }
}

// Pooled projections (conv 1x1 raw -> AveragePooling2D(3, 1, 'same') -> shift -> ReLU): when the heads
// launch that holds the raw 1x1 runs 128-cout tiles and whole maps fill a 256-pixel block to >= 90 %
// (10x25 = 250 pixels: 1 map; 4x12: 5 maps; 1x5: 51 maps), its blocks are laid over whole maps
// (ConvArgs::tile_g) and the pool happens in the epilogue (conv_epilogue_avg): the raw tensor is never
// written and the avg-pool launch is gone.  Not for split launches (their own kernel variants), not for
// heads that pool their input on the fly.  DV_NO_AVG_EPI keeps conv -> avgpool3s1_kernel (same bits).
void dv_model::choose_avg_epilogue() {
  if (getenv("DV_NO_AVG_EPI") != nullptr) return;
  const int min_g = getenv("DV_AVG_EPI_MIN_G") ? atoi(getenv("DV_AVG_EPI_MIN_G")) : 1;   // tuning knob: whole maps per block
  // whole maps must fill this share of the 256 pixel slots (percent).  Round 5: 90 (the ILLUMINA30 maps: 98 / 94 / 100 %);
  // round 6: 85, which takes in ONT_R104's 10x22 maps (86 %) -- PACBIO's 10x16 (62 %) keeps the separate pool
  const int min_fill = getenv("DV_AVG_EPI_MIN_FILL") ? atoi(getenv("DV_AVG_EPI_MIN_FILL")) : 85;
  for (size_t i = 0; i < ops.size(); ++i) {
    Op& lead = ops[i];
    if (lead.type != kOpConv) continue;
    const int followers = lead.group_followers;
    const int px = lead.oh * lead.ow;
    const bool ok = lead.kh == 1 && lead.kw == 1 && lead.stride == 1 && lead.nb == 4 && !lead.split && !lead.pool_in &&
                    !lead.pool_out && !lead.v2 && !lead.band && lead.chain_len == 0 && !lead.in_chain &&
                    !lead.first_u8 && !lead.stem_a && !lead.stem_b && px >= 5 && px <= 256 &&
                    (256 / px) * px * 100 >= 256 * min_fill && 256 / px >= min_g;
    if (ok) {
      for (int gi = 0; gi <= followers; ++gi) {
        Op& c = ops[i + gi];
        if (!c.raw) continue;
        for (size_t j = i + followers + 1; j < ops.size(); ++j) {
          Op& pl = ops[j];
          if (pl.type == kOpAvgPool && pl.in_buf == c.out_buf && pl.pool_shift_relu && pl.avg_partner < 0) {
            c.avg_partner = static_cast<int>(j);
            pl.avg_partner = static_cast<int>(i + gi);
            lead.avg_tile_g = 256 / px;
            break;
          }
        }
      }
    }
    i += followers;
  }
}

// Chains of stride-1 'same' convolutions in which every layer reads only its predecessor run in
// chain.hip, intermediates in LDS:
//   * maps of <= 96 pixels (the 17x17 stage at WGS width), 1 x k / k x 1 filters: the factorised
//     7x7 branches of mixed4..mixed8 -- G whole maps in a 192-pixel tile, two layers or more;
//   * maps of 97..256 pixels (the 35x35 stage), 3x3 / 5x5 filters with 64..96 couts: the
//     3x3 -> 3x3 branch of mixed0..2, and the single 5x5 / 3x3 layers next to it (one-layer
//     "chains": both operands from LDS, loader waves) -- one or two maps in a 256-pixel tile.
// A tile must be at least two thirds full and the activation tile plus two weight slabs must
// fit the CU's LDS.  DV_NO_CHAIN keeps the per-layer kernels; DV_NO_CHAIN2D only those of the
// 35x35 stage; DV_CHAIN2D_MIN_LEN=1 also takes its single layers from imgconv.
void dv_model::choose_chains() {
  if (getenv("DV_NO_CHAIN") != nullptr) return;
  const bool no_2d = getenv("DV_NO_CHAIN2D") != nullptr;
  // measured (profiles/r03_chain2d_ab.txt): the 3x3 -> 3x3 pairs gain 6 % over two imgconv launches;
  // single layers lose 5-30 % to imgconv (its tiles of two maps pipeline the next tile's input, a
  // one-layer chain exposes it), so they stay there unless DV_CHAIN2D_MIN_LEN=1
  const int min_len_2d = getenv("DV_CHAIN2D_MIN_LEN") ? atoi(getenv("DV_CHAIN2D_MIN_LEN")) : 2;
  std::vector<int> readers(buffers.size(), 0);
  for (const Op& o : ops) readers[o.in_buf]++;
  auto plain = [&](const Op& o) {
    return o.type == kOpConv && !buffers[o.out_buf].f32 && !o.in_wide && !buffers[o.out_buf].wide && o.stride == 1 && (o.kh & 1) && (o.kw & 1) && o.kh * o.kw > 1 &&
           o.pad_h == (o.kh - 1) / 2 && o.pad_w == (o.kw - 1) / 2 && o.group_followers == 0 &&
           !o.first_u8 && !o.pool_in && !o.pool_out && !o.raw && !o.stem_a && !o.stem_b && o.cin % kChunk == 0 &&
           o.cin == o.cin_real && o.oh == o.ih && o.ow == o.iw;
  };
  auto one_d = [&](const Op& o) {
    return plain(o) && (o.kh == 1) != (o.kw == 1) && std::max(o.kh, o.kw) <= dv::kChainMaxTaps;
  };
  auto two_d = [&](const Op& o) {
    const int subs = (o.cout + 31) / 32;
    return plain(o) && ((o.kh == 3 && o.kw == 3) || (o.kh == 5 && o.kw == 5)) && subs >= 2 && subs <= 3;
  };
  for (size_t i = 0; i < ops.size(); ++i) {
    const int P = ops[i].oh * ops[i].ow;
    const bool big = P > dv::kChainTilePx / 2;
    if (big ? (no_2d || P > dv::kChainTilePxBig || !two_d(ops[i])) : !one_d(ops[i])) continue;
    auto member = [&](const Op& o) { return big ? two_d(o) : one_d(o); };
    size_t len = 1;
    while (i + len < ops.size() && len < static_cast<size_t>(dv::kChainMaxLayers)) {
      const Op& prev = ops[i + len - 1];
      const Op& next = ops[i + len];
      if (!member(next) || next.in_buf != prev.out_buf || prev.out_coff != 0 || readers[prev.out_buf] != 1 ||
          prev.cout % 32 != 0 || buffers[prev.out_buf].c != prev.cout) {
        break;
      }
      ++len;
    }
    if (static_cast<int>(len) < (big ? min_len_2d : 2)) continue;
    const int tpx = big ? dv::kChainTilePxBig : dv::kChainTilePx;
    const int g = tpx / P;
    if (g * P < tpx * 2 / 3) continue;
    size_t act = 0, slot = 0;
    bool fits = true;
    for (size_t k = 0; k < len; ++k) {
      const Op& o = ops[i + k];
      act = std::max(act, static_cast<size_t>(o.cin / 8) * tpx * 16);
      slot = std::max(slot, static_cast<size_t>(o.kh * o.kw) * 2 * ((o.cout + 31) / 32 * 32) * 16);
      // the 192-pixel shape halves the couts between two waves: 4..6 subtiles of 32
      if (!big) fits = fits && (o.cout + 31) / 32 >= 4 && (o.cout + 31) / 32 <= 6;
    }
    if (!fits || act + 2 * slot + 16 > 160 * 1024) continue;
    ops[i].chain_len = static_cast<int>(len);
    ops[i].chain_g = g;
    ops[i].chain_tpx = tpx;
    for (size_t k = 1; k < len; ++k) {
      ops[i + k].in_chain = true;
      const int c = ops[i + k - 1].cout;
      buffers[ops[i + k].in_buf] = {1, 1, c, 0};   // LDS only
    }
    buffers[ops[i].in_buf].min_examples = std::max(buffers[ops[i].in_buf].min_examples, g);
    i += len - 1;
  }
}

// Inception-A blocks of the 35x35 stage (mixed0..2) as ONE launch each (block35.hip): the grouped 1x1 heads, their
// average pool, the 5x5 and the 3x3 -> 3x3 pair on tiles of one whole map, the reducers and the 3x3 intermediate
// in LDS only.  Recognises the pattern build() emits after grouping -- b1 (leader) + 5x5 reducer + 3x3 reducer +
// pooled projection, then 5x5, 3x3, 3x3, avg pool -- and declines, keeping the per-layer launches, for wide / split
// ops (precise mode), heads that max-pool their input (DV_NO_POOL2_IN_CONV) and maps of more than 256 pixels.
// DV_NO_BLOCK35 keeps the per-layer launches; DV_NO_CHAIN implies it.
void dv_model::choose_block35() {
  if (getenv("DV_NO_BLOCK35") != nullptr || getenv("DV_NO_CHAIN") != nullptr) return;
  std::vector<int> readers(buffers.size(), 0);
  for (const Op& o : ops) readers[o.in_buf]++;
  for (size_t i = 0; i + 7 < ops.size(); ++i) {
    const Op &b1 = ops[i], &r5 = ops[i + 1], &r3 = ops[i + 2], &pj = ops[i + 3];
    const Op &c5 = ops[i + 4], &c3a = ops[i + 5], &c3b = ops[i + 6], &ap = ops[i + 7];
    const int P = b1.oh * b1.ow;
    auto plain = [&](const Op& o) {
      return o.type == kOpConv && o.stride == 1 && !o.split && !o.in_wide && !buffers[o.out_buf].wide && !o.pool_in &&
             !o.pool_out && !o.first_u8 && !o.stem_a && !o.stem_b && !o.band && o.cin % kChunk == 0 &&
             o.cin == o.cin_real && o.oh == b1.oh && o.ow == b1.ow && o.ih == b1.oh && o.iw == b1.ow && o.b35 == 0;
    };
    auto head = [&](const Op& o, int cout) {
      return plain(o) && o.kh == 1 && o.kw == 1 && o.in_buf == b1.in_buf && o.cout == cout;
    };
    auto same = [&](const Op& o, int k, int in_buf, int cin, int cout) {
      return plain(o) && o.kh == k && o.kw == k && o.pad_h == k / 2 && o.pad_w == k / 2 && o.in_buf == in_buf &&
             o.cin == cin && o.cout == cout && !o.raw;
    };
    const int O = b1.out_buf;
    const bool ok =
        b1.group_followers == 3 && P <= dv::kBlock35TilePx && head(b1, dv::kBlock35B1) && !b1.raw &&
        head(r5, dv::kBlock35Red5) && !r5.raw && head(r3, dv::kBlock35Red3) && !r3.raw &&
        head(pj, pj.cout) && pj.raw && (pj.cout == 32 || pj.cout == 64) &&
        same(c5, 5, r5.out_buf, dv::kBlock35Red5, dv::kBlock35Out5) &&
        same(c3a, 3, r3.out_buf, dv::kBlock35Red3, dv::kBlock35Out3) &&
        same(c3b, 3, c3a.out_buf, dv::kBlock35Out3, dv::kBlock35Out3) &&
        ap.type == kOpAvgPool && ap.in_buf == pj.out_buf && ap.pool_shift_relu &&
        readers[r5.out_buf] == 1 && readers[r3.out_buf] == 1 && readers[c3a.out_buf] == 1 && readers[pj.out_buf] == 1 &&
        c5.out_buf == O && c3b.out_buf == O && ap.out_buf == O && !buffers[O].f32 && !buffers[O].wide &&
        b1.out_coff % 8 == 0 && c5.out_coff % 8 == 0 && c3b.out_coff % 8 == 0 && ap.out_coff % 8 == 0;
    if (!ok) continue;
    for (int k = 0; k < 8; ++k) {
      Op& o = ops[i + k];
      o.b35 = k + 1;
      o.chain_len = 0;
      o.in_chain = false;
      o.v2 = false;
      o.avg_partner = -1;
      o.avg_tile_g = 0;
    }
    for (int b : {r5.out_buf, r3.out_buf, c3a.out_buf, pj.out_buf}) {   // LDS only (the projection stays float32)
      const bool f32 = buffers[b].f32;
      buffers[b] = {1, 1, buffers[b].c, 0};
      buffers[b].f32 = f32;
    }
    i += 7;
  }
}

// mixed3's double-3x3 branch as ONE launch (mixed3.hip): a 1x1 Cin->64 that reads a full concat buffer, the 3x3 'same'
// 64->96 that alone reads it and the 3x3 / 2 'valid' 96->96 that alone reads that, on tiles of one whole input map
// with both intermediates in LDS only.  Declines, keeping the three launches (conv_mfma, imgconv, conv_mfma), for
// wide / split / float32 / pool_in / pool_out / band / grouped ops, maps of more than 256 pixels or smaller than 3x3,
// and anything else it does not recognise.  DV_NO_MIXED3_FUSE keeps the three launches; DV_NO_CHAIN implies it.
void dv_model::choose_mixed3() {
  if (getenv("DV_NO_MIXED3_FUSE") != nullptr || getenv("DV_NO_CHAIN") != nullptr) return;
  std::vector<int> readers(buffers.size(), 0);
  for (const Op& o : ops) readers[o.in_buf]++;
  for (size_t i = 0; i + 2 < ops.size(); ++i) {
    const Op &a = ops[i], &b = ops[i + 1], &c = ops[i + 2];
    auto plain = [&](const Op& o) {
      return o.type == kOpConv && !o.split && !o.in_wide && !buffers[o.out_buf].wide && !buffers[o.out_buf].f32 &&
             !o.pool_in && !o.pool_out && !o.first_u8 && !o.stem_a && !o.stem_b && !o.band && !o.raw &&
             o.group_followers == 0 && o.chain_len == 0 && !o.in_chain && o.b35 == 0 && o.m3 == 0 &&
             o.side_pool_partner < 0 && o.avg_partner < 0 && o.cin % kChunk == 0 && o.cin == o.cin_real;
    };
    bool follower = false;   // a sibling inside another op's grouped launch
    for (size_t j = 0; j < i; ++j) follower = follower || (ops[j].type == kOpConv && j + ops[j].group_followers >= i);
    const bool ok =
        !follower && plain(a) && plain(b) && plain(c) &&
        a.kh == 1 && a.kw == 1 && a.stride == 1 && a.cout == dv::kMixed3Red && a.cin == buffers[a.in_buf].c &&
        a.cin / kChunk >= dv::mixed3_min_chunks() && a.out_coff == 0 && buffers[a.out_buf].c == a.cout &&
        readers[a.out_buf] == 1 &&
        b.in_buf == a.out_buf && b.kh == 3 && b.kw == 3 && b.stride == 1 && b.pad_h == 1 && b.pad_w == 1 &&
        b.cin == dv::kMixed3Red && b.cout == dv::kMixed3Mid && b.out_coff == 0 && buffers[b.out_buf].c == b.cout &&
        readers[b.out_buf] == 1 &&
        c.in_buf == b.out_buf && c.kh == 3 && c.kw == 3 && c.stride == 2 && c.pad_h == 0 && c.pad_w == 0 &&
        c.cin == dv::kMixed3Mid && c.cout == dv::kMixed3Out && c.out_coff % 8 == 0 &&
        a.ih >= 3 && a.iw >= 3 && a.ih * a.iw <= dv::kMixed3TilePx && c.oh * c.ow <= dv::kMixed3MaxOutPx;
    if (!ok) continue;
    for (int k = 0; k < 3; ++k) {
      Op& o = ops[i + k];
      o.m3 = k + 1;
      o.v2 = false;
    }
    for (int buf : {a.out_buf, b.out_buf}) buffers[buf] = {1, 1, buffers[buf].c, 0};   // LDS only
    i += 2;
  }
}

// tf_keras applications/inception_v3.py, construction order = layer order.
void dv_model::build() {
  const int in_buf = new_buffer(desc.height, desc.width, 16);
  TensorRef x = full(in_buf);
  x = conv(x, 32, 3, 3, 2, false, -1, 0, desc.channels);
  if (desc.channels <= 16 && getenv("DV_NO_U8_CONV1") == nullptr &&
      (desc.channels <= 8 || getenv("DV_NO_U8_CONV1_WIDE") == nullptr)) {
    Op& f = ops.back();
    f.first_u8 = true;  // conv_first_u8_kernel: K chunk = 2 taps x 8 channels (C <= 8), 1 tap x 16 (C <= 16)
    f.nb = 1;
    f.n_chunks = desc.channels <= 8 ? (f.kh * f.kw + 1) / 2 : f.kh * f.kw;
    f.n_steps = 1;
    buffers[in_buf] = {1, 1, 16, 0};  // the fp16 staging image is never materialised
  }
  x = conv(x, 32, 3, 3, 1, false);
  x = conv(x, 64, 3, 3);
  // (layer order: the two remaining stem convs are created before the pools run)
  if (getenv("DV_NO_POOL_FUSE") == nullptr) {  // tuning knob
    // max-pool fused into the 1x1 that consumes it (conv_pool1x1_kernel)
    TensorRef pooled = x;
    pooled.h = (x.h - 3) / 2 + 1;
    pooled.w = (x.w - 3) / 2 + 1;
    const int ih = x.h, iw = x.w;
    x = conv(pooled, 80, 1, 1, 1, false);
    ops.back().pool_in = true;
    ops.back().ih = ih;
    ops.back().iw = iw;
  } else {
    x = pool(kOpMaxPool, x);
    x = conv(x, 80, 1, 1, 1, false);
  }
  // Fused stem kernels (stem.hip): conv1+conv2 and conv3+maxpool+1x1 as two persistent
  // launches whose intermediates stay in LDS.  DV_NO_STEM_FUSE keeps the per-layer path
  // (also used for inputs with more than 8 channels).
  if (getenv("DV_NO_STEM_FUSE") == nullptr) {
    // stem_a reads the uint8 image with two taps x 8 channels per chunk (C <= 8) or, round 6, one tap x 16
    // channels (C = 9..12: the long-read channel sets ONT_R104 9, PACBIO 10; DV_NO_STEM_A_WIDE keeps
    // conv_first_u8 (wide) + a per-layer conv2 for them).  stem_b (conv3 + max-pool + 1x1) reads conv2's fp16
    // output whatever produced it.
    const int stem_a_max = getenv("DV_NO_STEM_A_WIDE") == nullptr ? dv::kStemA_MaxChannels : 8;
    if (ops[0].first_u8 && desc.channels <= stem_a_max && ops[3].pool_in && ops[3].cout <= 96) {
      ops[0].stem_a = true;
      buffers[ops[0].out_buf] = {1, 1, 32, 0};  // conv1 output: LDS only
    }
    if (ops[3].pool_in && ops[3].cout <= 96 && (ops[0].stem_a || getenv("DV_NO_STEM_B_ALONE") == nullptr)) {
      ops[2].stem_b = true;
      buffers[ops[2].out_buf] = {1, 1, 64, 0};  // conv3 output: LDS only
    }
  }
  x = conv(x, 192, 3, 3, 1, false);
  blank_conv4_op = static_cast<int>(ops.size()) - 1;
  // The stem's second max-pool has ONE consumer launch -- mixed0's four 1x1 heads, grouped
  // (the pooled branch projects before it averages) -- so it is taken on the fly there
  // (conv_pool1x1_kernel) and the pooled tensor is never written.  DV_NO_POOL2_FUSE keeps
  // the separate max-pool kernel.
  const bool fuse_pool2 = getenv("DV_NO_POOL2_FUSE") == nullptr && getenv("DV_NO_POOL_FUSE") == nullptr &&
                          getenv("DV_NO_GROUPING") == nullptr;
  const int pool2_ih = x.h, pool2_iw = x.w;
  // Round 4: the pool moves into its PRODUCER (conv_pool_resident_kernel): the 21 x 51 x 192 tensor
  // is never written, mixed0's heads read the pooled 10 x 25 x 192 tensor like any other block's.
  // DV_NO_POOL2_IN_CONV keeps the round-3 arrangement (pool on load in the heads).
  const bool pool_in_conv = fuse_pool2 && getenv("DV_NO_POOL2_IN_CONV") == nullptr && ops.back().nb == 3 &&
                            x.h >= 3 && x.w >= 3;
  if (pool_in_conv) {
    x.h = (x.h - 3) / 2 + 1;
    x.w = (x.w - 3) / 2 + 1;
    ops.back().pool_out = true;
    buffers[x.buf] = {x.h, x.w, x.c, 0};
  } else if (fuse_pool2) {
    x.h = (x.h - 3) / 2 + 1;
    x.w = (x.w - 3) / 2 + 1;
  } else {
    x = pool(kOpMaxPool, x);
  }
  // Everything up to here is the "stem": big feature maps (0.2-0.7 MB per
  // example each).  It runs in sub-batches of stem_sub_batch() examples over
  // small, reused buffers so that every producer->consumer hand-off stays in
  // the 256 MB Infinity Cache instead of streaming through HBM; only the
  // 96 KB/example stem output is written at full-batch width.
  stem_ops_end = static_cast<int>(ops.size());
  stem_out_buf = x.buf;
  for (int pool_ch : {32, 64, 64}) {  // mixed0..2
    const int out = new_buffer(x.h, x.w, 64 + 64 + 96 + pool_ch);
    conv(x, 64, 1, 1, 1, true, out, 0);
    TensorRef b5 = conv(x, 48, 1, 1);
    conv(b5, 64, 5, 5, 1, true, out, 64);
    TensorRef b3 = conv(x, 64, 1, 1);
    b3 = conv(b3, 96, 3, 3);
    conv(b3, 96, 3, 3, 1, true, out, 128);
    pooled_projection(x, pool_ch, out, 224);
    named_views.push_back({"mixed" + std::to_string(named_views.size()), out, 0, buffers[out].c});
    if (fuse_pool2 && !pool_in_conv && x.buf == stem_out_buf) {  // mixed0: its 1x1 heads pool their input
      for (size_t k = stem_ops_end; k < ops.size(); ++k) {
        if (ops[k].type == kOpConv && ops[k].in_buf == x.buf) {
          ops[k].pool_in = true;
          ops[k].ih = pool2_ih;
          ops[k].iw = pool2_iw;
        }
      }
    }
    x = full(out);
  }
  {  // mixed3
    const int oh = (x.h - 3) / 2 + 1, ow = (x.w - 3) / 2 + 1;
    const int out = new_buffer(oh, ow, 384 + 96 + x.c);
    conv(x, 384, 3, 3, 2, false, out, 0);
    TensorRef b = conv(x, 64, 1, 1);
    b = conv(b, 96, 3, 3);
    conv(b, 96, 3, 3, 2, false, out, 384);
    pool(kOpMaxPool, x, out, 480);
    named_views.push_back({"mixed3", out, 0, buffers[out].c});
    x = full(out);
  }
  wide_stage = true;   // precise mode: the tensors created from here on (17x17 and 8x8 stages) are hi + lo
  for (int c7 : {128, 160, 160, 192}) {  // mixed4..7
    const int out = new_buffer(x.h, x.w, 768);
    conv(x, 192, 1, 1, 1, true, out, 0);
    TensorRef b = conv(x, c7, 1, 1);
    b = conv(b, c7, 1, 7);
    conv(b, 192, 7, 1, 1, true, out, 192);
    TensorRef d = conv(x, c7, 1, 1);
    d = conv(d, c7, 7, 1);
    d = conv(d, c7, 1, 7);
    d = conv(d, c7, 7, 1);
    conv(d, 192, 1, 7, 1, true, out, 384);
    pooled_projection(x, 192, out, 576);
    named_views.push_back({"mixed" + std::to_string(named_views.size()), out, 0, buffers[out].c});
    x = full(out);
  }
  {  // mixed8
    const int oh = (x.h - 3) / 2 + 1, ow = (x.w - 3) / 2 + 1;
    const int out = new_buffer(oh, ow, 320 + 192 + x.c);
    TensorRef b = conv(x, 192, 1, 1);
    conv(b, 320, 3, 3, 2, false, out, 0);
    TensorRef d = conv(x, 192, 1, 1);
    d = conv(d, 192, 1, 7);
    d = conv(d, 192, 7, 1);
    conv(d, 192, 3, 3, 2, false, out, 320);
    pool(kOpMaxPool, x, out, 512);
    named_views.push_back({"mixed8", out, 0, buffers[out].c});
    x = full(out);
  }
  for (int i = 0; i < 2; ++i) {  // mixed9, mixed10
    const int out = new_buffer(x.h, x.w, 2048);
    conv(x, 320, 1, 1, 1, true, out, 0);
    TensorRef b = conv(x, 384, 1, 1);
    conv(b, 384, 1, 3, 1, true, out, 320);
    conv(b, 384, 3, 1, 1, true, out, 704);
    named_views.push_back({"mixed9_" + std::to_string(i), out, 320, 2 * 384});   // Keras' concat of these two
    TensorRef d = conv(x, 448, 1, 1);
    d = conv(d, 384, 3, 3);
    conv(d, 384, 1, 3, 1, true, out, 1088);
    conv(d, 384, 3, 1, 1, true, out, 1472);
    pooled_projection(x, 192, out, 1856);
    named_views.push_back({"mixed" + std::to_string(9 + i), out, 0, buffers[out].c});
    x = full(out);
  }
  feat_buf = x.buf;
  buffers[feat_buf].f32 = true;            // the global pool reads float32
  buffers[feat_buf].wide = false;
  feat_p = x.h * x.w;
  feat_c = x.c;
  group_siblings();
  for (const Op& op : ops) {  // zero halo wide enough for every consumer
    int need = 0;
    if (op.type == kOpConv) need = std::max(op.pad_h, op.pad_w);
    if (op.type == kOpAvgPool) need = 1;  // avgpool3s1_kernel reads its taps unconditionally
    buffers[op.in_buf].halo = std::max(buffers[op.in_buf].halo, need);
  }
  choose_chains();
  if (getenv("DV_CHAIN_KEEP_HALO") == nullptr) {
    // A fused chain DMAs the INTERIOR of its input into LDS and handles the map border itself
    // (tap masks, the zero piece): its input tensor needs no halo in HBM.  Without one the rows
    // of a map are contiguous (a 4x12 map plane is 768 bytes = six whole 128-byte lines), so the
    // 1x1 head that produces the tensor stores whole lines instead of 192-byte row segments that
    // start mid-line, and the chain's input DMA is one run per plane.
    for (BufferDesc& b : buffers) b.halo = 0;
    for (const Op& op : ops) {
      if (op.in_chain) continue;
      int need = 0;
      if (op.type == kOpConv && op.chain_len == 0) need = std::max(op.pad_h, op.pad_w);
      if (op.type == kOpAvgPool) need = 1;
      buffers[op.in_buf].halo = std::max(buffers[op.in_buf].halo, need);
    }
  }
  choose_imgconv();
  choose_band();
  choose_split();
  choose_side_pool();
  choose_avg_epilogue();
  choose_block35();
  choose_mixed3();
  for (size_t i = 0; i < ops.size(); ++i) {  // packed-weight image per LAUNCH (after grouping)
    Op& op = ops[i];
    if (op.type != kOpConv) continue;
    int subs = 0;
    for (int gi = 0; gi <= op.group_followers; ++gi) subs += (ops[i + gi].cout + 31) / 32;
    const int n_tiles = (subs + op.nb - 1) / op.nb;
    for (int gi = 0; gi <= op.group_followers; ++gi) ops[i + gi].w_off = packed_halfs;
    packed_halfs += op.first_u8 ? static_cast<size_t>(kFirstMaxChunks) * 32 * kChunk
                    : op.b35 == 1 ? static_cast<size_t>(2) * (op.cin / kChunk) * 2 * 128 * 8   // block35.hip's heads
                    : op.m3 == 1 ? static_cast<size_t>(op.cin / kChunk) * 2 * dv::kMixed3Red * 8       // mixed3.hip's 1x1
                    : (op.chain_len > 0 || op.in_chain || op.b35 >= 5 || op.m3 >= 2)
                        ? static_cast<size_t>(op.n_chunks) * 2 * ((op.cout + 31) / 32 * 32) * 8
                    : op.v2     ? static_cast<size_t>(op.v2_tiles) * op.v2_steps *
                                      dv::imgconv_wslab_halfs(op.kh, op.kw, op.nb)
                                : static_cast<size_t>(op.band ? op.band : 1) * n_tiles * op.n_steps *
                                      kSlabChunks * (op.nb * 32) * kChunk;
    i += op.group_followers;
  }
  layers.push_back({1, 1, feat_c, desc.num_classes, n_params});
  n_params += static_cast<int64_t>(feat_c) * desc.num_classes + desc.num_classes;
}

std::vector<size_t> dv_model::correction_shift_offsets() const {
  std::vector<const Op*> by_layer(layers.size(), nullptr);
  for (const Op& op : ops) {
    if (op.type == kOpConv) by_layer[op.layer] = &op;
  }
  std::vector<size_t> at;
  for (size_t l = 0; l + 1 < layers.size(); ++l) {
    for (int co = 0; co < by_layer[l]->cout; ++co) at.push_back(by_layer[l]->shift_off + co);
  }
  return at;
}
