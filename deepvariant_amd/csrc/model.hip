// model.hip -- Inception-v3 call_variants classifier on gfx950 (MI355X).
//
// Replaces the model forward of deepvariant/call_variants.py:904-932
// (keras_modeling.inceptionv3, deepvariant/keras_modeling.py:246-336; graph =
// tf_keras InceptionV3(include_top=False, pooling='avg')).
//
// Data layout in HBM: activations are fp16 in the channel-blocked, zero-haloed layout
// [N][C/8][H+2h][W+2h][8] ("C8"): the 8 channels an MFMA fragment needs for one pixel
// are one 16-byte piece, and consecutive pixels of a row are consecutive
// pieces, so every fragment load and every store of a 32-pixel tile is one
// contiguous 512-byte run.  One buffer per graph tensor; concat outputs are
// written in place (each branch's last conv stores at its channel-group offset
// of the block's output buffer -- no concat kernel).  BatchNorm
// (scale=False, eps=1e-3, moving statistics) is folded into the fp16 conv
// weights and an fp32 per-channel shift at load time.
//
// The plan (tensors, ops, planning passes) is model_graph.h / model_graph.cpp; the kernels are conv_mfma.hip (MFMA
// convolutions), model_kernels.hip (front end, pools, head), stem.hip, imgconv.hip, chain.hip, block35.hip and mixed3.hip.  This
// file packs the weights, enqueues the plan's launches (run_ops) and holds the C entry points.
#include <algorithm>
#include <map>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

#include <hip/hip_fp16.h>

#include "model_graph.h"
#include "model_kernels.h"
#include "block35.h"
#include "mixed3.h"
#include "chain.h"
#include "stem_fused.h"
#include "calib.h"
#include "layer_export.h"

namespace {

// Examples per stem pass.  Measured on MI355X (round 1): sub-batching the stem to
// keep its hand-offs in the 256 MB Infinity Cache (64/128/256) LOSES 5-19 % at
// 2 K examples per launch -- the stem is not HBM-bound and the extra launches
// cost ~5 us each -- so it is off by default; DV_STEM_SB enables it for tuning.
static int stem_sub_batch() {
  static const int v = getenv("DV_STEM_SB") ? std::max(1, atoi(getenv("DV_STEM_SB"))) : (1 << 30);
  return v;
}

ExtPtrs* ext_table(const dv_model* m) { return static_cast<ExtPtrs*>(m->d_ext.ptr); }

// DV_OP_TRACE=1: per-launch table (ms, TFLOP/s, activation GB/s) on stderr after
// every eager forward -- the per-layer view rocprofv3's per-kernel-name stats cannot give.
struct OpTrace {
  hipEvent_t a, b;
  std::string label;
  double flops, bytes;
};
std::vector<OpTrace>* g_trace = nullptr;

struct TraceScope {
  hipStream_t stream;
  bool on;
  TraceScope(hipStream_t s, std::string label, double flops, double bytes) : stream(s), on(g_trace != nullptr) {
    if (!on) return;
    OpTrace t{nullptr, nullptr, std::move(label), flops, bytes};
    (void)hipEventCreate(&t.a);
    (void)hipEventCreate(&t.b);
    (void)hipEventRecord(t.a, stream);
    g_trace->push_back(std::move(t));
  }
  ~TraceScope() {
    if (on) (void)hipEventRecord(g_trace->back().b, stream);
  }
};

void dump_trace(hipStream_t stream) {
  (void)hipStreamSynchronize(stream);
  double tot = 0;
  for (OpTrace& t : *g_trace) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, t.a, t.b);
    tot += ms;
    fprintf(stderr, "[dv-op] %-58s %8.1f us %7.1f TF/s %7.0f GB/s\n", t.label.c_str(), ms * 1e3,
            t.flops / (ms * 1e-3) / 1e12, t.bytes / (ms * 1e-3) / 1e9);
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  fprintf(stderr, "[dv-op] total %.1f us\n", tot * 1e3);
  g_trace->clear();
}

// conv_resident_kernel applies when the whole 96-cout tile fits the LDS next to nothing else,
// the launch has enough pixels to give every wave of a persistent grid several tiles, and no
// special mode is on.  DV_RESIDENT=0 keeps conv_mfma_kernel everywhere; DV_RESIDENT=2 widens it
// from the 3x3 80->192 to every eligible 96-cout-tile layer (tuning).
bool resident_ok(const dv_model* m, const Op& op, const ConvArgs& a) {
  const char* env = getenv("DV_RESIDENT");   // read per launch set-up (tests toggle it between models)
  const int mode = env ? atoi(env) : 1;
  if (mode == 0 || op.nb != 3 || op.band || op.v2 || op.pool_in || op.split || a.blank_row != nullptr || a.wide_in) return false;
  if (resident_lds_bytes(a) > 150 * 1024 || m->n_cus < 8 * a.n_tiles) return false;
  static const long min_tiles = getenv("DV_RESIDENT_MIN_TILES") ? atol(getenv("DV_RESIDENT_MIN_TILES")) : 4;   // tuning knob
  if (static_cast<long>(a.M) < static_cast<long>(m->n_cus) * 8 * 64 * min_tiles) return false;
  if (mode >= 2) return true;
  return m->blank_conv4_op >= 0 && &op == &m->ops[m->blank_conv4_op];
}

// One pass of run_ops: ops [first, last) on `n` examples.  `out_example_off` shifts the output
// pointer of ops that write `shifted_buf` (the stem's full-batch output).
struct Pass {
  dv_model* m;
  int n;
  hipStream_t stream;
  int first, last;
  int shifted_buf, out_example_off;
  size_t images_off;
  std::vector<char> side_pooled;   // max-pools a convolution of this pass has taken on the side
  _Float16* out_ptr(int buf) const {
    const size_t halfs = static_cast<size_t>(out_example_off) * m->buffers[buf].bytes_per_example() / 2;
    return m->buf_ptr(buf) + (buf == shifted_buf ? halfs : 0);
  }
};

dv::C8Geom c8_geom(const BufferDesc& b) {
  const TensorGeom g = b.geom();
  return dv::C8Geom{g.h, g.w, g.halo, g.hp, g.wp, g.groups};
}

// The enqueue_* functions below issue the launch that starts at op `oi` and return how many ops it ran
// (or a negative dv_status).

int enqueue_stem_a(const Pass& ps, int oi) {
  const dv_model* m = ps.m;
  const int n = ps.n;
  const Op &op = m->ops[oi], &c2 = m->ops[oi + 1];
  dv::StemAArgs a{};
  a.in = nullptr;
  a.in_ind = &ext_table(m)->images;
  a.in_off = ps.images_off;
  a.w1 = m->w_ptr(op);
  a.w2 = m->w_ptr(c2);
  a.shift1 = m->shift_ptr(op);
  a.shift2 = m->shift_ptr(c2);
  a.out = m->buf_ptr(c2.out_buf);
  a.og = c8_geom(m->buffers[c2.out_buf]);
  a.N = n;
  a.H = op.ih;
  a.W = op.iw;
  a.C = op.cin_real;
  a.OH1 = op.oh;
  a.OW1 = op.ow;
  a.OH2 = c2.oh;
  a.OW2 = c2.ow;
  a.tiles_y = (c2.oh + dv::kStemA_TH - 1) / dv::kStemA_TH;
  a.tiles_x = (c2.ow + dv::kStemA_TW - 1) / dv::kStemA_TW;
  a.total_tiles = n * a.tiles_y * a.tiles_x;
  a.in_bytes = static_cast<unsigned>(static_cast<size_t>(n) * op.ih * op.iw * op.cin_real);
  if (m->blank_on()) {
    a.blank_thr = m->blank_thr(1);
    a.blank_src = static_cast<const _Float16*>(m->d_blank_c2.ptr);
    a.blank_need = m->blank_read_through() ? nullptr : m->blank_thr(5);
  }
  TraceScope tr(ps.stream, std::string(!m->blank_on() ? "" : m->blank_read_through() ? "[blank tiles left to stem_b] " : "[blank tiles copied] ") + "stem_a conv3x3s2 " + std::to_string(op.cin_real) + "->32 + conv3x3 32->32 (fused)",
                2.0 * n * (static_cast<double>(op.oh) * op.ow * op.kh * op.kw * op.cin_real * op.cout +
                           static_cast<double>(c2.oh) * c2.ow * 9 * 32 * 32),
                static_cast<double>(n) * (op.ih * op.iw * op.cin_real + 2.0 * c2.oh * c2.ow * 32));
  dv::ProfileScope prof(dv::kProfConv, ps.stream);
  dv::launch_stem_a(a, m->stem_a_grid, ps.stream);
  return 2;
}

// DV_STEM_PROF (tuning aid, eager only): stem_b with its per-wave phase counters read back and printed.
void report_stem_b_profile(dv::StemBArgs a, int grid, hipStream_t stream) {
  const size_t words = static_cast<size_t>(grid) * 16;
  unsigned long long* d = nullptr;
  if (hipMalloc(&d, words * 8) != hipSuccess) return;
  (void)hipMemsetAsync(d, 0, words * 8, stream);
  a.prof = d;
  dv::launch_stem_b(a, grid, stream);
  std::vector<unsigned long long> h(words);
  (void)hipStreamSynchronize(stream);
  (void)hipMemcpy(h.data(), d, words * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  for (int w = 0; w < 2; ++w) {
    double sum[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < grid; ++b)
      for (int i = 0; i < 7; ++i) sum[i] += static_cast<double>(h[(b * 2 + w) * 8 + i]);
    const double tiles = static_cast<double>(a.total_tiles);
    fprintf(stderr, "[dv-stem-b wave %d] cycles/tile: issue %.0f conv3 %.0f dma-wait %.0f barrierA %.0f pool %.0f "
                    "barrierB %.0f conv1x1+store %.0f\n", w ? 7 : 0, sum[0] / tiles, sum[1] / tiles,
            sum[6] / tiles, sum[2] / tiles, sum[3] / tiles, sum[4] / tiles, sum[5] / tiles);
  }
  // placement: which workgroups share a CU, their TG slots, and the phase sums of the two classes
  std::map<unsigned long long, std::vector<int>> where;
  for (int b = 0; b < grid; ++b) {
    const unsigned long long v = h[(b * 2) * 8 + 7];
    const unsigned hw = static_cast<unsigned>(v), xcc = static_cast<unsigned>(v >> 32);
    where[(static_cast<unsigned long long>(xcc) << 16) | ((hw >> 8) & 0xffu)].push_back(b);
  }
  int pairs = 0, same_parity = 0, apart256 = 0;
  for (const auto& kv : where) {
    if (kv.second.size() != 2) continue;
    ++pairs;
    const unsigned t0 = (static_cast<unsigned>(h[(kv.second[0] * 2) * 8 + 7]) >> 16) & 15u;
    const unsigned t1 = (static_cast<unsigned>(h[(kv.second[1] * 2) * 8 + 7]) >> 16) & 15u;
    same_parity += (t0 & 1u) == (t1 & 1u);
    apart256 += kv.second[1] - kv.second[0] == 256;
  }
  fprintf(stderr, "[dv-stem-b placement] %zu places for %d workgroups; %d pairs, %d with TG slots of EQUAL parity, "
                  "%d pairs are blocks b / b+256\n", where.size(), grid, pairs, same_parity, apart256);
  for (int cls = 0; cls < 2; ++cls) {
    double sum[7] = {0, 0, 0, 0, 0, 0, 0};
    int nb = 0;
    for (int b = 0; b < grid; ++b) {
      const unsigned tg = (static_cast<unsigned>(h[(b * 2) * 8 + 7]) >> 16) & 15u;
      if (static_cast<int>(tg & 1u) != cls) continue;
      ++nb;
      for (int i = 0; i < 7; ++i) sum[i] += static_cast<double>(h[(b * 2) * 8 + i]);
    }
    double tot = 0;
    for (double v : sum) tot += v;
    fprintf(stderr, "[dv-stem-b TG parity %d] %d workgroups, share of wave-0 cycles: issue %.3f conv3 %.3f dma-wait %.3f "
                    "barrierA %.3f pool %.3f barrierB %.3f conv1x1+store %.3f; cycles per workgroup %.0f\n", cls, nb,
            sum[0] / tot, sum[1] / tot, sum[6] / tot, sum[2] / tot, sum[3] / tot, sum[4] / tot, sum[5] / tot,
            nb ? tot / nb : 0.0);
  }
}

int enqueue_stem_b(const Pass& ps, int oi) {
  const dv_model* m = ps.m;
  const int n = ps.n;
  const Op &op = m->ops[oi], &c4 = m->ops[oi + 1];
  const BufferDesc& ib = m->buffers[op.in_buf];
  dv::StemBArgs a{};
  a.in = m->buf_ptr(op.in_buf);
  a.w3 = m->w_ptr(op);
  a.w4 = m->w_ptr(c4);
  a.shift3 = m->shift_ptr(op);
  a.shift4 = m->shift_ptr(c4);
  a.out = m->buf_ptr(c4.out_buf);
  a.ig = c8_geom(ib);
  a.og = c8_geom(m->buffers[c4.out_buf]);
  a.N = n;
  a.OH3 = op.oh;
  a.OW3 = op.ow;
  a.PH = c4.oh;
  a.PW = c4.ow;
  a.Cout4 = c4.cout;
  a.tiles_y = (c4.oh + dv::kStemB_PH - 1) / dv::kStemB_PH;
  a.tiles_x = (c4.ow + dv::kStemB_PW - 1) / dv::kStemB_PW;
  a.total_tiles = n * a.tiles_y * a.tiles_x;
  a.in_bytes = static_cast<size_t>(n) * ib.bytes_per_example();
  a.in_img_bytes = static_cast<unsigned>(ib.bytes_per_example());
  if (m->blank_on()) {
    a.blank_thr = m->blank_thr(2);
    a.blank_src = static_cast<const _Float16*>(m->d_blank_b.ptr);
    a.blank_need = m->blank_thr(6);
    a.blank_strip = m->blank_copy_tiles ? 0 : 1;
    if (m->blank_read_through()) {
      a.blank_cut = m->blank_thr(7);
      a.blank_in = static_cast<const _Float16*>(m->d_blank_c2.ptr);
    }
  }
  TraceScope tr(ps.stream, std::string(!m->blank_on() ? "" : m->blank_copy_tiles ? "[blank tiles copied] " : m->blank_read_through() ? "[blank rows read through, blank strip copied] " : "[blank strip copied] ") + "stem_b conv3x3 32->64 + maxpool3s2 + conv1x1 64->" + std::to_string(c4.cout) + " (fused)",
                2.0 * n * (static_cast<double>(op.oh) * op.ow * 9 * 32 * 64 +
                           static_cast<double>(c4.oh) * c4.ow * 64 * c4.cout),
                2.0 * n * (static_cast<double>(op.ih) * op.iw * 32 + static_cast<double>(c4.oh) * c4.ow * c4.cout));
  dv::ProfileScope prof(dv::kProfConv, ps.stream);
  static const bool stem_prof = getenv("DV_STEM_PROF") != nullptr;
  if (stem_prof && g_trace != nullptr) {
    report_stem_b_profile(a, m->stem_b_grid, ps.stream);
  } else {
    dv::launch_stem_b(a, m->stem_b_grid, ps.stream);
  }
  return 2;
}

int enqueue_block35(const Pass& ps, int oi) {
  const dv_model* m = ps.m;
  const int n = ps.n;
  const Op &op = m->ops[oi], &r5 = m->ops[oi + 1], &r3 = m->ops[oi + 2], &pj = m->ops[oi + 3];
  const Op &c5 = m->ops[oi + 4], &c3a = m->ops[oi + 5], &c3b = m->ops[oi + 6], &ap = m->ops[oi + 7];
  const BufferDesc& ib = m->buffers[op.in_buf];
  dv::Block35Args a{};
  a.in = m->buf_ptr(op.in_buf);
  a.ig = ib.geom();
  a.in_img_bytes = static_cast<unsigned>(ib.bytes_per_example());
  a.N = n;
  a.h = op.oh;
  a.w = op.ow;
  a.n_chunks = op.cin / kChunk;
  a.w1 = m->w_ptr(op);
  a.sh_red5 = m->shift_ptr(r5);
  a.sh_red3 = m->shift_ptr(r3);
  a.sh_b1 = m->shift_ptr(op);
  a.sh_pool = m->shift_ptr(ap);
  a.pool_c = pj.cout;
  a.w5 = m->w_ptr(c5);
  a.sh5 = m->shift_ptr(c5);
  a.w3a = m->w_ptr(c3a);
  a.sh3a = m->shift_ptr(c3a);
  a.w3b = m->w_ptr(c3b);
  a.sh3b = m->shift_ptr(c3b);
  a.out = m->buf_ptr(op.out_buf);
  a.og = m->buffers[op.out_buf].geom();
  a.goff_b1 = op.out_coff / 8;
  a.goff_5 = c5.out_coff / 8;
  a.goff_3 = c3b.out_coff / 8;
  a.goff_pool = ap.out_coff / 8;
  const double px = static_cast<double>(n) * op.oh * op.ow;
  const double tr_flops = 2.0 * px * (static_cast<double>(op.cin) * (op.cout + r5.cout + r3.cout + pj.cout) +
                                      25.0 * c5.cin * c5.cout + 9.0 * c3a.cin * c3a.cout + 9.0 * c3b.cin * c3b.cout);
  const std::string tr_label = "block35 " + std::to_string(op.cin) + "->" + std::to_string(op.cout) + "|" +
                               std::to_string(r5.cout) + "->" + std::to_string(c5.cout) + " 5x5|" +
                               std::to_string(r3.cout) + "->" + std::to_string(c3a.cout) + "->" +
                               std::to_string(c3b.cout) + " 3x3|" + std::to_string(pj.cout) + " pool @" +
                               std::to_string(op.oh) + "x" + std::to_string(op.ow);
  TraceScope tr(ps.stream, tr_label, tr_flops,
                2.0 * px * (static_cast<double>(op.cin) + op.cout + c5.cout + c3b.cout + pj.cout));
  dv::ProfileScope prof(dv::kProfConv, ps.stream);
  dv::launch_block35(a, m->n_cus, ps.stream);
  return 8;
}

// DV_MIXED3_PROF (tuning aid, eager only): the launch with its per-wave phase counters read back and printed.
void report_mixed3_profile(dv::Mixed3Args a, int n_cus, hipStream_t stream) {
  const int grid = std::min(a.N, n_cus);
  const size_t words = static_cast<size_t>(grid) * 4 * 12;
  unsigned long long* d = nullptr;
  if (hipMalloc(&d, words * 8) != hipSuccess) return;
  (void)hipMemsetAsync(d, 0, words * 8, stream);
  a.prof = d;
  dv::launch_mixed3(a, n_cus, stream);
  std::vector<unsigned long long> h(words);
  (void)hipStreamSynchronize(stream);
  (void)hipMemcpy(h.data(), d, words * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  for (int w = 0; w < 4; ++w) {
    double sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < grid; ++b)
      for (int i = 0; i < 9; ++i) sum[i] += static_cast<double>(h[(static_cast<size_t>(b) * 4 + w) * 12 + i]);
    const double tiles = static_cast<double>(a.N);
    fprintf(stderr, "[dv-mixed3 wave %d] cycles/tile (chunk-barrier wait, mfma steps, closing barrier + epilogue): 1x1 %.0f %.0f "
                    "%.0f | 3x3 %.0f %.0f %.0f | 3x3/2 %.0f %.0f %.0f\n", w, sum[0] / tiles, sum[1] / tiles, sum[2] / tiles,
            sum[3] / tiles, sum[4] / tiles, sum[5] / tiles, sum[6] / tiles, sum[7] / tiles, sum[8] / tiles);
  }
}

int enqueue_mixed3(const Pass& ps, int oi) {
  const dv_model* m = ps.m;
  const int n = ps.n;
  const Op &op = m->ops[oi], &c3a = m->ops[oi + 1], &c3b = m->ops[oi + 2];
  const BufferDesc& ib = m->buffers[op.in_buf];
  dv::Mixed3Args a{};
  a.in = m->buf_ptr(op.in_buf);
  a.ig = ib.geom();
  a.in_img_bytes = static_cast<unsigned>(ib.bytes_per_example());
  a.N = n;
  a.h = op.oh;
  a.w = op.ow;
  a.n_chunks = op.cin / kChunk;
  a.w1 = m->w_ptr(op);
  a.sh1 = m->shift_ptr(op);
  a.w3a = m->w_ptr(c3a);
  a.sh3a = m->shift_ptr(c3a);
  a.w3b = m->w_ptr(c3b);
  a.sh3b = m->shift_ptr(c3b);
  a.out = m->buf_ptr(c3b.out_buf);
  a.og = m->buffers[c3b.out_buf].geom();
  a.oh = c3b.oh;
  a.ow = c3b.ow;
  a.goff = c3b.out_coff / 8;
  const double px = static_cast<double>(n) * op.oh * op.ow, opx = static_cast<double>(n) * c3b.oh * c3b.ow;
  const std::string tr_label = "mixed3 dbl " + std::to_string(op.cin) + "->" + std::to_string(op.cout) + " 1x1|" +
                               std::to_string(c3a.cin) + "->" + std::to_string(c3a.cout) + " 3x3|" +
                               std::to_string(c3b.cin) + "->" + std::to_string(c3b.cout) + " 3x3/2 @" +
                               std::to_string(op.oh) + "x" + std::to_string(op.ow);
  TraceScope tr(ps.stream, tr_label,
                2.0 * (px * (static_cast<double>(op.cin) * op.cout + 9.0 * c3a.cin * c3a.cout) + opx * 9.0 * c3b.cin * c3b.cout),
                2.0 * (px * op.cin + opx * c3b.cout));
  dv::ProfileScope prof(dv::kProfConv, ps.stream);
  static const bool mixed3_prof = getenv("DV_MIXED3_PROF") != nullptr;
  if (mixed3_prof && g_trace != nullptr) {
    report_mixed3_profile(a, m->n_cus, ps.stream);
  } else {
    dv::launch_mixed3(a, m->n_cus, ps.stream);
  }
  return 3;
}

// DV_CHAIN_PROF (tuning aid, eager only): the chain with its per-wave phase counters read back and printed.
void report_chain_profile(dv::ChainArgs a, int n_cus, hipStream_t stream) {
  const int grid = std::min(a.n_tiles, n_cus);
  const size_t words = static_cast<size_t>(grid) * 4 * 8;
  unsigned long long* d = nullptr;
  if (hipMalloc(&d, words * 8) != hipSuccess) return;
  (void)hipMemsetAsync(d, 0, words * 8, stream);
  a.prof = d;
  dv::launch_chain(a, n_cus, stream);
  std::vector<unsigned long long> h(words);
  (void)hipStreamSynchronize(stream);
  (void)hipMemcpy(h.data(), d, words * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  for (int w = 0; w < 4; ++w) {
    double sum[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < grid; ++b)
      for (int i = 0; i < 6; ++i) sum[i] += static_cast<double>(h[(static_cast<size_t>(b) * 4 + w) * 8 + i]);
    const double tiles = static_cast<double>(a.n_tiles);
    fprintf(stderr, "[dv-chain wave %d] cycles/tile: chunk-barrier wait %.0f mfma steps %.0f layer-barrier wait %.0f "
                    "lds epilogue %.0f hbm epilogue %.0f set-up %.0f\n", w, sum[0] / tiles, sum[1] / tiles,
            sum[2] / tiles, sum[3] / tiles, sum[4] / tiles, sum[5] / tiles);
  }
}

int enqueue_chain(const Pass& ps, int oi) {
  const dv_model* m = ps.m;
  const int n = ps.n;
  const Op& op = m->ops[oi];
  const Op& last = m->ops[oi + op.chain_len - 1];
  const BufferDesc& ib = m->buffers[op.in_buf];
  dv::ChainArgs a{};
  a.in = m->buf_ptr(op.in_buf);
  a.ig = ib.geom();
  a.in_img_bytes = static_cast<unsigned>(ib.bytes_per_example());
  a.N = n;
  a.G = op.chain_g;
  a.tpx = op.chain_tpx;
  a.h = op.oh;
  a.w = op.ow;
  a.n_tiles = (n + a.G - 1) / a.G;
  a.n_layers = op.chain_len;
  double tr_flops = 0;
  std::string tr_label = "chain";
  size_t act = 0, slot = 0;
  for (int k = 0; k < op.chain_len; ++k) {
    const Op& o = m->ops[oi + k];
    dv::ChainLayer& cl = a.L[k];
    cl.w = m->w_ptr(o);
    cl.shift = m->shift_ptr(o);
    cl.n_chunks = o.cin / kChunk;
    cl.cout = o.cout;
    cl.cout_pad = (o.cout + 31) / 32 * 32;
    cl.kh = o.kh;
    cl.kw = o.kw;
    cl.slab_bytes = static_cast<unsigned>(o.kh * o.kw * 2 * cl.cout_pad * 16);
    act = std::max(act, static_cast<size_t>(o.cin / 8) * op.chain_tpx * 16);
    slot = std::max(slot, static_cast<size_t>(cl.slab_bytes));
    tr_flops += 2.0 * n * o.oh * o.ow * o.kh * o.kw * o.cin * o.cout;
    tr_label += " " + std::to_string(o.kh) + "x" + std::to_string(o.kw) + ":" + std::to_string(o.cin) + "->" +
                std::to_string(o.cout);
  }
  a.act_bytes = static_cast<unsigned>(act);
  a.slot_bytes = static_cast<unsigned>(slot);
  a.out = m->buf_ptr(last.out_buf);
  a.og = m->buffers[last.out_buf].geom();
  a.out_goff = last.out_coff / 8;
  tr_label += " @" + std::to_string(op.oh) + "x" + std::to_string(op.ow) + " [fused, G=" + std::to_string(a.G) + "]";
  TraceScope tr(ps.stream, tr_label, tr_flops,
                2.0 * n * op.oh * op.ow * (static_cast<double>(op.cin) + last.cout));
  dv::ProfileScope prof(dv::kProfConv, ps.stream);
  static const bool chain_prof = getenv("DV_CHAIN_PROF") != nullptr;
  if (chain_prof && g_trace != nullptr) {
    report_chain_profile(a, m->n_cus, ps.stream);
  } else {
    dv::launch_chain(a, m->n_cus, ps.stream);
  }
  return op.chain_len;
}

int enqueue_first_conv(const Pass& ps, int oi) {
  const dv_model* m = ps.m;
  const int n = ps.n;
  const Op& op = m->ops[oi];
  FirstConvArgs f{};
  f.ext = ext_table(m);
  f.in_off = ps.images_off;
  f.w = m->w_ptr(op);
  f.shift = m->shift_ptr(op);
  f.out = ps.out_ptr(op.out_buf);
  f.og = m->buffers[op.out_buf].geom();
  f.N = n;
  f.H = op.ih;
  f.W = op.iw;
  f.C = op.cin_real;
  f.Cout = op.cout;
  f.OH = op.oh;
  f.OW = op.ow;
  f.KH = op.kh;
  f.KW = op.kw;
  f.stride = op.stride;
  f.M = n * op.oh * op.ow;
  f.n_chunks = op.n_chunks;
  f.wide = op.cin_real > 8 ? 1 : 0;
  f.in_bytes = static_cast<unsigned>(static_cast<size_t>(n) * op.ih * op.iw * op.cin_real);
  f.rcp_ow = 1.0f / static_cast<float>(op.ow);
  f.rcp_ohow = 1.0f / static_cast<float>(op.oh * op.ow);
  TraceScope tr(ps.stream, "conv_first_u8 3x3 s2 " + std::to_string(op.cin_real) + "->" + std::to_string(op.cout),
                2.0 * f.M * op.kh * op.kw * op.cin_real * op.cout,
                static_cast<double>(n) * (op.ih * op.iw * op.cin_real + 2.0 * op.oh * op.ow * op.cout));
  dv::ProfileScope prof(dv::kProfConv, ps.stream);
  launch_conv_first_u8(f, ps.stream);
  return 1;
}

// Where branch `br` of a conv launch stores: the tensor `o` writes, at its channel offset.
void set_branch_output(const Pass& ps, const Op& o, ConvBranch& br) {
  const BufferDesc& b = ps.m->buffers[o.out_buf];
  br.out = ps.out_ptr(o.out_buf);
  br.out32 = b.f32 ? ps.m->buf_ptr<float>(o.out_buf) : nullptr;   // (never the stem's shifted buffer)
  br.og = b.geom();
  br.lo_groups = b.wide ? b.c / 8 : 0;
  br.out_goff = o.out_coff / 8;
}

// The generic path: op `oi` and the siblings grouped behind it as one launch of conv_mfma_kernel (plain, row-band,
// split, side-pooling), its resident / pooling variants or imgconv.
int enqueue_conv(Pass& ps, int oi) {
  const dv_model* m = ps.m;
  const int n = ps.n;
  const Op& op = m->ops[oi];
  ConvArgs a{};
  a.in = m->buf_ptr(op.in_buf);
  const BufferDesc& ib = m->buffers[op.in_buf];
  a.ig = ib.geom();
  a.N = n;
  a.Cin = op.cin;
  a.OH = op.oh;
  a.OW = op.ow;
  static const int cu_pair = getenv("DV_CU_PAIR") ? atoi(getenv("DV_CU_PAIR")) : 0;
  a.cu_pair = cu_pair;
  a.band = op.band;
  a.KH = op.band ? op.band : op.kh;
  a.KW = op.kw;
  a.stride = op.stride;
  a.pad_h = op.pad_h;
  a.pad_w = op.pad_w;
  a.chunk_stride = static_cast<unsigned>(2 * a.ig.hp * a.ig.wp * 16);
  a.M = n * op.oh * op.ow;
  a.n_chunks = op.n_chunks;
  a.n_slabs = op.n_steps;
  a.split = op.split ? 1 : 0;
  a.split_tiles = op.split_tiles;
  a.wide_in = op.in_wide ? 1 : 0;
  a.lo_off = op.in_wide ? static_cast<unsigned>(ib.c / 8) * static_cast<unsigned>(a.ig.hp * a.ig.wp) * 16u : 0u;
  a.in_bytes = static_cast<size_t>(n) * ib.bytes_per_example();
  a.img_bytes = static_cast<unsigned>(ib.bytes_per_example());
  a.rcp_ow = 1.0f / static_cast<float>(op.ow);
  a.rcp_ohow = 1.0f / static_cast<float>(op.oh * op.ow);
  // this op + the sibling convs grouped behind it (same input, same geometry)
  int subs = 0;
  a.n_branches = 0;
  double tr_flops = 0, tr_bytes = static_cast<double>(n) * op.ih * op.iw * op.cin * 2.0;
  std::string tr_label = "conv " + std::to_string(op.kh) + "x" + std::to_string(op.kw) + " s" +
                         std::to_string(op.stride) + " " + std::to_string(op.cin) + "->";
  for (int gi = 0; gi <= op.group_followers; ++gi) {
    const Op& bo = m->ops[oi + gi];
    tr_flops += 2.0 * n * op.oh * op.ow * op.kh * op.kw * op.cin_real * bo.cout;
    tr_bytes += 2.0 * n * op.oh * op.ow * bo.cout;
    tr_label += (gi ? "+" : "") + std::to_string(bo.cout);
    ConvBranch& br = a.br[a.n_branches++];
    br.shift = bo.raw ? nullptr : m->shift_ptr(bo);
    set_branch_output(ps, bo, br);
    br.Cout = bo.cout;
    br.relu = bo.raw ? 0 : 1;
    br.sub0 = subs;
    subs += (bo.cout + 31) / 32;
    if (op.avg_tile_g > 0 && bo.avg_partner >= 0 && bo.avg_partner < ps.last) {   // pooled in this launch's epilogue
      const Op& pl = m->ops[bo.avg_partner];
      br.avgpool = 1;
      br.shift = m->shift_ptr(pl);
      br.relu = 1;
      set_branch_output(ps, pl, br);
      a.tile_g = op.avg_tile_g;
      a.tile_p = op.oh * op.ow;
      a.rcp_tile_p = 1.0f / static_cast<float>(a.tile_p);
    }
  }
  if (a.tile_g > 0) tr_label += " [+ avgpool3s1 in the epilogue, " + std::to_string(a.tile_g) + " maps per block]";
  a.w = m->w_ptr(op);
  const int tiles = (subs + op.nb - 1) / op.nb;
  a.n_tiles = tiles;
  if (m->blank_on() && m->blank_conv4_op >= 0 && &op == &m->ops[m->blank_conv4_op] &&
      a.n_branches == 1 && !op.band && !op.v2 && !op.pool_in) {
    a.blank_row = m->blank_thr(op.pool_out ? 4 : 3);
    a.blank_src = static_cast<const _Float16*>(m->d_blank_conv4.ptr);
    tr_label += " [blank rows copied]";
  }
  if (m->blank_on() && oi == 1 && !m->ops[0].stem_a && a.n_branches == 1 && !op.band && !op.v2 && !op.pool_in &&
      !op.pool_out && !op.split && op.nb <= 4 && m->d_blank_c2.ptr != nullptr) {
    // inputs of 9..16 channels: conv2 runs per layer (conv_mfma_kernel) and skips like the fused stem_a does
    a.blank_row = m->blank_thr(1);
    a.blank_src = static_cast<const _Float16*>(m->d_blank_c2.ptr);
    if (m->ops[2].stem_b) a.blank_need = m->blank_thr(5);
    tr_label += " [blank rows copied]";
  }
  const int oi_last = oi + op.group_followers;  // the followers run in this launch
  tr_label += " @" + std::to_string(op.oh) + "x" + std::to_string(op.ow) + " nb" + std::to_string(op.nb) +
              " tiles" + std::to_string(tiles);
  if (op.pool_in) tr_label += " <- maxpool3s2";
  if (op.in_wide) tr_label += " [hi+lo input: 2 MFMAs per weight fragment]";
  if (op.v2) tr_label += " [imgconv G=" + std::to_string(op.v2_g) + "]";
  if (op.band) tr_label += " [band: " + std::to_string(op.band) + " of " + std::to_string(op.kh) + " tap rows]";
  if (op.split) tr_label += " [split W: " + std::to_string(op.split_tiles) + " of " + std::to_string(tiles) + " tiles]";
  if (op.side_pool_partner > oi_last && op.side_pool_partner < ps.last && op.nb == 4 && !resident_ok(m, op, a)) {
    const Op& pl = m->ops[op.side_pool_partner];
    a.side_pool_out = m->buf_ptr(pl.out_buf);
    a.side_pool_og = m->buffers[pl.out_buf].geom();
    a.side_pool_goff = pl.out_coff / 8;
    ps.side_pooled[op.side_pool_partner] = 1;
    tr_label += " + maxpool3s2 on the side";
    tr_bytes += 2.0 * n * pl.oh * pl.ow * pl.cin;
  }
  const bool resident = !op.v2 && !op.pool_in && !op.pool_out && resident_ok(m, op, a);
  if (resident) tr_label += " [weights resident in LDS]";
  if (op.pool_out) tr_label += " [weights resident in LDS] -> maxpool3s2";
  TraceScope tr(ps.stream, tr_label, tr_flops, tr_bytes);
  dv::ProfileScope prof(dv::kProfConv, ps.stream);
  if (op.pool_out) {
    launch_conv_pool_resident(a, m->n_cus, ps.stream);
  } else if (op.v2) {
    dv::ImgConvArgs ia = m->imgconv_geometry(op, op.v2_g);
    ia.c = a;
    ia.n_img_tiles = (n + op.v2_g - 1) / op.v2_g;
    ia.n_cout_tiles = op.v2_tiles;
    dv::launch_imgconv(ia, op.nb, m->n_cus, ps.stream);
  } else if (op.pool_in) {
    a.stride = 2;  // documentary: the window origin is (2 oh, 2 ow)
    launch_conv_pool1x1(a, op.nb, ps.stream);
  } else if (resident) {
    launch_conv_resident(a, m->n_cus, ps.stream);
  } else {
    launch_conv(a, op.nb, ps.stream);
  }
  return op.group_followers + 1;
}

int enqueue_pool(const Pass& ps, int oi) {
  const dv_model* m = ps.m;
  const int n = ps.n;
  const Op& op = m->ops[oi];
  const BufferDesc &ib = m->buffers[op.in_buf], &ob = m->buffers[op.out_buf];
  PoolArgs p{};
  p.in = m->buf_ptr(op.in_buf);
  p.in32 = m->buf_ptr<float>(op.in_buf);
  p.out = ps.out_ptr(op.out_buf);
  p.out32 = ob.f32 ? m->buf_ptr<float>(op.out_buf) : nullptr;
  p.lo_in_groups = ib.wide ? ib.c / 8 : 0;
  p.lo_out_groups = ob.wide ? ob.c / 8 : 0;
  p.ig = ib.geom();
  p.og = ob.geom();
  p.N = n;
  p.C = op.cin;
  p.OH = op.oh;
  p.OW = op.ow;
  p.out_goff = op.out_coff / 8;
  p.shift = op.pool_shift_relu ? m->shift_ptr(op) : nullptr;
  TraceScope tr(ps.stream, std::string(op.type == kOpMaxPool ? "maxpool3s2 " : "avgpool3s1 ") +
                               std::to_string(op.cin) + " @" + std::to_string(op.oh) + "x" + std::to_string(op.ow),
                0.0, 2.0 * n * op.cin * (static_cast<double>(op.ih) * op.iw + op.oh * op.ow));
  dv::ProfileScope prof(dv::kProfOther, ps.stream);
  if (op.type == kOpMaxPool) {
    if (ib.f32 || ob.f32) return dv::fail(DV_ERR_UNSUPPORTED, "max-pool of a float32 tensor");
    launch_maxpool3s2(p, ps.stream);
  } else {
    if (!ib.f32) return dv::fail(DV_ERR_UNSUPPORTED, "average pool of an fp16 tensor");
    launch_avgpool3s1(p, ps.stream);
  }
  return 1;
}

int run_ops(dv_model* m, int first, int last, int n, hipStream_t stream,
            int shifted_buf = -1, int out_example_off = 0, size_t images_off = 0) {
  Pass ps{m, n, stream, first, last, shifted_buf, out_example_off, images_off, std::vector<char>(m->ops.size(), 0)};
  for (int oi = first; oi < last;) {
    const Op& op = m->ops[oi];
    int ran = 1;
    if (ps.side_pooled[oi]) {
      // taken on the side by a convolution of this pass (choose_side_pool)
    } else if (op.type == kOpAvgPool && op.avg_partner >= 0 && m->ops[op.avg_partner].avg_partner == oi &&
               op.avg_partner >= first) {
      // averaged in the epilogue of the launch that holds its 1x1 (choose_avg_epilogue)
    } else if (op.type != kOpConv) {
      ran = enqueue_pool(ps, oi);
    } else if (op.stem_a) {
      ran = enqueue_stem_a(ps, oi);
    } else if (op.stem_b) {
      ran = enqueue_stem_b(ps, oi);
    } else if (op.b35 == 1) {
      ran = enqueue_block35(ps, oi);
    } else if (op.m3 == 1) {
      ran = enqueue_mixed3(ps, oi);
    } else if (op.chain_len > 0) {
      ran = enqueue_chain(ps, oi);
    } else if (op.first_u8) {
      ran = enqueue_first_conv(ps, oi);
    } else {
      ran = enqueue_conv(ps, oi);
    }
    if (ran < 0) return ran;
    oi += ran;
  }
  DV_HIP_CHECK(hipGetLastError());
  return DV_OK;
}

}  // namespace

extern "C" {

int dv_model_create(const dv_model_desc* desc, int device, dv_model** out) {
  if (!desc || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_create: null");
  if (desc->channels < 1 || desc->channels > 16 || desc->num_classes < 1 ||
      desc->num_classes > 8 || desc->max_batch < 1 || desc->max_batch > 8192 ||
      desc->height < 75 ||
      desc->width < 75) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT,
                    "dv_model_create: unsupported shape (need H,W >= 75, C <= 16, max_batch <= 8192)");
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    return dv::fail(DV_ERR_NO_DEVICE, "no HIP device: libdvhip has no CPU fallback");
  }
  if (device < 0 || device >= n_dev) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "bad device ordinal");
  }
  DV_HIP_CHECK(hipSetDevice(device));
  std::unique_ptr<dv_model> m(new dv_model());
  m->device = device;
  m->desc = *desc;
  // Precise mode: on by default for inputs of more than 8 channels (the long-read models, whose deeper pile-ups do not
  // hold 1e-3 on every weight seed with fp16 activations: DESIGN.md 6), off for the short-read shapes; DV_PRECISE=0 / 1
  // overrides either way.
  m->precise = getenv("DV_PRECISE") != nullptr ? atoi(getenv("DV_PRECISE")) != 0 : desc->channels > 8;
  m->build();
  m->stem_a_grid = dv::stem_a_blocks(device);
  m->stem_b_grid = dv::stem_b_blocks(device);
  m->n_cus = dv::stem_a_blocks(device) / 2;   // stem_a runs two workgroups per CU
  // 32-bit index ranges of the kernels at max_batch (see conv_mfma_kernel's prologue)
  for (const Op& op : m->ops) {
    const BufferDesc& ob = m->buffers[op.out_buf];
    const double pieces = static_cast<double>(desc->max_batch) * ob.bytes_per_example() / 16.0;
    const double pixels = static_cast<double>(desc->max_batch) * op.oh * op.ow;
    if (pieces >= 2147483648.0 || pixels >= 67108864.0) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT,
                      "dv_model_create: max_batch too large for this image size (N*OH*OW must stay "
                      "below 2^26 and every activation tensor below 2^31 16-byte pieces)");
    }
  }
  if (static_cast<double>(desc->max_batch) * desc->height * desc->width * desc->channels >=
      2147483648.0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_create: max_batch * H * W * C must be < 2^31");
  }
  m->dbuf.resize(m->buffers.size());
  for (size_t i = 0; i < m->buffers.size(); ++i) {
    const BufferDesc& b = m->buffers[i];
    const bool stem_buf = static_cast<int>(i) < m->stem_out_buf;
    // imgconv tiles read whole groups of images and (1x1 steps of 4 channel chunks) up to
    // three chunks past the last channel: both stay inside the allocation, which is zeroed
    // to its full capacity (finite values times zero-padded weights).
    const size_t examples = std::max(
        static_cast<size_t>(stem_buf ? std::min(desc->max_batch, stem_sub_batch()) : desc->max_batch),
        static_cast<size_t>(b.min_examples));
    const size_t bytes = examples * b.bytes_per_example() +
                         static_cast<size_t>(8) * (b.h + 2 * b.halo) * (b.w + 2 * b.halo) * 16;
    if (int rc = m->dbuf[i].reserve(bytes)) return rc;
    DV_HIP_CHECK(hipMemset(m->dbuf[i].ptr, 0, m->dbuf[i].cap));  // halos stay zero forever
  }
  if (int rc = m->d_w.reserve(m->packed_halfs * 2)) return rc;
  if (int rc = m->d_shift.reserve(m->shift_floats * 4)) return rc;
  if (int rc = m->d_dense_w.reserve(static_cast<size_t>(m->feat_c) * desc->num_classes * 4)) return rc;
  if (int rc = m->d_dense_b.reserve(desc->num_classes * 4)) return rc;
  if (int rc = m->d_ext.reserve(sizeof(ExtPtrs))) return rc;
  // Skip the stem work that only sees the zero rows below the pile-up (on unless DV_BLANK_SKIP=0): needs the uint8
  // front end (the scan reads the caller's image), a single-branch 3x3 80->192 and whole dwords per image
  if (!(getenv("DV_BLANK_SKIP") != nullptr && atoi(getenv("DV_BLANK_SKIP")) == 0) &&
      m->ops[0].first_u8 && m->blank_conv4_op >= 0 && m->ops[m->blank_conv4_op].group_followers == 0 &&
      (static_cast<size_t>(desc->height) * desc->width * desc->channels) % 4 == 0) {
    if (int rc = m->d_blank_thr.reserve(static_cast<size_t>(dv_model::kBlankThrRows) * desc->max_batch * sizeof(int))) return rc;
    DV_HIP_CHECK(hipMemset(m->d_blank_thr.ptr, 0, m->d_blank_thr.cap));
    m->blank_skip = true;
    m->blank_copy_tiles = getenv("DV_BLANK_COPY_TILES") != nullptr && atoi(getenv("DV_BLANK_COPY_TILES")) != 0;
  }
  *out = m.release();
  return DV_OK;
}

void dv_model_destroy(dv_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  for (auto& b : m->dbuf) b.release();
  m->d_w.release();
  m->d_shift.release();
  m->d_dense_w.release();
  m->d_dense_b.release();
  m->d_tbl.release();
  m->d_blank_thr.release();
  m->d_ext.release();
  m->d_blank_conv4.release();
  m->d_blank_c2.release();
  m->d_blank_b.release();
  for (auto& g : m->graphs) (void)hipGraphExecDestroy(g.exec);
  delete m;
}

int64_t dv_model_num_params(const dv_model* m) { return m ? m->n_params : 0; }

int64_t dv_model_conv_macs(const dv_model* m) {
  if (!m) return 0;
  int64_t macs = 0;
  for (const Op& op : m->ops) {
    if (op.type == kOpConv) {
      macs += static_cast<int64_t>(op.kh) * op.kw * op.cin_real * op.cout * op.oh * op.ow;
    }
  }
  return macs;
}

int dv_model_num_layers(const dv_model* m) {
  return m ? static_cast<int>(m->layers.size()) : 0;
}

int dv_model_layer_info(const dv_model* m, int layer, int32_t* kh, int32_t* kw,
                        int32_t* cin, int32_t* cout, int64_t* param_offset) {
  if (!m || layer < 0 || layer >= static_cast<int>(m->layers.size())) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_layer_info: bad layer");
  }
  const LayerInfo& l = m->layers[layer];
  if (kh) *kh = l.kh;
  if (kw) *kw = l.kw;
  if (cin) *cin = l.cin;
  if (cout) *cout = l.cout;
  if (param_offset) *param_offset = l.param_off;
  return DV_OK;
}

struct HeadOutputs {   // dv_model_infer_outputs: where the head also stores the pooled vector / the logits (or null)
  float* pooled;
  float* logits;
};
static int enqueue_forward(dv_model* m, int n, hipStream_t stream, const HeadOutputs* head_out = nullptr);
static void set_ext(dv_model* m, const uint8_t* images, float* probs, hipStream_t stream,
                    const int32_t* rows_hint = nullptr, int rows_add = 0) {
  launch_set_ext(ext_table(m), images, probs, rows_hint, rows_add, stream);
}

// Blank-row skipping: the stem's response to the all-blank (all-zero) image, computed once per
// set of weights by the ordinary kernels -- the same arithmetic that produces those values
// inside a real image -- and kept as the source of the blank tiles.
static int prepare_blank_responses(dv_model* m) {
  m->blank_ready = false;
  if (!m->blank_skip) return DV_OK;
  for (auto& g : m->graphs) {   // captured without the blank arguments
    (void)hipStreamSynchronize(g.stream);
    (void)hipGraphExecDestroy(g.exec);
  }
  m->graphs.clear();
  const size_t img_bytes = static_cast<size_t>(m->desc.height) * m->desc.width * m->desc.channels;
  dv::DeviceBuffer zero_img, probs;
  int rc = zero_img.reserve(img_bytes);
  if (rc == DV_OK) rc = probs.reserve(sizeof(float) * m->desc.num_classes);
  if (rc == DV_OK && hipMemset(zero_img.ptr, 0, img_bytes) != hipSuccess) rc = dv::fail(DV_ERR_HIP, "hipMemset");
  if (rc == DV_OK) {
    set_ext(m, static_cast<const uint8_t*>(zero_img.ptr), static_cast<float*>(probs.ptr), nullptr);
    rc = enqueue_forward(m, 1, nullptr);
  }
  if (rc == DV_OK && hipDeviceSynchronize() != hipSuccess) rc = dv::fail(DV_ERR_HIP, "blank forward failed");
  auto keep = [&](int buf, dv::DeviceBuffer* dst) {
    if (rc != DV_OK || buf < 0 || m->buffers[buf].h <= 1) return;   // (LDS-only tensors have no buffer)
    const size_t bytes = m->buffers[buf].bytes_per_example();
    rc = dst->reserve(bytes);
    if (rc == DV_OK && hipMemcpy(dst->ptr, m->dbuf[buf].ptr, bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
      rc = dv::fail(DV_ERR_HIP, "copying the blank response");
    }
  };
  keep(m->ops[m->blank_conv4_op].out_buf, &m->d_blank_conv4);
  keep(m->ops[1].out_buf, &m->d_blank_c2);                               // conv2 (stem_a's output)
  if (m->ops[2].stem_b) keep(m->ops[3].out_buf, &m->d_blank_b);          // the 1x1 64->80 (stem_b's output)
  zero_img.release();
  probs.release();
  if (rc != DV_OK) return rc;
  m->blank_ready = true;
  return DV_OK;
}

int dv_model_load_weights(dv_model* m, const float* weights, int64_t n) {
  if (!m || !weights) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_load_weights: null");
  if (n != m->n_params) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT,
                    "dv_model_load_weights: expected " + std::to_string(m->n_params) +
                        " values, got " + std::to_string(n));
  }
  DV_HIP_CHECK(hipSetDevice(m->device));
  std::vector<_Float16> packed(m->packed_halfs, static_cast<_Float16>(0.f));
  std::vector<float> shift(m->shift_floats, 0.f);
  for (const Op& op : m->ops) {
    if (op.type != kOpConv) continue;
    const LayerInfo& l = m->layers[op.layer];
    const float* var = weights + l.param_off + static_cast<size_t>(l.kh) * l.kw * l.cin * l.cout + 2 * l.cout;
    for (int co = 0; co < l.cout; ++co) {
      if (!(var[co] + 1e-3f > 0.f)) return dv::fail(DV_ERR_BAD_INPUT, "non-positive BatchNorm variance");
    }
  }
  // One conv layer's weights -> its fragment image.  Layers write disjoint parts of `packed` and
  // `shift` (the siblings of a grouped launch share a region but own different cout rows), so
  // they are packed on a few host threads: the 22 M weights are read with a stride of cout and
  // one thread needs 0.2-0.3 s for them -- as long as a 100 kb make_examples run takes.
  auto pack_op = [&](size_t oi) {
    const Op& op = m->ops[oi];
    if (op.type != kOpConv) return;
    const LayerInfo& l = m->layers[op.layer];
    const float* w = weights + l.param_off;  // HWIO
    const size_t wn = static_cast<size_t>(l.kh) * l.kw * l.cin * l.cout;
    const float* beta = w + wn;
    const float* mean = beta + l.cout;
    const float* var = mean + l.cout;
    std::vector<float> inv(l.cout);
    for (int co = 0; co < l.cout; ++co) {
      inv[co] = 1.0f / std::sqrt(var[co] + 1e-3f);
      shift[op.shift_off + co] = beta[co] - mean[co] * inv[co];
    }
    if ((m->ops[0].stem_a && oi < 2) || (m->ops[2].stem_b && (oi == 2 || oi == 3))) {
      _Float16* dst = packed.data() + op.w_off;   // fused stem: stem.hip's own fragment images
      if (oi == 0 && l.cin > 8) dv::pack_stem_a_w1_wide(w, inv.data(), l.cin, dst);
      if (oi == 0 && l.cin <= 8) dv::pack_stem_a_w1(w, inv.data(), l.cin, dst);
      if (oi == 1) dv::pack_stem_a_w2(w, inv.data(), dst);
      if (oi == 2) dv::pack_stem_b_w3(w, inv.data(), dst);
      if (oi == 3) dv::pack_stem_b_w4(w, inv.data(), l.cout, dst);
      return;
    }
    if (op.first_u8) {
      // C <= 8:  [chunk kc][k-group g = tap 2kc+g][cout][8]: channel c < cin_real, else zero
      // C <= 16: [chunk kc = tap][k-group g = channels 8g..8g+7][cout][8]
      const bool wide = l.cin > 8;
      for (int kc = 0; kc < op.n_chunks; ++kc)
        for (int g = 0; g < 2; ++g) {
          const int tap = wide ? kc : 2 * kc + g;
          if (tap >= op.kh * op.kw) continue;
          const int kh = tap / op.kw, kw = tap % op.kw;
          for (int co = 0; co < op.cout; ++co)
            for (int ci = wide ? 8 * g : 0; ci < (wide ? std::min(l.cin, 8 * g + 8) : l.cin); ++ci) {
              const float v = w[((static_cast<size_t>(kh) * l.kw + kw) * l.cin + ci) * l.cout + co];
              packed[op.w_off + ((static_cast<size_t>(kc) * 2 + g) * 32 + co) * 8 + (ci & 7)] =
                  static_cast<_Float16>(v * inv[co]);
            }
        }
      return;
    }
    if (op.b35 >= 1 && op.b35 <= 4) {
      // block35.hip's heads: [pass][channel chunk][k-group][128 couts][8]; pass 0 = 5x5 reducer (couts 0..) + 3x3
      // reducer (64..), pass 1 = b1 (0..) + pooled projection (64..)
      const int pass = op.b35 == 1 || op.b35 == 4 ? 1 : 0, base = op.b35 == 1 || op.b35 == 2 ? 0 : 64;
      const int n_chunks = l.cin / kChunk;
      _Float16* dst = packed.data() + op.w_off;
      for (int cc = 0; cc < n_chunks; ++cc)
        for (int co = 0; co < op.cout; ++co)
          for (int jj = 0; jj < kChunk; ++jj) {
            const float v = w[static_cast<size_t>(cc * kChunk + jj) * l.cout + co];
            dst[(((static_cast<size_t>(pass) * n_chunks + cc) * 2 + jj / 8) * 128 + base + co) * 8 + (jj % 8)] =
                static_cast<_Float16>(v * inv[co]);
          }
      return;
    }
    if (op.m3 == 1) {
      // mixed3.hip's 1x1: [channel chunk][k-group][64 couts][8]
      _Float16* dst = packed.data() + op.w_off;
      for (int cc = 0; cc < l.cin / kChunk; ++cc)
        for (int co = 0; co < op.cout; ++co)
          for (int jj = 0; jj < kChunk; ++jj) {
            const float v = w[static_cast<size_t>(cc * kChunk + jj) * l.cout + co];
            dst[((static_cast<size_t>(cc) * 2 + jj / 8) * dv::kMixed3Red + co) * 8 + (jj % 8)] = static_cast<_Float16>(v * inv[co]);
          }
      return;
    }
    if (op.chain_len > 0 || op.in_chain || op.b35 >= 5 || op.m3 >= 2) {
      // chain.hip, block35.hip, mixed3.hip: [channel chunk][tap][k-group][cout_pad][8]
      const int cout_pad = (op.cout + 31) / 32 * 32, taps = op.kh * op.kw;
      _Float16* dst = packed.data() + op.w_off;
      for (int cc = 0; cc < l.cin / kChunk; ++cc)
        for (int tap = 0; tap < taps; ++tap) {
          const int kh = tap / op.kw, kw = tap % op.kw;
          for (int co = 0; co < op.cout; ++co)
            for (int jj = 0; jj < kChunk; ++jj) {
              const int ci = cc * kChunk + jj;
              const float v = w[((static_cast<size_t>(kh) * l.kw + kw) * l.cin + ci) * l.cout + co];
              dst[(((static_cast<size_t>(cc) * taps + tap) * 2 + jj / 8) * cout_pad + co) * 8 + (jj % 8)] =
                  static_cast<_Float16>(v * inv[co]);
            }
        }
      return;
    }
    // Row of this op's cout `co` in the launch's concatenated cout space: the siblings
    // grouped before it (leader first) each occupy whole 32-cout subtiles.
    int sub0 = 0;
    {
      size_t lead = oi;
      while (lead > 0 && m->ops[lead].group_followers == 0 && m->ops[lead - 1].type == kOpConv &&
             m->ops[lead - 1].w_off == op.w_off) {
        --lead;  // walk back to the leader (all ops of a launch share w_off)
      }
      for (size_t j = lead; j < oi; ++j) sub0 += (m->ops[j].cout + 31) / 32;
    }
    const int bn = op.nb * 32;
    const int taps = op.kh * op.kw;
    {
      // the launch's leader carries the imgconv decision
      size_t lead = oi;
      while (lead > 0 && m->ops[lead].group_followers == 0 && m->ops[lead - 1].type == kOpConv &&
             m->ops[lead - 1].w_off == op.w_off) {
        --lead;
      }
      const Op& lo = m->ops[lead];
      if (lo.v2) {
        // [cout tile][step][chunk in step][tap][k-group][bn couts][8]
        const int kcs = dv::imgconv_kc(op.kh, op.kw);
        const size_t slab = dv::imgconv_wslab_halfs(op.kh, op.kw, op.nb);
        for (int cc = 0; cc < l.cin / kChunk + (l.cin % kChunk ? 1 : 0); ++cc) {
          const int st = cc / kcs, kc = cc % kcs;
          for (int tap = 0; tap < taps; ++tap) {
            const int kh = tap / op.kw, kw = tap % op.kw;
            for (int co = 0; co < op.cout; ++co) {
              const int row = sub0 * 32 + co;
              const int t = row / bn, r = row % bn;
              _Float16* sub = packed.data() + op.w_off +
                              (static_cast<size_t>(t) * lo.v2_steps + st) * slab +
                              (static_cast<size_t>(kc) * taps + tap) * 2 * bn * 8;
              for (int jj = 0; jj < kChunk; ++jj) {
                const int ci = cc * kChunk + jj;
                if (ci >= l.cin) continue;
                const float v = w[((static_cast<size_t>(kh) * l.kw + kw) * l.cin + ci) * l.cout + co];
                sub[(static_cast<size_t>(jj / 8) * bn + r) * 8 + (jj % 8)] = static_cast<_Float16>(v * inv[co]);
              }
            }
          }
        }
        return;
      }
    }
    // row-band mode: one image per output row `band_r`, holding the op.band tap rows
    // kh = pad_h - band_r + 0..band-1 that meet map rows 0..band-1
    const int eff_taps = op.band ? op.band * op.kw : taps;
    const int n_tiles_op = ((op.cout + 31) / 32 + op.nb - 1) / op.nb;   // band ops are never grouped
    // split rows: chunk 2q = W_hi, chunk 2q + 1 = W_lo of pixel chunk q; plain rows of a split launch
    // (siblings that are not split) use the first half of the launch's chunk slots
    const int parts = op.split_rows ? 2 : 1;
    const int op_chunks = op.split && !op.split_rows ? op.n_chunks / 2 : op.n_chunks;
    for (int band_r = 0; band_r < (op.band ? op.band : 1); ++band_r)
    for (int kc = 0; kc < op_chunks; ++kc) {
      const int sl = kc / kSlabChunks, j = kc % kSlabChunks;
      const int q = kc / parts, part = kc % parts;
      const int cc = q / eff_taps, tap = q % eff_taps;  // chunk-major, tap-minor (ChunkWalk)
      const int kh = tap / op.kw + (op.band ? op.pad_h - band_r : 0), kw = tap % op.kw;
      for (int co = 0; co < op.cout; ++co) {
        const int row = sub0 * 32 + co;
        const int t = row / bn + band_r * n_tiles_op, r = row % bn;
        // chunk image [k-group g][cout r][8]: matches conv_mfma_kernel's frag_off
        _Float16* chunk = packed.data() + op.w_off +
                          ((static_cast<size_t>(t) * op.n_steps + sl) * kSlabChunks + j) * bn * kChunk;
        for (int jj = 0; jj < kChunk; ++jj) {
          const int ci = cc * kChunk + jj;
          if (ci >= l.cin) continue;  // padded input channels
          const float v = w[((static_cast<size_t>(kh) * l.kw + kw) * l.cin + ci) * l.cout + co] * inv[co];
          const _Float16 hi = static_cast<_Float16>(v);
          chunk[(static_cast<size_t>(jj / 8) * bn + r) * 8 + (jj % 8)] =
              part == 0 ? hi : static_cast<_Float16>(v - static_cast<float>(hi));
        }
      }
    }
  };
  {
    std::atomic<size_t> next{0};
    auto work = [&] {
      for (size_t oi = next.fetch_add(1); oi < m->ops.size(); oi = next.fetch_add(1)) pack_op(oi);
    };
    const unsigned helpers = std::min(7u, std::max(1u, std::thread::hardware_concurrency()) - 1);
    std::vector<std::thread> threads;
    for (unsigned t = 0; t < helpers; ++t) threads.emplace_back(work);
    work();
    for (std::thread& t : threads) t.join();
  }
  const LayerInfo& dl = m->layers.back();
  const float* dw = weights + dl.param_off;
  DV_HIP_CHECK(hipMemcpy(m->d_w.ptr, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
  DV_HIP_CHECK(hipMemcpy(m->d_shift.ptr, shift.data(), shift.size() * 4, hipMemcpyHostToDevice));
  DV_HIP_CHECK(hipMemcpy(m->d_dense_w.ptr, dw, static_cast<size_t>(dl.cin) * dl.cout * 4,
                         hipMemcpyHostToDevice));
  DV_HIP_CHECK(hipMemcpy(m->d_dense_b.ptr, dw + static_cast<size_t>(dl.cin) * dl.cout,
                         dl.cout * 4, hipMemcpyHostToDevice));
  m->h_shift = shift;
  m->h_dense_b.assign(dw + static_cast<size_t>(dl.cin) * dl.cout, dw + static_cast<size_t>(dl.cin) * dl.cout + dl.cout);
  m->loaded = true;
  return prepare_blank_responses(m);
}

// The op list as calib.h's plan of plain NHWC tensors: fused pools unfolded (pool_in / pool_out), LDS-only
// tensors given their real size, and the tensors the product keeps wider than fp16 marked (keep_f32).
// Bump CALIBRATION_PLAN_VERSION (inception_v3.py) when keep_f32, the splits or the stem rounding points change.
static dv::CalibPlan calib_plan_of(const dv_model* m) {
  dv::CalibPlan plan;
  plan.bufs.resize(m->buffers.size());
  for (size_t b = 0; b < m->buffers.size(); ++b) plan.bufs[b] = {m->buffers[b].h, m->buffers[b].w, m->buffers[b].c};
  plan.bufs[0] = {m->desc.height, m->desc.width, m->desc.channels};
  for (const Op& op : m->ops) {
    dv::CalibOp c{};
    c.type = op.type == kOpConv ? 0 : op.type == kOpMaxPool ? 1 : 2;
    c.in_buf = op.in_buf;
    c.out_buf = op.out_buf;
    c.out_coff = op.out_coff;
    c.shift_off = -1;
    int oh = op.oh, ow = op.ow;
    if (op.type == kOpConv) {
      c.pool_in = op.pool_in;
      c.pool_out = op.pool_out;
      c.kh = op.kh;
      c.kw = op.kw;
      c.stride = op.stride;
      c.pad_h = op.pad_h;
      c.pad_w = op.pad_w;
      c.cin = op.cin_real;
      c.cout = op.cout;
      c.w_off = m->layers[op.layer].param_off;
      c.raw = op.raw;
      c.shift_off = static_cast<int64_t>(op.shift_off);
      c.split = op.split_rows;
      c.keep_f32 = m->buffers[op.out_buf].f32 || m->buffers[op.out_buf].wide ? 1 : 0;
      if (op.pool_in) {   // op.ih / op.iw: the tensor as stored, before the on-the-fly pool
        plan.bufs[op.in_buf].h = op.ih;
        plan.bufs[op.in_buf].w = op.iw;
      }
      if (op.pool_out) {
        oh = (oh - 3) / 2 + 1;
        ow = (ow - 3) / 2 + 1;
      }
    } else if (op.type == kOpAvgPool) {
      c.shift_relu = op.pool_shift_relu;
      if (op.pool_shift_relu) c.shift_off = static_cast<int64_t>(op.shift_off);
      c.cout = op.cout;
      c.keep_f32 = m->buffers[op.out_buf].f32 || m->buffers[op.out_buf].wide ? 1 : 0;
    } else {
      c.cout = op.cout;
    }
    plan.bufs[op.out_buf].h = oh;   // LDS-only tensors of the fused kernels are 1 x 1 in `buffers`
    plan.bufs[op.out_buf].w = ow;
    plan.ops.push_back(c);
  }
  plan.feat_buf = m->feat_buf;
  plan.num_classes = m->desc.num_classes;
  plan.dense_off = m->layers.back().param_off;
  return plan;
}

// Shift calibration (include/dvhip.h, csrc/calib.h): the op list as a plan of plain NHWC tensors --
// fused pools unfolded (pool_in / pool_out), LDS-only tensors given their real size -- run through
// the two fp32 pipelines; shifts and the Dense bias move by the mean differences.
int dv_model_calibrate(dv_model* m, const float* weights, int64_t n_weights, const uint8_t* images, int n_images,
                       float* corrections, int64_t capacity) {
  if (!m || !weights || !images) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_calibrate: null");
  if (!m->loaded) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_calibrate: load weights first");
  if (n_weights != m->n_params) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_calibrate: wrong number of weights");
  if (n_images < 1 || n_images > 4096) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_calibrate: 1..4096 images");
  const dv::CalibPlan plan = calib_plan_of(m);
  std::vector<float> corr, dense_corr;
  if (int rc = dv::run_calibration(plan, m->device, weights, n_weights, m->h_shift, images, n_images, &corr,
                                   &dense_corr)) {
    return rc;
  }
  std::vector<float> shift = m->h_shift, dense_b = m->h_dense_b;
  for (size_t i = 0; i < shift.size(); ++i) shift[i] -= corr[i];
  for (size_t k = 0; k < dense_b.size(); ++k) dense_b[k] -= dense_corr[k];
  DV_HIP_CHECK(hipSetDevice(m->device));
  DV_HIP_CHECK(hipDeviceSynchronize());
  DV_HIP_CHECK(hipMemcpy(m->d_shift.ptr, shift.data(), shift.size() * 4, hipMemcpyHostToDevice));
  DV_HIP_CHECK(hipMemcpy(m->d_dense_b.ptr, dense_b.data(), dense_b.size() * 4, hipMemcpyHostToDevice));
  if (corrections != nullptr) {
    int64_t at = 0;
    for (size_t off : m->correction_shift_offsets()) {
      if (at < capacity) corrections[at++] = corr[off];
    }
    for (size_t k = 0; k < dense_corr.size() && at < capacity; ++k) corrections[at++] = dense_corr[k];
  }
  return prepare_blank_responses(m);
}

int dv_model_apply_corrections(dv_model* m, const float* corrections, int64_t n) {
  if (!m || !corrections) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_apply_corrections: null");
  if (!m->loaded) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_apply_corrections: load weights first");
  const std::vector<size_t> offs = m->correction_shift_offsets();
  if (n != static_cast<int64_t>(offs.size() + m->h_dense_b.size())) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_apply_corrections: wrong number of corrections");
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(corrections[i])) return dv::fail(DV_ERR_BAD_INPUT, "dv_model_apply_corrections: non-finite correction");
  }
  std::vector<float> shift = m->h_shift, dense_b = m->h_dense_b;
  int64_t at = 0;
  for (size_t off : offs) shift[off] -= corrections[at++];
  for (size_t k = 0; k < dense_b.size(); ++k) dense_b[k] -= corrections[at++];
  DV_HIP_CHECK(hipSetDevice(m->device));
  DV_HIP_CHECK(hipDeviceSynchronize());
  DV_HIP_CHECK(hipMemcpy(m->d_shift.ptr, shift.data(), shift.size() * 4, hipMemcpyHostToDevice));
  DV_HIP_CHECK(hipMemcpy(m->d_dense_b.ptr, dense_b.data(), dense_b.size() * 4, hipMemcpyHostToDevice));
  return prepare_blank_responses(m);
}

// Diagnostic (include/dvhip.h): the calibration's two fp32 pipelines as a probe of WHERE the fp16 error enters.
int dv_model_num_ops(const dv_model* m) { return m ? static_cast<int>(m->ops.size()) : 0; }

int dv_model_op_label(const dv_model* m, int op_index, char* buf, int capacity) {
  if (!m || !buf || capacity < 1 || op_index < 0 || op_index >= static_cast<int>(m->ops.size())) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_op_label: bad argument");
  }
  const Op& op = m->ops[op_index];
  const char* kind = op.type == kOpConv ? "conv" : op.type == kOpMaxPool ? "maxpool" : "avgpool";
  snprintf(buf, static_cast<size_t>(capacity), "%s layer=%d k=%dx%d s=%d cin=%d cout=%d out=%dx%d raw=%d in_buf=%d out_buf=%d coff=%d lds_only=%d",
           kind, op.layer, op.kh, op.kw, op.stride, op.cin, op.cout, op.oh, op.ow, op.raw ? 1 : 0, op.in_buf, op.out_buf,
           op.out_coff, (op.type == kOpConv && (op.stem_a || op.stem_b)) || (op_index + 1 < static_cast<int>(m->ops.size()) && m->ops[op_index + 1].in_chain && m->ops[op_index + 1].in_buf == op.out_buf) ||
               (op.b35 >= 2 && op.b35 <= 4) || op.b35 == 6 || op.m3 == 1 || op.m3 == 2 ? 1 : 0);
  return DV_OK;
}

int dv_model_probe_rounding(dv_model* m, const float* weights, int64_t n_weights, const uint8_t* images, int n_images,
                            const uint8_t* keep_f32, int flags, const float* corrections, int64_t n_corrections,
                            float* logits_r, float* logits_e, float* corrections_out) {
  if (!m || !weights || !images || !logits_e) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_probe_rounding: null");
  if (!m->loaded) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_probe_rounding: load weights first");
  if (n_weights != m->n_params) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_probe_rounding: wrong number of weights");
  if (n_images < 1 || n_images > 4096) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_probe_rounding: 1..4096 images");
  dv::CalibPlan plan = calib_plan_of(m);
  if (keep_f32 != nullptr) {
    for (size_t i = 0; i < plan.ops.size(); ++i) plan.ops[i].keep_f32 = keep_f32[i] ? 1 : 0;
  }
  std::vector<float> corr_in(m->h_shift.size(), 0.f), dense_in(m->h_dense_b.size(), 0.f);
  if (corrections != nullptr) {
    const std::vector<size_t> offs = m->correction_shift_offsets();
    if (n_corrections != static_cast<int64_t>(offs.size() + dense_in.size())) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_probe_rounding: wrong number of corrections");
    int64_t at = 0;
    for (size_t off : offs) corr_in[off] = corrections[at++];
    for (size_t k = 0; k < dense_in.size(); ++k) dense_in[k] = corrections[at++];
  }
  const bool measure = (flags & 2) != 0;   // the calibration proper under this plan: corrections measured on these images
  if (measure && corrections != nullptr) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_probe_rounding: measure or apply");
  dv::CalibProbe probe;
  probe.corr_in = measure ? nullptr : corr_in.data();
  probe.dense_corr_in = measure ? nullptr : dense_in.data();
  probe.logits_r = logits_r;
  probe.logits_e = logits_e;
  probe.skip_r = logits_r == nullptr && !measure;
  probe.weights_f32 = (flags & 1) != 0;
  std::vector<float> corr, dense_corr;
  if (int rc = dv::run_calibration(plan, m->device, weights, n_weights, m->h_shift, images, n_images, &corr, &dense_corr,
                                   &probe)) {
    return rc;
  }
  if (corrections_out != nullptr) {
    int64_t at = 0;
    for (size_t off : m->correction_shift_offsets()) corrections_out[at++] = corr[off];
    for (float v : dense_corr) corrections_out[at++] = v;
  }
  return DV_OK;
}

// Testing hook: copies activation buffer `index` (NHWC fp16, first n examples)
// to host memory; returns its shape.  Buffer 0 is the preprocessed input.
int dv_model_debug_tensor(dv_model* m, int index, int n, void* host_out, int32_t* h,
                          int32_t* w, int32_t* c) {
  if (m && index == -1) index = m->feat_buf;      // the last block's output (input of the head)
  if (m && index == -2) index = m->stem_out_buf;  // the stem's output (input of mixed0)
  if (!m || index < 0 || index >= static_cast<int>(m->buffers.size())) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_debug_tensor: bad index");
  }
  const BufferDesc& b = m->buffers[index];
  // reports the PADDED plane size (interior + 2*halo on each axis)
  if (h) *h = b.h + 2 * b.halo;
  if (w) *w = b.w + 2 * b.halo;
  if (c) *c = b.c;
  if (host_out) {
    DV_HIP_CHECK(hipSetDevice(m->device));
    DV_HIP_CHECK(hipDeviceSynchronize());
    if (b.f32) {   // float32 tensors (BufferDesc::f32) leave as the fp16 numbers the hook's contract promises
      std::vector<float> tmp(static_cast<size_t>(n) * b.bytes_per_example() / 4);
      DV_HIP_CHECK(hipMemcpy(tmp.data(), m->dbuf[index].ptr, tmp.size() * 4, hipMemcpyDeviceToHost));
      _Float16* dst = static_cast<_Float16*>(host_out);
      for (size_t i = 0; i < tmp.size(); ++i) dst[i] = static_cast<_Float16>(tmp[i]);
    } else if (b.wide) {   // wide tensors (precise mode) leave as hi + lo, rounded to the fp16 the hook's contract promises
      const size_t half_halfs = b.bytes_per_example() / 4;   // fp16 numbers of the hi (= of the lo) part of one example
      std::vector<_Float16> tmp(static_cast<size_t>(n) * half_halfs * 2);
      DV_HIP_CHECK(hipMemcpy(tmp.data(), m->dbuf[index].ptr, tmp.size() * 2, hipMemcpyDeviceToHost));
      _Float16* dst = static_cast<_Float16*>(host_out);
      for (int e = 0; e < n; ++e)
        for (size_t i = 0; i < half_halfs; ++i) {
          dst[static_cast<size_t>(e) * half_halfs + i] = static_cast<_Float16>(
              static_cast<float>(tmp[static_cast<size_t>(e) * 2 * half_halfs + i]) +
              static_cast<float>(tmp[static_cast<size_t>(e) * 2 * half_halfs + half_halfs + i]));
        }
    } else {
      DV_HIP_CHECK(hipMemcpy(host_out, m->dbuf[index].ptr,
                             static_cast<size_t>(n) * b.bytes_per_example(),
                             hipMemcpyDeviceToHost));
    }
  }
  return DV_OK;
}

// Enqueues the whole forward for `n` examples on `stream` (eager launches).  The caller's image
// and probability pointers come from the device-side table (set_ext), not from kernel arguments.
// `head_out`: head_outputs_kernel instead of head_kernel.
static int enqueue_forward(dv_model* m, int n, hipStream_t stream, const HeadOutputs* head_out) {
  const size_t img_bytes = static_cast<size_t>(m->desc.height) * m->desc.width * m->desc.channels;
  const ExtPtrs* ext = ext_table(m);
  // split evenly so that no launch is left with a sliver of a batch
  const int n_parts = (n + m->desc.max_batch - 1) / m->desc.max_batch;
  const int part = n_parts ? (n + n_parts - 1) / n_parts : 0;
  for (int done = 0; done < n; done += part) {
    const int nb = std::min(part, n - done);
    for (int sb0 = 0; sb0 < nb; sb0 += stem_sub_batch()) {
      const int sb = std::min(stem_sub_batch(), nb - sb0);
      const size_t img_off = static_cast<size_t>(done + sb0) * img_bytes;
      if (m->blank_on()) {
        dv::ProfileScope prof(dv::kProfOther, stream);
        const Op& c4 = m->ops[m->blank_conv4_op];
        launch_blank_scan(ext, img_off, done + sb0, sb, m->desc.height, m->desc.width * m->desc.channels,
                          static_cast<int*>(m->d_blank_thr.ptr), m->desc.max_batch, m->ops[1].oh, m->ops[3].oh, c4.ow,
                          c4.pool_out ? m->buffers[c4.out_buf].h : c4.oh, m->ops[2].stem_b ? 1 : 0, c4.pool_out ? 1 : 0,
                          stream);
      }
      if (!m->ops[0].first_u8) {
        dv::ProfileScope prof(dv::kProfOther, stream);
        launch_preprocess(ext, img_off, m->buf_ptr(0), sb, m->desc.channels, m->desc.height, m->desc.width,
                          m->buffers[0].geom(), stream);
      }
      if (int rc = run_ops(m, 0, m->stem_ops_end, sb, stream, m->stem_out_buf, sb0, img_off)) return rc;
    }
    if (int rc = run_ops(m, m->stem_ops_end, static_cast<int>(m->ops.size()), nb, stream)) {
      return rc;
    }
    {
      dv::ProfileScope prof(dv::kProfOther, stream);
      const bool outs = head_out != nullptr;
      launch_head(m->buf_ptr<float>(m->feat_buf), static_cast<const float*>(m->d_dense_w.ptr),
                  static_cast<const float*>(m->d_dense_b.ptr), ext, static_cast<size_t>(done) * m->desc.num_classes,
                  m->buffers[m->feat_buf].geom(), m->desc.num_classes, nb, outs,
                  outs && head_out->pooled ? head_out->pooled + static_cast<size_t>(done) * m->feat_c : nullptr,
                  outs && head_out->logits ? head_out->logits + static_cast<size_t>(done) * m->desc.num_classes : nullptr,
                  stream);
    }
  }
  return DV_OK;
}

int dv_model_infer(dv_model* m, const uint8_t* images, int n, float* probs, void* stream_v) {
  return dv_model_infer_rows(m, images, n, probs, nullptr, 0, stream_v);
}

int dv_model_infer_rows(dv_model* m, const uint8_t* images, int n, float* probs, const int32_t* rows_used, int rows_add,
                        void* stream_v) {
  if (!m || !images || !probs || n < 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_infer: bad argument");
  }
  if (!m->loaded) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_infer: no weights loaded");
  if (n == 0) return DV_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  DV_HIP_CHECK(hipSetDevice(m->device));
  // The forward is ~65 launches; replaying it as one hipGraph removes the per-launch gaps
  // (measured +0.6 % at 8 K examples per forward, more for small batches).  Graphs are keyed by
  // (n, stream) only: the caller's pointers travel through the ExtPtrs table, written in stream
  // order ahead of every forward, so fresh image tensors per region replay the same graph.
  // Per-launch event profiling and DV_OP_TRACE need eager launches, and the legacy default
  // stream cannot be captured.
  static const bool op_trace = getenv("DV_OP_TRACE") != nullptr;
  static const bool no_graph = getenv("DV_NO_GRAPH") != nullptr || op_trace;
  // a caller that is already capturing this stream gets plain launches (they join ITS graph)
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (stream != nullptr) (void)hipStreamIsCapturing(stream, &capturing);
  set_ext(m, images, probs, stream, rows_used, rows_add);
  if (no_graph || dv::profiling_enabled() || stream == nullptr ||
      capturing != hipStreamCaptureStatusNone) {
    static std::vector<OpTrace> trace_store;
    g_trace = op_trace ? &trace_store : nullptr;
    if (int rc = enqueue_forward(m, n, stream)) return rc;
    DV_HIP_CHECK(hipGetLastError());
    if (op_trace) dump_trace(stream);
    return DV_OK;
  }
  for (const dv_model::GraphEntry& g : m->graphs) {
    if (g.n == n && g.stream == stream) {
      DV_HIP_CHECK(hipGraphLaunch(g.exec, stream));
      ++m->graph_replays;
      return DV_OK;
    }
  }
  hipGraph_t graph = nullptr;
  DV_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
  const int rc = enqueue_forward(m, n, stream);
  const hipError_t ce = hipStreamEndCapture(stream, &graph);
  if (rc != DV_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (ce != hipSuccess || graph == nullptr) {
    return dv::fail(DV_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
  }
  dv_model::GraphEntry e{n, stream, nullptr};
  const hipError_t ie = hipGraphInstantiate(&e.exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ie != hipSuccess) {
    return dv::fail(DV_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
  }
  if (m->graphs.size() >= 8) {  // bounded cache; the evicted replay may still be in flight
    (void)hipStreamSynchronize(m->graphs.front().stream);
    (void)hipGraphExecDestroy(m->graphs.front().exec);
    m->graphs.erase(m->graphs.begin());
  }
  m->graphs.push_back(e);
  ++m->graph_captures;
  DV_HIP_CHECK(hipGraphLaunch(e.exec, stream));
  return DV_OK;
}

// 1 when the model runs in precise mode (include/dvhip.h).
int dv_model_is_precise(const dv_model* m) { return m && m->precise ? 1 : 0; }

// Blank-row skipping on / off at run time (include/dvhip.h): bench.py times the dense path on the same model.
int dv_model_set_blank_skip(dv_model* m, int enabled) {
  if (!m) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_set_blank_skip: null");
  const bool on = enabled != 0;
  if (on == m->blank_enabled) return DV_OK;
  DV_HIP_CHECK(hipSetDevice(m->device));
  for (auto& g : m->graphs) {   // captured with the other setting
    (void)hipStreamSynchronize(g.stream);
    (void)hipGraphExecDestroy(g.exec);
  }
  m->graphs.clear();
  m->blank_enabled = on;
  return DV_OK;
}

// The thresholds the last forward's scan found for its first `n` examples: out[k * n + i], k = 0 rows used (first
// all-zero row), 1 conv2 rows, 2 stem_b rows, 3 the 3x3 80->192's rows, 4 its pooled rows.  Returns
// DV_ERR_UNSUPPORTED when the model does not skip (shape without the uint8 front end, DV_BLANK_SKIP=0, switched off).
int dv_model_blank_thresholds(dv_model* m, int n, int32_t* out) {
  if (!m || !out || n < 1 || n > m->desc.max_batch) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_blank_thresholds: bad argument");
  if (!m->blank_on()) return dv::fail(DV_ERR_UNSUPPORTED, "dv_model_blank_thresholds: blank-row skipping is off for this model");
  DV_HIP_CHECK(hipSetDevice(m->device));
  DV_HIP_CHECK(hipDeviceSynchronize());
  for (int k = 0; k < 5; ++k) {
    DV_HIP_CHECK(hipMemcpy(out + static_cast<size_t>(k) * n,
                           static_cast<const int*>(m->d_blank_thr.ptr) + static_cast<size_t>(k) * m->desc.max_batch,
                           static_cast<size_t>(n) * sizeof(int), hipMemcpyDeviceToHost));
  }
  return DV_OK;
}

// dv_model_infer_outputs' names: the block outputs of named_views, then the head's two vectors.
namespace {
struct OutputView {
  int buf = -1;            // named_views' buffer, or -1: a head output
  int coff = 0, c = 0;     // channel range
  int h = 1, w = 1;
  bool logits = false;     // head output: the logits (else the pooled vector)
};
}  // namespace

static int resolve_output(const dv_model* m, const char* name, OutputView* v, const char* fn) {
  const std::string s = name != nullptr ? name : "";
  std::string known;
  for (const dv_model::NamedView& nv : m->named_views) {
    if (s == nv.name) {
      const BufferDesc& b = m->buffers[nv.buf];
      *v = OutputView{nv.buf, nv.coff, nv.c, b.h, b.w, false};
      return DV_OK;
    }
    known += nv.name + ", ";
  }
  if (s == "prelogits") {
    *v = OutputView{-1, 0, m->feat_c, 1, 1, false};
    return DV_OK;
  }
  if (s == "logits") {
    *v = OutputView{-1, 0, m->desc.num_classes, 1, 1, true};
    return DV_OK;
  }
  return dv::fail(DV_ERR_INVALID_ARGUMENT, std::string(fn) + ": unknown output name '" + s + "' (accepted: " + known +
                                               "prelogits, logits)");
}

int dv_model_output_info(const dv_model* m, const char* name, int32_t* h, int32_t* w, int32_t* c) {
  if (!m) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_output_info: null");
  OutputView v;
  if (int rc = resolve_output(m, name, &v, "dv_model_output_info")) return rc;
  if (h) *h = v.h;
  if (w) *w = v.w;
  if (c) *c = v.c;
  return DV_OK;
}

// One forward of at most max_batch examples with eager launches (never captured: the plain forward's graphs stay as
// they are), the head that also stores its two vectors, then one export launch per requested block output -- every
// block output is still live at the end of the forward (dv_model::named_views).
int dv_model_infer_outputs(dv_model* m, const uint8_t* images, int n, float* probs, int n_outputs,
                           const char* const* names, float* const* outs, void* stream_v) {
  if (!m || !images || !probs || n < 0 || n_outputs < 0 || (n_outputs > 0 && (!names || !outs))) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_infer_outputs: bad argument");
  }
  if (n > m->desc.max_batch) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_infer_outputs: n = " + std::to_string(n) + " is above max_batch = " +
                                                 std::to_string(m->desc.max_batch));
  }
  if (!m->loaded) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_infer_outputs: no weights loaded");
  std::vector<OutputView> views(n_outputs);
  HeadOutputs head{nullptr, nullptr};
  for (int k = 0; k < n_outputs; ++k) {
    if (int rc = resolve_output(m, names[k], &views[k], "dv_model_infer_outputs")) return rc;
    if (outs[k] == nullptr || reinterpret_cast<uintptr_t>(outs[k]) % 16 != 0) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, std::string("dv_model_infer_outputs: the output for '") + names[k] +
                                                   "' is null or not 16-byte aligned");
    }
    for (int j = 0; j < k; ++j) {
      if (std::strcmp(names[j], names[k]) == 0) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, std::string("dv_model_infer_outputs: '") + names[k] + "' requested twice");
      }
    }
    if (views[k].buf < 0) (views[k].logits ? head.logits : head.pooled) = outs[k];
  }
  if (n_outputs == 0) return dv_model_infer(m, images, n, probs, stream_v);
  if (n == 0) return DV_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  DV_HIP_CHECK(hipSetDevice(m->device));
  set_ext(m, images, probs, stream);
  if (int rc = enqueue_forward(m, n, stream, &head)) return rc;
  for (int k = 0; k < n_outputs; ++k) {
    const OutputView& v = views[k];
    if (v.buf < 0) continue;
    const BufferDesc& b = m->buffers[v.buf];
    const TensorGeom g = b.geom();
    dv::LayerExportArgs a{};
    a.src = m->dbuf[v.buf].ptr;
    a.kind = b.f32 ? dv::kExportF32 : b.wide ? dv::kExportWide : dv::kExportF16;
    a.n = n;
    a.h = g.h;
    a.w = g.w;
    a.halo = g.halo;
    a.hp = g.hp;
    a.wp = g.wp;
    a.src_groups = g.groups;
    a.lo_groups = b.c / 8;
    a.goff = v.coff / 8;
    a.groups = v.c / 8;
    a.dst = outs[k];
    dv::ProfileScope prof(dv::kProfOther, stream);
    dv::launch_layer_export(a, stream);
  }
  DV_HIP_CHECK(hipGetLastError());
  return DV_OK;
}

// Testing hook: how many forwards were captured into a new hipGraph / replayed from the cache.
int dv_model_graph_stats(const dv_model* m, int64_t* captures, int64_t* replays) {
  if (!m) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_model_graph_stats: null");
  if (captures) *captures = m->graph_captures;
  if (replays) *replays = m->graph_replays;
  return DV_OK;
}

}  // extern "C"
