// gvcf_rows.hip -- the rows of a gVCF behind the merge: dv_gvcf_rows (host code),
// dv_gvcf_rows_device and their result handle (include/dvhip.h).
//
// The row rule is gvcf_rows.h and the merge rule gvcf_merge.h, both compiled for both sides.  Device: one staged upload,
// up to sixteen launches queued on one stream, a wait for the 16-byte header, a download of exactly the text.
//   1-9    the merge's own stages (gvcf_merge_device.h): cm, the count, the sum, the pieces, the variants' slots
//   10     per block, one lane: walk again, store every piece's base (the block's, or the base at a variant's end)
//   11     per piece and per variant, one lane: len[slot] = the length of its row
//   12-14  row_off = the exclusive sum of len over the B + 2V slots there can be; the total goes into the header
//   15     per piece, one lane: write its row at row_off[slot], byte by byte
//   16     per variant, one wave: copy its finished row, the lanes striding over the bytes
// No workgroup reads what another workgroup writes in the same launch.  The text buffer is sized on the host before
// the launches by a bound (every block's longest possible row, V more rows of the longest of all, the variants' text);
// the kernels skip a row that would pass it and the host refuses a total that does.
//
// dv_gvcf_rows_bgzf[_device] are the same rows behind a caller's prefix, compressed by bgzf.hip
// instead of returned: on the device the launches above stop at the wait for the header (rows_text_on_device), the
// text stays where it is and is deflated there; only row_off, when asked for, comes back beside the file.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bgzf_internal.h"
#include "device_round_trip.h"
#include "gvcf_merge.h"
#include "gvcf_merge_device.h"
#include "gvcf_rows.h"

static_assert(sizeof(dv_gvcf_block) == 56, "dv_gvcf_block layout");
static_assert(sizeof(dv_gvcf_rows_input) == 96, "dv_gvcf_rows_input layout");
static_assert(sizeof(dv_gvcf_text_view) == 48, "dv_gvcf_text_view layout");
static_assert(sizeof(dv_gvcf_rows_stats) == 64, "dv_gvcf_rows_stats layout");
static_assert(sizeof(dv_gvcf_rows_meta) == 32, "dv_gvcf_rows_meta layout");

struct dv_gvcf_text {
  std::unique_ptr<char[]> text;
  int64_t n_bytes = 0, n_rows = 0, n_pieces = 0;
  std::vector<int64_t> row_off;         // [n_rows + 1] when asked for
  bool has_row_off = false;
  int32_t med_dp = 0;
};

namespace {

namespace gr = dv::gr;

struct RowTables {              // what the text needs beyond the merge's tables, all on the device
  Tables t;
  const dv_gvcf_block* blocks;  // [B]
  const uint8_t* var_end_base;  // [V]
  const int64_t* var_text_off;  // [V + 1]
  const char* var_text;
  const int64_t* name_off;      // [G + 1]
  const char* names;
  uint8_t* piece_base;          // [B + V]
  int64_t* len;                 // [B + 2V], by slot
  int64_t* row_off;             // [B + 2V], exclusive
  char* text;
  int64_t text_cap;             // the bytes behind `text`
  int32_t med_dp;
};

__global__ __launch_bounds__(kThreads) void piece_bases_kernel(RowTables r) {
  const Tables& t = r.t;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kThreads + static_cast<int64_t>(threadIdx.x);
  if (b >= t.n_blocks) return;
  const int32_t g = gm::group_of(t.block_off, t.n_groups, b);
  const int64_t at = t.piece_off[b];
  const uint8_t own = r.blocks[b].ref_base;
  gr::walk_block_src(t.block_start[b], t.block_end[b], t.var_start, t.var_end, t.cm, t.var_off[g], t.var_off[g + 1],
                     [&](int32_t k, int64_t, int64_t, int64_t src) {
                       r.piece_base[at + k] = src < 0 ? own : r.var_end_base[src];
                     });
}

// Lane i: piece i's row length and variant i's, each to its slot.  The grid covers B + V lanes, which is at least P
// and at least V.
__global__ __launch_bounds__(kThreads) void row_lengths_kernel(RowTables r) {
  const Tables& t = r.t;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + static_cast<int64_t>(threadIdx.x);
  if (i < *t.n_pieces) {
    const int32_t b = t.piece_block[i];
    const int32_t g = gm::group_of(t.block_off, t.n_groups, b);
    r.len[t.piece_slot[i]] =
        gr::piece_row_length(r.name_off[g + 1] - r.name_off[g], t.piece_start[i], t.piece_end[i], r.blocks[b], r.med_dp != 0);
  }
  if (i < t.n_vars) r.len[t.var_slot[i]] = r.var_text_off[i + 1] - r.var_text_off[i];
}

struct LenSource {              // element i = slot i's row length, 0 from P + V on; the exclusive sum is kept
  const int64_t* len;
  const int64_t* n_pieces;
  int64_t n_vars;
  int64_t* row_off;
  __device__ int64_t load(int64_t i) const { return i < *n_pieces + n_vars ? len[i] : 0; }
  __device__ void store(int64_t i, int64_t before, int64_t /*with*/) const { row_off[i] = before; }
};

__global__ __launch_bounds__(kThreads) void piece_rows_kernel(RowTables r) {
  const Tables& t = r.t;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + static_cast<int64_t>(threadIdx.x);
  if (i >= *t.n_pieces) return;
  const int64_t slot = t.piece_slot[i], at = r.row_off[slot];
  if (at < 0 || at + r.len[slot] > r.text_cap) return;       // the host refuses the total
  const int32_t b = t.piece_block[i];
  const int32_t g = gm::group_of(t.block_off, t.n_groups, b);
  gr::write_piece_row(r.text + at, r.names + r.name_off[g], r.name_off[g + 1] - r.name_off[g], t.piece_start[i],
                      t.piece_end[i], r.piece_base[i], r.blocks[b], r.med_dp != 0);
}

constexpr int kWave = 64;
constexpr int kWavesPerGroup = kThreads / kWave;

// A wave per variant: a row can be kilobytes long (long alleles), so the lanes stride over its bytes.
__global__ __launch_bounds__(kThreads) void variant_rows_kernel(RowTables r) {
  const Tables& t = r.t;
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kWavesPerGroup + static_cast<int64_t>(threadIdx.x / kWave);
  if (j >= t.n_vars) return;
  const int64_t from = r.var_text_off[j], n = r.var_text_off[j + 1] - from, at = r.row_off[t.var_slot[j]];
  if (at < 0 || at + n > r.text_cap) return;
  const char* src = r.var_text + from;
  char* dst = r.text + at;
  for (int64_t k = static_cast<int64_t>(threadIdx.x % kWave); k < n; k += kWave) dst[k] = src[k];
}

dv_gvcf_rows_stats& last_stats() {
  static thread_local dv_gvcf_rows_stats stats;
  return stats;
}

// What the checks leave behind for both sides.
struct Checked {
  int64_t nb = 0, nv = 0;
  bool med_dp = false;
  std::vector<int64_t> block_start, block_end;      // the blocks' spans as the merge takes them
  int64_t text_bound = 0;       // no call's text is longer
};

// The pieces of group g in order: emit(block, piece_start, piece_end, src), src as gr::walk_range_src gives it.  As in
// dv_gvcf_merge's host code the blocks ascend, so lo and hi only move forward.  cm: scratch for V entries.
template <class Emit>
void group_pieces(const dv_gvcf_rows_input& in, const Checked& c, int32_t g, std::vector<int64_t>* cm, Emit&& emit) {
  const int64_t v0 = in.var_off[g], v1 = in.var_off[g + 1];
  for (int64_t j = v0; j < v1; ++j) {
    (*cm)[j] = j > v0 && (*cm)[j - 1] > in.var_end[j] ? (*cm)[j - 1] : in.var_end[j];
  }
  int64_t lo = v0, hi = v0;
  for (int64_t b = in.block_off[g]; b < in.block_off[g + 1]; ++b) {
    const int64_t s = c.block_start[b], e = c.block_end[b];
    while (lo < v1 && (*cm)[lo] <= s) ++lo;
    while (hi < v1 && in.var_start[hi] < e) ++hi;
    gr::walk_range_src(s, e, in.var_start, in.var_end, lo, hi,
                       [&](int32_t, int64_t piece_start, int64_t piece_end, int64_t src) { emit(b, piece_start, piece_end, src); });
  }
}

std::string hex(uint8_t c) {
  char text[8];
  std::snprintf(text, sizeof text, "0x%02X", static_cast<unsigned>(c));
  return text;
}

// The arguments, checked on the host for both entry points.
int parse(const char* who, const dv_gvcf_rows_input* in, dv_gvcf_text** out, Checked* c) {
  const std::string name(who);
  if (out) *out = nullptr;
  if (!in || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer or negative count");
  if (in->med_dp < -1 || in->med_dp > 1) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": med_dp must be -1, 0 or 1");
  const int32_t ng = in->n_groups;
  bool offsets_ok = ng >= 0 && in->block_off && in->var_off && in->block_off[0] == 0 && in->var_off[0] == 0;
  for (int32_t g = 0; offsets_ok && g < ng; ++g) {
    offsets_ok = in->block_off[g + 1] >= in->block_off[g] && in->var_off[g + 1] >= in->var_off[g];
  }
  if (offsets_ok && in->blocks) {
    const size_t nb = static_cast<size_t>(in->block_off[ng]);
    c->block_start.resize(nb);
    c->block_end.resize(nb);
    for (size_t b = 0; b < nb; ++b) {
      c->block_start[b] = in->blocks[b].start;
      c->block_end[b] = in->blocks[b].end;
    }
  }
  const bool have_blocks = offsets_ok && in->blocks;
  if (int rc = check_merge_arguments(name, true, ng, in->block_off, in->var_off, have_blocks ? c->block_start.data() : nullptr,
                                     have_blocks ? c->block_end.data() : nullptr, in->var_start, in->var_end)) {
    return rc;
  }
  c->nb = in->block_off[ng];
  c->nv = in->var_off[ng];
  if ((c->nv > 0 && (!in->var_end_base || !in->var_text_off || !in->var_text)) || (ng > 0 && !in->name_off)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer");
  }
  int64_t var_bytes = 0;
  if (c->nv > 0) {
    if (in->var_text_off[0] != 0) return dv::fail(DV_ERR_BAD_INPUT, name + ": var_text_off must ascend from 0");
    for (int64_t j = 0; j < c->nv; ++j) {
      const int64_t from = in->var_text_off[j], to = in->var_text_off[j + 1];
      if (to < from) return dv::fail(DV_ERR_BAD_INPUT, name + ": var_text_off must ascend from 0");
      if (to == from || in->var_text[to - 1] != '\n') {
        return dv::fail(DV_ERR_BAD_INPUT, name + ": variant " + std::to_string(j) + "'s row is empty or does not end in a newline");
      }
    }
    var_bytes = in->var_text_off[c->nv];
  }
  if (ng > 0) {
    if (in->name_off[0] < 0) return dv::fail(DV_ERR_BAD_INPUT, name + ": name_off must ascend from >= 0");
    for (int32_t g = 0; g < ng; ++g) {
      if (in->name_off[g + 1] < in->name_off[g]) return dv::fail(DV_ERR_BAD_INPUT, name + ": name_off must ascend from >= 0");
    }
    if (in->name_off[ng] > in->name_off[0] && !in->names) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer");
  }
  bool any_med_dp = false;
  for (int64_t b = 0; b < c->nb; ++b) {
    const dv_gvcf_block& block = in->blocks[b];
    if (!gr::printable(block.ref_base)) {
      return dv::fail(DV_ERR_BAD_INPUT, name + ": block " + std::to_string(b) + ": ref_base " + hex(block.ref_base) +
                                            " is not a printable character");
    }
    for (int k = 0; k < 3; ++k) {
      if (!gr::likelihood_ok(block.likelihoods[k])) {
        return dv::fail(DV_ERR_BAD_INPUT, name + ": block " + std::to_string(b) +
                                              ": a likelihood is not finite or too large to round");
      }
    }
    any_med_dp = any_med_dp || block.med_dp >= 0;
  }
  c->med_dp = in->med_dp < 0 ? any_med_dp : in->med_dp != 0;
  // the bases the pieces take, and the bound: a block's pieces are one and one more per variant that cuts it
  std::vector<int64_t> cm(static_cast<size_t>(c->nv));
  int64_t bad = -1, longest = 0, bound = var_bytes;
  for (int32_t g = 0; g < ng; ++g) {
    const int64_t name_len = in->name_off[g + 1] - in->name_off[g];
    for (int64_t b = in->block_off[g]; b < in->block_off[g + 1]; ++b) {
      const int64_t most = gr::longest_piece_row(name_len, in->blocks[b], c->med_dp);
      bound += most;
      if (most > longest) longest = most;
    }
    group_pieces(*in, *c, g, &cm, [&](int64_t, int64_t, int64_t, int64_t src) {
      if (src >= 0 && bad < 0 && !gr::printable(in->var_end_base[src])) bad = src;
    });
    if (bad >= 0) {
      return dv::fail(DV_ERR_BAD_INPUT, name + ": variant " + std::to_string(bad) + ": var_end_base " +
                                            hex(in->var_end_base[bad]) + " is not a printable character");
    }
  }
  c->text_bound = bound + c->nv * longest;
  return DV_OK;
}

// The host code: per group its pieces, then the two-way merge of the pieces and the variants straight into the text --
// variant j stands before piece k iff var_start[j] < piece_end[k] (gvcf_merge.h).  lead: bytes left free in front of
// the rows for the caller's prefix; n_bytes and row_off count them.
void rows_on_host(const dv_gvcf_rows_input& in, const Checked& c, dv_gvcf_text* r, int64_t lead = 0) {
  struct Piece {
    int64_t start, end, block;
    uint8_t base;
  };
  r->text.reset(new char[static_cast<size_t>(lead + c.text_bound) + 1]);
  char* const text = r->text.get();
  int64_t at = lead;
  if (in.want_row_off) r->row_off.reserve(static_cast<size_t>(c.nb + 2 * c.nv + 1));
  std::vector<int64_t> cm(static_cast<size_t>(c.nv));
  std::vector<Piece> pieces;
  for (int32_t g = 0; g < in.n_groups; ++g) {
    pieces.clear();
    group_pieces(in, c, g, &cm, [&](int64_t b, int64_t s, int64_t e, int64_t src) {
      pieces.push_back(Piece{s, e, b, src < 0 ? in.blocks[b].ref_base : in.var_end_base[src]});
    });
    const char* name = in.names + in.name_off[g];
    const int64_t name_len = in.name_off[g + 1] - in.name_off[g];
    size_t p = 0;
    int64_t j = in.var_off[g];
    const int64_t v1 = in.var_off[g + 1];
    while (p < pieces.size() || j < v1) {
      if (in.want_row_off) r->row_off.push_back(at);
      if (j < v1 && (p == pieces.size() || in.var_start[j] < pieces[p].end)) {
        const int64_t from = in.var_text_off[j], n = in.var_text_off[j + 1] - from;
        std::memcpy(text + at, in.var_text + from, static_cast<size_t>(n));
        at += n;
        ++j;
      } else {
        const Piece& piece = pieces[p];
        at += gr::write_piece_row(text + at, name, name_len, piece.start, piece.end, piece.base, in.blocks[piece.block],
                                  c.med_dp);
        ++p;
        ++r->n_pieces;
      }
    }
  }
  if (in.want_row_off) r->row_off.push_back(at);
  r->n_bytes = at;
  r->n_rows = r->n_pieces + c.nv;
}

// What rows_text_on_device leaves on the device, valid until the calling thread's next call.
struct DeviceText {
  const char* text = nullptr;           // the prefix, then the rows
  const int64_t* row_off = nullptr;     // [n_rows], exclusive, into the rows
  int64_t n_bytes = 0, pieces = 0;      // of the rows
  hipStream_t stream = nullptr;
};

// The launches and the wait for the header; the text stays on the device, `n_prefix` bytes of `prefix` in front of it.
int rows_text_on_device(const std::string& who, const dv_gvcf_rows_input& in, const Checked& c, void* stream,
                        const void* prefix, size_t n_prefix, DeviceText* d) {
  dv_gvcf_rows_stats& stats = last_stats();
  const size_t ng = static_cast<size_t>(in.n_groups);
  const size_t nb = static_cast<size_t>(c.nb), nv = static_cast<size_t>(c.nv);
  const size_t cap = nb + nv;                                // P <= B + V
  const size_t rows_cap = cap + nv;                          // P + V
  const size_t block_chunks = (nb + kChunk - 1) / kChunk, var_chunks = (nv + kChunk - 1) / kChunk;
  const size_t row_chunks = (rows_cap + kChunk - 1) / kChunk;
  const size_t var_bytes = nv > 0 ? static_cast<size_t>(in.var_text_off[nv]) : 0;
  const size_t name_bytes = ng > 0 ? static_cast<size_t>(in.name_off[ng]) : 0;   // from names[0]; name_off[0] >= 0
  const size_t text_cap = static_cast<size_t>(c.text_bound);

  dv::Layout up;
  const size_t u_block_off = up.add((ng + 1) * sizeof(int64_t));
  const size_t u_var_off = up.add((ng + 1) * sizeof(int64_t));
  const size_t u_name_off = up.add((ng + 1) * sizeof(int64_t));
  const size_t u_block_start = up.add(nb * sizeof(int64_t));
  const size_t u_block_end = up.add(nb * sizeof(int64_t));
  const size_t u_blocks = up.add(nb * sizeof(dv_gvcf_block));
  const size_t u_var_start = up.add(nv * sizeof(int64_t));
  const size_t u_var_end = up.add(nv * sizeof(int64_t));
  const size_t u_var_text_off = up.add((nv + 1) * sizeof(int64_t));
  const size_t u_var_end_base = up.add(nv);
  const size_t u_names = up.add(name_bytes);
  const size_t u_var_text = up.add(var_bytes);
  const size_t u_prefix = up.add(n_prefix);
  dv::Layout down;
  const size_t d_header = down.add(2 * sizeof(int64_t));     // the number of pieces, the number of bytes
  dv::Layout scratch;
  const size_t s_cm = scratch.add(nv * sizeof(int64_t));
  const size_t s_count = scratch.add(nb * sizeof(int32_t));
  const size_t s_piece_off = scratch.add(nb * sizeof(int64_t));
  const size_t s_max_totals = scratch.add(var_chunks * sizeof(SegMax::T));
  const size_t s_sum_totals = scratch.add(block_chunks * sizeof(int64_t));
  const size_t s_len_totals = scratch.add(row_chunks * sizeof(int64_t));
  const size_t s_var_slot = scratch.add(nv * sizeof(int64_t));
  const size_t s_piece_start = scratch.add(cap * sizeof(int64_t));
  const size_t s_piece_end = scratch.add(cap * sizeof(int64_t));
  const size_t s_piece_slot = scratch.add(cap * sizeof(int64_t));
  const size_t s_piece_block = scratch.add(cap * sizeof(int32_t));
  const size_t s_piece_base = scratch.add(cap);
  const size_t s_len = scratch.add(rows_cap * sizeof(int64_t));
  const size_t s_row_off = scratch.add(rows_cap * sizeof(int64_t));
  const size_t s_text = scratch.add(n_prefix + text_cap + 16);       // never empty

  static thread_local dv::RoundTrip rt;
  if (int rc = rt.begin(who + ": no HIP device (dv_gvcf_rows is the host code)", stream, up.bytes(),
                        down.bytes(), scratch.bytes())) {
    return rc;
  }
  std::memcpy(rt.host_up<int64_t>(u_block_off), in.block_off, (ng + 1) * sizeof(int64_t));
  std::memcpy(rt.host_up<int64_t>(u_var_off), in.var_off, (ng + 1) * sizeof(int64_t));
  if (ng > 0) {
    std::memcpy(rt.host_up<int64_t>(u_name_off), in.name_off, (ng + 1) * sizeof(int64_t));
    if (name_bytes > 0) std::memcpy(rt.host_up<char>(u_names), in.names, name_bytes);
  } else {
    *rt.host_up<int64_t>(u_name_off) = 0;
  }
  if (nb > 0) {
    std::memcpy(rt.host_up<int64_t>(u_block_start), c.block_start.data(), nb * sizeof(int64_t));
    std::memcpy(rt.host_up<int64_t>(u_block_end), c.block_end.data(), nb * sizeof(int64_t));
    std::memcpy(rt.host_up<dv_gvcf_block>(u_blocks), in.blocks, nb * sizeof(dv_gvcf_block));
  }
  if (nv > 0) {
    std::memcpy(rt.host_up<int64_t>(u_var_start), in.var_start, nv * sizeof(int64_t));
    std::memcpy(rt.host_up<int64_t>(u_var_end), in.var_end, nv * sizeof(int64_t));
    std::memcpy(rt.host_up<int64_t>(u_var_text_off), in.var_text_off, (nv + 1) * sizeof(int64_t));
    std::memcpy(rt.host_up<uint8_t>(u_var_end_base), in.var_end_base, nv);
    std::memcpy(rt.host_up<char>(u_var_text), in.var_text, var_bytes);
  }
  if (n_prefix > 0) std::memcpy(rt.host_up<char>(u_prefix), prefix, n_prefix);
  if (int rc = rt.upload(up.bytes())) return rc;
  stats.bytes_up = static_cast<int64_t>(up.bytes());

  uint8_t* const scratch_base = static_cast<uint8_t*>(rt.d_scratch.ptr);
  int64_t* const header = rt.dev_down<int64_t>(d_header);
  RowTables rows;
  Tables& t = rows.t;
  t.n_groups = in.n_groups;
  t.n_blocks = static_cast<int64_t>(nb);
  t.n_vars = static_cast<int64_t>(nv);
  t.block_off = rt.dev_up<const int64_t>(u_block_off);
  t.var_off = rt.dev_up<const int64_t>(u_var_off);
  t.block_start = rt.dev_up<const int64_t>(u_block_start);
  t.block_end = rt.dev_up<const int64_t>(u_block_end);
  t.var_start = rt.dev_up<const int64_t>(u_var_start);
  t.var_end = rt.dev_up<const int64_t>(u_var_end);
  int64_t* const cm = reinterpret_cast<int64_t*>(scratch_base + s_cm);
  int64_t* const piece_off = reinterpret_cast<int64_t*>(scratch_base + s_piece_off);
  t.cm = cm;
  t.count = reinterpret_cast<int32_t*>(scratch_base + s_count);
  t.piece_off = piece_off;
  t.n_pieces = header;
  t.piece_start = reinterpret_cast<int64_t*>(scratch_base + s_piece_start);
  t.piece_end = reinterpret_cast<int64_t*>(scratch_base + s_piece_end);
  t.piece_slot = reinterpret_cast<int64_t*>(scratch_base + s_piece_slot);
  t.var_slot = reinterpret_cast<int64_t*>(scratch_base + s_var_slot);
  t.piece_block = reinterpret_cast<int32_t*>(scratch_base + s_piece_block);
  rows.blocks = rt.dev_up<const dv_gvcf_block>(u_blocks);
  rows.var_end_base = rt.dev_up<const uint8_t>(u_var_end_base);
  rows.var_text_off = rt.dev_up<const int64_t>(u_var_text_off);
  rows.var_text = rt.dev_up<const char>(u_var_text);
  rows.name_off = rt.dev_up<const int64_t>(u_name_off);
  rows.names = rt.dev_up<const char>(u_names);
  rows.piece_base = scratch_base + s_piece_base;
  rows.len = reinterpret_cast<int64_t*>(scratch_base + s_len);
  rows.row_off = reinterpret_cast<int64_t*>(scratch_base + s_row_off);
  rows.text = reinterpret_cast<char*>(scratch_base + s_text) + n_prefix;
  if (n_prefix > 0) {
    DV_HIP_CHECK(hipMemcpyAsync(scratch_base + s_text, rt.dev_up<const char>(u_prefix), n_prefix, hipMemcpyDeviceToDevice,
                                rt.stream()));
  }
  rows.text_cap = static_cast<int64_t>(text_cap);
  rows.med_dp = c.med_dp ? 1 : 0;
  {
    dv::ProfileScope prof(dv::kProfOther, rt.stream());
    const dim3 threads(kThreads);
    const dim3 block_grid(static_cast<unsigned>((nb + kThreads - 1) / kThreads));
    const dim3 record_grid(static_cast<unsigned>((cap + kThreads - 1) / kThreads));
    const dim3 wave_grid(static_cast<unsigned>((nv + kWavesPerGroup - 1) / kWavesPerGroup));
    if (int rc = merge_stages_on_device(t, cm, piece_off, header, reinterpret_cast<SegMax::T*>(scratch_base + s_max_totals),
                                        reinterpret_cast<int64_t*>(scratch_base + s_sum_totals), rt.stream(),
                                        &stats.launches)) {
      return rc;
    }
    if (nb > 0) {
      hipLaunchKernelGGL(piece_bases_kernel, block_grid, threads, 0, rt.stream(), rows);
      DV_HIP_CHECK(hipGetLastError());
      ++stats.launches;
    }
    hipLaunchKernelGGL(row_lengths_kernel, record_grid, threads, 0, rt.stream(), rows);
    DV_HIP_CHECK(hipGetLastError());
    ++stats.launches;
    const LenSource src{rows.len, header, t.n_vars, rows.row_off};
    if (int rc = scan_on_device<Sum>(src, static_cast<int64_t>(rows_cap), reinterpret_cast<int64_t*>(scratch_base + s_len_totals),
                                     header + 1, rt.stream(), &stats.launches)) {
      return rc;
    }
    if (nb > 0) {
      hipLaunchKernelGGL(piece_rows_kernel, record_grid, threads, 0, rt.stream(), rows);
      DV_HIP_CHECK(hipGetLastError());
      ++stats.launches;
    }
    if (nv > 0) {
      hipLaunchKernelGGL(variant_rows_kernel, wave_grid, threads, 0, rt.stream(), rows);
      DV_HIP_CHECK(hipGetLastError());
      ++stats.launches;
    }
  }
  // the one extra wait: the header says how much there is to fetch
  if (int rc = rt.finish(down.bytes())) return rc;
  const int64_t pieces = rt.host_down<int64_t>(d_header)[0], n_bytes = rt.host_down<int64_t>(d_header)[1];
  if (pieces < 0 || static_cast<size_t>(pieces) > cap || n_bytes < 0 || static_cast<size_t>(n_bytes) > text_cap) {
    return dv::fail(DV_ERR_HIP, who + ": the device counted " + std::to_string(pieces) + " pieces and " +
                                    std::to_string(n_bytes) + " bytes for " + std::to_string(cap) + " records and a bound of " +
                                    std::to_string(text_cap) + " bytes");
  }
  d->text = reinterpret_cast<const char*>(scratch_base + s_text);
  d->row_off = rows.row_off;
  d->n_bytes = n_bytes;
  d->pieces = pieces;
  d->stream = rt.stream();
  stats.bytes_down = static_cast<int64_t>(down.bytes());
  return DV_OK;
}

// row_off[0 .. n_rows] from the device; queued on d.stream, not waited for.
int fetch_row_off(const DeviceText& d, int64_t n_rows, std::vector<int64_t>* row_off) {
  row_off->resize(static_cast<size_t>(n_rows) + 1);
  if (n_rows > 0) {
    DV_HIP_CHECK(hipMemcpyAsync(row_off->data(), d.row_off, static_cast<size_t>(n_rows) * sizeof(int64_t),
                                hipMemcpyDeviceToHost, d.stream));
    last_stats().bytes_down += n_rows * static_cast<int64_t>(sizeof(int64_t));
  }
  row_off->back() = d.n_bytes;
  return DV_OK;
}

int rows_on_device(const dv_gvcf_rows_input& in, const Checked& c, void* stream, dv_gvcf_text* r) {
  DeviceText d;
  if (int rc = rows_text_on_device("dv_gvcf_rows_device", in, c, stream, nullptr, 0, &d)) return rc;
  r->n_pieces = d.pieces;
  r->n_rows = d.pieces + c.nv;
  r->n_bytes = d.n_bytes;
  r->text.reset(new char[static_cast<size_t>(d.n_bytes) + 1]);
  last_stats().bytes_down += d.n_bytes;
  if (d.n_bytes > 0) {
    DV_HIP_CHECK(hipMemcpyAsync(r->text.get(), d.text, static_cast<size_t>(d.n_bytes), hipMemcpyDeviceToHost, d.stream));
  }
  if (in.want_row_off) {
    if (int rc = fetch_row_off(d, r->n_rows, &r->row_off)) return rc;
  }
  DV_HIP_CHECK(hipStreamSynchronize(d.stream));
  return DV_OK;
}

}  // namespace

extern "C" {

int dv_gvcf_rows(const dv_gvcf_rows_input* in, dv_gvcf_text** out) {
  return dv::guarded("dv_gvcf_rows", [&]() -> int {
    Checked c;
    if (int rc = parse("dv_gvcf_rows", in, out, &c)) return rc;
    auto res = std::make_unique<dv_gvcf_text>();
    res->med_dp = c.med_dp ? 1 : 0;
    res->has_row_off = in->want_row_off != 0;
    rows_on_host(*in, c, res.get());
    *out = res.release();
    return DV_OK;
  });
}

int dv_gvcf_rows_device(const dv_gvcf_rows_input* in, dv_gvcf_text** out, void* stream) {
  return dv::guarded("dv_gvcf_rows_device", [&]() -> int {
    last_stats() = dv_gvcf_rows_stats();
    // every array is a host array: all of it is checked before any device work
    Checked c;
    if (int rc = parse("dv_gvcf_rows_device", in, out, &c)) return rc;
    auto res = std::make_unique<dv_gvcf_text>();
    res->med_dp = c.med_dp ? 1 : 0;
    res->has_row_off = in->want_row_off != 0;
    dv_gvcf_rows_stats& stats = last_stats();
    stats.blocks = c.nb;
    stats.variants = c.nv;
    if (c.nb + c.nv > 0) {
      if (int rc = rows_on_device(*in, c, stream, res.get())) return rc;
    } else {
      res->text.reset(new char[1]);
      if (in->want_row_off) res->row_off.assign(1, 0);
    }
    stats.pieces = res->n_pieces;
    stats.rows = res->n_rows;
    stats.text_bytes = res->n_bytes;
    *out = res.release();
    return DV_OK;
  });
}

// The arguments of the two compressed entry points: their own, then dv_gvcf_rows's through the same `parse`.
static int parse_compressed(const char* who, const dv_gvcf_rows_input* in, const void* prefix, int64_t n_prefix,
                            dv_gvcf_rows_meta* meta, dv_bgzf_file** file, Checked* c) {
  if (file) *file = nullptr;
  if (meta) *meta = dv_gvcf_rows_meta();
  if (!meta || !file || n_prefix < 0 || (!prefix && n_prefix > 0)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer or negative count");
  }
  if (in && in->med_dp < 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, std::string(who) + ": med_dp must be 0 or 1 (the header is written already)");
  }
  dv_gvcf_text* none = nullptr;
  return parse(who, in, &none, c);
}

int dv_gvcf_rows_bgzf(const dv_gvcf_rows_input* in, const void* prefix, int64_t n_prefix, dv_gvcf_rows_meta* meta,
                      dv_bgzf_file** file) {
  return dv::guarded("dv_gvcf_rows_bgzf", [&]() -> int {
    Checked c;
    if (int rc = parse_compressed("dv_gvcf_rows_bgzf", in, prefix, n_prefix, meta, file, &c)) return rc;
    dv_gvcf_text text;
    rows_on_host(*in, c, &text, n_prefix);
    if (n_prefix > 0) std::memcpy(text.text.get(), prefix, static_cast<size_t>(n_prefix));
    auto res = std::make_unique<dv_bgzf_file>();
    dv::bgzf_compress_on_host(reinterpret_cast<const uint8_t*>(text.text.get()), text.n_bytes, res.get());
    if (in->want_row_off) res->row_off = std::move(text.row_off);
    meta->n_rows = text.n_rows;
    meta->n_pieces = text.n_pieces;
    meta->text_bytes = text.n_bytes;
    meta->row_off = in->want_row_off ? res->row_off.data() : nullptr;
    *file = res.release();
    return DV_OK;
  });
}

int dv_gvcf_rows_bgzf_device(const dv_gvcf_rows_input* in, const void* prefix, int64_t n_prefix, dv_gvcf_rows_meta* meta,
                             dv_bgzf_file** file, void* stream) {
  return dv::guarded("dv_gvcf_rows_bgzf_device", [&]() -> int {
    const char* const who = "dv_gvcf_rows_bgzf_device";
    last_stats() = dv_gvcf_rows_stats();
    Checked c;
    if (int rc = parse_compressed(who, in, prefix, n_prefix, meta, file, &c)) return rc;
    dv_gvcf_rows_stats& stats = last_stats();
    stats.blocks = c.nb;
    stats.variants = c.nv;
    auto res = std::make_unique<dv_bgzf_file>();
    int64_t pieces = 0, text_bytes = n_prefix;
    if (c.nb + c.nv > 0) {
      DeviceText d;
      if (int rc = rows_text_on_device(who, *in, c, stream, prefix, static_cast<size_t>(n_prefix), &d)) return rc;
      pieces = d.pieces;
      text_bytes += d.n_bytes;
      // the text is deflated where it lies, on the stream that wrote it
      if (int rc = dv::bgzf_compress_on_device(who, reinterpret_cast<const uint8_t*>(d.text), true, text_bytes, d.stream,
                                               res.get())) {
        return rc;
      }
      if (in->want_row_off) {
        // after the compressor, which has waited for the stream: no copy into row_off is pending when an error frees it
        const int rc = fetch_row_off(d, pieces + c.nv, &res->row_off);
        const hipError_t waited = hipStreamSynchronize(d.stream);
        if (rc != DV_OK) return rc;
        DV_HIP_CHECK(waited);
        for (int64_t& off : res->row_off) off += n_prefix;
      }
    } else {
      if (int rc = dv::bgzf_compress_on_device(who, static_cast<const uint8_t*>(prefix), false, n_prefix, stream, res.get())) {
        return rc;
      }
      if (in->want_row_off) res->row_off.assign(1, n_prefix);
    }
    stats.pieces = pieces;
    stats.rows = pieces + c.nv;
    stats.text_bytes = text_bytes;
    meta->n_rows = pieces + c.nv;
    meta->n_pieces = pieces;
    meta->text_bytes = text_bytes;
    meta->row_off = in->want_row_off ? res->row_off.data() : nullptr;
    *file = res.release();
    return DV_OK;
  });
}

int dv_gvcf_text_arrays(const dv_gvcf_text* t, dv_gvcf_text_view* out) {
  if (!t || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_gvcf_text_arrays: null");
  out->text = t->text.get();
  out->n_bytes = t->n_bytes;
  out->row_off = t->has_row_off ? t->row_off.data() : nullptr;
  out->n_rows = t->n_rows;
  out->n_pieces = t->n_pieces;
  out->med_dp = t->med_dp;
  out->reserved = 0;
  return DV_OK;
}

void dv_gvcf_text_free(dv_gvcf_text* t) { delete t; }

int dv_gvcf_rows_last_stats(dv_gvcf_rows_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_gvcf_rows_last_stats: null");
  *out = last_stats();
  return DV_OK;
}

}  // extern "C"
