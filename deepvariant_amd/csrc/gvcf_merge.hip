// gvcf_merge.hip -- the merge of the gVCF reference blocks with the variant records:
// dv_gvcf_merge (host code), dv_gvcf_merge_device and their result handle (include/dvhip.h).
//
// The rule is gvcf_merge.h, compiled for both sides.  Device: one staged upload (the six input arrays), nine launches
// queued on one stream, one download, one wait.
//   1-3  cm = the running maximum of the variants' ends, restarted at every group's first variant
//   4    per block, one lane: bisect, walk, count its pieces
//   5-7  piece_off = the exclusive sum of the counts; the total goes into the download's header
//   8    per block again: write its pieces and their slots
//   9    per variant: its slot, by bisection over the piece ends of its group
// Both scans are chunk totals (one workgroup per chunk of kChunk elements), a scan of the totals by one workgroup,
// and an apply pass that redoes the chunk with its carry: three launches each, ordered by the stream.  No workgroup
// reads what another workgroup writes in the same launch.  The outputs are sized for B + V pieces before the launch
// (a variant ends at most one piece and every block ends one), so nothing is read back in between.  The kernels, the
// scan and the argument checks are gvcf_merge_device.h, which gvcf_rows.hip (section 23) includes as well.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_round_trip.h"
#include "gvcf_merge.h"
#include "gvcf_merge_device.h"

static_assert(sizeof(dv_gvcf_merge_stats) == 48, "dv_gvcf_merge_stats layout");
static_assert(sizeof(dv_gvcf_merged_view) == 56, "dv_gvcf_merged_view layout");

struct dv_gvcf_merged {
  std::vector<int64_t> piece_start, piece_end, piece_slot, var_slot;
  std::vector<int32_t> piece_block;
};

namespace {

dv_gvcf_merge_stats& last_stats() {
  static thread_local dv_gvcf_merge_stats stats;
  return stats;
}

// The arguments, checked on the host for both entry points.
int parse(const char* who, int32_t n_groups, const int64_t* block_off, const int64_t* var_off, const int64_t* block_start,
          const int64_t* block_end, const int64_t* var_start, const int64_t* var_end, dv_gvcf_merged** out) {
  if (out) *out = nullptr;
  return check_merge_arguments(who, out != nullptr, n_groups, block_off, var_off, block_start, block_end, var_start,
                               var_end);
}

// The host code: one pass over each group.  The blocks ascend, so the bounds that a lane finds by bisection only move
// forward here: lo (the first variant whose running maximum passes the block's start), hi (the first that starts at
// or after its end), the variant a piece's slot counts up to, and the piece a variant's slot counts up to.
void merge_on_host(int32_t n_groups, const int64_t* block_off, const int64_t* var_off, const int64_t* block_start,
                   const int64_t* block_end, const int64_t* var_start, const int64_t* var_end, dv_gvcf_merged* r) {
  const int64_t nv = var_off[n_groups];
  const size_t cap = static_cast<size_t>(block_off[n_groups] + nv);     // P <= B + V
  std::vector<int64_t> cm(static_cast<size_t>(nv));
  r->var_slot.assign(static_cast<size_t>(nv), 0);
  r->piece_start.reserve(cap);
  r->piece_end.reserve(cap);
  r->piece_slot.reserve(cap);
  r->piece_block.reserve(cap);
  for (int32_t g = 0; g < n_groups; ++g) {
    const int64_t v0 = var_off[g], v1 = var_off[g + 1];
    for (int64_t j = v0; j < v1; ++j) cm[j] = j > v0 && cm[j - 1] > var_end[j] ? cm[j - 1] : var_end[j];
    const int64_t p0 = static_cast<int64_t>(r->piece_end.size());
    int64_t lo = v0, hi = v0, before = v0;
    for (int64_t b = block_off[g]; b < block_off[g + 1]; ++b) {
      const int64_t s = block_start[b], e = block_end[b];
      while (lo < v1 && cm[lo] <= s) ++lo;
      while (hi < v1 && var_start[hi] < e) ++hi;
      gm::walk_range(s, e, var_start, var_end, lo, hi, [&](int32_t, int64_t piece_start, int64_t piece_end) {
        while (before < v1 && var_start[before] < piece_end) ++before;   // gm::piece_slot, the piece ends ascend
        r->piece_slot.push_back(static_cast<int64_t>(r->piece_end.size()) + before);
        r->piece_start.push_back(piece_start);
        r->piece_end.push_back(piece_end);
        r->piece_block.push_back(static_cast<int32_t>(b));
      });
    }
    const int64_t p1 = static_cast<int64_t>(r->piece_end.size());
    int64_t p = p0;
    for (int64_t j = v0; j < v1; ++j) {                                  // gm::var_slot, the variant starts ascend
      while (p < p1 && r->piece_end[static_cast<size_t>(p)] <= var_start[j]) ++p;
      r->var_slot[j] = j + p;
    }
  }
}


int merge_on_device(int32_t n_groups, const int64_t* block_off, const int64_t* var_off, const int64_t* block_start,
                    const int64_t* block_end, const int64_t* var_start, const int64_t* var_end, void* stream,
                    dv_gvcf_merged* r) {
  dv_gvcf_merge_stats& stats = last_stats();
  const size_t ng = static_cast<size_t>(n_groups);
  const size_t nb = static_cast<size_t>(block_off[n_groups]), nv = static_cast<size_t>(var_off[n_groups]);
  const size_t cap = nb + nv;                                // P <= B + V
  const size_t block_chunks = (nb + kChunk - 1) / kChunk, var_chunks = (nv + kChunk - 1) / kChunk;

  dv::Layout up;
  const size_t u_block_off = up.add((ng + 1) * sizeof(int64_t));
  const size_t u_var_off = up.add((ng + 1) * sizeof(int64_t));
  const size_t u_block_start = up.add(nb * sizeof(int64_t));
  const size_t u_block_end = up.add(nb * sizeof(int64_t));
  const size_t u_var_start = up.add(nv * sizeof(int64_t));
  const size_t u_var_end = up.add(nv * sizeof(int64_t));
  dv::Layout down;
  const size_t d_header = down.add(sizeof(int64_t));         // the number of pieces
  const size_t d_var_slot = down.add(nv * sizeof(int64_t));
  const size_t d_piece_start = down.add(cap * sizeof(int64_t));
  const size_t d_piece_end = down.add(cap * sizeof(int64_t));
  const size_t d_piece_slot = down.add(cap * sizeof(int64_t));
  const size_t d_piece_block = down.add_last(cap * sizeof(int32_t));
  dv::Layout scratch;
  const size_t s_cm = scratch.add(nv * sizeof(int64_t));
  const size_t s_count = scratch.add(nb * sizeof(int32_t));
  const size_t s_piece_off = scratch.add(nb * sizeof(int64_t));
  const size_t s_max_totals = scratch.add(var_chunks * sizeof(SegMax::T));
  const size_t s_sum_totals = scratch.add(block_chunks * sizeof(int64_t));
  scratch.add(16);                                           // never empty

  static thread_local dv::RoundTrip rt;
  if (int rc = rt.begin("dv_gvcf_merge_device: no HIP device (dv_gvcf_merge is the host code)", stream, up.bytes(),
                        down.bytes(), scratch.bytes())) {
    return rc;
  }
  std::memcpy(rt.host_up<int64_t>(u_block_off), block_off, (ng + 1) * sizeof(int64_t));
  std::memcpy(rt.host_up<int64_t>(u_var_off), var_off, (ng + 1) * sizeof(int64_t));
  if (nb > 0) {
    std::memcpy(rt.host_up<int64_t>(u_block_start), block_start, nb * sizeof(int64_t));
    std::memcpy(rt.host_up<int64_t>(u_block_end), block_end, nb * sizeof(int64_t));
  }
  if (nv > 0) {
    std::memcpy(rt.host_up<int64_t>(u_var_start), var_start, nv * sizeof(int64_t));
    std::memcpy(rt.host_up<int64_t>(u_var_end), var_end, nv * sizeof(int64_t));
  }
  if (int rc = rt.upload(up.bytes())) return rc;
  stats.bytes_up = static_cast<int64_t>(up.bytes());

  uint8_t* const scratch_base = static_cast<uint8_t*>(rt.d_scratch.ptr);
  Tables t;
  t.n_groups = n_groups;
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
  t.n_pieces = rt.dev_down<int64_t>(d_header);
  t.piece_start = rt.dev_down<int64_t>(d_piece_start);
  t.piece_end = rt.dev_down<int64_t>(d_piece_end);
  t.piece_slot = rt.dev_down<int64_t>(d_piece_slot);
  t.var_slot = rt.dev_down<int64_t>(d_var_slot);
  t.piece_block = rt.dev_down<int32_t>(d_piece_block);
  {
    dv::ProfileScope prof(dv::kProfOther, rt.stream());
    if (int rc = merge_stages_on_device(t, cm, piece_off, rt.dev_down<int64_t>(d_header),
                                        reinterpret_cast<SegMax::T*>(scratch_base + s_max_totals),
                                        reinterpret_cast<int64_t*>(scratch_base + s_sum_totals), rt.stream(),
                                        &stats.launches)) {
      return rc;
    }
  }
  if (int rc = rt.finish(down.bytes())) return rc;
  stats.bytes_down = static_cast<int64_t>(down.bytes());
  const int64_t pieces = *rt.host_down<int64_t>(d_header);
  if (pieces < 0 || static_cast<size_t>(pieces) > cap) {
    return dv::fail(DV_ERR_HIP, "dv_gvcf_merge_device: the device counted " + std::to_string(pieces) + " pieces for " +
                                    std::to_string(cap) + " records");
  }
  const size_t np = static_cast<size_t>(pieces);
  r->piece_start.assign(rt.host_down<int64_t>(d_piece_start), rt.host_down<int64_t>(d_piece_start) + np);
  r->piece_end.assign(rt.host_down<int64_t>(d_piece_end), rt.host_down<int64_t>(d_piece_end) + np);
  r->piece_slot.assign(rt.host_down<int64_t>(d_piece_slot), rt.host_down<int64_t>(d_piece_slot) + np);
  r->piece_block.assign(rt.host_down<int32_t>(d_piece_block), rt.host_down<int32_t>(d_piece_block) + np);
  r->var_slot.assign(rt.host_down<int64_t>(d_var_slot), rt.host_down<int64_t>(d_var_slot) + nv);
  return DV_OK;
}

}  // namespace

extern "C" {

int dv_gvcf_merge(int32_t n_groups, const int64_t* block_off, const int64_t* var_off, const int64_t* block_start,
                  const int64_t* block_end, const int64_t* var_start, const int64_t* var_end, dv_gvcf_merged** out) {
  return dv::guarded("dv_gvcf_merge", [&]() -> int {
    if (int rc = parse("dv_gvcf_merge", n_groups, block_off, var_off, block_start, block_end, var_start, var_end, out)) {
      return rc;
    }
    auto res = std::make_unique<dv_gvcf_merged>();
    merge_on_host(n_groups, block_off, var_off, block_start, block_end, var_start, var_end, res.get());
    *out = res.release();
    return DV_OK;
  });
}

int dv_gvcf_merge_device(int32_t n_groups, const int64_t* block_off, const int64_t* var_off, const int64_t* block_start,
                         const int64_t* block_end, const int64_t* var_start, const int64_t* var_end,
                         dv_gvcf_merged** out, void* stream) {
  return dv::guarded("dv_gvcf_merge_device", [&]() -> int {
    last_stats() = dv_gvcf_merge_stats();
    // every array is a host array: all of it is checked before any device work
    if (int rc = parse("dv_gvcf_merge_device", n_groups, block_off, var_off, block_start, block_end, var_start, var_end,
                       out)) {
      return rc;
    }
    auto res = std::make_unique<dv_gvcf_merged>();
    dv_gvcf_merge_stats& stats = last_stats();
    stats.blocks = block_off[n_groups];
    stats.variants = var_off[n_groups];
    if (stats.blocks + stats.variants > 0) {
      if (int rc = merge_on_device(n_groups, block_off, var_off, block_start, block_end, var_start, var_end, stream,
                                   res.get())) {
        return rc;
      }
    }
    stats.pieces = static_cast<int64_t>(res->piece_end.size());
    *out = res.release();
    return DV_OK;
  });
}

int dv_gvcf_merged_arrays(const dv_gvcf_merged* m, dv_gvcf_merged_view* out) {
  if (!m || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_gvcf_merged_arrays: null");
  out->n_pieces = static_cast<int64_t>(m->piece_end.size());
  out->n_variants = static_cast<int64_t>(m->var_slot.size());
  out->piece_start = m->piece_start.data();
  out->piece_end = m->piece_end.data();
  out->piece_block = m->piece_block.data();
  out->piece_slot = m->piece_slot.data();
  out->var_slot = m->var_slot.data();
  return DV_OK;
}

void dv_gvcf_merged_free(dv_gvcf_merged* m) { delete m; }

int32_t dv_gvcf_merge_scan_chunk(void) { return kChunk; }

int dv_gvcf_merge_last_stats(dv_gvcf_merge_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_gvcf_merge_last_stats: null");
  *out = last_stats();
  return DV_OK;
}

}  // extern "C"
