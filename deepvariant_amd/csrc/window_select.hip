// window_select.hip -- the realigner's window selection (deepvariant/realigner/window_selector.py:40-238,
// window_selector.cc:53-207) over the counts and events the counter kernel left on the device
// (allele_counter.hip), queued behind it on the same stream.  The host restatement and checker is
// deepvariant_amd/realigner/window_selector.py: _candidates_from_counter and _candidates_to_windows.
//
// Which events stand, and which standing events are one allele, is what the candidate pass' link, resolve and
// group kernels work out (candidates.hip, cand_group_launch); this file reads their scratch.  Behind them, per
// batch of regions (blockIdx.y / blockIdx.x = region), no synchronisation:
//   win_first   per standing event: the first event of its read key at its position -- the slot the host's dict
//               keeps for the key -- and one more standing event for the position
//   win_scan    one workgroup per region: where each position's standing events start in the ordered list
//   win_place   per standing event: its place among its position's (by first-of-key), its clipped footprint,
//               and whether it counts for the VARIANT_READS model -> one ordered record
//   win_score   one workgroup per region: each lane owns positions j and walks the ordered records once, tile by
//               tile through LDS, so every float32 score is summed in the host's order whatever order the atomics
//               of the kernels before landed in: footprints from positions < j, the reference term of j,
//               footprints from positions >= j.  Then the candidates (ballot) and the windows (prefix scan)
//   win_pack    the windows of all regions back to back in region order
// The float32 sums use __fadd_rn / __fmul_rn: each step is one round-to-nearest operation and none is contracted.
#include <algorithm>

#include "cand_slices.h"
#include "event_lists.h"
#include "window_select.h"

// the layout deepvariant_amd/_lib.py mirrors
static_assert(sizeof(dv_window_options) == 64, "dv_window_options layout");

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
enum : uint32_t { kRef = 1, kSub = 2, kIns = 3, kDel = 4, kSoft = 5 };   // AlleleType
constexpr int32_t kCounts = 1 << 8;                                      // record flag: counts for VARIANT_READS

__device__ __forceinline__ uint32_t type_of(const dv_allele_event& ev) { return (ev.length_type >> 28) & 7u; }
__device__ __forceinline__ uint32_t length_of(const dv_allele_event& ev) { return ev.length_type & 0x0fffffffu; }
__device__ __forceinline__ bool low_quality(const dv_allele_event& ev) { return (ev.length_type >> 31) != 0; }

// scratch slices (dv::win_scratch_ints)
struct WinSlices {
  int32_t *n_stand, *first_slot;                 // per position
  int32_t *key_read, *key_off;                   // per event: the first event of its key at its position
  int32_t *r_pos, *r_lo, *r_hi, *r_flag;         // the ordered records
  int32_t* n_records;
};
__device__ __forceinline__ WinSlices win_slices(const dv::CandRegion& g, const dv::WindowRegion& w) {
  const size_t len = static_cast<size_t>(g.len), cap = g.event_cap;
  WinSlices s;
  s.n_stand = w.scratch;
  s.first_slot = s.n_stand + len;
  s.key_read = s.first_slot + len;
  s.key_off = s.key_read + cap;
  s.r_pos = s.key_off + cap;
  s.r_lo = s.r_pos + cap;
  s.r_hi = s.r_lo + cap;
  s.r_flag = s.r_hi + cap;
  s.n_records = s.r_flag + cap;
  return s;
}

__device__ __forceinline__ uint32_t n_events(const dv::CandRegion& g) {
  const uint32_t n = *g.n_events;
  return n < g.event_cap ? n : g.event_cap;
}

__global__ __launch_bounds__(kThreads) void win_first_kernel(const dv::CandRegion* cand, const dv::WindowRegion* win) {
  const dv::CandRegion& g = cand[blockIdx.y];
  const dv::CandSlices c = dv::cand_slices(g);
  const WinSlices s = win_slices(g, win[blockIdx.y]);
  const dv::EventLists l{g.events, g.read_key, c.head, c.next};
  const uint32_t n = n_events(g);
  for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += gridDim.x * kThreads) {
    if (!c.stands[e]) continue;
    const dv_allele_event ev = g.events[e];
    const int32_t key = dv::key_of(l, ev.read);
    dv_allele_event first = ev;
    for (int32_t j = c.head[ev.position]; j != 0; j = c.next[j - 1]) {
      const dv_allele_event o = g.events[j - 1];
      if (dv::key_of(l, o.read) == key && dv::stored_before(o, first)) first = o;
    }
    s.key_read[e] = static_cast<int32_t>(first.read);
    s.key_off[e] = static_cast<int32_t>(first.read_offset);
    atomicAdd(&s.n_stand[ev.position], 1);       // an integer count: the same whatever the order
  }
}

// Exclusive prefix sum of `v` over the workgroup; *total = the sum.  `shared` holds kWaves ints.
__device__ int block_exclusive_scan(int v, int* shared, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  __syncthreads();                       // the previous use of `shared` is over
  if (lane == 63) shared[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) before += shared[w];
    all += shared[w];
  }
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kThreads) void win_scan_kernel(const dv::CandRegion* cand, const dv::WindowRegion* win) {
  const dv::CandRegion& g = cand[blockIdx.x];
  const WinSlices s = win_slices(g, win[blockIdx.x]);
  __shared__ int scan[kWaves];
  int n_records = 0;                     // uniform over the workgroup
  for (int32_t base = 0; base < g.len; base += kThreads) {
    const int32_t p = base + threadIdx.x;
    const int k = p < g.len ? s.n_stand[p] : 0;
    int chunk = 0;
    const int at = n_records + block_exclusive_scan(k, scan, &chunk);
    if (p < g.len) s.first_slot[p] = at;
    n_records += chunk;
  }
  if (threadIdx.x == 0) *s.n_records = n_records;
}

__device__ __forceinline__ bool key_before(int32_t read_a, int32_t off_a, int32_t read_b, int32_t off_b) {
  const uint32_t ra = static_cast<uint32_t>(read_a), rb = static_cast<uint32_t>(read_b);
  return ra < rb || (ra == rb && static_cast<uint32_t>(off_a) < static_cast<uint32_t>(off_b));
}

__global__ __launch_bounds__(kThreads) void win_place_kernel(const dv::CandRegion* cand, const dv::WindowRegion* win,
                                                             dv_window_options opt) {
  const dv::CandRegion& g = cand[blockIdx.y];
  const dv::CandSlices c = dv::cand_slices(g);
  const WinSlices s = win_slices(g, win[blockIdx.y]);
  const uint32_t n = n_events(g);
  const int64_t len = g.len;
  for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += gridDim.x * kThreads) {
    if (!c.stands[e]) continue;
    const dv_allele_event ev = g.events[e];
    const int32_t kr = s.key_read[e], ko = s.key_off[e];
    int rank = 0;
    for (int32_t j = c.head[ev.position]; j != 0; j = c.next[j - 1]) {
      const int32_t o = j - 1;
      if (c.stands[o] && key_before(s.key_read[o], s.key_off[o], kr, ko)) ++rank;
    }
    const uint32_t type = type_of(ev);
    const int64_t i = ev.position, m = length_of(ev);
    int64_t lo = i, hi = i + 1;          // a substitution or a REFERENCE event
    if (type == kIns || type == kSoft) {
      lo = i + 1 - m;
      hi = i + 1 + m;
    } else if (type == kDel) {
      lo = i + 1;
      hi = i + 1 + m;
    }
    lo = lo < 0 ? 0 : lo > len ? len : lo;
    hi = hi < 0 ? 0 : hi > len ? len : hi;
    // AlleleFilter over SumAlleleCounts: the event's allele is the group of its representative
    bool counts = !low_quality(ev) && type != kRef;
    if (counts) {
      const int32_t count = c.count[c.rep[e]];
      counts = count >= opt.min_allele_support;
      if (counts && opt.enable_strict_insertion_filter && type == kIns && m <= 1) {
        // float32 division, correctly rounded: the double quotient of two float32 values rounds to it (53 >= 2 * 24 + 2)
        const float total = static_cast<float>(g.ref_count[ev.position] + c.alt[ev.position]);
        const float fraction = static_cast<float>(static_cast<double>(static_cast<float>(count)) / static_cast<double>(total));
        counts = static_cast<double>(fraction) >= 0.08;
      }
    }
    const int32_t slot = s.first_slot[ev.position] + rank;
    s.r_pos[slot] = ev.position;
    s.r_lo[slot] = static_cast<int32_t>(lo);
    s.r_hi[slot] = static_cast<int32_t>(hi);
    s.r_flag[slot] = static_cast<int32_t>(type) | (counts ? kCounts : 0);
  }
}

__global__ __launch_bounds__(kThreads) void win_score_kernel(const dv::CandRegion* cand, const dv::WindowRegion* win,
                                                             dv_window_options opt) {
  const dv::CandRegion& g = cand[blockIdx.x];
  const dv::WindowRegion& w = win[blockIdx.x];
  const WinSlices s = win_slices(g, w);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int4 tile[kThreads];
  __shared__ float coeff[8];
  __shared__ int wave_last[kWaves], scan[kWaves];
  if (threadIdx.x < 8) {
    const uint32_t t = threadIdx.x;
    coeff[t] = t == kRef ? opt.coeff_reference : t == kSub ? opt.coeff_substitution : t == kIns ? opt.coeff_insertion
             : t == kDel ? opt.coeff_deletion : t == kSoft ? opt.coeff_soft_clip : 0.0f;
  }
  __syncthreads();
  const bool linear = opt.model_type == DV_WINDOW_MODEL_ALLELE_COUNT_LINEAR;
  const int32_t n_records = *s.n_records;
  const int64_t d = opt.min_windows_distance;
  const size_t n_mask_words = (static_cast<size_t>(g.len) + 31) / 32;
  int n_win = 0, last = -1;              // uniform over the workgroup: windows started, the last candidate so far
  for (int32_t base = 0; base < g.len; base += kThreads) {
    const int32_t j = base + threadIdx.x;
    const bool live = j < g.len;
    float score = opt.bias;
    int32_t count = 0;
    const float ref_term = live ? __fmul_rn(static_cast<float>(g.ref_count[j]), opt.coeff_reference) : 0.0f;
    bool ref_done = false;
    for (int32_t t0 = 0; t0 < n_records; t0 += kThreads) {
      __syncthreads();                   // the previous tile is read
      const int32_t t = t0 + threadIdx.x;
      if (t < n_records) tile[threadIdx.x] = make_int4(s.r_pos[t], s.r_lo[t], s.r_hi[t], s.r_flag[t]);
      __syncthreads();
      if (!live) continue;
      const int m = min(kThreads, n_records - t0);
      for (int i = 0; i < m; ++i) {
        const int4 r = tile[i];
        if (!ref_done && r.x >= j) {
          score = __fadd_rn(score, ref_term);
          ref_done = true;
        }
        if (r.y <= j && j < r.z) {
          score = __fadd_rn(score, coeff[r.w & 7]);
          count += r.w >> 8;
        }
      }
    }
    if (!ref_done) score = __fadd_rn(score, ref_term);
    const bool is_candidate =
        live && (linear ? static_cast<double>(score) > opt.decision_boundary
                        : opt.min_num_supporting_reads <= count && count <= opt.max_num_supporting_reads);
    const uint64_t ballot = __ballot(is_candidate);
    if (w.scores && live) w.scores[j] = linear ? __float_as_uint(score) : static_cast<uint32_t>(count);
    if (w.mask && lane < 2) {
      const size_t word = static_cast<size_t>(base + wave * 64) / 32 + lane;
      if (word < n_mask_words) w.mask[word] = static_cast<uint32_t>(ballot >> (32 * lane));
    }
    // the candidate before j: in this wave, in an earlier wave of this chunk, or in an earlier chunk
    __syncthreads();                     // the previous round's wave_last are read
    if (lane == 0) wave_last[wave] = ballot ? base + wave * 64 + 63 - __clzll(static_cast<long long>(ballot)) : -1;
    const uint64_t below = ballot & ((1ull << lane) - 1ull);
    int32_t prev = below ? base + wave * 64 + 63 - __clzll(static_cast<long long>(below)) : -1;
    __syncthreads();
    for (int v = wave - 1; v >= 0 && prev < 0; --v) prev = wave_last[v];
    if (prev < 0) prev = last;
    const bool starts = is_candidate && (prev < 0 || static_cast<int64_t>(j) - prev > 2 * d);
    int chunk_starts = 0;
    const int at = n_win + block_exclusive_scan(starts ? 1 : 0, scan, &chunk_starts);
    if (starts) {
      w.windows[2 * static_cast<size_t>(at)] = w.interval_start + j - d;
      if (prev >= 0) w.windows[2 * static_cast<size_t>(at - 1) + 1] = w.interval_start + prev + d;
    }
    n_win += chunk_starts;
    for (int v = 0; v < kWaves; ++v) last = wave_last[v] >= 0 ? wave_last[v] : last;
  }
  if (threadIdx.x == 0) {
    if (last >= 0) w.windows[2 * static_cast<size_t>(n_win - 1) + 1] = w.interval_start + last + d;
    *w.n_windows = n_win;
  }
}

__device__ __forceinline__ int wave_add(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// The windows of all regions packed back to back in region order (one copy to the host): workgroup k finds its
// offset as the sum of the window counts of regions 0 .. k-1.
__global__ __launch_bounds__(kThreads) void win_pack_kernel(const dv::WindowRegion* win, int64_t* packed) {
  const dv::WindowRegion& w = win[blockIdx.x];
  __shared__ int partial[kWaves];
  int off = 0;
  for (unsigned j = threadIdx.x; j < blockIdx.x; j += kThreads) off += *win[j].n_windows;
  off = wave_add(off);
  if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = off;
  __syncthreads();
  off = 0;
  for (int v = 0; v < kWaves; ++v) off += partial[v];
  const int n = 2 * *w.n_windows;
  for (int i = threadIdx.x; i < n; i += kThreads) packed[2 * static_cast<size_t>(off) + i] = w.windows[i];
}

}  // namespace

namespace dv {

int window_check_options(const dv_window_options* w, const char* who) {
  const std::string name(who);
  if (!w) return fail(DV_ERR_INVALID_ARGUMENT, name + ": window options are null");
  if (w->model_type != DV_WINDOW_MODEL_VARIANT_READS && w->model_type != DV_WINDOW_MODEL_ALLELE_COUNT_LINEAR) {
    return fail(DV_ERR_INVALID_ARGUMENT, name + ": unknown window selector model type");
  }
  if (w->max_num_supporting_reads < w->min_num_supporting_reads) {
    return fail(DV_ERR_INVALID_ARGUMENT, name + ": max_num_supporting_reads is below min_num_supporting_reads");
  }
  if (w->min_windows_distance < 0) return fail(DV_ERR_INVALID_ARGUMENT, name + ": min_windows_distance must be >= 0");
  return DV_OK;
}

int window_launch(const CandRegion* d_cand, const WindowRegion* d_win, int32_t n, uint32_t max_events,
                  const dv_window_options* w, int64_t* packed, hipStream_t stream) {
  if (n <= 0) return DV_OK;
  if (int rc = cand_group_launch(d_cand, n, max_events, stream)) return rc;
  const unsigned ev_blocks =
      static_cast<unsigned>(std::min<int64_t>((static_cast<int64_t>(max_events) + kThreads - 1) / kThreads, 1024));
  const dim3 ev_grid(ev_blocks, static_cast<unsigned>(n)), region_grid(static_cast<unsigned>(n));
  ProfileScope prof(kProfOther, stream);
  if (max_events > 0) hipLaunchKernelGGL(win_first_kernel, ev_grid, dim3(kThreads), 0, stream, d_cand, d_win);
  hipLaunchKernelGGL(win_scan_kernel, region_grid, dim3(kThreads), 0, stream, d_cand, d_win);
  if (max_events > 0) hipLaunchKernelGGL(win_place_kernel, ev_grid, dim3(kThreads), 0, stream, d_cand, d_win, *w);
  hipLaunchKernelGGL(win_score_kernel, region_grid, dim3(kThreads), 0, stream, d_cand, d_win, *w);
  if (packed) hipLaunchKernelGGL(win_pack_kernel, region_grid, dim3(kThreads), 0, stream, d_win, packed);
  DV_HIP_CHECK(hipGetLastError());
  return DV_OK;
}

}  // namespace dv
