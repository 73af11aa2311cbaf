// The device side of the gVCF merge and the checks of its arguments: the two scans' operators,
// the three-launch scan, the merge's tables and its three kernels.  Private to gvcf_merge.hip (dv_gvcf_merge[_device])
// and gvcf_rows.hip (dv_gvcf_rows[_device], section 23), which runs the same stages and goes on to the text.  All of
// it sits in an anonymous namespace: each of the two files gets its own copy of the kernels, and nothing is exported.
#ifndef DV_GVCF_MERGE_DEVICE_H_
#define DV_GVCF_MERGE_DEVICE_H_

#include <hip/hip_runtime.h>

#include <string>

#include "dv_internal.h"
#include "gvcf_merge.h"

namespace {

namespace gm = dv::gm;

constexpr int kThreads = 256;
constexpr int kItems = 4;                       // consecutive elements per lane
constexpr int kChunk = kThreads * kItems;       // elements per workgroup of a scan

// ---- the two scans' operators.  combine(a, b) folds b, which comes later, onto a; both are associative.
struct SegMax {                 // the maximum since the last group start
  struct T {
    int64_t v;
    int32_t head;               // a group starts somewhere in the span
  };
  static __device__ T identity() { return T{INT64_MIN, 0}; }
  static __device__ T combine(const T& a, const T& b) { return b.head ? b : T{a.v > b.v ? a.v : b.v, a.head}; }
};
struct Sum {
  using T = int64_t;
  static __device__ T identity() { return 0; }
  static __device__ T combine(T a, T b) { return a + b; }
};

struct MaxSource {              // element i = variant i's end; a head where a group's variants begin
  const int64_t* var_end;
  const int64_t* var_off;
  int32_t n_groups;
  int64_t* cm;
  __device__ SegMax::T load(int64_t i) const {
    return SegMax::T{var_end[i], var_off[gm::group_of(var_off, n_groups, i)] == i ? 1 : 0};
  }
  __device__ void store(int64_t i, const SegMax::T& /*before*/, const SegMax::T& with) const { cm[i] = with.v; }
};
struct SumSource {              // element b = block b's piece count; the exclusive sum is kept
  const int32_t* count;
  int64_t* piece_off;
  __device__ int64_t load(int64_t i) const { return count[i]; }
  __device__ void store(int64_t i, int64_t before, int64_t /*with*/) const { piece_off[i] = before; }
};

// The inclusive scan of one value per lane across the workgroup (Hillis-Steele over two LDS rows, a barrier a step).
// -> the row that holds every lane's inclusive value, valid until the rows are written again.  Every lane of the
// workgroup must call it.
template <class Op>
__device__ const typename Op::T* workgroup_scan(typename Op::T x, typename Op::T (*rows)[kThreads]) {
  const int t = static_cast<int>(threadIdx.x);
  int cur = 0;
  rows[cur][t] = x;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    typename Op::T y = rows[cur][t];
    if (t >= d) y = Op::combine(rows[cur][t - d], y);
    rows[cur ^ 1][t] = y;
    __syncthreads();
    cur ^= 1;
  }
  return rows[cur];
}

// The fold of a lane's kItems consecutive elements of chunk `chunk`, those below n.
template <class Op, class Source>
__device__ typename Op::T lane_fold(const Source& src, int64_t chunk, int64_t n) {
  typename Op::T acc = Op::identity();
  const int64_t first = chunk * kChunk + static_cast<int64_t>(threadIdx.x) * kItems;
  for (int k = 0; k < kItems; ++k) {
    if (first + k < n) acc = Op::combine(acc, src.load(first + k));
  }
  return acc;
}

// Launch 1 of a scan: totals[chunk] = the fold of the chunk.  One workgroup per chunk.
template <class Op, class Source>
__global__ __launch_bounds__(kThreads) void scan_totals_kernel(Source src, int64_t n, typename Op::T* totals) {
  __shared__ typename Op::T rows[2][kThreads];
  const typename Op::T* scanned = workgroup_scan<Op>(lane_fold<Op>(src, blockIdx.x, n), rows);
  if (threadIdx.x == 0) totals[blockIdx.x] = scanned[kThreads - 1];
}

// Launch 2: totals[c] becomes the fold of the chunks before c, by ONE workgroup that walks the totals kThreads at a
// time with a carry; the fold of all of them goes to *all when `all` is given.
template <class Op>
__global__ __launch_bounds__(kThreads) void scan_carries_kernel(typename Op::T* totals, int64_t n_chunks,
                                                                typename Op::T* all) {
  __shared__ typename Op::T rows[2][kThreads];
  typename Op::T carry = Op::identity();
  for (int64_t base = 0; base < n_chunks; base += kThreads) {
    const int64_t c = base + static_cast<int64_t>(threadIdx.x);
    const typename Op::T mine = c < n_chunks ? totals[c] : Op::identity();
    const typename Op::T* scanned = workgroup_scan<Op>(mine, rows);
    typename Op::T before = carry;                       // exclusive: up to the lane before
    if (threadIdx.x > 0) before = Op::combine(carry, scanned[threadIdx.x - 1]);
    if (c < n_chunks) totals[c] = before;
    carry = Op::combine(carry, scanned[kThreads - 1]);
    __syncthreads();            // the rows are rewritten by the next tile
  }
  if (all != nullptr && threadIdx.x == 0) *all = carry;
}

// Launch 3: the chunk again, each element stored with the fold of everything before it and with itself.
template <class Op, class Source>
__global__ __launch_bounds__(kThreads) void scan_apply_kernel(Source src, int64_t n, const typename Op::T* carries) {
  __shared__ typename Op::T rows[2][kThreads];
  const typename Op::T* scanned = workgroup_scan<Op>(lane_fold<Op>(src, blockIdx.x, n), rows);
  typename Op::T acc = carries[blockIdx.x];
  if (threadIdx.x > 0) acc = Op::combine(acc, scanned[threadIdx.x - 1]);
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kItems;
  for (int k = 0; k < kItems; ++k) {
    if (first + k >= n) break;
    const typename Op::T with = Op::combine(acc, src.load(first + k));
    src.store(first + k, acc, with);
    acc = with;
  }
}

struct Tables {                 // one call's arrays, all on the device
  int32_t n_groups;
  int64_t n_blocks, n_vars;
  const int64_t *block_off, *var_off, *block_start, *block_end, *var_start, *var_end;
  const int64_t* cm;            // [V]
  int32_t* count;               // [B]
  const int64_t* piece_off;     // [B], exclusive
  const int64_t* n_pieces;      // the total
  int64_t *piece_start, *piece_end, *piece_slot, *var_slot;
  int32_t* piece_block;
};

__device__ int64_t pieces_before(const Tables& t, int64_t block) {
  return block < t.n_blocks ? t.piece_off[block] : *t.n_pieces;
}

__global__ __launch_bounds__(kThreads) void count_pieces_kernel(Tables t) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kThreads + static_cast<int64_t>(threadIdx.x);
  if (b >= t.n_blocks) return;
  const int32_t g = gm::group_of(t.block_off, t.n_groups, b);
  t.count[b] = gm::walk_block(t.block_start[b], t.block_end[b], t.var_start, t.var_end, t.cm, t.var_off[g],
                              t.var_off[g + 1], [](int32_t, int64_t, int64_t) {});
}

__global__ __launch_bounds__(kThreads) void write_pieces_kernel(Tables t) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kThreads + static_cast<int64_t>(threadIdx.x);
  if (b >= t.n_blocks) return;
  const int32_t g = gm::group_of(t.block_off, t.n_groups, b);
  const int64_t v0 = t.var_off[g], v1 = t.var_off[g + 1], at = t.piece_off[b];
  gm::walk_block(t.block_start[b], t.block_end[b], t.var_start, t.var_end, t.cm, v0, v1,
                 [&](int32_t k, int64_t s, int64_t e) {
                   t.piece_start[at + k] = s;
                   t.piece_end[at + k] = e;
                   t.piece_block[at + k] = static_cast<int32_t>(b);
                   t.piece_slot[at + k] = gm::piece_slot(at + k, e, t.var_start, v0, v1);
                 });
}

__global__ __launch_bounds__(kThreads) void variant_slots_kernel(Tables t) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + static_cast<int64_t>(threadIdx.x);
  if (j >= t.n_vars) return;
  const int32_t g = gm::group_of(t.var_off, t.n_groups, j);
  t.var_slot[j] = gm::var_slot(j, t.var_start[j], t.piece_end, pieces_before(t, t.block_off[g]),
                               pieces_before(t, t.block_off[g + 1]));
}

// One scan, three launches queued on `stream`; `launches` is the caller's count of them.
template <class Op, class Source>
int scan_on_device(const Source& src, int64_t n, typename Op::T* totals, typename Op::T* all, hipStream_t stream,
                   int64_t* launches) {
  const int64_t n_chunks = (n + kChunk - 1) / kChunk;
  const dim3 grid(static_cast<unsigned>(n_chunks)), one(1), threads(kThreads);
  hipLaunchKernelGGL((scan_totals_kernel<Op, Source>), grid, threads, 0, stream, src, n, totals);
  DV_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((scan_carries_kernel<Op>), one, threads, 0, stream, totals, n_chunks, all);
  DV_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((scan_apply_kernel<Op, Source>), grid, threads, 0, stream, src, n, totals);
  DV_HIP_CHECK(hipGetLastError());
  *launches += 3;
  return DV_OK;
}

// The merge's stages queued on `stream`, every array of `t` on the device and *t.n_pieces not yet written: the running
// maximum (3 launches, with variants), the count, the sum and the pieces (5, with blocks), the variants' slots (1).
// max_totals: one SegMax::T per chunk of variants; sum_totals: one int64 per chunk of blocks.
inline int merge_stages_on_device(const Tables& t, int64_t* cm, int64_t* piece_off, int64_t* n_pieces,
                                  SegMax::T* max_totals, int64_t* sum_totals, hipStream_t stream, int64_t* launches) {
  const dim3 threads(kThreads);
  const dim3 block_grid(static_cast<unsigned>((t.n_blocks + kThreads - 1) / kThreads));
  const dim3 var_grid(static_cast<unsigned>((t.n_vars + kThreads - 1) / kThreads));
  DV_HIP_CHECK(hipMemsetAsync(n_pieces, 0, sizeof(int64_t), stream));   // no block: no piece
  if (t.n_vars > 0) {
    const MaxSource src{t.var_end, t.var_off, t.n_groups, cm};
    if (int rc = scan_on_device<SegMax>(src, t.n_vars, max_totals, static_cast<SegMax::T*>(nullptr), stream, launches)) {
      return rc;
    }
  }
  if (t.n_blocks > 0) {
    hipLaunchKernelGGL(count_pieces_kernel, block_grid, threads, 0, stream, t);
    DV_HIP_CHECK(hipGetLastError());
    ++*launches;
    const SumSource src{t.count, piece_off};
    if (int rc = scan_on_device<Sum>(src, t.n_blocks, sum_totals, n_pieces, stream, launches)) return rc;
    hipLaunchKernelGGL(write_pieces_kernel, block_grid, threads, 0, stream, t);
    DV_HIP_CHECK(hipGetLastError());
    ++*launches;
  }
  if (t.n_vars > 0) {
    hipLaunchKernelGGL(variant_slots_kernel, var_grid, threads, 0, stream, t);
    DV_HIP_CHECK(hipGetLastError());
    ++*launches;
  }
  return DV_OK;
}

// The merge's arguments, checked on the host for every entry point; have_out: the caller's result pointer is not null.
inline int check_merge_arguments(const std::string& name, bool have_out, int32_t n_groups, const int64_t* block_off,
                                 const int64_t* var_off, const int64_t* block_start, const int64_t* block_end,
                                 const int64_t* var_start, const int64_t* var_end) {
  if (!have_out || n_groups < 0 || !block_off || !var_off) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer or negative count");
  }
  if (block_off[0] != 0 || var_off[0] != 0) return dv::fail(DV_ERR_BAD_INPUT, name + ": the offsets must start at 0");
  for (int32_t g = 0; g < n_groups; ++g) {
    if (block_off[g + 1] < block_off[g] || var_off[g + 1] < var_off[g]) {
      return dv::fail(DV_ERR_BAD_INPUT, name + ": the offsets descend at group " + std::to_string(g));
    }
  }
  const int64_t nb = block_off[n_groups], nv = var_off[n_groups];
  if ((nb > 0 && (!block_start || !block_end)) || (nv > 0 && (!var_start || !var_end))) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer");
  }
  if (nb + nv > 0x7fffffff) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": more than 2^31 - 1 records in one call");
  for (int32_t g = 0; g < n_groups; ++g) {
    for (int64_t b = block_off[g]; b < block_off[g + 1]; ++b) {
      if (block_start[b] >= block_end[b]) return dv::fail(DV_ERR_BAD_INPUT, name + ": block " + std::to_string(b) + " is empty");
      if (b > block_off[g] && block_start[b] < block_end[b - 1]) {
        return dv::fail(DV_ERR_BAD_INPUT, name + ": block " + std::to_string(b) + " is out of order or overlaps the one before it");
      }
    }
    for (int64_t j = var_off[g]; j < var_off[g + 1]; ++j) {
      if (var_start[j] >= var_end[j]) return dv::fail(DV_ERR_BAD_INPUT, name + ": variant " + std::to_string(j) + " is empty");
      if (j > var_off[g] && (var_start[j] < var_start[j - 1] || (var_start[j] == var_start[j - 1] && var_end[j] < var_end[j - 1]))) {
        return dv::fail(DV_ERR_BAD_INPUT, name + ": variant " + std::to_string(j) + " is out of order: (start, end) must ascend");
      }
    }
  }
  return DV_OK;
}

}  // namespace

#endif  // DV_GVCF_MERGE_DEVICE_H_
