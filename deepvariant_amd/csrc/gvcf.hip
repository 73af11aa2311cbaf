// gvcf.hip -- VariantCaller.make_gvcfs (deepvariant/variant_caller.py) over the allele counts the
// counter kernel left on the device (allele_counter.hip), queued behind it on the same stream.
//
// Five launches per batch of regions (blockIdx.y / blockIdx.x = region), no synchronisation:
//   gvcf_link     every event pushed on a per-position list (atomicExch on the list head; event_lists.h,
//                 shared with candidates.hip)
//   gvcf_resolve  per event: is it the last allele of its read key at its position (read_alleles is a
//                 map keyed by read key: a later allele of the same key overwrites)?  If so and it is
//                 neither low quality nor REFERENCE, it adds one to the position's non-reference count
//   gvcf_sites    per site: n_total, the rescale of deep sites, the table lookup, the quantised GQ
//   gvcf_blocks   one workgroup per region: run starts in order (ballot scans), then one wave per run
//                 for MIN(GQ), MIN_DP and the exact median depth (binary search on the value)
//   gvcf_pack     the records of all regions back to back in region order: one copy to the host
// Only the block records leave the device.  The likelihood model itself is a host table
// (dv_gvcf_options.table): the device does integer and IEEE-double bookkeeping only, so its records
// equal the host restatement's bit for bit.
#include <algorithm>
#include <cstring>
#include <vector>

#include "event_lists.h"
#include "gvcf.h"

// the layouts deepvariant_amd/_lib.py mirrors
static_assert(sizeof(dv_gvcf_site) == 32, "dv_gvcf_site layout");
static_assert(sizeof(dv_gvcf_block) == 56, "dv_gvcf_block layout");
static_assert(sizeof(dv_gvcf_options) == 48, "dv_gvcf_options layout");

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ bool canonical_base(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }

// scratch slices (dv::gvcf_scratch_ints)
struct Slices {
  int32_t *head, *alt, *key, *gq, *dp, *tix, *next;
};
__device__ __forceinline__ Slices slices(const dv::GvcfRegion& g) {
  const size_t len = static_cast<size_t>(g.len);
  Slices s;
  s.head = g.scratch;
  s.alt = s.head + len + 1;
  s.key = s.alt + len + 1;
  s.gq = s.key + len;
  s.dp = s.gq + len;
  s.tix = s.dp + len;
  s.next = s.tix + len;
  return s;
}

__device__ __forceinline__ uint32_t n_events(const dv::GvcfRegion& g) {
  const uint32_t n = *g.n_events;
  return n < g.event_cap ? n : g.event_cap;
}

__device__ __forceinline__ dv::EventLists lists(const dv::GvcfRegion& g, const Slices& s) {
  return dv::EventLists{g.events, g.read_key, s.head, s.next};
}

__global__ __launch_bounds__(kThreads) void gvcf_link_kernel(const dv::GvcfRegion* regions) {
  const dv::GvcfRegion& g = regions[blockIdx.y];
  const dv::EventLists l = lists(g, slices(g));
  const uint32_t n = n_events(g);
  for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += gridDim.x * kThreads) dv::link_event(l, e);
}

__global__ __launch_bounds__(kThreads) void gvcf_resolve_kernel(const dv::GvcfRegion* regions) {
  const dv::GvcfRegion& g = regions[blockIdx.y];
  const Slices s = slices(g);
  const dv::EventLists l = lists(g, s);
  const uint32_t n = n_events(g);
  for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += gridDim.x * kThreads) {
    const dv_allele_event ev = g.events[e];
    const uint32_t type = (ev.length_type >> 28) & 7u;
    if ((ev.length_type >> 31) || type == 1u) continue;        // low quality or REFERENCE: never counted
    if (dv::event_stands(l, e, ev)) atomicAdd(&s.alt[ev.position], 1);
  }
}

__global__ __launch_bounds__(kThreads) void gvcf_sites_kernel(const dv::GvcfRegion* regions, const dv_gvcf_site* table,
                                                              int32_t max_cov, int32_t resolution) {
  const dv::GvcfRegion& g = regions[blockIdx.y];
  const Slices s = slices(g);
  for (int32_t p = g.lo + blockIdx.x * kThreads + threadIdx.x; p < g.hi; p += gridDim.x * kThreads) {
    const int32_t n_ref = g.ref_count[p];
    const int32_t n_total = n_ref + s.alt[p];
    s.dp[p] = n_total;
    if (!canonical_base(g.ref[p])) {                           // N and the other IUPAC codes: no record
      s.key[p] = -1;
      s.gq[p] = 0;
      s.tix[p] = 0;
      continue;
    }
    int64_t t = n_total, r = n_ref;
    if (t > max_cov) {
      // _rescale_read_counts_if_necessary: int(math.ceil(n_ref / (1.0 * n_total) * M)) in IEEE double
      const double ratio = static_cast<double>(n_ref) / (1.0 * static_cast<double>(n_total));
      r = static_cast<int64_t>(ceil(ratio * static_cast<double>(max_cov)));
      t = max_cov;
      r = r < t ? r : t;                                        // ratio <= 1: a guard, never taken
    }
    const int32_t ix = static_cast<int32_t>(t * (t + 1) / 2 + r);
    const dv_gvcf_site site = table[ix];
    const int32_t raw = site.gq;
    const int32_t q = raw < 1 ? 0 : ((raw - 1) / resolution) * resolution + 1;
    s.key[p] = (q << 1) | (site.has_valid_gl ? 1 : 0);
    s.gq[p] = raw;
    s.tix[p] = ix;
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int wave_add(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// The k-th smallest (0-based) of dp[s, e), whose values lie in [lo, hi]: the least v with
// #{dp <= v} > k.  Wave-uniform.
__device__ int wave_select(const int32_t* dp, int32_t s, int32_t e, int k, int lo, int hi, int lane) {
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    int c = 0;
    for (int32_t p = s + lane; p < e; p += 64) c += dp[p] <= mid ? 1 : 0;
    if (wave_add(c) > k) {
      hi = mid;
    } else {
      lo = mid + 1;
    }
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void gvcf_blocks_kernel(const dv::GvcfRegion* regions, const dv_gvcf_site* table,
                                                               int32_t include_med_dp) {
  const dv::GvcfRegion& g = regions[blockIdx.x];
  const Slices s = slices(g);
  int32_t* runs = s.head;      // the lists are no longer needed: run starts [n_runs + 1]
  int32_t* ords = s.alt;       // and each run's record index (-1: no record)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int wave_runs[kThreads / 64], wave_recs[kThreads / 64];
  __shared__ int n_runs, n_recs;
  if (threadIdx.x == 0) n_runs = n_recs = 0;
  __syncthreads();
  for (int32_t base = g.lo; base < g.hi; base += kThreads) {
    const int32_t p = base + threadIdx.x;
    const bool in = p < g.hi;
    const int32_t k = in ? s.key[p] : 0;
    const bool start = in && (p == g.lo || s.key[p - 1] != k);
    const bool rec = start && k >= 0;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t bs = __ballot(start), br = __ballot(rec);
    if (lane == 0) {
      wave_runs[wave] = __popcll(bs);
      wave_recs[wave] = __popcll(br);
    }
    __syncthreads();
    int run_at = n_runs, rec_at = n_recs;
    for (int w = 0; w < wave; ++w) {
      run_at += wave_runs[w];
      rec_at += wave_recs[w];
    }
    if (start) {
      const int i = run_at + __popcll(bs & below);
      runs[i] = p;
      ords[i] = rec ? rec_at + __popcll(br & below) : -1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 0; w < kThreads / 64; ++w) {
        n_runs += wave_runs[w];
        n_recs += wave_recs[w];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    runs[n_runs] = g.hi;
    *g.n_blocks = n_recs;
  }
  __syncthreads();             // runs / ords are read back by other waves of this workgroup
  for (int r = wave; r < n_runs; r += kThreads / 64) {
    const int o = ords[r];
    if (o < 0) continue;
    const int32_t a = runs[r], b = runs[r + 1];
    int mn_gq = 0x7fffffff, mn_dp = 0x7fffffff, mx_dp = 0;
    for (int32_t p = a + lane; p < b; p += 64) {
      mn_gq = min(mn_gq, s.gq[p]);
      mn_dp = min(mn_dp, s.dp[p]);
      mx_dp = max(mx_dp, s.dp[p]);
    }
    mn_gq = wave_min(mn_gq);
    mn_dp = wave_min(mn_dp);
    mx_dp = wave_max(mx_dp);
    int med = -1;
    if (include_med_dp) {
      const int n = b - a;
      // int(statistics.median(...)): the middle value, or the floor of the mean of the two middle ones
      const int hi_mid = wave_select(s.dp, a, b, n / 2, mn_dp, mx_dp, lane);
      if (n & 1) {
        med = hi_mid;
      } else {
        const int lo_mid = wave_select(s.dp, a, b, n / 2 - 1, mn_dp, mx_dp, lane);
        med = static_cast<int>((static_cast<int64_t>(lo_mid) + hi_mid) / 2);
      }
    }
    if (lane == 0) {
      const dv_gvcf_site first = table[s.tix[a]];
      dv_gvcf_block blk;
      blk.start = g.interval_start + a;
      blk.end = g.interval_start + b;
      blk.likelihoods[0] = first.likelihoods[0];
      blk.likelihoods[1] = first.likelihoods[1];
      blk.likelihoods[2] = first.likelihoods[2];
      blk.gq = mn_gq;
      blk.min_dp = mn_dp;
      blk.med_dp = med;
      blk.ref_base = g.ref[a];
      blk.has_valid_gl = static_cast<uint8_t>(s.key[a] & 1);
      blk.reserved[0] = blk.reserved[1] = 0;
      g.blocks[o] = blk;
    }
  }
}

// The records of all regions packed back to back in region order (one copy to the host): workgroup k
// finds its offset as the sum of the record counts of regions 0 .. k-1.
__global__ __launch_bounds__(kThreads) void gvcf_pack_kernel(const dv::GvcfRegion* regions, dv_gvcf_block* packed) {
  const dv::GvcfRegion& g = regions[blockIdx.x];
  __shared__ int partial[kThreads / 64];
  int off = 0;
  for (unsigned j = threadIdx.x; j < blockIdx.x; j += kThreads) off += *regions[j].n_blocks;
  off = wave_add(off);
  if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = off;
  __syncthreads();
  off = 0;
  for (int w = 0; w < kThreads / 64; ++w) off += partial[w];
  const int nb = *g.n_blocks;
  for (int i = threadIdx.x; i < nb; i += kThreads) packed[off + i] = g.blocks[i];
}

bool iupac_non_canonical(char b) { return b != 0 && std::strchr("NRYKMSWBDHV", b) != nullptr; }

}  // namespace

namespace dv {

int gvcf_check_options(const dv_gvcf_options* g, const char* who) {
  const std::string name(who);
  if (!g) return fail(DV_ERR_INVALID_ARGUMENT, name + ": gvcf options are null");
  if (g->gq_resolution < 1 || g->max_cache_coverage < 0 || g->left_padding < 0 || g->right_padding < 0 || !g->table) {
    return fail(DV_ERR_INVALID_ARGUMENT, name + ": bad gvcf options");
  }
  const int64_t m = g->max_cache_coverage;
  if (m > 10000) return fail(DV_ERR_INVALID_ARGUMENT, name + ": max_cache_coverage above 10000");
  if (g->n_table != (m + 1) * (m + 2) / 2) {
    return fail(DV_ERR_INVALID_ARGUMENT, name + ": the table must have (M + 1) * (M + 2) / 2 entries");
  }
  for (int64_t i = 0; i < g->n_table; ++i) {
    if (g->table[i].gq < 0) return fail(DV_ERR_INVALID_ARGUMENT, name + ": negative GQ in the table");
  }
  return DV_OK;
}

int gvcf_check_region(const dv_allele_counter_options* o, const dv_gvcf_options* g, const char* who) {
  if (!o || !o->ref_bases || o->ref_start > o->interval_start || o->ref_start + o->n_ref_bases < o->interval_end) {
    return fail(DV_ERR_INVALID_ARGUMENT, std::string(who) + ": the reference window must cover the interval");
  }
  const int64_t len = o->interval_end - o->interval_start;
  if (len > 0x7fffffff - 2) return fail(DV_ERR_INVALID_ARGUMENT, std::string(who) + ": interval too long for gVCF");
  // AlleleCounter.summary_counts: CHECK(left_padding + right_padding < counts_.size())
  if (static_cast<int64_t>(g->left_padding) + g->right_padding >= len) {
    return fail(DV_ERR_INVALID_ARGUMENT, std::string(who) + ": left_padding + right_padding must be < the interval length");
  }
  const char* ref = o->ref_bases + (o->interval_start - o->ref_start);
  for (int64_t p = g->left_padding; p < len - g->right_padding; ++p) {
    const char b = ref[p];
    if (b != 'A' && b != 'C' && b != 'G' && b != 'T' && !iupac_non_canonical(b)) {
      return fail(DV_ERR_BAD_INPUT, std::string(who) + ": reference base '" + std::string(1, b) +
                                        "' is not an IUPAC nucleotide code");
    }
  }
  return DV_OK;
}

int gvcf_table_on_device(const dv_gvcf_options* g, const dv_gvcf_site** d_table, hipStream_t stream) {
  static thread_local DeviceBuffer buf;
  static thread_local std::vector<dv_gvcf_site> host;
  const size_t n = static_cast<size_t>(g->n_table);
  int device = -1;
  DV_HIP_CHECK(hipGetDevice(&device));
  const bool same = buf.ptr && buf.device == device && host.size() == n &&
                    std::memcmp(host.data(), g->table, n * sizeof(dv_gvcf_site)) == 0;
  if (!same) {
    if (int rc = buf.reserve_on_current_device(n * sizeof(dv_gvcf_site))) return rc;
    host.assign(g->table, g->table + n);     // the copy's source stays alive until the next upload
    DV_HIP_CHECK(hipMemcpyAsync(buf.ptr, host.data(), n * sizeof(dv_gvcf_site), hipMemcpyHostToDevice, stream));
  }
  *d_table = static_cast<const dv_gvcf_site*>(buf.ptr);
  return DV_OK;
}

int gvcf_launch(const GvcfRegion* d_regions, int32_t n, int64_t max_len, uint32_t max_events,
                const dv_gvcf_options* g, const dv_gvcf_site* d_table, dv_gvcf_block* packed, hipStream_t stream) {
  if (n <= 0) return DV_OK;
  // grid-stride in x; a region's surplus workgroups leave at once
  auto blocks_for = [](int64_t items) {
    return static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>((items + kThreads - 1) / kThreads, 1), 1024));
  };
  const dim3 ev_grid(blocks_for(max_events), static_cast<unsigned>(n));
  const dim3 site_grid(blocks_for(max_len), static_cast<unsigned>(n));
  ProfileScope prof(kProfOther, stream);
  if (max_events > 0) {
    hipLaunchKernelGGL(gvcf_link_kernel, ev_grid, dim3(kThreads), 0, stream, d_regions);
    hipLaunchKernelGGL(gvcf_resolve_kernel, ev_grid, dim3(kThreads), 0, stream, d_regions);
  }
  hipLaunchKernelGGL(gvcf_sites_kernel, site_grid, dim3(kThreads), 0, stream, d_regions, d_table,
                     g->max_cache_coverage, g->gq_resolution);
  hipLaunchKernelGGL(gvcf_blocks_kernel, dim3(static_cast<unsigned>(n)), dim3(kThreads), 0, stream, d_regions, d_table,
                     g->include_med_dp);
  if (packed) hipLaunchKernelGGL(gvcf_pack_kernel, dim3(static_cast<unsigned>(n)), dim3(kThreads), 0, stream, d_regions, packed);
  DV_HIP_CHECK(hipGetLastError());
  return DV_OK;
}

}  // namespace dv
