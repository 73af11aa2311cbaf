// candidates.hip -- VariantCaller::CallsFromAlleleCounter / CallPositionsFromAlleleCounts
// (deepvariant/variant_calling.cc:365-382, variant_calling_multisample.cc:940-1004; SelectAltAlleles /
// IsGoodAltAllele :232-258 over SumAlleleCounts / TotalAlleleCounts, allelecounter.cc:78-203) over the
// counts and events the counter kernel left on the device (allele_counter.hip), queued behind it on the
// same stream.  The host restatement and checker is deepvariant_amd/variant_calling.py VariantCaller.
//
// Five launches per batch of regions (blockIdx.y / blockIdx.x = region), no synchronisation:
//   cand_link     every event pushed on a per-position list (event_lists.h, shared with gvcf.hip)
//   cand_resolve  per event: does it stand, i.e. is it the last event of its read key at its position?
//                 A standing event that is neither low quality nor REFERENCE adds one to the position's
//                 total (TotalAlleleCounts without the reference-supporting reads)
//   cand_group    per standing non-REFERENCE event: the standing events of its position with the same
//                 (type, text) are its allele; their good ones are the allele's count, the first of them
//                 in event order its representative.  The representative applies IsGoodAltAllele
//   cand_emit     one workgroup per region: candidate sites in position order (ballot scan), their
//                 selected alleles (prefix sums), then one word per event
//   cand_pack     the site and allele records of all regions back to back in region order
// Texts never exist: a substitution is its base, a deletion its length and anchor base, an insertion or
// soft clip its length, anchor base and read bases, compared in place.  Integer work plus one IEEE-double
// division and comparison per allele, so the selection equals the host restatement's exactly.
#include <algorithm>

#include "cand_slices.h"
#include "candidates.h"
#include "event_lists.h"

// the layouts deepvariant_amd/_lib.py mirrors
static_assert(sizeof(dv_candidate_options) == 24, "dv_candidate_options layout");
static_assert(sizeof(dv_candidate_site) == 20, "dv_candidate_site layout");
static_assert(sizeof(dv_candidate_allele) == 16, "dv_candidate_allele layout");

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
enum : uint32_t { kRef = 1, kSub = 2, kIns = 3, kDel = 4, kSoft = 5 };   // AlleleType

__device__ __forceinline__ bool canonical_base(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }
__device__ __forceinline__ uint32_t type_of(const dv_allele_event& ev) { return (ev.length_type >> 28) & 7u; }
__device__ __forceinline__ uint32_t length_of(const dv_allele_event& ev) { return ev.length_type & 0x0fffffffu; }
__device__ __forceinline__ bool low_quality(const dv_allele_event& ev) { return (ev.length_type >> 31) != 0; }

using Slices = dv::CandSlices;
__device__ __forceinline__ Slices slices(const dv::CandRegion& g) { return dv::cand_slices(g); }

__device__ __forceinline__ uint32_t n_events(const dv::CandRegion& g) {
  const uint32_t n = *g.n_events;
  return n < g.event_cap ? n : g.event_cap;
}

__device__ __forceinline__ dv::EventLists lists(const dv::CandRegion& g, const Slices& s) {
  return dv::EventLists{g.events, g.read_key, s.head, s.next};
}

// The base an indel is anchored on: the read's previous base, or the reference base when the read
// starts with the indel (GetPrevBase, allelecounter.cc:386-400).
__device__ __forceinline__ uint8_t anchor_base(const dv::CandRegion& g, const dv_allele_event& ev) {
  return ev.read_offset > 0 ? g.bases[g.seq_off[ev.read] + ev.read_offset - 1] : g.ref[ev.position];
}

// Allele.bases equality of two events of one position and one type.
__device__ bool same_text(const dv::CandRegion& g, const dv_allele_event& a, const dv_allele_event& b) {
  const uint32_t type = type_of(a);
  const uint8_t* pa = g.bases + g.seq_off[a.read] + a.read_offset;
  const uint8_t* pb = g.bases + g.seq_off[b.read] + b.read_offset;
  if (type == kSub) return pa[0] == pb[0];
  const uint32_t n = length_of(a);
  if (n != length_of(b) || anchor_base(g, a) != anchor_base(g, b)) return false;
  if (type == kDel) return true;             // the deleted bases are the reference's behind one anchor position
  for (uint32_t i = 0; i < n; ++i) {
    if (pa[i] != pb[i]) return false;
  }
  return true;
}

__global__ __launch_bounds__(kThreads) void cand_link_kernel(const dv::CandRegion* regions) {
  const dv::CandRegion& g = regions[blockIdx.y];
  const dv::EventLists l = lists(g, slices(g));
  const uint32_t n = n_events(g);
  for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += gridDim.x * kThreads) dv::link_event(l, e);
}

__global__ __launch_bounds__(kThreads) void cand_resolve_kernel(const dv::CandRegion* regions) {
  const dv::CandRegion& g = regions[blockIdx.y];
  const Slices s = slices(g);
  const dv::EventLists l = lists(g, s);
  const uint32_t n = n_events(g);
  for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += gridDim.x * kThreads) {
    const dv_allele_event ev = g.events[e];
    if (!dv::event_stands(l, e, ev)) continue;                  // stands[] was zeroed
    s.stands[e] = 1;
    if (!low_quality(ev) && type_of(ev) != kRef) atomicAdd(&s.alt[ev.position], 1);
  }
}

__global__ __launch_bounds__(kThreads) void cand_group_kernel(const dv::CandRegion* regions, dv_candidate_options opt) {
  const dv::CandRegion& g = regions[blockIdx.y];
  const Slices s = slices(g);
  const uint32_t n = n_events(g);
  for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += gridDim.x * kThreads) {
    const dv_allele_event ev = g.events[e];
    const uint32_t type = type_of(ev);
    if (!s.stands[e] || type == kRef) continue;
    int32_t count = 0;
    uint32_t rep = e;
    dv_allele_event rep_ev = ev;
    for (int32_t j = s.head[ev.position]; j != 0; j = s.next[j - 1]) {
      const uint32_t o = static_cast<uint32_t>(j - 1);
      if (!s.stands[o]) continue;
      const dv_allele_event other = g.events[o];
      if (type_of(other) != type || (o != e && !same_text(g, ev, other))) continue;
      count += low_quality(other) ? 0 : 1;
      if (dv::stored_before(other, rep_ev)) {
        rep = o;
        rep_ev = other;
      }
    }
    s.rep[e] = static_cast<int32_t>(rep);
    if (rep != e) continue;
    s.count[e] = count;
    // IsGoodAltAllele.  An allele without a good read is not in SumAlleleCounts at all.
    const int32_t total = g.ref_count[ev.position] + s.alt[ev.position];
    const bool snp = type == kSub;
    const int32_t min_count = snp ? opt.min_count_snps : opt.min_count_indels;
    const double min_fraction = static_cast<double>(snp ? opt.min_fraction_snps : opt.min_fraction_indels);
    if (type != kSoft && count >= 1 && count >= min_count &&
        (1.0 * static_cast<double>(count)) / static_cast<double>(total) >= min_fraction &&
        canonical_base(g.ref[ev.position])) {
      s.sel[e] = 1;
      atomicAdd(&s.nsel[ev.position], 1);
    }
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

__global__ __launch_bounds__(kThreads) void cand_emit_kernel(const dv::CandRegion* regions, int32_t positions_only) {
  const dv::CandRegion& g = regions[blockIdx.x];
  const Slices s = slices(g);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int wave_sites[kWaves], scan[kWaves];
  int n_sites = 0, n_alleles = 0;        // uniform over the workgroup
  for (int32_t base = 0; base < g.len; base += kThreads) {
    const int32_t p = base + threadIdx.x;
    const int32_t k = p < g.len ? s.nsel[p] : 0;
    const uint64_t sites = __ballot(k > 0);
    __syncthreads();                     // the previous round's wave_sites are read
    if (lane == 0) wave_sites[wave] = __popcll(sites);
    int chunk_alleles = 0;
    const int allele_at = n_alleles + block_exclusive_scan(k, scan, &chunk_alleles);   // (synchronises)
    int site_at = n_sites, chunk_sites = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) site_at += wave_sites[w];
      chunk_sites += wave_sites[w];
    }
    if (k > 0) {
      dv_candidate_site site;
      site.offset = p;
      site.ref_count = g.ref_count[p];
      site.total = site.ref_count + s.alt[p];
      site.first_allele = allele_at;
      site.n_alleles = k;
      g.sites[site_at + __popcll(sites & ((1ull << lane) - 1ull))] = site;
      if (!positions_only) {
        // the site's selected alleles in the event order of their representatives
        for (int32_t j = s.head[p]; j != 0; j = s.next[j - 1]) {
          if (!s.sel[j - 1]) continue;
          const dv_allele_event ev = g.events[j - 1];
          int ord = 0;
          for (int32_t i = s.head[p]; i != 0; i = s.next[i - 1]) {
            if (i != j && s.sel[i - 1] && dv::stored_before(g.events[i - 1], ev)) ++ord;
          }
          dv_candidate_allele a;
          a.length_type = ev.length_type & 0x7fffffffu;
          a.count = s.count[j - 1];
          a.read = ev.read;
          a.read_offset = ev.read_offset;
          g.alleles[allele_at + ord] = a;
          s.sel[j - 1] = ord + 1;        // still non-zero for the inner loop's test
        }
      }
    }
    n_sites += chunk_sites;
    n_alleles += chunk_alleles;
  }
  if (threadIdx.x == 0) {
    g.n_out[0] = n_sites;
    g.n_out[1] = n_alleles;
  }
  if (positions_only) return;
  __syncthreads();                       // sel[] now holds ordinals, written by other threads of this workgroup
  const uint32_t n = n_events(g);
  for (uint32_t e = threadIdx.x; e < n; e += kThreads) {
    int32_t word = DV_CANDIDATE_EVENT_OVERWRITTEN;
    if (s.stands[e]) {
      word = DV_CANDIDATE_EVENT_UNCALLED;
      if (type_of(g.events[e]) != kRef) {
        const int32_t ord = s.sel[s.rep[e]];
        if (ord > 0) word = ord - 1;
      }
    }
    g.words[e] = word;
  }
}

__device__ __forceinline__ int wave_add(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// The records of all regions packed back to back in region order (one copy to the host each): workgroup
// k finds its offsets as the sums of the record counts of regions 0 .. k-1.
__global__ __launch_bounds__(kThreads) void cand_pack_kernel(const dv::CandRegion* regions, dv_candidate_site* packed_sites,
                                                             dv_candidate_allele* packed_alleles) {
  const dv::CandRegion& g = regions[blockIdx.x];
  __shared__ int partial[2][kWaves];
  int site_off = 0, allele_off = 0;
  for (unsigned j = threadIdx.x; j < blockIdx.x; j += kThreads) {
    site_off += regions[j].n_out[0];
    allele_off += regions[j].n_out[1];
  }
  site_off = wave_add(site_off);
  allele_off = wave_add(allele_off);
  if ((threadIdx.x & 63) == 0) {
    partial[0][threadIdx.x >> 6] = site_off;
    partial[1][threadIdx.x >> 6] = allele_off;
  }
  __syncthreads();
  site_off = allele_off = 0;
  for (int w = 0; w < kWaves; ++w) {
    site_off += partial[0][w];
    allele_off += partial[1][w];
  }
  const int ns = g.n_out[0], na = g.n_out[1];
  for (int i = threadIdx.x; i < ns; i += kThreads) packed_sites[site_off + i] = g.sites[i];
  if (packed_alleles) {
    for (int i = threadIdx.x; i < na; i += kThreads) packed_alleles[allele_off + i] = g.alleles[i];
  }
}

}  // namespace

namespace dv {

int cand_check_options(const dv_candidate_options* c, const char* who) {
  const std::string name(who);
  if (!c) return fail(DV_ERR_INVALID_ARGUMENT, name + ": candidate options are null");
  // CHECK_GE in VariantCaller's constructor (a NaN threshold fails the comparison too)
  if (c->min_count_snps < 0 || c->min_count_indels < 0 || !(c->min_fraction_snps >= 0.0f) ||
      !(c->min_fraction_indels >= 0.0f)) {
    return fail(DV_ERR_INVALID_ARGUMENT, name + ": candidate thresholds must be >= 0");
  }
  return DV_OK;
}

int cand_group_launch(const CandRegion* d_regions, int32_t n, uint32_t max_events, hipStream_t stream) {
  if (n <= 0 || max_events == 0) return DV_OK;
  const unsigned ev_blocks =
      static_cast<unsigned>(std::min<int64_t>((static_cast<int64_t>(max_events) + kThreads - 1) / kThreads, 1024));
  const dim3 ev_grid(ev_blocks, static_cast<unsigned>(n));
  const dv_candidate_options none{};           // the selection (sel, nsel) is of no use to the caller
  ProfileScope prof(kProfOther, stream);
  hipLaunchKernelGGL(cand_link_kernel, ev_grid, dim3(kThreads), 0, stream, d_regions);
  hipLaunchKernelGGL(cand_resolve_kernel, ev_grid, dim3(kThreads), 0, stream, d_regions);
  hipLaunchKernelGGL(cand_group_kernel, ev_grid, dim3(kThreads), 0, stream, d_regions, none);
  DV_HIP_CHECK(hipGetLastError());
  return DV_OK;
}

int cand_launch(const CandRegion* d_regions, int32_t n, uint32_t max_events,
                const dv_candidate_options* c, dv_candidate_site* packed_sites, dv_candidate_allele* packed_alleles,
                hipStream_t stream) {
  if (n <= 0) return DV_OK;
  // grid-stride in x; a region's surplus workgroups leave at once
  const unsigned ev_blocks =
      static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>((static_cast<int64_t>(max_events) + kThreads - 1) / kThreads, 1), 1024));
  const dim3 ev_grid(ev_blocks, static_cast<unsigned>(n));
  ProfileScope prof(kProfOther, stream);
  if (max_events > 0) {
    hipLaunchKernelGGL(cand_link_kernel, ev_grid, dim3(kThreads), 0, stream, d_regions);
    hipLaunchKernelGGL(cand_resolve_kernel, ev_grid, dim3(kThreads), 0, stream, d_regions);
    hipLaunchKernelGGL(cand_group_kernel, ev_grid, dim3(kThreads), 0, stream, d_regions, *c);
  }
  hipLaunchKernelGGL(cand_emit_kernel, dim3(static_cast<unsigned>(n)), dim3(kThreads), 0, stream, d_regions,
                     c->positions_only);
  if (packed_sites) {
    hipLaunchKernelGGL(cand_pack_kernel, dim3(static_cast<unsigned>(n)), dim3(kThreads), 0, stream, d_regions,
                       packed_sites, c->positions_only ? nullptr : packed_alleles);
  }
  DV_HIP_CHECK(hipGetLastError());
  return DV_OK;
}

}  // namespace dv
