// Read phasing for a batch of regions from arrays: dv_phase_reads_batch (host code: the checker in a loop) and
// dv_phase_reads_batch_device (one kernel, a workgroup per region), include/dvhip.h.
//
// The contract is dv::DirectPhasing::phase_reads (direct_phasing.cpp), which stays the checker; the kernel gives its
// read_phases, allele_phases and allele_flags value for value.  What of the checker makes an array kernel possible:
//
// Only substitution sites enter the graph.  candidate_filter refuses a site whose called alleles are not all as long as
//   the reference span, and an earlier indel's span shadows later sites through indel_end, the refused ones included.
// Vertex order and texts.  A vertex text is "REF" or the allele's bases; within a site the texts are distinct.  Vertex
//   order is REF first (only with >= 3 support entries, counted before the low-quality filter), then alleles by bases.
//   compare_vertex_pair_by_bases compares texts as strings, so "REF" sorts after A, C, G, N and before T.  The plan
//   (phasing.h) compares the alleles' bytes and hands the kernel each vertex's RANK among its site's texts; every
//   comparison the checker makes is between vertices of one site, so ranks decide them all.
// Read sets.  A vertex's reads are its support entries with 0 <= read < n_reads that are not low quality.
//   is_first_allele is per (vertex, read) in vertex insertion order.
// Edges.  An edge joins a read's consecutive vertices when they sit at consecutive graph positions (build's quirk --
//   the later vertex at positions_[1] takes an edge from whatever came before -- adds nothing when every read has at
//   most one vertex per site: whatever came before then sits at positions_[0]).  A read listed under two entries of one
//   site is legal input and gives edges within the site: such a region goes to the host code.
//   With one vertex per read and site: edge(u, v) <=> reads(u) & reads(v) != 0 for u one position before v, and
//   first_allele_reads(v) = reads(v) & ~(reads of all earlier graph sites).
// Two live positions.  A position's scores depend only on the previous position's scores (value, from-pair and the two
//   read sets per ordered vertex pair) and on the vertices' read sets; the backtrack needs, for every position, per
//   ordered pair: present or not, score, from-pair.
// The per-position step is an arg-max per to-pair over the present from-pairs, ordered by (score, from-pair by
//   compare_vertex_pair_by_bases): a total order, so the result does not depend on iteration order.
//   found_advancing_score and AllScoresAreTheSame are reductions over the same combinations.  A vertex without in-edges
//   at a position that has incoming edges is joined to every vertex of the previous position.  update_starting_score
//   erases all pairs of the position and then sets only pairs i <= j in vertex order.  Presence of a pair matters
//   everywhere (find == end).
// Set arithmetic (calculate_score) on bitmaps: cont[p] = prev.support[p] & reads(to[p]); first[p] =
//   first_allele_reads(to[p]); score = prev + |cont0 | cont1| + |first0 | first1| / 2 (integer division), reset to prev
//   when both |cont[p]| < 2; new support[p] = cont[p] | first[p].  Starting scores compare the two read sets for equality.
// Tail.  max_score / assign_phases_to_vertices and AssignPhasesToReads are serial and cheap: one thread runs the
//   backtrack literally as the checker does, "unexpected phasing score" and "loop detected" included.
//
// Kernel.  One workgroup of 256 threads per region; the position loop is serial.  Per position: the site's vertices'
// read bitmaps are built in LDS from the support lists (atomicOr on 64-bit words: a union, the order does not matter);
// first-allele bitmaps come from a running "seen" bitmap, the sites being walked in order; edges are bitmap
// intersections with the previous position.  Four adjacent lanes share a to-pair: each scores every fourth from-pair
// with popcounts over the words, a shuffle reduction over the four picks the arg-max of the packed key (score, rank
// pair), and the four then write the winner's two new read sets.  The position's (score, from) table goes to global
// memory for the backtrack.  Thread 0 backtracks; all threads then count, per read, its vertices of phase 1 and 2
// (integer atomicAdd in LDS: a sum) and write the reads' phases.  No atomic decides a value.
//
// Host side: one upload image, the launch, one download image per call (device_round_trip.h's Layout, RoundTrip); the
// regions outside the limits are phased by the checker on the calling thread while the kernel runs.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "device_round_trip.h"
#include "phasing.h"

namespace {

using dv::phasing::DevRegion;
using dv::phasing::DevSite;
using dv::phasing::DevVertex;

constexpr int kThreads = 256;
constexpr int kV = DV_PHASING_DEVICE_MAX_VERTICES;      // vertices per site
constexpr int kPairs = kV * kV;                         // ordered pairs per position
constexpr int kWords = DV_PHASING_DEVICE_MAX_READS / 64;
constexpr int kLanesPerPair = kThreads / kPairs;        // 4
constexpr int kAbsent = -2, kStart = -1;                // Entry::from otherwise: u1 * kV + u2 at the previous position
static_assert(kLanesPerPair == 4 && (kV & (kV - 1)) == 0, "the lane mapping below");
static_assert(2 * DV_PHASING_DEVICE_MAX_READS * sizeof(int) <= sizeof(unsigned long long) * 2 * kPairs * 2 * kWords,
              "the reads' phase counts reuse the support bitmaps' LDS");

struct Entry {           // one ordered pair of one position, as the backtrack reads it
  int32_t score;
  int32_t from;
};

struct Tables {          // device pointers into the upload
  const DevRegion* regions;
  const DevSite* sites;
  const DevVertex* vertices;
  const int32_t* support_reads;
  const uint8_t* support_low_quality;
  int32_t min_alleles_to_phase;
};

struct Outputs {         // device pointers into the download, and the work space
  int32_t* read_phases;      // the device regions' reads, concatenated
  int32_t* allele_phases;    // whole allele table
  uint8_t* allele_flags;
  unsigned long long* combinations;   // per device region
  Entry* tables;             // work space: [sites][kPairs]
};

// MaxScore: the best-scoring present pair at a position (ties: larger texts), or nothing if all present pairs score the same.
__device__ bool max_score(const Entry* tab, const DevVertex* verts, int nv, int* b1, int* b2) {
  bool have = false;
  int best_score = 0;
  for (int v1 = 0; v1 < nv; ++v1) {
    for (int v2 = 0; v2 < nv; ++v2) {
      const Entry e = tab[v1 * kV + v2];
      if (e.from == kAbsent) continue;
      bool take = false;
      if (e.score > best_score) {
        take = true;
      } else if (e.score == best_score) {
        // compare_vertex_pair_by_bases(v1, v2, best)
        take = !have || verts[v1].rank > verts[*b1].rank ||
               (verts[v1].rank == verts[*b1].rank && verts[v2].rank > verts[*b2].rank);
      }
      if (take) {
        *b1 = v1;
        *b2 = v2;
        best_score = e.score;
        have = true;
      }
    }
  }
  for (int p = 0; p < nv * kV; ++p) {
    if ((p & (kV - 1)) < nv && tab[p].from != kAbsent && tab[p].score != best_score) return have;
  }
  return false;
}

// assign_phases_to_vertices, block by block from the last position; a pair is (position, v1, v2).
__device__ void backtrack(const Tables& t, const Outputs& o, const DevRegion& reg) {
  const DevSite* sites = t.sites + reg.site_off;
  const Entry* tabs = o.tables + reg.table_off * kPairs;
  auto allele = [&](int pos, int v) { return t.vertices[sites[pos].vertex_off + v].allele; };
  int i = reg.n_sites - 1;
  bool have_cur = false, have_prev = false;
  int c1 = 0, c2 = 0, p_pos = -1, p1 = 0, p2 = 0;       // cur sits at position i
  while (i >= 0) {
    have_cur = false;
    while (i >= 0) {
      have_cur = max_score(tabs + static_cast<long long>(i) * kPairs, t.vertices + sites[i].vertex_off, sites[i].n_vertices,
                           &c1, &c2);
      if (have_cur) break;
      --i;
    }
    if (!have_prev) {
      p_pos = i;
      p1 = c1;
      p2 = c2;
      have_prev = have_cur;
    } else {
      o.allele_flags[allele(p_pos, p1)] = 1;
      o.allele_flags[allele(p_pos, p2)] = 1;
    }
    int verts_in_block = 0;
    while (have_cur) {
      ++verts_in_block;
      const bool het = c1 != c2;
      o.allele_phases[allele(i, c1)] = het ? 1 : 0;
      o.allele_phases[allele(i, c2)] = het ? 2 : 0;
      const Entry e = tabs[static_cast<long long>(i) * kPairs + c1 * kV + c2];
      const bool cur_is_prev = i == p_pos && c1 == p1 && c2 == p2;
      if (!cur_is_prev && verts_in_block > 1 && have_prev &&
          e.score == tabs[static_cast<long long>(p_pos) * kPairs + p1 * kV + p2].score) {
        o.allele_phases[allele(i, c1)] = 0;             // "unexpected phasing score"
        o.allele_phases[allele(i, c2)] = 0;
        --i;
        break;
      }
      if (e.from < 0) {                                 // the block's first position
        if (verts_in_block == 1) {
          o.allele_phases[allele(i, c1)] = 0;
          o.allele_phases[allele(i, c2)] = 0;
        }
        p_pos = i;
        p1 = c1;
        p2 = c2;
        have_prev = true;
        --i;
        break;
      }
      // "loop detected" (cur == next) cannot hold: next sits one position before cur
      p_pos = i;
      p1 = c1;
      p2 = c2;
      have_prev = true;
      c1 = e.from / kV;
      c2 = e.from % kV;
      --i;
    }
  }
  if (have_prev && have_cur) {
    // cur was left at position i + 1 by the break that ended the last block
    o.allele_flags[allele(i + 1, c1)] = 1;
    o.allele_flags[allele(i + 1, c2)] = 1;
  }
}

__global__ __launch_bounds__(kThreads) void phase_regions_kernel(Tables t, Outputs o) {
  // the two live positions: per ordered pair the two read sets, score and from-pair; per vertex reads and rank
  __shared__ unsigned long long support[2][kPairs][2][kWords];     // 32 KiB
  __shared__ unsigned long long reads[2][kV][kWords];
  __shared__ unsigned long long first[kV][kWords];
  __shared__ unsigned long long seen[kWords];
  __shared__ int score[2][kPairs], from[2][kPairs], rank[2][kV];
  __shared__ unsigned char edge[kV][kV];
  __shared__ int has_incoming, advancing, min_score, max_score_here;
  __shared__ unsigned long long combinations;

  const int tid = threadIdx.x;
  const DevRegion reg = t.regions[blockIdx.x];
  const DevSite* sites = t.sites + reg.site_off;
  const int n_words = (reg.n_reads + 63) >> 6;
  Entry* tabs = o.tables + reg.table_off * kPairs;

  for (int a = tid; a < reg.n_alleles; a += kThreads) {
    o.allele_phases[reg.allele_off + a] = -1;
    o.allele_flags[reg.allele_off + a] = 0;
  }
  if (tid < kWords) seen[tid] = 0;
  if (tid == 0) combinations = 0;
  __syncthreads();

  const int pair = tid / kLanesPerPair, sub = tid % kLanesPerPair;    // this thread's to-pair and its share of it
  const int v1 = pair / kV, v2 = pair % kV;
  int nv_prev = 0;
  for (int i = 0; i < reg.n_sites; ++i) {
    const int cur = i & 1, prv = cur ^ 1;
    const DevSite site = sites[i];
    const int nv = site.n_vertices;
    const DevVertex* verts = t.vertices + site.vertex_off;
    for (int k = tid; k < nv * n_words; k += kThreads) reads[cur][k / n_words][k % n_words] = 0;
    if (tid < kPairs) {
      score[cur][tid] = 0;
      from[cur][tid] = kAbsent;
    }
    if (tid < nv) {
      rank[cur][tid] = verts[tid].rank;
      o.allele_phases[verts[tid].allele] = 0;           // a vertex: phase 0 until the backtrack says otherwise
    }
    if (tid == 0) {
      has_incoming = 0;
      advancing = 0;
      min_score = INT_MAX;
      max_score_here = 0;
    }
    __syncthreads();
    for (int v = 0; v < nv; ++v) {
      const DevVertex vert = verts[v];
      for (int k = tid; k < vert.n_support; k += kThreads) {
        const int r = t.support_reads[vert.support_off + k];
        if (r >= 0 && r < reg.n_reads && !t.support_low_quality[vert.support_off + k]) {
          atomicOr(&reads[cur][v][r >> 6], 1ull << (r & 63));
        }
      }
    }
    __syncthreads();
    if (tid < n_words) {                                // is_first_allele: no earlier graph site lists the read
      unsigned long long here = 0;
      for (int v = 0; v < nv; ++v) {
        first[v][tid] = reads[cur][v][tid] & ~seen[tid];
        here |= reads[cur][v][tid];
      }
      seen[tid] |= here;
    }
    if (i > 0 && tid < kPairs) {                        // edge(u, v): a read carries both
      const int u = tid / kV, v = tid % kV;
      bool shared = false;
      if (u < nv_prev && v < nv) {
        for (int w = 0; w < n_words; ++w) shared = shared || (reads[prv][u][w] & reads[cur][v][w]) != 0;
      }
      edge[u][v] = shared;
      if (shared) atomicOr(&has_incoming, 1);
    }
    __syncthreads();
    bool restart = i == 0 || !has_incoming;
    if (!restart) {
      if (tid < nv) {                                   // a vertex no read reaches: joined to every vertex before it
        bool any = false;
        for (int u = 0; u < nv_prev; ++u) any = any || edge[u][tid];
        if (!any) {
          for (int u = 0; u < nv_prev; ++u) edge[u][tid] = 1;
        }
      }
      __syncthreads();
      long long best = -1;                              // (score << 16) | (from-pair's ranks << 8) | from-pair
      bool adv = false;
      int scored = 0;
      if (v1 < nv && v2 < nv) {
        for (int fp = sub; fp < kPairs; fp += kLanesPerPair) {
          const int u1 = fp / kV, u2 = fp % kV;
          if (u1 >= nv_prev || u2 >= nv_prev || from[prv][fp] == kAbsent || !edge[u1][v1] || !edge[u2][v2]) continue;
          int c0 = 0, c1 = 0, cont = 0, firsts = 0;
          for (int w = 0; w < n_words; ++w) {
            const unsigned long long a = support[prv][fp][0][w] & reads[cur][v1][w];
            const unsigned long long b = support[prv][fp][1][w] & reads[cur][v2][w];
            c0 += __popcll(a);
            c1 += __popcll(b);
            cont += __popcll(a | b);
            firsts += __popcll(first[v1][w] | first[v2][w]);
          }
          const int before = score[prv][fp];
          int s = before + cont + firsts / 2;
          if (c0 < 2 && c1 < 2) s = before;
          adv = adv || before < s;
          ++scored;
          const long long key = (static_cast<long long>(s) << 16) | ((rank[prv][u1] * kV + rank[prv][u2]) << 8) | fp;
          best = key > best ? key : best;
        }
      }
      // the four lanes of a to-pair are neighbours in one wave
      for (int d = 1; d < kLanesPerPair; d <<= 1) {
        const long long other = __shfl_xor(best, d, 64);
        best = other > best ? other : best;
      }
      if (best >= 0) {
        const int fp = static_cast<int>(best & 0xff);
        for (int w = sub; w < n_words; w += kLanesPerPair) {
          support[cur][pair][0][w] = (support[prv][fp][0][w] & reads[cur][v1][w]) | first[v1][w];
          support[cur][pair][1][w] = (support[prv][fp][1][w] & reads[cur][v2][w]) | first[v2][w];
        }
        if (sub == 0) {
          const int s = static_cast<int>(best >> 16);
          score[cur][pair] = s;
          from[cur][pair] = fp;
          atomicMin(&min_score, s);
          atomicMax(&max_score_here, s);
        }
      }
      if (adv) atomicOr(&advancing, 1);
      if (scored) atomicAdd(&combinations, static_cast<unsigned long long>(scored));
      __syncthreads();
      // AllScoresAreTheSame: the scores reached here differ by at most one (none reached: 0 - INT_MAX)
      restart = i + 1 < reg.n_sites && (!advancing || !(max_score_here - min_score > 1));
    }
    if (restart) {                                      // update_starting_score: a new phase block starts
      const bool set = v1 < nv && v2 < nv && v1 <= v2;
      if (v1 < nv && v2 < nv) {
        for (int w = sub; w < n_words; w += kLanesPerPair) {
          support[cur][pair][0][w] = reads[cur][v1][w];
          support[cur][pair][1][w] = reads[cur][v2][w];
        }
        if (sub == 0) {
          int n1 = 0, n2 = 0;
          bool same = true;
          for (int w = 0; w < n_words; ++w) {
            n1 += __popcll(reads[cur][v1][w]);
            n2 += __popcll(reads[cur][v2][w]);
            same = same && reads[cur][v1][w] == reads[cur][v2][w];
          }
          score[cur][pair] = set ? (same ? n1 : n1 + n2) : 0;
          from[cur][pair] = set ? kStart : kAbsent;
        }
      }
    }
    __syncthreads();
    if (tid < kPairs) tabs[static_cast<long long>(i) * kPairs + tid] = Entry{score[cur][tid], from[cur][tid]};
    nv_prev = nv;
  }
  __syncthreads();
  if (tid == 0) {
    backtrack(t, o, reg);
    o.combinations[blockIdx.x] = combinations;
  }
  __syncthreads();

  // AssignPhasesToReads: per read, its vertices of phase 1 and of phase 2
  int* count = reinterpret_cast<int*>(&support[0][0][0][0]);       // [2][DV_PHASING_DEVICE_MAX_READS]
  for (int k = tid; k < 2 * DV_PHASING_DEVICE_MAX_READS; k += kThreads) count[k] = 0;
  __syncthreads();
  for (int i = 0; i < reg.n_sites; ++i) {
    const DevSite site = sites[i];
    for (int v = 0; v < site.n_vertices; ++v) {
      const DevVertex vert = t.vertices[site.vertex_off + v];
      const int phase = o.allele_phases[vert.allele];
      if (phase != 1 && phase != 2) continue;
      for (int k = tid; k < vert.n_support; k += kThreads) {
        const int r = t.support_reads[vert.support_off + k];
        if (r >= 0 && r < reg.n_reads && !t.support_low_quality[vert.support_off + k]) {
          atomicAdd(&count[(phase - 1) * DV_PHASING_DEVICE_MAX_READS + r], 1);
        }
      }
    }
  }
  __syncthreads();
  for (int r = tid; r < reg.n_reads; r += kThreads) {
    const int n1 = count[r], n2 = count[DV_PHASING_DEVICE_MAX_READS + r];
    int phase = 0;
    if (n1 > n2 && n1 >= t.min_alleles_to_phase) {
      phase = 1;
    } else if (n2 > n1 && n2 >= t.min_alleles_to_phase) {
      phase = 2;
    }
    o.read_phases[reg.phase_off + r] = phase;
  }
}

dv_phasing_stats& last_stats() {
  static thread_local dv_phasing_stats stats;
  return stats;
}

int run_on_device(const std::string& who, const dv::phasing::Args& a, int32_t* read_phases, int32_t* allele_phases,
                  uint8_t* allele_flags, dv_phasing_stats* stats, void* stream_in) {
  last_stats() = dv_phasing_stats{0, 0, 0, 0, 0, 0};
  if (int rc = dv::phasing::check(who, a, read_phases)) return rc;
  dv::phasing::Plan plan;
  dv::phasing::make_plan(a, &plan);
  dv::phasing::Results res(a);
  auto phase_host_regions = [&]() -> int {
    for (int32_t k : plan.host_regions) {
      if (int rc = dv::phasing::phase_region_on_host(who, a, k, res.read_phases.data() + res.read_off[k],
                                                     res.allele_phases.data(), res.allele_flags.data())) {
        return rc;
      }
    }
    return DV_OK;
  };
  if (plan.candidates_in_regions == 0 || plan.regions.empty()) {      // nothing to launch
    // without candidates every read's phase is 0 and there is no allele to report
    if (int rc = phase_host_regions()) return rc;
    for (const DevRegion& reg : plan.regions) {
      for (int32_t j = 0; j < reg.n_alleles; ++j) res.allele_phases[reg.allele_off + j] = -1;
    }
  } else {
    const size_t n_dev = plan.regions.size(), n_sites = plan.sites.size(), n_vertices = plan.vertices.size();
    const size_t n_support = static_cast<size_t>(a.n_support), n_alleles = static_cast<size_t>(a.n_alleles);
    const size_t n_reads = static_cast<size_t>(plan.device_reads);
    dv::Layout up, down, work;
    // upload image: regions | sites | vertices | support_reads | support_low_quality
    const size_t u_regions = up.add(n_dev * sizeof(DevRegion));
    const size_t u_sites = up.add(n_sites * sizeof(DevSite));
    const size_t u_vertices = up.add(n_vertices * sizeof(DevVertex));
    const size_t u_reads = up.add(n_support * sizeof(int32_t));
    const size_t u_low = up.add(n_support);
    // download image: combinations per region | read phases | allele phases | allele flags
    const size_t d_comb = down.add(n_dev * sizeof(unsigned long long));
    const size_t d_phases = down.add(n_reads * sizeof(int32_t));
    const size_t d_allele_phases = down.add(n_alleles * sizeof(int32_t));
    const size_t d_allele_flags = down.add(n_alleles);
    // device-only work space: the per-position tables
    work.add((n_sites ? n_sites : 1) * kPairs * sizeof(Entry));
    static thread_local dv::RoundTrip rt;
    if (int rc = rt.begin(who + ": no HIP device (dv_phase_reads_batch is the host code)", stream_in, up.bytes(),
                          down.bytes(), work.bytes())) {
      return rc;
    }
    std::memcpy(rt.host_up<DevRegion>(u_regions), plan.regions.data(), n_dev * sizeof(DevRegion));
    if (n_sites) std::memcpy(rt.host_up<DevSite>(u_sites), plan.sites.data(), n_sites * sizeof(DevSite));
    if (n_vertices) std::memcpy(rt.host_up<DevVertex>(u_vertices), plan.vertices.data(), n_vertices * sizeof(DevVertex));
    if (n_support) {
      std::memcpy(rt.host_up<int32_t>(u_reads), a.support_reads, n_support * sizeof(int32_t));
      std::memcpy(rt.host_up<uint8_t>(u_low), a.support_low_quality, n_support);
    }
    Tables t;
    t.regions = rt.dev_up<const DevRegion>(u_regions);
    t.sites = rt.dev_up<const DevSite>(u_sites);
    t.vertices = rt.dev_up<const DevVertex>(u_vertices);
    t.support_reads = rt.dev_up<const int32_t>(u_reads);
    t.support_low_quality = rt.dev_up<const uint8_t>(u_low);
    t.min_alleles_to_phase = a.min_alleles_to_phase;
    Outputs o;
    o.combinations = rt.dev_down<unsigned long long>(d_comb);
    o.read_phases = rt.dev_down<int32_t>(d_phases);
    o.allele_phases = rt.dev_down<int32_t>(d_allele_phases);
    o.allele_flags = rt.dev_down<uint8_t>(d_allele_flags);
    o.tables = static_cast<Entry*>(rt.d_scratch.ptr);
    hipStream_t stream = rt.stream();
    if (int rc = rt.upload(up.bytes())) return rc;
    {
      dv::ProfileScope prof(dv::kProfOther, stream);
      hipLaunchKernelGGL(phase_regions_kernel, dim3(static_cast<unsigned>(n_dev)), dim3(kThreads), 0, stream, t, o);
      DV_HIP_CHECK(hipGetLastError());
    }
    const int host_rc = phase_host_regions();           // while the kernel runs; the stream is waited for either way
    if (int rc = rt.finish(down.bytes())) return rc;
    if (host_rc) return host_rc;
    plan.stats.launches = 1;
    const unsigned long long* comb = rt.host_down<unsigned long long>(d_comb);
    const int32_t* phases = rt.host_down<int32_t>(d_phases);
    const int32_t* al_phases = rt.host_down<int32_t>(d_allele_phases);
    const uint8_t* al_flags = rt.host_down<uint8_t>(d_allele_flags);
    for (size_t k = 0; k < n_dev; ++k) {
      const DevRegion& reg = plan.regions[k];
      plan.stats.combinations += static_cast<int64_t>(comb[k]);
      std::memcpy(res.read_phases.data() + res.read_off[reg.region], phases + reg.phase_off,
                  static_cast<size_t>(reg.n_reads) * sizeof(int32_t));
      std::memcpy(res.allele_phases.data() + reg.allele_off, al_phases + reg.allele_off,
                  static_cast<size_t>(reg.n_alleles) * sizeof(int32_t));
      std::memcpy(res.allele_flags.data() + reg.allele_off, al_flags + reg.allele_off, static_cast<size_t>(reg.n_alleles));
    }
  }
  res.hand_out(a, read_phases, allele_phases, allele_flags);
  last_stats() = plan.stats;
  if (stats) *stats = plan.stats;
  return DV_OK;
}

}  // namespace

extern "C" {

int dv_phase_reads_batch(const dv_phasing_region* regions, int32_t n_regions, const dv_phasing_candidate* candidates,
                         int32_t n_candidates, const dv_phasing_allele* alleles, int32_t n_alleles, const char* bases,
                         int64_t n_bases, const int32_t* support_reads, const uint8_t* support_low_quality,
                         int64_t n_support, int64_t n_reads_total, int32_t min_alleles_to_phase, int32_t* read_phases,
                         int32_t* allele_phases, uint8_t* allele_flags, dv_phasing_stats* stats) {
  return dv::guarded("dv_phase_reads_batch", [&]() -> int {
    const dv::phasing::Args a{regions, n_regions, candidates, n_candidates, alleles, n_alleles, bases, n_bases,
                              support_reads, support_low_quality, n_support, n_reads_total, min_alleles_to_phase};
    return dv::phasing::run_on_host("dv_phase_reads_batch", a, read_phases, allele_phases, allele_flags, stats);
  });
}

int dv_phase_reads_batch_device(const dv_phasing_region* regions, int32_t n_regions,
                                const dv_phasing_candidate* candidates, int32_t n_candidates,
                                const dv_phasing_allele* alleles, int32_t n_alleles, const char* bases, int64_t n_bases,
                                const int32_t* support_reads, const uint8_t* support_low_quality, int64_t n_support,
                                int64_t n_reads_total, int32_t min_alleles_to_phase, int32_t* read_phases,
                                int32_t* allele_phases, uint8_t* allele_flags, dv_phasing_stats* stats, void* stream) {
  return dv::guarded("dv_phase_reads_batch_device", [&]() -> int {
    const dv::phasing::Args a{regions, n_regions, candidates, n_candidates, alleles, n_alleles, bases, n_bases,
                              support_reads, support_low_quality, n_support, n_reads_total, min_alleles_to_phase};
    return run_on_device("dv_phase_reads_batch_device", a, read_phases, allele_phases, allele_flags, stats, stream);
  });
}

int dv_phase_device_last_stats(dv_phasing_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_phase_device_last_stats: null");
  *out = last_stats();
  return DV_OK;
}

}  // extern "C"
