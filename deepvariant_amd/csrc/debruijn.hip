// debruijn.hip -- the realigner's local assembly up to pruning (debruijn_graph.cpp: DeBruijnGraph::build's choice of
// k, the constructor, has_cycle) for every window of a batch in one kernel launch, and the C entry points
// dv_debruijn_compact_batch / dv_debruijn_compact_batch_device / dv_debruijn_from_compact; behind that kernel, pruning
// and the candidate haplotypes themselves in a second launch (dv_debruijn_paths_batch / dv_debruijn_paths_batch_device).
//
// Contract: DeBruijnGraph::build up to, but not including, prune / prune_lite, restated without the maps.  For a
// window with reference bytes ref (raw, never upper-cased), reads (upper-cased by the call), options o:
//   1. k range: max_k = min(o.max_k, |ref| - 1); the schedule is k = o.min_k, + o.step_k, ... <= max_k.
//   2. start: the first k of the schedule for which no two reference k-mers are equal, byte for byte; none: no graph.
//      A repeat-free k stays repeat-free for every larger k, so the test runs only until it first passes.
//   3. reference occurrences: the reference's k-mers at 0 .. |ref| - k are vertex occurrences, consecutive ones are
//      edges with is_ref set.
//   4. read occurrences: a read of n bytes takes part with mapq >= o.min_mapq and n > k.  A bad position is a byte
//      outside ACGT or with quality below o.min_base_quality.  Segment starts are 0 and b + 1 for every bad position
//      b; only starts below n - k count.  For a start i let bad be the first bad position >= i, or n.  When
//      bad - k <= 0 (absolute, not relative to i) the segment contributes nothing.  Otherwise position i is a vertex
//      occurrence -- even if its k-mer runs over the bad base, even if i itself is bad -- and positions
//      i + 1 .. bad - k are vertex occurrences with an edge from their predecessor each.
//      Per position, without the walk: g is a start iff g = 0 or g - 1 is bad; a start occurs iff g < n - k and
//      nb(g) > k; any other g occurs, with an edge from g - 1, iff g + k <= nb(g), where nb(g) is the first bad
//      position >= g, or n (no bad position lies between such a g and its segment's start, so nb is the segment's).
//   5. two k-mers are equal iff their k bytes are equal -- the hash only picks the slot and spares comparisons; a
//      vertex is a distinct k-mer, an edge a distinct (from, to); weight counts the walks over an edge, the
//      reference's too; is_ref is the OR over them; the first occurrence is the minimum of (seq, pos), an edge's
//      being that of its `from` k-mer.
//   6. the first k from the start upwards whose graph has no directed cycle (a self-loop is one) wins; none: no graph.
//
// Shape: one workgroup of 256 threads per window, the k loop inside.  A window's sequences lie back to back, the
// reference first, so a byte offset g orders occurrences as (seq, pos) does and serves as the occurrence key.  Once
// per window: uint64 polynomial prefix hashes over the bytes (a chunk per thread, the 256 chunk sums scanned by one
// thread), so a k-mer's hash costs two loads for any k; per read position the next bad position and the read's
// number (a read per thread, backwards).  Per k: the vertex table is open addressing on the occurrence key
// (atomicCAS claims a slot; on an occupied slot the hashes, then the bytes, are compared against the slot's
// representative; atomicMin keeps the first occurrence) and each position remembers its slot; the edge table is
// keyed by the two slots (atomicAdd weight, atomicOr is_ref, atomicMin occurrence), and a newly claimed edge is
// pushed on its `from` vertex's list and counts into its `to` vertex's in-degree.  The cycle test peels: the vertices
// of in-degree 0 form the first worklist; a thread removes a vertex, decrements its successors, follows the first
// one that reaches 0 itself -- a de Bruijn graph is mostly chains -- and appends the others to the list for the next
// round; the graph is acyclic iff every vertex was removed.  At the winning k the used slots are stored as
// occurrence keys; the host sorts them by first occurrence and renumbers, so the races that decide slot order never
// reach the caller.  The tables are sized by the window (at most twice the limits of include/dvhip.h) and live in
// the window's slice of a device scratch buffer the calling thread reuses (RoundTrip::d_scratch; the upload and
// download images and the thread's stream are device_round_trip.h's too): at the measured sizes they do not fit
// LDS.  Every loop is bounded: a probe sequence by the table's size (then the window's
// overflow flag is set and the host builds it), the peel by vertices + 1 rounds, a chain by the vertex count, an
// edge list by the edge count, the k loop by the schedule; no workgroup waits for another.
//
// Pruning and path enumeration (dv_debruijn_paths_batch_device): debruijn_paths_kernel, launched on the same stream
// right behind debruijn_kernel with the same grid, works on a window's tables while they are still in its scratch
// slice (vkey, ekey, ew, the per-vertex edge lists head / enext, slot_of for the source and the sink, the bytes) and
// on debruijn_kernel's header; debruijn_paths.h has the rule (prune + candidate_haplotypes as a closed form, pruning
// on) and its serial pieces.  Per window: (a) one pass over the edge table counts every vertex's alive out-edges
// (`pending`) and threads every alive edge on its target's in-edge list (inhead / innext); the sink's out-edges are
// left out, a walk ends there.  (b) cnt[] by a reverse peel: the vertices with nothing pending form the first
// worklist (the sink with cnt 1, dead ends with 0); a thread that resolves a vertex decrements its predecessors, sums
// a predecessor's count over its out-edges when it brings it to zero (saturating at max_num_paths + 1: all its targets
// are resolved by then, so the sum does not depend on who computes it), follows the first such predecessor itself and
// appends the others to the list for the next round.  (c) T = cnt[source]; T > max_num_paths: status "too many".
// (d) one lane per walk number, striding by the workgroup: a first pass unranks each walk for its length, the lengths
// are scanned (a chunk per thread, the 256 chunk sums by one thread) into offsets inside the window's haplotype slice,
// a second pass unranks again and writes the bytes.  Nothing depends on slot numbers but the tables' own links, so
// the bytes are a pure function of the input.  The paths tables (cnt, pending, inhead, the worklist, innext) are
// appended to the window's slice.  Every loop is bounded here too: the peel by vertices + 1 rounds, a chain by the
// vertex count, an edge list by the edge count, the choice of a walk's next edge by the edge count, a walk by the
// vertex count.  A window whose peel does not resolve every vertex, whose walk runs out of its bound or finds no
// edge, or whose text passes its slice gets status "host" and is computed there: termination and every store's
// bound hold for a cyclic or inconsistent table as well.  No workgroup waits for another.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>

#include "debruijn_device.h"
#include "debruijn_paths.h"
#include "device_round_trip.h"

static_assert(sizeof(dv_debruijn_device_stats) == 48, "dv_debruijn_device_stats layout");
static_assert(sizeof(dv_debruijn_window) == 16, "dv_debruijn_window layout");
static_assert(sizeof(dv_debruijn_paths_stats) == 48, "dv_debruijn_paths_stats layout");

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kNone = 0xffffffffu;
constexpr unsigned long long kNoEdge = ~0ull;
constexpr uint64_t kBase = 0x9E3779B97F4A7C15ull;     // odd: the polynomial's base, modulo 2^64
constexpr uint64_t kMix = 0xD6E8FEB86659FD93ull;
constexpr uint32_t kRefBit = 0x80000000u;             // of an edge's weight word

struct Item {              // one window of the launch
  int64_t bytes_off;       // its bytes in the base and quality tables, the reference first
  int64_t scratch_off;     // its slice of the scratch buffer
  int64_t vout_off, eout_off;   // its vertices / edges in the output pools, in elements
  int32_t seq_table;       // its first entry in the offset and mapq tables
  int32_t n_seqs;          // 1 + reads
  int32_t n_bytes, ref_len;
  int32_t vcap, ecap;      // table sizes, powers of two
  int32_t vmax, emax;      // room in the output pools
};

struct Header {            // what a window's workgroup reports
  int32_t k, n_vertices, n_edges, k_tries, overflow, reserved;
  uint64_t kmers;
};

struct Params {
  int min_k, max_k, step_k, min_mapq, min_base_quality, max_vertices, max_edges;
};

// a window's slice: P | ekey | nb | sid | slot_of | vkey | indeg | head | work | ew | eocc | enext, and for the paths
// kernel behind them: cnt | pending | inhead | pwork | innext
size_t slice_bytes(size_t n, size_t vcap, size_t ecap, bool paths = false) {
  return dv::align16(8 * (n + 1) + 8 * ecap + 4 * (3 * n + 4 * vcap + 3 * ecap) + (paths ? 4 * (4 * vcap + ecap) : 0));
}

__device__ inline uint32_t ld(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline unsigned long long ld(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline bool same_bytes(const uint8_t* a, const uint8_t* b, int k) {
  for (int j = 0; j < k; ++j) {
    if (a[j] != b[j]) return false;
  }
  return true;
}

// the value every thread of the workgroup agrees on, safe to overwrite afterwards
__device__ inline uint32_t agreed(const uint32_t* shared) {
  __syncthreads();
  const uint32_t v = *reinterpret_cast<const volatile uint32_t*>(shared);
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(kThreads) void debruijn_kernel(const uint8_t* __restrict__ bases,
                                                            const uint8_t* __restrict__ quals,
                                                            const int32_t* __restrict__ seq_off,
                                                            const uint8_t* __restrict__ mapq,
                                                            const Item* __restrict__ items, const Params prm,
                                                            uint8_t* __restrict__ scratch, uint32_t* __restrict__ vpool,
                                                            uint4* __restrict__ epool, Header* __restrict__ headers) {
  __shared__ uint64_t s_hash[kThreads], s_pow[kThreads];
  __shared__ uint32_t s_nv, s_ne, s_dup, s_overflow, s_wcount, s_removed, s_vout, s_eout;
  __shared__ unsigned long long s_kmers;
  const Item it = items[blockIdx.x];
  const int tid = threadIdx.x;
  const int N = it.n_bytes, R = it.ref_len;
  const uint32_t vcap = static_cast<uint32_t>(it.vcap), ecap = static_cast<uint32_t>(it.ecap);
  const uint32_t vmask = vcap - 1, emask = ecap - 1;
  const uint8_t* seq = bases + it.bytes_off;
  const uint8_t* ql = quals + it.bytes_off;
  const int32_t* off = seq_off + it.seq_table;
  const uint8_t* mq = mapq + it.seq_table;
  uint8_t* sp = scratch + it.scratch_off;
  uint64_t* P = reinterpret_cast<uint64_t*>(sp);
  sp += 8 * (static_cast<size_t>(N) + 1);
  unsigned long long* ekey = reinterpret_cast<unsigned long long*>(sp);
  sp += 8 * static_cast<size_t>(ecap);
  uint32_t* nb = reinterpret_cast<uint32_t*>(sp);
  uint32_t* sid = nb + N;
  uint32_t* slot_of = sid + N;
  uint32_t* vkey = slot_of + N;
  uint32_t* indeg = vkey + vcap;
  uint32_t* head = indeg + vcap;
  uint32_t* work = head + vcap;
  uint32_t* ew = work + vcap;
  uint32_t* eocc = ew + ecap;
  uint32_t* enext = eocc + ecap;

  if (tid == 0) {
    s_nv = s_ne = s_dup = s_overflow = s_wcount = s_removed = s_vout = s_eout = 0;
    s_kmers = 0;
  }
  // ---- once: prefix hashes.  P[g] is the hash of bytes [0, g); a k-mer's is P[g + k] - P[g] * base^k.
  {
    const int chunk = (N + kThreads - 1) / kThreads;
    const int lo = min(tid * chunk, N), hi = min(lo + chunk, N);
    uint64_t h = 0, pw = 1;
    for (int g = lo; g < hi; ++g) {
      h = h * kBase + (seq[g] + 1u);
      pw *= kBase;
    }
    s_hash[tid] = h;
    s_pow[tid] = pw;
    __syncthreads();
    if (tid == 0) {
      uint64_t carry = 0;
      for (int t = 0; t < kThreads; ++t) {
        const uint64_t own = s_hash[t];
        s_hash[t] = carry;
        carry = carry * s_pow[t] + own;
      }
    }
    __syncthreads();
    h = s_hash[tid];
    for (int g = lo; g < hi; ++g) {
      P[g] = h;
      h = h * kBase + (seq[g] + 1u);
    }
    if ((hi == N && lo < N) || (N == 0 && tid == 0)) P[N] = h;
  }
  // ---- once: per read position the next bad position (the read's end if none) and the read's number (kNone for a
  // read below min_mapq), as offsets into the window's bytes
  for (int s = 1 + tid; s < it.n_seqs; s += kThreads) {
    const int r0 = off[s], r1 = off[s + 1];
    const uint32_t number = mq[s] >= prm.min_mapq ? static_cast<uint32_t>(s) : kNone;
    uint32_t next = static_cast<uint32_t>(r1);
    for (int g = r1 - 1; g >= r0; --g) {
      const uint8_t c = seq[g];
      const bool bad = !(c == 'A' || c == 'C' || c == 'G' || c == 'T') || ql[g] < prm.min_base_quality;
      if (bad) next = static_cast<uint32_t>(g);
      nb[g] = next;
      sid[g] = number;
    }
  }
  __syncthreads();

  auto insert_vertex = [&](uint32_t g, int k, uint64_t bk) -> uint32_t {
    const uint64_t h = P[g + k] - P[g] * bk;
    uint32_t idx = static_cast<uint32_t>((h * kMix) >> 32) & vmask;
    for (uint32_t probe = 0; probe <= vmask; ++probe) {
      const uint32_t cur = atomicCAS(&vkey[idx], kNone, g);
      if (cur == kNone) {
        atomicAdd(&s_nv, 1u);
        return idx;
      }
      if (cur == g) return idx;
      // the representative may be lowered meanwhile: to another occurrence of the same bytes
      if (P[cur + k] - P[cur] * bk == h && same_bytes(seq + cur, seq + g, k)) {
        atomicMin(&vkey[idx], g);
        s_dup = 1;
        return idx;
      }
      idx = (idx + 1) & vmask;
    }
    s_overflow = 1;
    return kNone;
  };
  auto insert_edge = [&](uint32_t from, uint32_t to, bool is_ref, uint32_t occ) {
    if (from == kNone || to == kNone) return;          // a vertex table overflow, already flagged
    const unsigned long long key = (static_cast<unsigned long long>(from) << 32) | to;
    uint32_t idx = static_cast<uint32_t>((key * kMix) >> 32) & emask;
    for (uint32_t probe = 0; probe <= emask; ++probe) {
      unsigned long long cur = atomicCAS(&ekey[idx], kNoEdge, key);
      if (cur == kNoEdge) {
        atomicAdd(&s_ne, 1u);
        enext[idx] = atomicExch(&head[from], idx);
        atomicAdd(&indeg[to], 1u);
        cur = key;
      }
      if (cur == key) {
        atomicAdd(&ew[idx], 1u);
        if (is_ref) atomicOr(&ew[idx], kRefBit);
        atomicMin(&eocc[idx], occ);
        return;
      }
      idx = (idx + 1) & emask;
    }
    s_overflow = 1;
  };

  const int max_k = min(prm.max_k, R - 1);
  int k_win = 0;
  uint32_t tries = 0, n_vertices = 0, n_edges = 0;
  unsigned long long hashed = 0;
  bool started = false, overflow = false;
  for (int k = prm.min_k; k <= max_k; k += prm.step_k) {
    ++tries;
    uint64_t bk = 1;
    for (int j = 0; j < k; ++j) bk *= kBase;
    // ---- the reference's vertices; until the start of the search is found this is the repeat test too
    for (uint32_t i = tid; i < vcap; i += kThreads) vkey[i] = kNone;
    if (tid == 0) s_nv = s_dup = 0;
    __syncthreads();
    for (int g = tid; g + k <= R; g += kThreads) {
      slot_of[g] = insert_vertex(static_cast<uint32_t>(g), k, bk);
      ++hashed;
    }
    overflow = agreed(&s_overflow) != 0;
    if (overflow) break;
    if (!started) {
      if (agreed(&s_dup) != 0) continue;
      started = true;
    }
    // ---- the reads' vertices
    for (uint32_t i = tid; i < vcap; i += kThreads) {
      indeg[i] = 0;
      head[i] = kNone;
    }
    for (uint32_t i = tid; i < ecap; i += kThreads) {
      ekey[i] = kNoEdge;
      ew[i] = 0;
      eocc[i] = kNone;
    }
    if (tid == 0) s_ne = s_wcount = s_removed = 0;
    for (int g = R + tid; g < N; g += kThreads) {
      const uint32_t s = sid[g];
      bool occurs = false;
      if (s != kNone) {
        const int r0 = off[s], r1 = off[s + 1];
        if (r1 - r0 > k) {
          const int bad = static_cast<int>(nb[g]);
          const bool is_start = g == r0 || nb[g - 1] == static_cast<uint32_t>(g - 1);
          occurs = is_start ? (g < r1 - k && bad - r0 > k) : g + k <= bad;
        }
      }
      uint32_t slot = kNone;
      if (occurs) {
        slot = insert_vertex(static_cast<uint32_t>(g), k, bk);
        ++hashed;
      }
      slot_of[g] = slot;
    }
    __syncthreads();
    // ---- edges: the reference's, then the reads'
    for (int g = 1 + tid; g + k <= R; g += kThreads) {
      insert_edge(slot_of[g - 1], slot_of[g], true, static_cast<uint32_t>(g - 1));
    }
    for (int g = R + tid; g < N; g += kThreads) {
      const uint32_t s = sid[g];
      if (s == kNone) continue;
      const int r0 = off[s], r1 = off[s + 1];
      if (r1 - r0 <= k || g == r0) continue;
      if (nb[g - 1] == static_cast<uint32_t>(g - 1)) continue;         // a segment's start has no predecessor
      if (g + k <= static_cast<int>(nb[g])) {
        insert_edge(slot_of[g - 1], slot_of[g], false, static_cast<uint32_t>(g - 1));
      }
    }
    n_vertices = agreed(&s_nv);
    n_edges = agreed(&s_ne);
    overflow = agreed(&s_overflow) != 0 || n_vertices > static_cast<uint32_t>(prm.max_vertices) ||
               n_edges > static_cast<uint32_t>(prm.max_edges);
    if (overflow) break;
    // ---- the cycle test: peel the vertices of in-degree 0
    for (uint32_t i = tid; i < vcap; i += kThreads) {
      if (ld(&vkey[i]) != kNone && ld(&indeg[i]) == 0) {
        const uint32_t w = atomicAdd(&s_wcount, 1u);
        if (w < vcap) work[w] = i;
      }
    }
    uint32_t begin = 0, removed = 0;
    for (uint32_t round = 0; round <= n_vertices; ++round) {
      const uint32_t end = min(agreed(&s_wcount), vcap);
      if (begin == end) break;
      for (uint32_t w = begin + tid; w < end; w += kThreads) {
        uint32_t v = work[w];
        for (uint32_t steps = 0; v != kNone && steps <= n_vertices; ++steps) {
          ++removed;
          uint32_t next = kNone;
          uint32_t e = ld(&head[v]);
          for (uint32_t seen = 0; e != kNone && seen <= n_edges; ++seen) {
            const uint32_t to = static_cast<uint32_t>(ld(&ekey[e]));
            if (atomicSub(&indeg[to], 1u) == 1u) {
              if (next == kNone) {
                next = to;
              } else {
                const uint32_t w2 = atomicAdd(&s_wcount, 1u);
                if (w2 < vcap) work[w2] = to;
              }
            }
            e = enext[e];
          }
          v = next;
        }
      }
      begin = end;
    }
    atomicAdd(&s_removed, removed);
    if (agreed(&s_removed) == n_vertices) {
      k_win = k;
      break;
    }
  }
  // ---- the winning k's graph: used slots as occurrence keys, in slot order (the host sorts)
  if (k_win != 0 && !overflow) {
    uint32_t* vout = vpool + it.vout_off;
    uint4* eout = epool + it.eout_off;
    for (uint32_t i = tid; i < vcap; i += kThreads) {
      const uint32_t key = ld(&vkey[i]);
      if (key == kNone) continue;
      const uint32_t o = atomicAdd(&s_vout, 1u);
      if (o < static_cast<uint32_t>(it.vmax)) vout[o] = key;
    }
    for (uint32_t i = tid; i < ecap; i += kThreads) {
      const unsigned long long key = ld(&ekey[i]);
      if (key == kNoEdge) continue;
      const uint32_t o = atomicAdd(&s_eout, 1u);
      if (o < static_cast<uint32_t>(it.emax)) {
        eout[o] = make_uint4(ld(&vkey[static_cast<uint32_t>(key >> 32)]), ld(&vkey[static_cast<uint32_t>(key)]),
                             ld(&ew[i]), ld(&eocc[i]));
      }
    }
  }
  atomicAdd(&s_kmers, hashed);
  __syncthreads();
  if (tid == 0) {
    Header h;
    h.k = overflow ? 0 : k_win;
    h.n_vertices = static_cast<int32_t>(s_vout);
    h.n_edges = static_cast<int32_t>(s_eout);
    h.k_tries = static_cast<int32_t>(tries);
    h.overflow = overflow ? 1 : 0;
    h.reserved = 0;
    h.kmers = s_kmers;
    headers[blockIdx.x] = h;
  }
}

// ---- pruning and path enumeration

constexpr int32_t kPathsHost = 3;          // a window's status on the device only: the host computes it

struct PathsHeader {       // what a window's workgroup reports
  int32_t status, k, n_paths, n_bytes;
};

struct PathsParams {
  int min_edge_weight, max_num_paths;
  int lens_per_window;     // entries of a window in the length pool: min(max_num_paths, kDebruijnMaxPaths)
  int max_hap_bytes;       // bytes of a window's haplotype slice
};

__device__ inline void st(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void debruijn_paths_kernel(const uint8_t* __restrict__ bases,
                                                                  const Item* __restrict__ items,
                                                                  const Header* __restrict__ headers,
                                                                  const PathsParams prm, uint8_t* __restrict__ scratch,
                                                                  uint32_t* __restrict__ lens_pool,
                                                                  uint8_t* __restrict__ text_pool,
                                                                  PathsHeader* __restrict__ out) {
  __shared__ uint32_t s_len[dv::kDebruijnMaxPaths], s_off[dv::kDebruijnMaxPaths], s_sum[kThreads];
  __shared__ uint32_t s_wcount, s_resolved, s_fail, s_total;
  const Item it = items[blockIdx.x];
  const Header hd = headers[blockIdx.x];
  const int tid = threadIdx.x;
  const int N = it.n_bytes, R = it.ref_len, k = hd.k;
  const uint32_t vcap = static_cast<uint32_t>(it.vcap), ecap = static_cast<uint32_t>(it.ecap);
  const uint32_t n_vertices = static_cast<uint32_t>(hd.n_vertices), n_edges = static_cast<uint32_t>(hd.n_edges);
  auto report = [&](int32_t status, uint32_t n_paths, uint32_t n_bytes) {
    if (tid == 0) {
      out[blockIdx.x] = PathsHeader{status, status == kPathsHost ? 0 : k, static_cast<int32_t>(n_paths),
                                    static_cast<int32_t>(n_bytes)};
    }
  };
  // the header is the same for every thread, so these returns are the whole workgroup's
  if (hd.overflow != 0) return report(kPathsHost, 0, 0);
  if (k == 0) return report(DV_DEBRUIJN_PATHS_NO_GRAPH, 0, 0);
  if (k < 0 || k >= R || n_vertices > vcap || n_edges > ecap) return report(kPathsHost, 0, 0);
  // the slice as debruijn_kernel laid it out, then the tables of this kernel
  const uint8_t* seq = bases + it.bytes_off;
  uint8_t* sp = scratch + it.scratch_off + 8 * (static_cast<size_t>(N) + 1);
  const unsigned long long* ekey = reinterpret_cast<const unsigned long long*>(sp);
  sp += 8 * static_cast<size_t>(ecap);
  const uint32_t* slot_of = reinterpret_cast<const uint32_t*>(sp) + 2 * static_cast<size_t>(N);
  const uint32_t* vkey = slot_of + N;
  const uint32_t* head = vkey + 2 * static_cast<size_t>(vcap);
  const uint32_t* ew = head + 2 * static_cast<size_t>(vcap);
  const uint32_t* enext = ew + 2 * static_cast<size_t>(ecap);
  uint32_t* cnt = const_cast<uint32_t*>(enext) + ecap;
  uint32_t* pending = cnt + vcap;
  uint32_t* inhead = pending + vcap;
  uint32_t* pwork = inhead + vcap;
  uint32_t* innext = pwork + vcap;

  const uint32_t cap = dv::paths::count_cap(prm.max_num_paths);
  const uint32_t source = slot_of[0], sink = slot_of[R - k];
  if (source >= vcap || sink >= vcap) return report(kPathsHost, 0, 0);
  auto alive = [&](uint32_t e) {
    const uint32_t w = ld(&ew[e]);
    return dv::paths::edge_alive(w & ~kRefBit, (w & kRefBit) != 0, prm.min_edge_weight);
  };
  for (uint32_t i = tid; i < vcap; i += kThreads) {
    cnt[i] = i == sink ? 1u : 0u;
    pending[i] = 0;
    inhead[i] = kNone;
  }
  if (tid == 0) s_wcount = s_resolved = s_fail = s_total = 0;
  __syncthreads();
  // ---- (a) alive edges: pending out-edges per vertex, in-edge lists per target
  for (uint32_t i = tid; i < ecap; i += kThreads) {
    const unsigned long long key = ld(&ekey[i]);
    if (key == kNoEdge) continue;
    const uint32_t from = static_cast<uint32_t>(key >> 32), to = static_cast<uint32_t>(key);
    if (from == sink || from >= vcap || to >= vcap || !alive(i)) continue;
    atomicAdd(&pending[from], 1u);
    innext[i] = atomicExch(&inhead[to], i);
  }
  __syncthreads();
  // ---- (b) cnt[] by a reverse peel from the vertices with nothing pending
  for (uint32_t i = tid; i < vcap; i += kThreads) {
    if (ld(&vkey[i]) != kNone && ld(&pending[i]) == 0) {
      const uint32_t w = atomicAdd(&s_wcount, 1u);
      if (w < vcap) pwork[w] = i;
    }
  }
  uint32_t begin = 0, resolved = 0;
  for (uint32_t round = 0; round <= n_vertices; ++round) {
    const uint32_t end = min(agreed(&s_wcount), vcap);
    if (begin == end) break;
    for (uint32_t w = begin + tid; w < end; w += kThreads) {
      uint32_t v = pwork[w];
      for (uint32_t steps = 0; v != kNone && steps <= n_vertices; ++steps) {
        ++resolved;
        uint32_t next = kNone;
        uint32_t e = ld(&inhead[v]);
        for (uint32_t seen = 0; e != kNone && e < ecap && seen <= n_edges; ++seen) {
          const uint32_t u = static_cast<uint32_t>(ld(&ekey[e]) >> 32);
          if (atomicSub(&pending[u], 1u) == 1u) {
            // every target of u is resolved, and its count stored before its resolver came here
            __threadfence();
            uint32_t sum = 0;
            uint32_t f = ld(&head[u]);
            for (uint32_t seen2 = 0; f != kNone && f < ecap && seen2 <= n_edges; ++seen2) {
              const uint32_t to = static_cast<uint32_t>(ld(&ekey[f]));
              if (to < vcap && alive(f)) sum = dv::paths::saturating_add(sum, ld(&cnt[to]), cap);
              f = ld(&enext[f]);
            }
            st(&cnt[u], sum);
            __threadfence();
            if (next == kNone) {
              next = u;
            } else {
              const uint32_t w2 = atomicAdd(&s_wcount, 1u);
              if (w2 < vcap) pwork[w2] = u;
            }
          }
          e = ld(&innext[e]);
        }
        v = next;
      }
    }
    begin = end;
  }
  atomicAdd(&s_resolved, resolved);
  if (agreed(&s_resolved) != n_vertices) return report(kPathsHost, 0, 0);
  // ---- (c) the number of walks
  const uint32_t T = ld(&cnt[source]);
  if (T >= cap) return report(DV_DEBRUIJN_PATHS_TOO_MANY, 0, 0);
  if (T == 0 || T > static_cast<uint32_t>(prm.lens_per_window) || T > static_cast<uint32_t>(dv::kDebruijnMaxPaths)) {
    return report(kPathsHost, 0, 0);
  }
  // ---- (d) walk number r, unranked: its length; with dst also its bytes, never past dst[limit).  0: no such walk.
  auto walk = [&](uint32_t r, uint8_t* dst, uint32_t limit) -> uint32_t {
    uint32_t v = source, len = static_cast<uint32_t>(k);
    if (dst) {
      if (len > limit) return 0;
      for (uint32_t j = 0; j < len; ++j) dst[j] = seq[j];
    }
    for (uint32_t steps = 0; v != sink; ++steps) {
      if (steps >= n_vertices) return 0;
      int after = dv::paths::kNoByte, byte = 0;
      uint32_t chosen = kNone;
      for (uint32_t rounds = 0; rounds <= n_edges; ++rounds) {
        int best = dv::paths::kPastBytes;
        uint32_t best_to = kNone;
        uint32_t e = ld(&head[v]);
        for (uint32_t seen = 0; e != kNone && e < ecap && seen <= n_edges; ++seen) {
          const uint32_t to = static_cast<uint32_t>(ld(&ekey[e]));
          if (to < vcap && alive(e)) {
            const uint32_t at = ld(&vkey[to]) + static_cast<uint32_t>(k) - 1u;
            const int b = at < static_cast<uint32_t>(N) ? seq[at] : 0;
            if (dv::paths::next_in_order(after, b, best)) {
              best = b;
              best_to = to;
            }
          }
          e = ld(&enext[e]);
        }
        if (best_to == kNone) break;                     // out of edges
        if (dv::paths::take_edge(&r, ld(&cnt[best_to]))) {
          chosen = best_to;
          byte = best;
          break;
        }
        after = best;
      }
      if (chosen == kNone) return 0;
      if (dst) {
        if (len >= limit) return 0;
        dst[len] = static_cast<uint8_t>(byte);
      }
      ++len;
      v = chosen;
    }
    return len;
  };
  for (uint32_t r = tid; r < T; r += kThreads) {
    const uint32_t len = walk(r, nullptr, 0);
    if (len == 0) s_fail = 1;
    s_len[r] = len;
  }
  __syncthreads();
  // offsets: a chunk of walk numbers per thread, the chunk sums scanned by one thread
  {
    const uint32_t chunk = (T + kThreads - 1) / kThreads;
    const uint32_t lo = min(tid * chunk, T), hi = min(lo + chunk, T);
    uint32_t sum = 0;
    for (uint32_t r = lo; r < hi; ++r) sum += s_len[r];    // <= 1024 walks of at most 8192 + k bytes each
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      uint32_t carry = 0;
      for (int t = 0; t < kThreads; ++t) {
        const uint32_t own = s_sum[t];
        s_sum[t] = carry;
        carry += own;
      }
      s_total = carry;
    }
    __syncthreads();
    uint32_t at = s_sum[tid];
    for (uint32_t r = lo; r < hi; ++r) {
      s_off[r] = at;
      at += s_len[r];
    }
  }
  if (agreed(&s_fail) != 0) return report(kPathsHost, 0, 0);
  const uint32_t total = agreed(&s_total);
  if (total > static_cast<uint32_t>(prm.max_hap_bytes)) return report(kPathsHost, 0, 0);
  uint8_t* text = text_pool + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(prm.max_hap_bytes);
  uint32_t* lens = lens_pool + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(prm.lens_per_window);
  for (uint32_t r = tid; r < T; r += kThreads) {
    const uint32_t len = s_len[r];
    if (walk(r, text + s_off[r], len) != len) s_fail = 1;
    lens[r] = len;
  }
  if (agreed(&s_fail) != 0) return report(kPathsHost, 0, 0);
  report(DV_DEBRUIJN_PATHS_OK, T, total);
}

uint32_t pow2_at_least(uint32_t x) {
  uint32_t p = 64;
  while (p < x) p <<= 1;
  return p;
}

// a window's device result as a CompactGraph: vertices and edges sorted by first occurrence and renumbered.  Nothing
// is indexed by a value the device returned without a check; what does not resolve becomes -1 and from_compact
// refuses it.
void to_compact(const dv::AssemblyWindow& w, const Header& h, const uint32_t* vkeys, const uint4* edges,
                dv::CompactGraph* out) {
  *out = dv::CompactGraph();
  out->k_tries = h.k_tries;
  out->k = h.k;
  if (h.k == 0) return;
  std::vector<uint32_t> start(1, 0);                     // sequence s is bytes [start[s], start[s + 1])
  start.push_back(static_cast<uint32_t>(w.ref.size()));
  for (const dv::AssemblyRead& r : w.reads) start.push_back(start.back() + static_cast<uint32_t>(r.bases.size()));
  auto occurrence = [&](uint32_t key, int32_t* seq, int32_t* pos) {
    if (key >= start.back()) {
      *seq = *pos = -1;
      return;
    }
    const size_t s = static_cast<size_t>(std::upper_bound(start.begin(), start.end(), key) - start.begin()) - 1;
    *seq = static_cast<int32_t>(s);
    *pos = static_cast<int32_t>(key - start[s]);
  };
  std::vector<uint32_t> keys(vkeys, vkeys + h.n_vertices);
  std::sort(keys.begin(), keys.end());
  out->vertex_seq.resize(keys.size());
  out->vertex_pos.resize(keys.size());
  for (size_t v = 0; v < keys.size(); ++v) occurrence(keys[v], &out->vertex_seq[v], &out->vertex_pos[v]);
  auto vertex = [&](uint32_t key) {
    const auto at = std::lower_bound(keys.begin(), keys.end(), key);
    return at != keys.end() && *at == key ? static_cast<int32_t>(at - keys.begin()) : -1;
  };
  std::vector<int32_t> order(static_cast<size_t>(h.n_edges));
  for (size_t e = 0; e < order.size(); ++e) order[e] = static_cast<int32_t>(e);
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return edges[a].w < edges[b].w; });
  const size_t ne = order.size();
  out->edge_from.resize(ne);
  out->edge_to.resize(ne);
  out->edge_weight.resize(ne);
  out->edge_is_ref.resize(ne);
  out->edge_seq.resize(ne);
  out->edge_pos.resize(ne);
  for (size_t e = 0; e < ne; ++e) {
    const uint4& d = edges[order[e]];
    out->edge_from[e] = vertex(d.x);
    out->edge_to[e] = vertex(d.y);
    out->edge_weight[e] = static_cast<int32_t>(d.z & ~kRefBit);
    out->edge_is_ref[e] = (d.z & kRefBit) ? 1 : 0;
    occurrence(d.w, &out->edge_seq[e], &out->edge_pos[e]);
  }
}

// The windows of a call as launch items.  A window over the limits known before the launch is left to the host.
struct Plan {
  std::vector<Item> items;
  std::vector<size_t> item_window;      // an item's window
  std::vector<size_t> order;            // the items in launch order: the heaviest first, early workgroups start first
  std::vector<size_t> on_host;          // the windows without an item
  int64_t n_bytes = 0, n_entries = 0, scratch_bytes = 0, vout = 0, eout = 0;
};

// pools: room for the winning graphs in the output pools; paths: the paths kernel's tables in every slice
Plan plan_windows(const std::vector<dv::AssemblyWindow>& windows, bool pools, bool paths) {
  constexpr int64_t kScratchBudget = int64_t{2} << 30;      // bytes of table scratch per call
  // the paths kernel's haplotype slices are downloaded whole: 1 GiB of them per call
  const size_t max_items = paths ? (size_t{1} << 30) / static_cast<size_t>(dv::kDebruijnMaxHapBytes) : windows.size();
  Plan p;
  for (size_t wi = 0; wi < windows.size(); ++wi) {
    const dv::AssemblyWindow& w = windows[wi];
    int64_t n = static_cast<int64_t>(w.ref.size());
    for (const dv::AssemblyRead& r : w.reads) n += static_cast<int64_t>(r.bases.size());
    if (n > dv::kDebruijnMaxBases || p.items.size() >= max_items) {
      p.on_host.push_back(wi);
      continue;
    }
    Item it;
    it.n_bytes = static_cast<int32_t>(n);
    it.ref_len = static_cast<int32_t>(w.ref.size());
    it.n_seqs = static_cast<int32_t>(w.reads.size()) + 1;
    it.vcap = static_cast<int32_t>(std::min(pow2_at_least(2u * dv::kDebruijnMaxVertices), pow2_at_least(it.n_bytes)));
    it.ecap = static_cast<int32_t>(std::min(pow2_at_least(2u * dv::kDebruijnMaxEdges), pow2_at_least(it.n_bytes)));
    it.vmax = pools ? std::min(dv::kDebruijnMaxVertices, it.n_bytes) : 0;
    it.emax = pools ? std::min(dv::kDebruijnMaxEdges, it.n_bytes) : 0;
    const int64_t slice = static_cast<int64_t>(slice_bytes(static_cast<size_t>(n), it.vcap, it.ecap, paths));
    if (p.scratch_bytes + slice > kScratchBudget || p.n_bytes + n >= (int64_t{1} << 30)) {
      p.on_host.push_back(wi);
      continue;
    }
    it.bytes_off = p.n_bytes;
    it.scratch_off = p.scratch_bytes;
    it.vout_off = p.vout;
    it.eout_off = p.eout;
    it.seq_table = static_cast<int32_t>(p.n_entries);
    p.items.push_back(it);
    p.item_window.push_back(wi);
    p.n_bytes += n;
    p.n_entries += it.n_seqs + 1;
    p.scratch_bytes += slice;
    p.vout += it.vmax;
    p.eout += it.emax;
  }
  p.order.resize(p.items.size());
  for (size_t x = 0; x < p.order.size(); ++x) p.order[x] = x;
  std::stable_sort(p.order.begin(), p.order.end(),
                   [&](size_t a, size_t b) { return p.items[a].n_bytes > p.items[b].n_bytes; });
  return p;
}

// the upload image of a plan: items | offsets | mapq | bases | quals
struct UploadImage {
  size_t items, off, mapq, bases, quals;
  explicit UploadImage(const Plan& p, dv::Layout* up)
      : items(up->add(p.items.size() * sizeof(Item))),
        off(up->add(static_cast<size_t>(p.n_entries) * sizeof(int32_t))),
        mapq(up->add(static_cast<size_t>(p.n_entries))),
        bases(up->add(static_cast<size_t>(p.n_bytes))),
        quals(up->add(static_cast<size_t>(p.n_bytes))) {}
};

void stage_windows(const std::vector<dv::AssemblyWindow>& windows, const Plan& p, const UploadImage& image,
                   const dv::RoundTrip& rt) {
  Item* up_items = rt.host_up<Item>(image.items);
  int32_t* up_off = rt.host_up<int32_t>(image.off);
  uint8_t* up_mapq = rt.host_up<uint8_t>(image.mapq);
  for (size_t x = 0; x < p.items.size(); ++x) {
    const Item& it = p.items[p.order[x]];
    up_items[x] = it;
    const dv::AssemblyWindow& w = windows[p.item_window[p.order[x]]];
    uint8_t* b = rt.host_up<uint8_t>(image.bases) + it.bytes_off;
    uint8_t* q = rt.host_up<uint8_t>(image.quals) + it.bytes_off;
    int32_t* offs = up_off + it.seq_table;
    uint8_t* mq = up_mapq + it.seq_table;
    std::memcpy(b, w.ref.data(), w.ref.size());
    std::memset(q, 0, w.ref.size());
    int32_t at = static_cast<int32_t>(w.ref.size());
    offs[0] = 0;
    offs[1] = at;
    mq[0] = 0;
    for (size_t r = 0; r < w.reads.size(); ++r) {
      const dv::AssemblyRead& read = w.reads[r];
      const size_t len = read.bases.size();
      for (size_t i = 0; i < len; ++i) {                 // the contract's upper-casing
        const char c = read.bases[i];
        b[at + i] = static_cast<uint8_t>(c >= 'a' && c <= 'z' ? c - 'a' + 'A' : c);
      }
      if (len) std::memcpy(q + at, read.quals, len);
      at += static_cast<int32_t>(len);
      offs[r + 2] = at;
      mq[r + 1] = static_cast<uint8_t>(std::min(std::max(read.mapq, 0), 255));
    }
    mq[w.reads.size() + 1] = 0;
  }
}

}  // namespace

namespace dv {

AssemblyStats& last_assembly_stats() {
  static thread_local AssemblyStats stats;
  return stats;
}

bool device_assembly_enabled() { return env_switch("DV_REALIGN_DEVICE_ASSEMBLY", false); }

void compact_on_host(const std::vector<AssemblyWindow>& windows, const DeBruijnOptions& options,
                     std::vector<CompactGraph>* out) {
  out->assign(windows.size(), CompactGraph());
  for (size_t w = 0; w < windows.size(); ++w) {
    DeBruijnGraph::build_compact(windows[w].ref, windows[w].reads, options, &(*out)[w]);
  }
}

int compact_on_device(const std::vector<AssemblyWindow>& windows, const DeBruijnOptions& options, void* stream_in,
                      std::vector<CompactGraph>* out, AssemblyStats* stats) {
  out->assign(windows.size(), CompactGraph());
  Plan plan = plan_windows(windows, /*pools=*/true, /*paths=*/false);
  if (stats) {
    stats->windows += static_cast<int64_t>(windows.size());
    stats->windows_on_host += static_cast<int64_t>(plan.on_host.size());
  }
  if (!plan.items.empty()) {
    const size_t n_items = plan.items.size();
    Layout up, down;
    const UploadImage image(plan, &up);
    // download image: headers | vertex keys | edges
    const size_t o_headers = down.add(n_items * sizeof(Header));
    const size_t o_vout = down.add(static_cast<size_t>(plan.vout) * sizeof(uint32_t));
    const size_t o_eout = down.add_last(static_cast<size_t>(plan.eout) * sizeof(uint4));
    static thread_local RoundTrip rt;     // its scratch: the windows' tables
    if (int rc = rt.begin("de Bruijn assembly: no HIP device (the device route has no CPU fallback)", stream_in,
                          up.bytes(), down.bytes(), static_cast<size_t>(plan.scratch_bytes))) {
      return rc;
    }
    stage_windows(windows, plan, image, rt);
    if (int rc = rt.upload(up.bytes())) return rc;
    {
      ProfileScope prof(kProfOther, rt.stream());
      const Params prm{options.min_k, options.max_k, options.step_k, options.min_mapq, options.min_base_quality,
                       kDebruijnMaxVertices, kDebruijnMaxEdges};
      hipLaunchKernelGGL(debruijn_kernel, dim3(static_cast<unsigned>(n_items)), dim3(kThreads), 0, rt.stream(),
                         rt.dev_up<const uint8_t>(image.bases), rt.dev_up<const uint8_t>(image.quals),
                         rt.dev_up<const int32_t>(image.off), rt.dev_up<const uint8_t>(image.mapq),
                         rt.dev_up<const Item>(image.items), prm, static_cast<uint8_t*>(rt.d_scratch.ptr),
                         rt.dev_down<uint32_t>(o_vout), rt.dev_down<uint4>(o_eout), rt.dev_down<Header>(o_headers));
      DV_HIP_CHECK(hipGetLastError());
    }
    if (int rc = rt.finish(down.bytes())) return rc;
    if (stats) stats->launches += 1;
    const Header* headers = rt.host_down<Header>(o_headers);
    const uint32_t* vkeys = rt.host_down<uint32_t>(o_vout);
    const uint4* edges = rt.host_down<uint4>(o_eout);
    for (size_t x = 0; x < n_items; ++x) {
      const Item& it = plan.items[plan.order[x]];
      const size_t wi = plan.item_window[plan.order[x]];
      const Header& h = headers[x];
      if (stats) stats->kmers += static_cast<int64_t>(h.kmers);
      if (h.overflow || h.n_vertices < 0 || h.n_vertices > it.vmax || h.n_edges < 0 || h.n_edges > it.emax) {
        plan.on_host.push_back(wi);
        if (stats) stats->windows_on_host += 1;
        continue;
      }
      if (stats) stats->k_tries += h.k_tries;
      to_compact(windows[wi], h, vkeys + it.vout_off, edges + it.eout_off, &(*out)[wi]);
    }
  }
  for (size_t wi : plan.on_host) {
    DeBruijnGraph::build_compact(windows[wi].ref, windows[wi].reads, options, &(*out)[wi]);
    if (stats) stats->k_tries += (*out)[wi].k_tries;
  }
  return DV_OK;
}

PathsStats& last_paths_stats() {
  static thread_local PathsStats stats;
  return stats;
}

bool device_paths_enabled() { return env_switch("DV_REALIGN_DEVICE_PATHS", false); }

void paths_of_window(const AssemblyWindow& window, const DeBruijnOptions& options, WindowPaths* out) {
  *out = WindowPaths();
  const std::unique_ptr<DeBruijnGraph> graph = DeBruijnGraph::build(window.ref, window.reads, options);
  if (!graph) return;
  out->k = graph->kmer_size();
  out->haplotypes = graph->candidate_haplotypes();
  out->status = out->haplotypes.empty() ? DV_DEBRUIJN_PATHS_TOO_MANY : DV_DEBRUIJN_PATHS_OK;
}

int paths_on_device(const std::vector<AssemblyWindow>& windows, const DeBruijnOptions& options, void* stream_in,
                    bool compute_on_host, std::vector<WindowPaths>* out, PathsStats* stats, AssemblyStats* assembly) {
  out->assign(windows.size(), WindowPaths());
  // what the kernel covers: the closed form needs pruning, and a window's lengths have kDebruijnMaxPaths places
  const bool covered = !options.disable_graph_pruning && options.max_num_paths <= kDebruijnMaxPaths;
  Plan plan;
  if (covered) {
    plan = plan_windows(windows, /*pools=*/false, /*paths=*/true);
  } else {
    for (size_t wi = 0; wi < windows.size(); ++wi) plan.on_host.push_back(wi);
  }
  if (stats) stats->windows += static_cast<int64_t>(windows.size());
  if (assembly) {
    assembly->windows += static_cast<int64_t>(windows.size());
    assembly->windows_on_host += static_cast<int64_t>(plan.on_host.size());
  }
  if (!plan.items.empty()) {
    const size_t n_items = plan.items.size();
    const size_t lens_per_window = static_cast<size_t>(std::max(1, std::min(options.max_num_paths, kDebruijnMaxPaths)));
    Layout up, down;
    const UploadImage image(plan, &up);
    // download image: the graph kernel's headers | this kernel's | haplotype lengths | haplotype text slices
    const size_t o_headers = down.add(n_items * sizeof(Header));
    const size_t o_paths = down.add(n_items * sizeof(PathsHeader));
    const size_t o_lens = down.add(n_items * lens_per_window * sizeof(uint32_t));
    const size_t o_text = down.add_last(n_items * static_cast<size_t>(kDebruijnMaxHapBytes));
    static thread_local RoundTrip rt;     // its scratch: the windows' tables, both kernels'
    if (int rc = rt.begin("de Bruijn paths: no HIP device (the device route has no CPU fallback)", stream_in, up.bytes(),
                          down.bytes(), static_cast<size_t>(plan.scratch_bytes))) {
      return rc;
    }
    stage_windows(windows, plan, image, rt);
    if (int rc = rt.upload(up.bytes())) return rc;
    {
      ProfileScope prof(kProfOther, rt.stream());
      const Params prm{options.min_k, options.max_k, options.step_k, options.min_mapq, options.min_base_quality,
                       kDebruijnMaxVertices, kDebruijnMaxEdges};
      // no room in the pools (vmax = emax = 0): the graph stays in the slices, the header still counts it
      hipLaunchKernelGGL(debruijn_kernel, dim3(static_cast<unsigned>(n_items)), dim3(kThreads), 0, rt.stream(),
                         rt.dev_up<const uint8_t>(image.bases), rt.dev_up<const uint8_t>(image.quals),
                         rt.dev_up<const int32_t>(image.off), rt.dev_up<const uint8_t>(image.mapq),
                         rt.dev_up<const Item>(image.items), prm, static_cast<uint8_t*>(rt.d_scratch.ptr),
                         rt.dev_down<uint32_t>(o_lens), rt.dev_down<uint4>(o_text), rt.dev_down<Header>(o_headers));
      DV_HIP_CHECK(hipGetLastError());
      const PathsParams pp{options.min_edge_weight, options.max_num_paths, static_cast<int>(lens_per_window),
                           kDebruijnMaxHapBytes};
      hipLaunchKernelGGL(debruijn_paths_kernel, dim3(static_cast<unsigned>(n_items)), dim3(kThreads), 0, rt.stream(),
                         rt.dev_up<const uint8_t>(image.bases), rt.dev_up<const Item>(image.items),
                         rt.dev_down<const Header>(o_headers), pp, static_cast<uint8_t*>(rt.d_scratch.ptr),
                         rt.dev_down<uint32_t>(o_lens), rt.dev_down<uint8_t>(o_text), rt.dev_down<PathsHeader>(o_paths));
      DV_HIP_CHECK(hipGetLastError());
    }
    if (int rc = rt.finish(down.bytes())) return rc;
    if (stats) {
      stats->launches += 2;
      stats->bytes_down += static_cast<int64_t>(down.bytes());
    }
    if (assembly) assembly->launches += 1;
    const Header* headers = rt.host_down<Header>(o_headers);
    const PathsHeader* paths = rt.host_down<PathsHeader>(o_paths);
    for (size_t x = 0; x < n_items; ++x) {
      const size_t wi = plan.item_window[plan.order[x]];
      const Header& h = headers[x];
      const PathsHeader& ph = paths[x];
      WindowPaths& w = (*out)[wi];
      if (assembly) assembly->kmers += static_cast<int64_t>(h.kmers);
      // nothing is sized or indexed by a value the device returned without a check
      bool ok = !h.overflow && ph.status >= DV_DEBRUIJN_PATHS_OK && ph.status <= DV_DEBRUIJN_PATHS_TOO_MANY && ph.k == h.k;
      if (ok && ph.status == DV_DEBRUIJN_PATHS_OK) {
        ok = ph.n_paths >= 1 && static_cast<size_t>(ph.n_paths) <= lens_per_window && ph.n_bytes >= 0 &&
             ph.n_bytes <= kDebruijnMaxHapBytes && ph.k > 0;
        const uint32_t* lens = rt.host_down<uint32_t>(o_lens) + x * lens_per_window;
        int64_t sum = 0;
        for (int32_t r = 0; ok && r < ph.n_paths; ++r) sum += lens[r];
        ok = ok && sum == ph.n_bytes;
        if (ok) {
          const char* text = rt.host_down<char>(o_text) + x * static_cast<size_t>(kDebruijnMaxHapBytes);
          w.haplotypes.reserve(static_cast<size_t>(ph.n_paths));
          for (int32_t r = 0; r < ph.n_paths; ++r) {
            w.haplotypes.emplace_back(text, lens[r]);
            text += lens[r];
          }
        }
      } else if (ok) {
        ok = (ph.status == DV_DEBRUIJN_PATHS_NO_GRAPH) == (ph.k == 0);
      }
      if (!ok) {
        w = WindowPaths();
        plan.on_host.push_back(wi);
        if (h.overflow && assembly) assembly->windows_on_host += 1;
        continue;
      }
      w.k = ph.k;
      w.status = ph.status;
      if (assembly) assembly->k_tries += h.k_tries;
      if (stats) {
        stats->paths += static_cast<int64_t>(w.haplotypes.size());
        stats->hap_bytes += ph.status == DV_DEBRUIJN_PATHS_OK ? ph.n_bytes : 0;
      }
    }
  }
  if (stats) stats->windows_on_host += static_cast<int64_t>(plan.on_host.size());
  for (size_t wi : plan.on_host) {
    if (compute_on_host) {
      paths_of_window(windows[wi], options, &(*out)[wi]);
    } else {
      (*out)[wi].on_host = true;
    }
  }
  return DV_OK;
}

}  // namespace dv

namespace {

struct Batch {            // a call's arguments as windows
  std::vector<dv::AssemblyWindow> windows;
  dv::DeBruijnOptions options;
};

dv::DeBruijnOptions options_of(const dv_debruijn_options& o) {
  dv::DeBruijnOptions opt;
  opt.min_k = o.min_k;
  opt.max_k = o.max_k;
  opt.step_k = o.step_k;
  opt.min_mapq = o.min_mapq;
  opt.min_base_quality = o.min_base_quality;
  opt.min_edge_weight = o.min_edge_weight;
  opt.max_num_paths = o.max_num_paths;
  opt.disable_graph_pruning = o.disable_graph_pruning != 0;
  return opt;
}

template <class Result, class Arrays>
int parse(const char* who, int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
          const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows, const dv_debruijn_options* o,
          Result** out, Arrays* arrays, Batch* b) {
  const std::string name(who);
  if (out) *out = nullptr;
  if (!out || !arrays || !o || n_seqs < 0 || n_windows < 0 || (n_seqs > 0 && (!seq_off || !mapq)) ||
      (n_windows > 0 && !windows)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer or negative count");
  }
  if (o->step_k <= 0 || o->min_k <= 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": min_k and step_k must be positive");
  }
  if (int rc = dv::check_sequence_table(name, n_seqs, seq_off)) return rc;
  if (n_seqs > 0 && seq_off[n_seqs] > seq_off[0] && (!bases || !quals)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null bases or qualities");
  }
  b->options = options_of(*o);
  auto view = [&](int32_t s) {
    return std::string_view(bases + seq_off[s], static_cast<size_t>(seq_off[s + 1] - seq_off[s]));
  };
  for (int32_t w = 0; w < n_windows; ++w) {
    const dv_debruijn_window& win = windows[w];
    if (win.reference < 0 || win.reference >= n_seqs || win.n_reads < 0 || win.first_read < 0 ||
        static_cast<int64_t>(win.first_read) + win.n_reads > n_seqs) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": a window's reference or read range is outside the table");
    }
    dv::AssemblyWindow aw;
    aw.ref = view(win.reference);
    for (int32_t r = 0; r < win.n_reads; ++r) {
      const int32_t s = win.first_read + r;
      aw.reads.push_back(dv::AssemblyRead{view(s), quals + seq_off[s], mapq[s]});
    }
    b->windows.push_back(std::move(aw));
  }
  return DV_OK;
}

}  // namespace

struct dv_debruijn_compact_result {
  std::vector<int32_t> k, k_tries;
  std::vector<int64_t> vertex_off, edge_off;
  std::vector<int32_t> vertex_seq, vertex_pos, edge_from, edge_to, edge_weight, edge_is_ref, edge_seq, edge_pos;
};

namespace {

void publish(const std::vector<dv::CompactGraph>& graphs, dv_debruijn_compact_result** out, dv_debruijn_compact* arrays) {
  auto res = std::make_unique<dv_debruijn_compact_result>();
  res->vertex_off.assign(1, 0);
  res->edge_off.assign(1, 0);
  auto append = [](std::vector<int32_t>* to, const std::vector<int32_t>& from) {
    to->insert(to->end(), from.begin(), from.end());
  };
  for (const dv::CompactGraph& g : graphs) {
    res->k.push_back(g.k);
    res->k_tries.push_back(g.k_tries);
    append(&res->vertex_seq, g.vertex_seq);
    append(&res->vertex_pos, g.vertex_pos);
    append(&res->edge_from, g.edge_from);
    append(&res->edge_to, g.edge_to);
    append(&res->edge_weight, g.edge_weight);
    append(&res->edge_is_ref, g.edge_is_ref);
    append(&res->edge_seq, g.edge_seq);
    append(&res->edge_pos, g.edge_pos);
    res->vertex_off.push_back(static_cast<int64_t>(res->vertex_seq.size()));
    res->edge_off.push_back(static_cast<int64_t>(res->edge_from.size()));
  }
  arrays->k = res->k.data();
  arrays->k_tries = res->k_tries.data();
  arrays->vertex_off = res->vertex_off.data();
  arrays->vertex_seq = res->vertex_seq.data();
  arrays->vertex_pos = res->vertex_pos.data();
  arrays->edge_off = res->edge_off.data();
  arrays->edge_from = res->edge_from.data();
  arrays->edge_to = res->edge_to.data();
  arrays->edge_weight = res->edge_weight.data();
  arrays->edge_is_ref = res->edge_is_ref.data();
  arrays->edge_seq = res->edge_seq.data();
  arrays->edge_pos = res->edge_pos.data();
  *out = res.release();
}

}  // namespace

struct dv_debruijn_paths_result {
  std::vector<int32_t> k, status, hap_first;
  std::vector<int64_t> hap_off;
  std::string hap_text;
};

namespace {

void publish_paths(const std::vector<dv::WindowPaths>& paths, dv_debruijn_paths_result** out, dv_debruijn_paths* arrays) {
  auto res = std::make_unique<dv_debruijn_paths_result>();
  res->hap_first.assign(1, 0);
  res->hap_off.assign(1, 0);
  for (const dv::WindowPaths& w : paths) {
    res->k.push_back(w.k);
    res->status.push_back(w.status);
    for (const std::string& h : w.haplotypes) {
      res->hap_text += h;
      res->hap_off.push_back(static_cast<int64_t>(res->hap_text.size()));
    }
    res->hap_first.push_back(static_cast<int32_t>(res->hap_off.size() - 1));
  }
  arrays->k = res->k.data();
  arrays->status = res->status.data();
  arrays->hap_first = res->hap_first.data();
  arrays->hap_off = res->hap_off.data();
  arrays->hap_text = res->hap_text.data();
  *out = res.release();
}

}  // namespace

extern "C" {

int dv_debruijn_compact_batch(int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
                              const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows,
                              const dv_debruijn_options* options, dv_debruijn_compact_result** out,
                              dv_debruijn_compact* arrays) {
  return dv::guarded("dv_debruijn_compact_batch", [&]() -> int {
    Batch b;
    if (int rc = parse("dv_debruijn_compact_batch", n_seqs, bases, quals, seq_off, mapq, n_windows, windows, options,
                       out, arrays, &b)) {
      return rc;
    }
    std::vector<dv::CompactGraph> graphs;
    dv::compact_on_host(b.windows, b.options, &graphs);
    publish(graphs, out, arrays);
    return DV_OK;
  });
}

int dv_debruijn_compact_batch_device(int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
                                     const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows,
                                     const dv_debruijn_options* options, void* stream,
                                     dv_debruijn_compact_result** out, dv_debruijn_compact* arrays) {
  return dv::guarded("dv_debruijn_compact_batch_device", [&]() -> int {
    dv::last_assembly_stats() = dv::AssemblyStats();
    Batch b;
    if (int rc = parse("dv_debruijn_compact_batch_device", n_seqs, bases, quals, seq_off, mapq, n_windows, windows,
                       options, out, arrays, &b)) {
      return rc;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
      return dv::fail(DV_ERR_NO_DEVICE,
                      "dv_debruijn_compact_batch_device: no HIP device (dv_debruijn_compact_batch is the host code)");
    }
    std::vector<dv::CompactGraph> graphs;
    if (int rc = dv::compact_on_device(b.windows, b.options, stream, &graphs, &dv::last_assembly_stats())) return rc;
    publish(graphs, out, arrays);
    return DV_OK;
  });
}

void dv_debruijn_compact_free(dv_debruijn_compact_result* r) { delete r; }

int dv_debruijn_paths_batch(int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
                            const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows,
                            const dv_debruijn_options* options, dv_debruijn_paths_result** out,
                            dv_debruijn_paths* arrays) {
  return dv::guarded("dv_debruijn_paths_batch", [&]() -> int {
    Batch b;
    if (int rc = parse("dv_debruijn_paths_batch", n_seqs, bases, quals, seq_off, mapq, n_windows, windows, options, out,
                       arrays, &b)) {
      return rc;
    }
    std::vector<dv::WindowPaths> paths(b.windows.size());
    for (size_t w = 0; w < paths.size(); ++w) dv::paths_of_window(b.windows[w], b.options, &paths[w]);
    publish_paths(paths, out, arrays);
    return DV_OK;
  });
}

int dv_debruijn_paths_batch_device(int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
                                   const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows,
                                   const dv_debruijn_options* options, void* stream, dv_debruijn_paths_result** out,
                                   dv_debruijn_paths* arrays) {
  return dv::guarded("dv_debruijn_paths_batch_device", [&]() -> int {
    dv::last_paths_stats() = dv::PathsStats();
    Batch b;
    if (int rc = parse("dv_debruijn_paths_batch_device", n_seqs, bases, quals, seq_off, mapq, n_windows, windows,
                       options, out, arrays, &b)) {
      return rc;
    }
    // no look for a device here: a call without device work (no windows, or none the kernel covers) needs none, and
    // the round trip reports DV_ERR_NO_DEVICE when there is some
    std::vector<dv::WindowPaths> paths;
    if (int rc = dv::paths_on_device(b.windows, b.options, stream, /*compute_on_host=*/true, &paths,
                                     &dv::last_paths_stats(), nullptr)) {
      return rc;
    }
    publish_paths(paths, out, arrays);
    return DV_OK;
  });
}

void dv_debruijn_paths_free(dv_debruijn_paths_result* r) { delete r; }

int dv_debruijn_paths_last_stats(dv_debruijn_paths_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_debruijn_paths_last_stats: null");
  const dv::PathsStats& s = dv::last_paths_stats();
  out->windows = s.windows;
  out->windows_on_host = s.windows_on_host;
  out->paths = s.paths;
  out->hap_bytes = s.hap_bytes;
  out->launches = s.launches;
  out->bytes_down = s.bytes_down;
  return DV_OK;
}

int dv_debruijn_device_last_stats(dv_debruijn_device_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_debruijn_device_last_stats: null");
  const dv::AssemblyStats& s = dv::last_assembly_stats();
  out->windows = s.windows;
  out->windows_on_host = s.windows_on_host;
  out->kmers = s.kmers;
  out->k_tries = s.k_tries;
  out->launches = s.launches;
  out->windows_rejected = s.windows_rejected;
  return DV_OK;
}

}  // extern "C"
