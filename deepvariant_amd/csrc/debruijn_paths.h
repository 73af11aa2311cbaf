// The rule behind DeBruijnGraph::prune + candidate_haplotypes (debruijn_graph.cpp) as a closed form, in the serial
// pieces the paths kernel of debruijn.hip and the host check (tools/debruijn_paths_check.cpp) both compile.  It holds
// with pruning on (disable_graph_pruning false) and for an acyclic graph:
//   an edge is alive iff is_ref or weight >= min_edge_weight; the sink's out-edges do not count (a walk ends there);
//   cnt[v] = the number of walks over alive edges from v to the sink (the vertex of the reference's last k-mer),
//            cnt[sink] = 1, saturating at max_num_paths + 1;
//   T = cnt[source] (the vertex of the reference's first k-mer); candidate_haplotypes() is empty iff T > max_num_paths;
//   otherwise it is the T walks, each spelled ref[0, k) + the last byte of every following vertex's k-mer, in
//   lexicographic order: the order of the walk numbers when every vertex's out-edges are taken in ascending unsigned
//   order of that byte (two out-edges of a vertex lead to k-mers that share k - 1 bytes, so their bytes differ);
//   walk r is found by unranking: at a vertex go through the out-edges in that order and take the first whose
//   cnt[to] > r, after subtracting from r the counts of those passed over.
#ifndef DV_DEBRUIJN_PATHS_H_
#define DV_DEBRUIJN_PATHS_H_

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DV_PATHS_HD __host__ __device__ __forceinline__
#else
#define DV_PATHS_HD inline
#endif

namespace dv {
namespace paths {

constexpr int kNoByte = -1;       // "before every byte"
constexpr int kPastBytes = 256;   // "after every byte"

// where the counts saturate: one past the largest T that is still reported
DV_PATHS_HD uint32_t count_cap(int max_num_paths) {
  return static_cast<uint32_t>(max_num_paths < 0 ? 0 : max_num_paths) + 1u;
}

// prune()'s first loop; weight without the is_ref mark
DV_PATHS_HD bool edge_alive(uint32_t weight, bool is_ref, int min_edge_weight) {
  return is_ref || static_cast<int64_t>(weight) >= static_cast<int64_t>(min_edge_weight);
}

// a + b, at most cap: the sum is formed in 64 bits, so it cannot wrap whatever a and b are
DV_PATHS_HD uint32_t saturating_add(uint32_t a, uint32_t b, uint32_t cap) {
  const uint64_t sum = static_cast<uint64_t>(a) + static_cast<uint64_t>(b);
  return sum > cap ? cap : static_cast<uint32_t>(sum);
}

// The order of a vertex's out-edges, without a sort: with `after` the byte of the edge handled last (kNoByte at the
// start) and `best` the smallest candidate seen so far in this scan of the list (kPastBytes at its start), an edge
// whose appended byte is `byte` is the better candidate iff this holds.  A scan that ends with best == kPastBytes
// has run out of edges.
DV_PATHS_HD bool next_in_order(int after, int byte, int best) { return byte > after && byte < best; }

// One unranking step at an edge whose target has `count` walks to the sink: true = the walk numbered *r among those
// not passed over yet goes through this edge; false = it does not, and *r now numbers it among the rest.
DV_PATHS_HD bool take_edge(uint32_t* r, uint32_t count) {
  if (count > *r) return true;
  *r -= count;
  return false;
}

}  // namespace paths
}  // namespace dv

#endif  // DV_DEBRUIJN_PATHS_H_
