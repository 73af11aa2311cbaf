// The merge of one contig's gVCF reference blocks with its variant records, written once and
// compiled for both sides: dv_gvcf_merge walks the blocks with it on the host, the kernels of gvcf_merge.hip give
// every block and every variant a lane.  Integer comparisons only, so both sides agree exactly.
//
// Per group (contig): blocks [s, e) sorted and disjoint, variants [s, e) sorted by (start, end), cm[j] the running
// maximum of the variants' ends within the group.  A block loses what the variants cover; what is left of it are its
// pieces.  With the pieces in block order and the variants in theirs, piece k and variant j are ordered by
// "variant first iff start[j] < piece_end[k]", which gives both their slots in the merged sequence by bisection.
#ifndef DV_GVCF_MERGE_H_
#define DV_GVCF_MERGE_H_

#include <cstdint>

#if defined(__HIPCC__)
#define DV_GM_HD __host__ __device__ inline
#else
#define DV_GM_HD inline
#endif

namespace dv {
namespace gm {

// The first i in [lo, hi) with a[i] >= x (a ascending over the range); hi when there is none.
DV_GM_HD int64_t first_at_least(const int64_t* a, int64_t lo, int64_t hi, int64_t x) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a[mid] < x) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// The first i in [lo, hi) with a[i] > x.
DV_GM_HD int64_t first_above(const int64_t* a, int64_t lo, int64_t hi, int64_t x) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a[mid] <= x) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// The group of element i: the last g in [0, n_groups) with off[g] <= i (groups may be empty; off ascends to > i).
DV_GM_HD int32_t group_of(const int64_t* off, int32_t n_groups, int64_t i) {
  return static_cast<int32_t>(first_above(off, 0, n_groups, i)) - 1;
}

// The pieces of the block [s, e) among the variants [lo, hi) of its group, in order: emit(k, piece_start, piece_end)
// for k = 0, 1, ...  -> their number.  lo: the group's first variant with cm > s; hi: its first with start >= e.
template <class Emit>
DV_GM_HD int32_t walk_range(int64_t s, int64_t e, const int64_t* var_start, const int64_t* var_end, int64_t lo,
                            int64_t hi, Emit&& emit) {
  int64_t cursor = s;
  int32_t n = 0;
  for (int64_t j = lo; j < hi && cursor < e; ++j) {
    if (cursor < var_start[j]) {
      emit(n, cursor, var_start[j]);
      ++n;
    }
    if (var_end[j] > cursor) cursor = var_end[j];
  }
  if (cursor < e) {
    emit(n, cursor, e);
    ++n;
  }
  return n;
}

// The same with [lo, hi) found by bisection among the group's variants [v0, v1): what a lane does for its block.
// (The host code walks the blocks in order and moves lo and hi forward instead.)
template <class Emit>
DV_GM_HD int32_t walk_block(int64_t s, int64_t e, const int64_t* var_start, const int64_t* var_end, const int64_t* cm,
                            int64_t v0, int64_t v1, Emit&& emit) {
  return walk_range(s, e, var_start, var_end, first_above(cm, v0, v1, s), first_at_least(var_start, v0, v1, e), emit);
}

// Piece k (its index in the whole call) of a group whose variants are [v0, v1): k + the index of the group's first
// variant that does not start below the piece's end -- the variants of earlier groups all come before it.
DV_GM_HD int64_t piece_slot(int64_t k, int64_t piece_end, const int64_t* var_start, int64_t v0, int64_t v1) {
  return k + first_at_least(var_start, v0, v1, piece_end);
}

// Variant j (its index in the whole call) of a group whose pieces are [p0, p1): j + the index of the group's first
// piece that ends above the variant's start.
DV_GM_HD int64_t var_slot(int64_t j, int64_t start, const int64_t* piece_end, int64_t p0, int64_t p1) {
  return j + first_above(piece_end, p0, p1, start);
}

}  // namespace gm
}  // namespace dv

#endif  // DV_GVCF_MERGE_H_
