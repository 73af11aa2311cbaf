// cand_slices.h -- how the candidate kernels slice a region's scratch (dv::cand_scratch_ints), for the device code
// of candidates.hip and of the passes that read what its link, resolve and group kernels leave there.
#ifndef DV_CAND_SLICES_H_
#define DV_CAND_SLICES_H_

#include "candidates.h"

namespace dv {

struct CandSlices {
  int32_t *head, *alt, *nsel;                    // per position
  int32_t *next, *stands, *rep, *count, *sel;    // per event
};
__device__ __forceinline__ CandSlices cand_slices(const CandRegion& g) {
  const size_t len = static_cast<size_t>(g.len), cap = g.event_cap;
  CandSlices s;
  s.head = g.scratch;
  s.alt = s.head + len;
  s.nsel = s.alt + len;
  s.next = s.nsel + len;
  s.stands = s.next + cap;
  s.rep = s.stands + cap;
  s.count = s.rep + cap;
  s.sel = s.count + cap;
  return s;
}

}  // namespace dv

#endif  // DV_CAND_SLICES_H_
