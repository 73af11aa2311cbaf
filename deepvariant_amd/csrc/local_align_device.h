// The two sweeps of the local aligner (local_align.h: LocalAligner::sweep forward, then the
// reverse sweep of LocalAligner::finish) for a list of (reference, query) pairs in one kernel
// launch.  CIGARs stay on the host: the corner points returned here go to
// LocalAligner::complete.  Kernel and runtime: local_align.hip.
#ifndef DV_LOCAL_ALIGN_DEVICE_H_
#define DV_LOCAL_ALIGN_DEVICE_H_

#include <cstdint>
#include <vector>

#include "dvhip.h"
#include "local_align.h"

namespace dv {

// A pair is swept on the device when its query has at most this many bases (64 lanes x the
// widest rows-per-lane bucket, all held in registers) and its reference at most that many
// (the 16-bit read offsets of the realigner).  Any other pair is the caller's to align on the host.
constexpr int kDeviceAlignMaxQuery = DV_LOCAL_ALIGN_DEVICE_MAX_QUERY;
constexpr int kDeviceAlignMaxReference = DV_LOCAL_ALIGN_DEVICE_MAX_REFERENCE;
// scoring values the kernel's packed (score, row) keys have room for; LocalAligner's own score
// matrix is int8_t, so larger ones have no host meaning either
constexpr int kDeviceAlignMaxScoringValue = 127;

enum DeviceAlignRoute : uint8_t {
  kRouteDevice = 0,   // corners[k] holds the device's result
  kRouteHost = 1,     // outside the kernel's limits: not swept
  kRouteEmpty = 2     // an empty sequence: align() fails
};

struct DeviceAlignStats {
  int64_t pairs = 0, pairs_on_host = 0, cells = 0, launches = 0;
};

inline bool device_align_fits(size_t ref_len, size_t query_len) {
  return query_len <= static_cast<size_t>(kDeviceAlignMaxQuery) &&
         ref_len <= static_cast<size_t>(kDeviceAlignMaxReference);
}

// Sweeps pair k = (*sequences[pair_ref[k]], *sequences[pair_query[k]]) for every pair inside the
// limits: one upload, one launch, one download on `stream` (null: a non-blocking stream the
// library owns), then waits for it.  Indices must be valid.  route[k] says what became of pair k;
// stats (may be null) is added to.  Buffers are the calling thread's and are reused.
// Returns a dv_status; DV_ERR_NO_DEVICE without a GPU (only when there is device work).
int sweep_pairs_on_device(const std::vector<const CodedSequence*>& sequences, const std::vector<int32_t>& pair_ref,
                          const std::vector<int32_t>& pair_query, int match, int mismatch, int gap_open,
                          int gap_extend, void* stream, std::vector<SweepCorners>* corners,
                          std::vector<uint8_t>* route, DeviceAlignStats* stats);

}  // namespace dv

#endif  // DV_LOCAL_ALIGN_DEVICE_H_
