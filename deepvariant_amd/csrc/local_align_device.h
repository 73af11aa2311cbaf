// The two sweeps of the local aligner (local_align.h: LocalAligner::sweep forward, then the
// reverse sweep of LocalAligner::finish) for a list of (reference, query) pairs in one kernel
// launch, and in the same launch the banded trace-back between the corner points it found.  The
// corner points, and the M/I/D runs of the pairs the kernel traced back, return to the host, where
// complete_on_device_route() writes the text form.  Kernel and runtime: local_align.hip.
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

// The trace-back of a call.  Pair k's runs, where traced[k], are words[first[k] .. first[k] + count[k]) in
// alignment order: (length << 2) | 0 M / 1 I / 2 D; band[k] is the band banded_cigar would have ended with.
// A pair with traced[k] == 0 holds no runs at all (band past DV_LOCAL_ALIGN_DEVICE_MAX_BAND, more than
// DV_LOCAL_ALIGN_DEVICE_MAX_RUNS runs, scratch budget used up, or nothing to trace).
struct DeviceRuns {
  std::vector<uint8_t> traced;
  std::vector<int32_t> band, first, count;
  std::vector<uint32_t> words;
};

struct TracebackStats {   // dv_realign_traceback_stats
  int64_t traced_on_device = 0, traced_on_host = 0, band_cells = 0, widest_band = 0;
};
// of the calling thread's last sweep_pairs_on_device; the C entry points reset it before they check anything
TracebackStats& last_traceback_stats();

// DV_REALIGN_DEVICE_TRACEBACK, read now; unset: kTracebackByDefault
constexpr bool kTracebackByDefault = false;
bool device_traceback_enabled();

inline bool device_align_fits(size_t ref_len, size_t query_len) {
  return query_len <= static_cast<size_t>(kDeviceAlignMaxQuery) &&
         ref_len <= static_cast<size_t>(kDeviceAlignMaxReference);
}

// A sweep call's buffers as it left them on the device, for a caller that goes on working there (realign_finish.hip):
// the pairs' words stay in the calling thread's download buffer, its items, sequence offsets and codes in its upload
// buffer.  Valid until the calling thread's next sweep_pairs_on_device.
struct ResidentSweep {
  const int32_t* d_out = nullptr;      // out_words per item: 6 corner values, traced, runs | band << 16, the runs
  int32_t out_words = 0, n_items = 0;
  const void* d_items = nullptr;       // {ref slot, query slot, rows, pair, area} per item
  const int32_t* d_seq_off = nullptr;  // [slots + 1] into d_codes
  const uint8_t* d_codes = nullptr;
  void* stream = nullptr;              // the stream the sweep ran on
  std::vector<int32_t> item_of_pair;   // -1: the pair was not swept on the device
  std::vector<uint8_t> traced;         // per pair: the kernel traced it back; its runs are in d_out
  int64_t bytes_down = 0;              // what the call downloaded
};

// Sweeps pair k = (*sequences[pair_ref[k]], *sequences[pair_query[k]]) for every pair inside the
// limits: one upload, one launch, one download on `stream` (null: a non-blocking stream the
// library owns), then waits for it.  Indices must be valid.  route[k] says what became of pair k;
// stats (may be null) is added to.  Buffers are the calling thread's and are reused.
// `traced` (may be null: no trace-back) receives the runs of the pairs the kernel traced back, when
// device_traceback_enabled(); last_traceback_stats() says how the pairs holding an alignment were split.
// `keep` (may be null: exactly the call above): the trace-back runs whatever the switch says, the result buffer stays
// on the device and *keep says where; of each pair only the corners, the traced flag, the run count and the band are
// downloaded (8 words instead of 8 + DV_LOCAL_ALIGN_DEVICE_MAX_RUNS), and `traced` receives no runs: a pair the
// caller finishes on the host goes through LocalAligner::complete.
// Returns a dv_status; DV_ERR_NO_DEVICE without a GPU (only when there is device work).
int sweep_pairs_on_device(const std::vector<const CodedSequence*>& sequences, const std::vector<int32_t>& pair_ref,
                          const std::vector<int32_t>& pair_query, int match, int mismatch, int gap_open,
                          int gap_extend, void* stream, std::vector<SweepCorners>* corners,
                          std::vector<uint8_t>* route, DeviceAlignStats* stats, DeviceRuns* traced,
                          ResidentSweep* keep = nullptr);

// LocalAligner::complete for pair k of a device call: the text form around the device's runs where the
// kernel traced the pair back, complete() itself otherwise.  Returns what complete() returns.
bool complete_on_device_route(const LocalAligner& aligner, const CodedSequence& ref, const CodedSequence& q,
                              const SweepCorners& corners, const DeviceRuns* traced, size_t k, LocalAlignment* out);

}  // namespace dv

#endif  // DV_LOCAL_ALIGN_DEVICE_H_
