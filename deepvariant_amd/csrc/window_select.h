// window_select.h -- the realigner's window selection behind the allele counter: what allele_counter.hip hands
// to the kernels of window_select.hip.
#ifndef DV_WINDOW_SELECT_H_
#define DV_WINDOW_SELECT_H_

#include "candidates.h"

struct dv_windows {
  std::vector<int64_t> starts, ends;
  std::vector<uint32_t> mask;      // want_debug: one bit per position of the interval
  std::vector<uint32_t> scores;    // want_debug: float32 scores (linear model) or int32 counts, per position
};

namespace dv {

// One counter interval as the window kernels see it, beside the CandRegion of the same slot: the grouping kernels
// of candidates.hip leave the standing flags and allele groups in that region's scratch, and these kernels read
// them there.
struct WindowRegion {
  int64_t interval_start;
  int32_t* scratch;                // win_scratch_ints(len, event_cap) ints, zeroed before the launch
  int64_t* windows;                // [win_cap(len, d)][2] start, end in contig coordinates
  int32_t* n_windows;              // device word: windows written
  uint32_t* mask;                  // [mask words of len] candidate bits; null without want_debug
  uint32_t* scores;                // [len]; null without want_debug
};

// Scratch of one region: standing events and their first list slot [len] each; the first event of each event's key
// (read, read_offset) and the four fields of the ordered records [event_cap] each; the number of records.
inline size_t win_scratch_ints(int64_t len, uint32_t event_cap) {
  return 2 * static_cast<size_t>(len) + 6 * static_cast<size_t>(event_cap) + 4;
}

// Windows start more than 2d apart, so at most ceil(len / (2d + 1)) fit.
inline size_t win_cap(int64_t len, int32_t min_windows_distance) {
  const int64_t step = 2 * static_cast<int64_t>(min_windows_distance) + 1;
  return static_cast<size_t>((len + step - 1) / step);
}

// Argument checks of the options; no device work.
int window_check_options(const dv_window_options* w, const char* who);
// Queues the pass over `n` regions whose two descriptors are in device memory: the candidate pass' link, resolve
// and group kernels, then the ordering, scoring and window kernels; no synchronisation.  With `packed`, the
// windows of all regions are also gathered back to back there, in region order.
int window_launch(const CandRegion* d_cand, const WindowRegion* d_win, int32_t n, uint32_t max_events,
                  const dv_window_options* w, int64_t* packed, hipStream_t stream);

}  // namespace dv

#endif  // DV_WINDOW_SELECT_H_
