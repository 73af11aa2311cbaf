// The finish step of FastPassAligner::align_reads for a batch of windows on the device, behind the sweep + trace-back
// launch whose result stayed there (local_align_device.h, ResidentSweep).  The rule is realign_finish.h; kernels,
// runtime and the C entry points (dv_align_windows_batch, dv_align_windows_batch_device): realign_finish.hip.
#ifndef DV_REALIGN_FINISH_DEVICE_H_
#define DV_REALIGN_FINISH_DEVICE_H_

#include <cstdint>
#include <vector>

#include "dvhip.h"
#include "fast_pass_aligner.h"
#include "local_align_device.h"

namespace dv {

struct FinishStats {       // dv_realign_finish_stats
  int64_t windows = 0, windows_on_host = 0, reads = 0, cigar_words = 0, launches = 0, bytes_down = 0;
};
// of the calling thread's last dv_align_windows_batch_device or dv_realign_regions_device; both reset it first
FinishStats& last_finish_stats();

// DV_REALIGN_DEVICE_FINISH, read now; unset: off
bool device_finish_enabled();

// A window is finished on the device only if every one of its pairs [first_pair, first_pair + n_pairs) of the sweep
// call went kRouteDevice and every pair that holds an alignment was traced back there.
bool window_finishes_on_device(size_t first_pair, size_t n_pairs, const std::vector<uint8_t>& route,
                               const std::vector<SweepCorners>& corners, const ResidentSweep& sweep);

struct FinishWindow {      // a window after collect_alignments, its pairs swept by `sweep`'s call
  const FastPassAligner* aligner;
  const AlignmentPairs* pairs;
  size_t first_pair;       // of the window in the sweep call's pair list
  std::vector<RealignedRead>* out;   // what finish_alignments would return
};

// finish_alignments for every window of the list: one upload, four launches (haplotypes, pick + count, scan, write) on
// the sweep's stream, one download, one synchronisation.  force_alignment / normalize_reads: the aligners' (the same
// for every window).  stats is added to.  Returns a dv_status.
int finish_windows_on_device(const std::vector<FinishWindow>& windows, const ResidentSweep& sweep,
                             bool force_alignment, bool normalize_reads, FinishStats* stats);

}  // namespace dv

#endif  // DV_REALIGN_FINISH_DEVICE_H_
