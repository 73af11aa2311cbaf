// The fast pass of FastPassAligner (fast_pass_aligner.h, step 1) for every (window, haplotype) of a batch in one
// kernel launch, restated without the k-mer index and the serial walk: include/dvhip.h, "the fast pass over
// many windows in one call", has the contract.  Kernel, runtime and the C entry points: fast_pass.hip.
#ifndef DV_FAST_PASS_DEVICE_H_
#define DV_FAST_PASS_DEVICE_H_

#include <cstdint>
#include <string_view>
#include <vector>

#include "dvhip.h"
#include "fast_pass_aligner.h"

namespace dv {

constexpr int kFastPassMaxHaplotype = DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE;
constexpr int kFastPassMaxScoring = DV_FAST_PASS_DEVICE_MAX_SCORING;

struct FastPassWindow {
  std::vector<std::string_view> reads;        // upper-cased already
  std::vector<std::string_view> haplotypes;
  std::string_view reference;                 // a haplotype with these bytes is never discarded
  bool has_reference = true;
  int ref_prefix_len = 0, ref_suffix_len = 0;
};

struct FastPassScoring {                      // the class's resolved values
  int kmer_size, max_num_of_mismatches, match, mismatch;
};

struct FastPassStats {                        // dv_fast_pass_stats
  int64_t haplotypes = 0, haplotypes_on_host = 0, pairs = 0, cells = 0, launches = 0;
};
// of the calling thread's last device fast pass; the C entry points reset it before they check anything
FastPassStats& last_fast_pass_stats();

// DV_REALIGN_DEVICE_FASTPASS, read now; unset: off
bool device_fast_pass_enabled();

// Output layout of both functions: haplotype h = the h-th of all windows' haplotypes in window order; its reads'
// rows are [first_row[h], first_row[h] + its window's reads).  The vectors are sized by the call.
struct FastPassResults {
  std::vector<int32_t> haplotype_score, haplotype_discarded, read_position, read_score;
  std::vector<int64_t> first_row;             // [haplotypes + 1]
};

// A set-up aligner (reference, haplotypes, padding, options; its reads added) as a window of a batch.  The views
// point into the aligner.
inline FastPassWindow fast_pass_window_of(const FastPassAligner& a) {
  FastPassWindow w;
  w.reads.assign(a.reads().begin(), a.reads().end());
  w.haplotypes.assign(a.haplotypes().begin(), a.haplotypes().end());
  w.reference = a.reference();
  w.ref_prefix_len = a.ref_prefix_len();
  w.ref_suffix_len = a.ref_suffix_len();
  return w;
}
inline FastPassScoring fast_pass_scoring_of(const FastPassAligner& a) {
  return FastPassScoring{a.kmer_size(), a.max_num_of_mismatches(), a.match(), a.mismatch()};
}

// FastPassAligner's own code, window by window.
void fast_pass_on_host(const std::vector<FastPassWindow>& windows, const FastPassScoring& sc, FastPassResults* out);
// One upload, one launch, one download on `stream` (null: a non-blocking stream the library owns), then waits.
// A haplotype outside the kernel's limits runs through the host code inside the call.  Buffers are the calling
// thread's and are reused.  Returns a dv_status; DV_ERR_NO_DEVICE without a GPU (only when there is device work).
int fast_pass_on_device(const std::vector<FastPassWindow>& windows, const FastPassScoring& sc, void* stream,
                        FastPassResults* out, FastPassStats* stats);

}  // namespace dv

#endif  // DV_FAST_PASS_DEVICE_H_
