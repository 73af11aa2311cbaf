// candidates.h -- the candidate caller behind the allele counter: what allele_counter.hip hands to the
// kernels of candidates.hip.
#ifndef DV_CANDIDATES_H_
#define DV_CANDIDATES_H_

#include "dv_internal.h"

struct dv_candidates {
  std::vector<dv_candidate_site> sites;
  std::vector<dv_candidate_allele> alleles;
  std::vector<int32_t> words;      // per event, in the order of dv_allele_counts_arrays
};

namespace dv {

// One counter interval as the candidate kernels see it: the counts and events where the counter left
// them on the device, the read bases the events point into, and the region's slices of the scratch
// and result images.
struct CandRegion {
  const int32_t* ref_count;        // [len] ref_supporting_read_count
  const dv_allele_event* events;   // the counter's events, in any order
  const uint32_t* n_events;        // device word: events the counter wanted (only event_cap of them are there)
  uint32_t event_cap;
  const int32_t* read_key;         // [n_reads] read-key id per read; null = every read is its own key
  const uint8_t* ref;              // [len] reference bases of the interval
  const uint8_t* bases;            // the read table's bases and per-read offsets into them
  const uint32_t* seq_off;
  int32_t len;
  int32_t* scratch;                // cand_scratch_ints(len, event_cap) ints, zeroed before the launch
  dv_candidate_site* sites;        // [len] records, in position order
  dv_candidate_allele* alleles;    // [event_cap] records, site by site
  int32_t* words;                  // [event_cap] one word per event
  int32_t* n_out;                  // two device words: sites and allele records written
};

// Scratch of one region: list heads, good non-reference counts and selected-allele counts [len] each;
// event links, standing flags, group representatives, group counts and selection ordinals [event_cap] each.
inline size_t cand_scratch_ints(int64_t len, uint32_t event_cap) {
  return 3 * static_cast<size_t>(len) + 5 * static_cast<size_t>(event_cap);
}

// Argument checks of the options; no device work.
int cand_check_options(const dv_candidate_options* c, const char* who);
// Queues the pass over `n` regions whose descriptors are in device memory; no synchronisation.  The
// With `packed_sites`, the site and allele records of all regions are also gathered back to back, in
// region order, there and in `packed_alleles` (not needed with positions_only).
int cand_launch(const CandRegion* d_regions, int32_t n, uint32_t max_events,
                const dv_candidate_options* c, dv_candidate_site* packed_sites, dv_candidate_allele* packed_alleles,
                hipStream_t stream);

// The first three launches only (link, resolve, group), for a pass that reads the standing flags, the positions'
// good non-reference totals and the allele groups out of the scratch (cand_slices.h): window_select.hip.
int cand_group_launch(const CandRegion* d_regions, int32_t n, uint32_t max_events, hipStream_t stream);

}  // namespace dv

#endif  // DV_CANDIDATES_H_
