// gvcf.h -- the reference-confidence (gVCF) pass behind the allele counter: what allele_counter.hip
// hands to the kernels of gvcf.hip.
#ifndef DV_GVCF_H_
#define DV_GVCF_H_

#include "dv_internal.h"

struct dv_gvcf_blocks {
  std::vector<dv_gvcf_block> blocks;
};

namespace dv {

// One counter interval as the gVCF kernels see it: the counts where the counter left them on the
// device, and the region's slice of the scratch image (gvcf_scratch_ints).
struct GvcfRegion {
  const int32_t* ref_count;        // [len] ref_supporting_read_count
  const dv_allele_event* events;   // the counter's events, in any order
  const uint32_t* n_events;        // device word: events the counter wanted (only event_cap of them are there)
  uint32_t event_cap;
  const int32_t* read_key;         // [n_reads] read-key id per read; null = every read is its own key
  const uint8_t* ref;              // [len] reference bases of the interval
  int64_t interval_start;
  int32_t len, lo, hi;             // sites are [lo, hi): the interval minus left / right padding
  int32_t* scratch;                // gvcf_scratch_ints(len, event_cap) ints, zeroed before the launch
  dv_gvcf_block* blocks;           // [hi - lo] records, in order
  int32_t* n_blocks;               // device word: records written
};

// Scratch of one region: list heads / run starts [len + 1], alternate counts / run ordinals [len + 1],
// per site key, raw GQ, depth and table index [len] each, event links [event_cap].
inline size_t gvcf_scratch_ints(int64_t len, uint32_t event_cap) {
  return 2 * static_cast<size_t>(len + 1) + 4 * static_cast<size_t>(len) + event_cap;
}

// Argument checks of the options and of one region (padding, reference bases); no device work.
int gvcf_check_options(const dv_gvcf_options* g, const char* who);
int gvcf_check_region(const dv_allele_counter_options* o, const dv_gvcf_options* g, const char* who);
// The options' table on the current device (uploaded when it differs from the last one).
int gvcf_table_on_device(const dv_gvcf_options* g, const dv_gvcf_site** d_table, hipStream_t stream);
// Queues the pass over `n` regions whose descriptors are in device memory; no synchronisation.  With
// `packed`, the records of all regions are also gathered there back to back, in region order.
int gvcf_launch(const GvcfRegion* d_regions, int32_t n, int64_t max_len, uint32_t max_events,
                const dv_gvcf_options* g, const dv_gvcf_site* d_table, dv_gvcf_block* packed, hipStream_t stream);

}  // namespace dv

#endif  // DV_GVCF_H_
