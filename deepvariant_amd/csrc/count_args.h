// count_args.h -- the counting kernels' descriptor of one region (allele_counter.hip).  It is the one-region kernel's
// by-value argument and, with DV_COUNT_ONE_LAUNCH, an entry of the table in the batch's staging image that
// count_alleles_batch_kernel reads; allele_counter_plan.h sizes that table, so the struct lives where both see it.
#ifndef DV_COUNT_ARGS_H_
#define DV_COUNT_ARGS_H_

#include <cstdint>

#include "dvhip.h"

namespace dv {

constexpr int kCountReadsPerBlock = 64;   // consecutive reads of a region that one workgroup of either kernel takes

struct CountArgs {
  int32_t n_reads;
  const int32_t* read_pos;
  const uint32_t* seq_off;
  const uint32_t* cigar_off;
  const uint8_t* mapq;
  const uint8_t* bases;
  const uint8_t* quals;
  const uint32_t* cigar;
  const uint8_t* ref;        // reference bases of [ref_start, ref_start + n_ref)
  int64_t ref_start, n_ref;
  int64_t reads_start, reads_end;   // IsValidRefOffset: the reads interval
  int64_t interval_start, interval_len;
  int64_t contig_len;
  int32_t min_mapq, min_bq, legacy;
  int32_t* ref_count;        // [interval_len]
  const uint32_t* candidate_mask;   // track_ref_reads: bit p set = keep the reference reads of position p by name
  dv_allele_event* events;
  uint32_t event_cap;
  uint32_t* counters;        // [0] events wanted, [1] reads counted, [2] reference window too small
};

// a region's workgroups in either kernel
inline int64_t count_blocks(int32_t n_reads) { return (static_cast<int64_t>(n_reads) + kCountReadsPerBlock - 1) / kCountReadsPerBlock; }

}  // namespace dv

#endif  // DV_COUNT_ARGS_H_
