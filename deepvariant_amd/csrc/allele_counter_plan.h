// allele_counter_plan.h -- where everything of one dv_count_alleles_batch call lies: the staging image that goes up,
// the result image that comes back first, and the second image (events and packed records) whose sizes the first
// one tells.  Pure host arithmetic without a HIP call, so that tools/count_batch_layout_check.cpp can hold it
// against a transcription of the hand-kept offsets it replaced.
#ifndef DV_ALLELE_COUNTER_PLAN_H_
#define DV_ALLELE_COUNTER_PLAN_H_

#include "candidates.h"
#include "count_args.h"
#include "device_round_trip.h"
#include "gvcf.h"
#include "window_select.h"

namespace dv {

inline int64_t reads_start(const dv_allele_counter_options* o) { return std::min(o->interval_start, o->reads_interval_start); }
inline int64_t reads_end(const dv_allele_counter_options* o) { return std::max(o->interval_end, o->reads_interval_end); }

// track_ref_reads: the positions whose reference reads are kept by name (each adds events)
inline size_t n_candidate_refs(const dv_allele_counter_options* o) {
  return o->track_ref_reads && o->n_candidate_positions > 0 ? static_cast<size_t>(o->n_candidate_positions) : 0;
}
inline size_t mask_words(int64_t len) { return static_cast<size_t>((len + 31) / 32); }

// The first guess of a region's event capacity: substitutions are a few per cent of the bases, indels at most one
// per CIGAR op; the kernel's counter keeps counting past the capacity, so the caller learns the exact number.
inline uint32_t first_event_cap(const dv_batch* b, size_t n_candidate_refs) {
  return b->n_cigar + b->n_bases / 16 + 4096 + static_cast<uint32_t>(std::min<size_t>(n_candidate_refs * 64, 1u << 24));
}

struct RegionPlan {
  bool batched = false;       // false: no reads, no interval or a device-resident table -- the one-region path
  int64_t len = 0;
  uint32_t cap = 0;
  struct Upload {             // byte offsets in the staging image
    size_t read_pos = 0, seq_off = 0, cigar_off = 0, mapq = 0, bases = 0, quals = 0, cigar = 0, ref = 0;
    size_t mask = 0, keys = 0;                    // present with mask_words / has_keys
  } up;
  size_t mask_words = 0;
  bool has_keys = false;
  size_t cnt_off = 0, ev_off = 0;                 // in ints / events: the region's counts, and its events and words
  int count_slot = -1;                            // index among the batched regions: its CountArgs and block range
  struct Gvcf {
    int slot = -1;                                // index among the batched regions
    size_t scratch_off = 0, block_off = 0;        // in ints / records
  } gv;
  struct Cand {
    int slot = -1;
    size_t scratch_off = 0;                       // in ints; sites lie at cnt_off, alleles and words at ev_off
  } cd;
  struct Win {
    int slot = -1;
    size_t scratch_off = 0;                       // in ints: the candidate kernels' scratch, then the window kernels'
    size_t window_off = 0, mask_off = 0;          // in windows / mask words; scores lie at cnt_off
  } win;
};

struct BatchPlan {
  std::vector<RegionPlan> regions;
  int n_batched = 0;
  size_t up_bytes = 0;                            // the staging image: every region's arrays, then the descriptors
  size_t cnt_ints = 0, ev_total = 0;
  uint32_t max_cap = 0;                           // over the regions of either pass
  // the result image: counters [n][4] | counts | gVCF record counts [n] | candidate site and allele counts [n][2]
  // | window counts [n]
  size_t counters_at = 0, counts_at = 0, n_blocks_at = 0, n_cand_at = 0, n_win_at = 0, res_bytes = 0;
  struct Gvcf {
    int n = 0;
    size_t desc_up = 0;                           // the GvcfRegion descriptors in the staging image
    size_t scratch_ints = 0, blocks = 0;
    int64_t max_len = 0;
  } gv;
  struct Cand {
    int n = 0;
    size_t desc_up = 0;                           // the CandRegion descriptors
    size_t scratch_ints = 0;
  } cd;
  struct Win {
    int n = 0;
    size_t cand_desc_up = 0, desc_up = 0;         // the CandRegion and the WindowRegion descriptors, slot by slot
    size_t scratch_ints = 0, windows = 0, mask_words = 0;
  } win;
  struct Count {
    bool one_launch = false;                      // the two sections below exist
    size_t args_up = 0;                           // CountArgs[n_batched] in the staging image, slot by slot
    size_t first_up = 0;                          // uint32_t[n_batched + 1]: the first workgroup of every slot, and the grid
    int64_t workgroups = 0;                       // of all batched regions, whichever way they are launched
  } cnt;
};

// One grid holds at most this many workgroups; a batch beyond it (1.4e11 reads) is counted region by region.
constexpr int64_t kMaxCountWorkgroups = 0x7fffffff;

// `gv` / `co` / `wo`: the optional passes (null = off).  read_keys may be null, and so may each of its entries.
// `one_launch`: the staging image ends with the table and the block prefix of count_alleles_batch_kernel; without
// it no offset or total differs from a plan that knows nothing of them.
inline BatchPlan plan_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                            const int32_t* const* read_keys, const dv_gvcf_options* gv, const dv_candidate_options* co,
                            const dv_window_options* wo = nullptr, bool one_launch = false) {
  BatchPlan plan;
  plan.regions.resize(static_cast<size_t>(n > 0 ? n : 0));
  Layout up;
  for (int32_t k = 0; k < n; ++k) {
    const dv_batch* b = reads[k];
    const dv_allele_counter_options* o = options[k];
    RegionPlan& p = plan.regions[k];
    p.len = o->interval_end - o->interval_start;
    if (b->n_reads == 0 || p.len == 0 || b->memory != DV_MEM_HOST) continue;
    p.batched = true;
    p.count_slot = plan.n_batched++;
    plan.cnt.workgroups += count_blocks(b->n_reads);
    const size_t nr = static_cast<size_t>(b->n_reads);
    auto field = [&up](size_t bytes) { return up.add(std::max<size_t>(bytes, 1)); };
    p.up.read_pos = field(nr * 4);
    p.up.seq_off = field((nr + 1) * 4);
    p.up.cigar_off = field((nr + 1) * 4);
    p.up.mapq = field(nr);
    p.up.bases = field(b->n_bases);
    p.up.quals = field(b->n_bases);
    p.up.cigar = field(static_cast<size_t>(b->n_cigar) * 4);
    p.up.ref = field(static_cast<size_t>(o->n_ref_bases));
    const size_t n_refs = n_candidate_refs(o);
    if (n_refs) {
      p.mask_words = mask_words(p.len);
      p.up.mask = up.add(p.mask_words * 4);
    }
    p.cnt_off = plan.cnt_ints;
    plan.cnt_ints += static_cast<size_t>(p.len);
    p.cap = first_event_cap(b, n_refs);
    p.ev_off = plan.ev_total;
    plan.ev_total += p.cap;
    if ((gv || co || wo) && read_keys && read_keys[k]) {
      p.has_keys = true;
      p.up.keys = up.add(nr * 4);
    }
    if (gv || co || wo) plan.max_cap = std::max(plan.max_cap, p.cap);
    if (co) {
      p.cd.slot = plan.cd.n++;
      p.cd.scratch_off = plan.cd.scratch_ints;
      plan.cd.scratch_ints += cand_scratch_ints(p.len, p.cap);
    }
    if (wo) {
      p.win.slot = plan.win.n++;
      p.win.scratch_off = plan.win.scratch_ints;
      plan.win.scratch_ints += cand_scratch_ints(p.len, p.cap) + win_scratch_ints(p.len, p.cap);
      p.win.window_off = plan.win.windows;
      plan.win.windows += win_cap(p.len, wo->min_windows_distance);
      p.win.mask_off = plan.win.mask_words;
      plan.win.mask_words += mask_words(p.len);
    }
    if (gv) {
      p.gv.slot = plan.gv.n++;
      p.gv.scratch_off = plan.gv.scratch_ints;
      plan.gv.scratch_ints += gvcf_scratch_ints(p.len, p.cap);
      p.gv.block_off = plan.gv.blocks;
      plan.gv.blocks += static_cast<size_t>(p.len - gv->left_padding - gv->right_padding);
      plan.gv.max_len = std::max(plan.gv.max_len, p.len);
    }
  }
  if (plan.gv.n) plan.gv.desc_up = up.add(static_cast<size_t>(plan.gv.n) * sizeof(GvcfRegion));
  if (plan.cd.n) plan.cd.desc_up = up.add(static_cast<size_t>(plan.cd.n) * sizeof(CandRegion));
  if (plan.win.n) {
    plan.win.cand_desc_up = up.add(static_cast<size_t>(plan.win.n) * sizeof(CandRegion));
    plan.win.desc_up = up.add(static_cast<size_t>(plan.win.n) * sizeof(WindowRegion));
  }
  if (one_launch && plan.n_batched && plan.cnt.workgroups <= kMaxCountWorkgroups) {
    plan.cnt.one_launch = true;
    plan.cnt.args_up = up.add(static_cast<size_t>(plan.n_batched) * sizeof(CountArgs));
    plan.cnt.first_up = up.add((static_cast<size_t>(plan.n_batched) + 1) * sizeof(uint32_t));
  }
  plan.up_bytes = up.bytes();
  // the image's end is its last section's, unpadded
  Layout res;
  auto section = [&res](size_t bytes, bool last) { return last ? res.add_last(bytes) : res.add(bytes); };
  const size_t regions = plan.regions.size();
  plan.counters_at = res.add(regions * 4 * sizeof(uint32_t));
  plan.counts_at = section(plan.cnt_ints * sizeof(int32_t), !gv && !co && !wo);
  if (gv) plan.n_blocks_at = section(regions * sizeof(int32_t), !co && !wo);
  if (co) plan.n_cand_at = section(regions * 2 * sizeof(int32_t), !wo);
  if (wo) plan.n_win_at = res.add_last(regions * sizeof(int32_t));
  plan.res_bytes = res.bytes();
  return plan;
}

// Where the second download lies in its pinned image, from the numbers the first one brought: region by region the
// events, then the packed gVCF records, the event words region by region, the packed sites and the packed alleles,
// then the packed windows and -- with want_debug -- the scores and candidate masks of all batched regions.
// The device packs the records of EVERY region that was planned into a pass, the overflowed ones' included (their
// events exceeded `cap`; they go alone afterwards and `kept` is false): those records are skipped, not dropped.
// Nothing here is padded: the image is read with memcpy only.
struct SecondImage {
  struct Region {
    bool kept = false;                            // answered by the batch: events, words and records are copied out
    size_t n_events = 0, events_at = 0, words_at = 0;
    size_t n_blocks = 0, blocks_at = 0;
    size_t n_sites = 0, sites_at = 0, n_alleles = 0, alleles_at = 0;
    size_t n_windows = 0, windows_at = 0;
  };
  std::vector<Region> regions;
  size_t packed_blocks = 0, blocks_at = 0;        // records of all regions of the pass, and where they start
  size_t packed_sites = 0, sites_at = 0;
  size_t packed_alleles = 0, alleles_at = 0;
  size_t packed_windows = 0, windows_at = 0;      // two int64 each
  size_t scores_at = 0, masks_at = 0;             // want_debug: [cnt_ints] words and [win.mask_words] words
  size_t bytes = 0;
};

// counters: [n][4] as the kernel leaves them; n_blocks: [n] (gVCF pass on); n_cand: [n][2] (candidate pass on);
// n_win: [n] (window pass on).
inline SecondImage second_image(const BatchPlan& plan, const uint32_t* counters, const int32_t* n_blocks,
                                const int32_t* n_cand, bool positions_only, const int32_t* n_win = nullptr,
                                bool window_debug = false) {
  SecondImage s;
  const size_t n = plan.regions.size();
  s.regions.resize(n);
  Layout lay;
  for (size_t k = 0; k < n; ++k) {                // the events; and every region's record counts
    const RegionPlan& p = plan.regions[k];
    SecondImage::Region& r = s.regions[k];
    r.kept = p.batched && counters[4 * k] <= p.cap;
    if (r.kept && !positions_only) {
      r.n_events = counters[4 * k];
      r.events_at = lay.add_last(r.n_events * sizeof(dv_allele_event));
    }
    if (p.gv.slot >= 0) s.packed_blocks += r.n_blocks = static_cast<size_t>(n_blocks[k]);
    if (p.cd.slot >= 0) s.packed_sites += r.n_sites = static_cast<size_t>(n_cand[2 * k]);
    if (p.cd.slot >= 0) s.packed_alleles += r.n_alleles = static_cast<size_t>(n_cand[2 * k + 1]);
    if (p.win.slot >= 0) s.packed_windows += r.n_windows = static_cast<size_t>(n_win[k]);
  }
  s.blocks_at = lay.add_last(s.packed_blocks * sizeof(dv_gvcf_block));
  for (size_t k = 0; k < n; ++k) {                // the event words
    SecondImage::Region& r = s.regions[k];
    if (plan.regions[k].cd.slot >= 0 && r.kept && !positions_only) r.words_at = lay.add_last(r.n_events * sizeof(int32_t));
  }
  s.sites_at = lay.add_last(s.packed_sites * sizeof(dv_candidate_site));
  s.alleles_at = lay.add_last(positions_only ? 0 : s.packed_alleles * sizeof(dv_candidate_allele));
  s.windows_at = lay.add_last(s.packed_windows * 2 * sizeof(int64_t));
  s.scores_at = lay.add_last(window_debug ? plan.cnt_ints * sizeof(uint32_t) : 0);
  s.masks_at = lay.add_last(window_debug ? plan.win.mask_words * sizeof(uint32_t) : 0);
  s.bytes = lay.bytes();
  size_t blocks_at = s.blocks_at, sites_at = s.sites_at, alleles_at = s.alleles_at, windows_at = s.windows_at;
  for (SecondImage::Region& r : s.regions) {      // each region's records within the packed ones (none: nothing moves)
    r.blocks_at = blocks_at;
    r.sites_at = sites_at;
    r.alleles_at = alleles_at;
    blocks_at += r.n_blocks * sizeof(dv_gvcf_block);
    sites_at += r.n_sites * sizeof(dv_candidate_site);
    alleles_at += r.n_alleles * sizeof(dv_candidate_allele);
    r.windows_at = windows_at;
    windows_at += r.n_windows * 2 * sizeof(int64_t);
  }
  return s;
}

}  // namespace dv

#endif  // DV_ALLELE_COUNTER_PLAN_H_
