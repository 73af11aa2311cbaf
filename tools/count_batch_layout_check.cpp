// count_batch_layout_check.cpp -- holds dv::plan_batch and dv::second_image (deepvariant_amd/csrc/allele_counter_plan.h)
// against a transcription of the hand-kept offset arithmetic they replaced in allele_counter.hip's batch entry point:
// every offset and total of the staging image, the result image and the second download, over region counts {0, 1, 3},
// table sizes and interval lengths from {0, 1, 15, 16, 17, 1000}, with and without candidate positions, read keys, the
// gVCF pass, the candidate pass, positions_only and the window pass (with and without counts, at window distances 0
// and 80, with and without the debug arrays), and every subset of regions overflowing its first guess.  The window
// pass' sections came after the hand-kept arithmetic: they are held against a second statement of them here.  So are
// the two sections of the one-launch counting kernel (plan_batch's one_launch: the CountArgs table and the block
// prefix behind every other section of the staging image), the regions' count slots and the workgroup total: every
// case without an overflowed region runs a second time with one_launch on, where everything else must stay as it is.
// Host arithmetic only: no HIP call is made and no device is needed.  Not part of the library's build:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Ideepvariant_amd/csrc \
//       tools/count_batch_layout_check.cpp -o /tmp/count_batch_layout_check && /tmp/count_batch_layout_check
#include <cstdio>
#include <cstdlib>

#include "allele_counter_plan.h"

namespace dv {   // dv_internal.h declares it; the library defines it in common.hip
int fail(int status, const std::string&) { return status; }
}  // namespace dv

namespace {

size_t align16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

// ---- the arithmetic as the batch entry point did it by hand
struct OldPlan {
  bool batched = false;
  size_t up[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  size_t cnt_off = 0, ev_off = 0;
  int64_t len = 0;
  uint32_t cap = 0;
  size_t mask_words = 0;
  size_t key_up = 0, scr_off = 0, blk_off = 0;
  int gv_slot = -1;
  int cd_slot = -1;
  size_t cscr_off = 0;
  int win_slot = -1;
  size_t wscr_off = 0, wwin_off = 0, wmask_off = 0;
};

struct OldTotals {
  size_t up_bytes = 0, cnt_ints = 0, ev_total = 0;
  int n_batched = 0, n_gv = 0, n_cd = 0;
  size_t scr_ints = 0, blk_total = 0, cscr_ints = 0;
  int64_t max_len = 0;
  uint32_t max_cap = 0;
  size_t desc_up = 0, cdesc_up = 0;
  size_t ctr_bytes = 0, nblk_off = 0, ncand_off = 0, res_bytes = 0;
  int n_win = 0;
  size_t wscr_ints = 0, win_total = 0, wmask_total = 0, wcdesc_up = 0, wdesc_up = 0, nwin_off = 0;
};

OldTotals old_plan(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                   const int32_t* const* read_keys, const dv_gvcf_options* gv, const dv_candidate_options* co,
                   const dv_window_options* wo, std::vector<OldPlan>* plan) {
  OldTotals t;
  plan->assign(static_cast<size_t>(n), OldPlan());
  for (int32_t k = 0; k < n; ++k) {
    const dv_batch* b = reads[k];
    const dv_allele_counter_options* o = options[k];
    OldPlan& p = (*plan)[k];
    p.len = o->interval_end - o->interval_start;
    if (b->n_reads == 0 || p.len == 0 || b->memory != DV_MEM_HOST) continue;
    p.batched = true;
    ++t.n_batched;
    const size_t nr = static_cast<size_t>(b->n_reads);
    const size_t sizes[9] = {nr * 4, (nr + 1) * 4, (nr + 1) * 4, nr, b->n_bases, b->n_bases,
                             static_cast<size_t>(b->n_cigar) * 4, static_cast<size_t>(o->n_ref_bases), 0};
    for (int f = 0; f < 8; ++f) {
      p.up[f] = t.up_bytes;
      t.up_bytes += align16(std::max<size_t>(sizes[f], 1));
    }
    size_t n_candidate_refs = 0;
    if (o->track_ref_reads && o->n_candidate_positions > 0) {
      p.mask_words = static_cast<size_t>((p.len + 31) / 32);
      p.up[8] = t.up_bytes;
      t.up_bytes += align16(p.mask_words * 4);
      n_candidate_refs = static_cast<size_t>(o->n_candidate_positions);
    }
    p.cnt_off = t.cnt_ints;
    t.cnt_ints += static_cast<size_t>(p.len);
    p.cap = b->n_cigar + b->n_bases / 16 + 4096 + static_cast<uint32_t>(std::min<size_t>(n_candidate_refs * 64, 1u << 24));
    p.ev_off = t.ev_total;
    t.ev_total += p.cap;
    if ((gv || co || wo) && read_keys && read_keys[k]) {
      p.key_up = t.up_bytes;
      t.up_bytes += align16(nr * 4);
    }
    if (co) {
      p.cd_slot = t.n_cd;
      ++t.n_cd;
      p.cscr_off = t.cscr_ints;
      t.cscr_ints += dv::cand_scratch_ints(p.len, p.cap);
      t.max_cap = std::max(t.max_cap, p.cap);
    }
    if (wo) {
      p.win_slot = t.n_win;
      ++t.n_win;
      p.wscr_off = t.wscr_ints;
      // the candidate kernels' eight slices, then two per position, six per event and the record count
      t.wscr_ints += 3 * static_cast<size_t>(p.len) + 5 * static_cast<size_t>(p.cap) + 2 * static_cast<size_t>(p.len) +
                     6 * static_cast<size_t>(p.cap) + 4;
      p.wwin_off = t.win_total;
      const int64_t step = 2 * static_cast<int64_t>(wo->min_windows_distance) + 1;
      t.win_total += static_cast<size_t>((p.len + step - 1) / step);
      p.wmask_off = t.wmask_total;
      t.wmask_total += static_cast<size_t>((p.len + 31) / 32);
      t.max_cap = std::max(t.max_cap, p.cap);
    }
    if (gv) {
      p.gv_slot = t.n_gv;
      ++t.n_gv;
      p.scr_off = t.scr_ints;
      t.scr_ints += dv::gvcf_scratch_ints(p.len, p.cap);
      p.blk_off = t.blk_total;
      t.blk_total += static_cast<size_t>(p.len - gv->left_padding - gv->right_padding);
      t.max_len = std::max(t.max_len, p.len);
      t.max_cap = std::max(t.max_cap, p.cap);
    }
  }
  t.desc_up = t.up_bytes;
  if (t.n_gv) t.up_bytes += align16(static_cast<size_t>(t.n_gv) * sizeof(dv::GvcfRegion));
  t.cdesc_up = t.up_bytes;
  if (t.n_cd) t.up_bytes += align16(static_cast<size_t>(t.n_cd) * sizeof(dv::CandRegion));
  t.wcdesc_up = t.up_bytes;
  if (t.n_win) t.up_bytes += align16(static_cast<size_t>(t.n_win) * sizeof(dv::CandRegion));
  t.wdesc_up = t.up_bytes;
  if (t.n_win) t.up_bytes += align16(static_cast<size_t>(t.n_win) * sizeof(dv::WindowRegion));
  t.ctr_bytes = align16(static_cast<size_t>(n) * 4 * sizeof(uint32_t));
  t.nblk_off = align16(t.ctr_bytes + t.cnt_ints * sizeof(int32_t));
  t.res_bytes = gv ? t.nblk_off + static_cast<size_t>(n) * sizeof(int32_t) : t.ctr_bytes + t.cnt_ints * sizeof(int32_t);
  t.ncand_off = align16(t.res_bytes);
  if (co) t.res_bytes = t.ncand_off + static_cast<size_t>(n) * 2 * sizeof(int32_t);
  t.nwin_off = align16(t.res_bytes);
  if (wo) t.res_bytes = t.nwin_off + static_cast<size_t>(n) * sizeof(int32_t);
  return t;
}

// The second download: the first walk sized it, a second one issued the copies and a third unpacked them.
struct OldSecond {
  struct Region {
    bool kept = false;
    size_t n_ev = 0, ev_at = 0, words_at = 0, sites_at = 0, alleles_at = 0, blocks_at = 0, windows_at = 0;
  };
  std::vector<Region> regions;
  size_t packed_blocks = 0, packed_at = 0, words_at = 0, packed_sites = 0, sites_at = 0, packed_alleles = 0,
         alleles_at = 0, ev_bytes = 0;
  size_t packed_windows = 0, windows_at = 0, scores_at = 0, masks_at = 0;
};

OldSecond old_second(int32_t n, std::vector<OldPlan> plan, const uint32_t* ctrs, const int32_t* nblk, const int32_t* ncand,
                     bool gv, bool co, bool pos_only, const int32_t* nwin, bool win_debug, size_t cnt_ints,
                     size_t wmask_total) {
  OldSecond s;
  s.regions.resize(static_cast<size_t>(n));
  size_t ev_bytes = 0;
  for (int32_t k = 0; k < n; ++k) {
    OldPlan& p = plan[k];
    if (!p.batched) continue;
    const uint32_t* ctr = ctrs + static_cast<size_t>(k) * 4;
    if (ctr[0] > p.cap) {
      p.batched = false;
      continue;
    }
    s.regions[k].kept = true;
    if (pos_only) continue;
    ev_bytes += static_cast<size_t>(ctr[0]) * sizeof(dv_allele_event);
  }
  if (gv) {
    for (int32_t k = 0; k < n; ++k) {
      if (plan[k].gv_slot >= 0) s.packed_blocks += static_cast<size_t>(nblk[k]);
    }
  }
  s.packed_at = ev_bytes;
  ev_bytes += s.packed_blocks * sizeof(dv_gvcf_block);
  s.words_at = ev_bytes;
  if (co) {
    for (int32_t k = 0; k < n; ++k) {
      if (plan[k].cd_slot < 0) continue;
      s.packed_sites += static_cast<size_t>(ncand[2 * k]);
      s.packed_alleles += static_cast<size_t>(ncand[2 * k + 1]);
      if (plan[k].batched && !pos_only) ev_bytes += static_cast<size_t>(ctrs[static_cast<size_t>(k) * 4]) * sizeof(int32_t);
    }
  }
  s.sites_at = ev_bytes;
  ev_bytes += s.packed_sites * sizeof(dv_candidate_site);
  s.alleles_at = ev_bytes;
  if (!pos_only) ev_bytes += s.packed_alleles * sizeof(dv_candidate_allele);
  s.windows_at = ev_bytes;
  for (int32_t k = 0; k < n; ++k) {
    if (plan[k].win_slot < 0) continue;
    s.regions[k].windows_at = s.windows_at + s.packed_windows * 16;
    s.packed_windows += static_cast<size_t>(nwin[k]);
  }
  ev_bytes += s.packed_windows * 16;
  s.scores_at = ev_bytes;
  if (win_debug) ev_bytes += cnt_ints * 4;
  s.masks_at = ev_bytes;
  if (win_debug) ev_bytes += wmask_total * 4;
  s.ev_bytes = ev_bytes;
  // the copies' walk
  size_t at = 0, wat = s.words_at;
  for (int32_t k = 0; k < n; ++k) {
    const OldPlan& p = plan[k];
    if (!p.batched || pos_only) continue;
    const size_t n_ev = ctrs[static_cast<size_t>(k) * 4];
    s.regions[k].n_ev = n_ev;
    s.regions[k].ev_at = at;
    s.regions[k].words_at = wat;
    at += n_ev * sizeof(dv_allele_event);
    if (co) wat += n_ev * sizeof(int32_t);
  }
  // the unpacking walks
  if (co) {
    size_t sat = s.sites_at, aat = s.alleles_at;
    for (int32_t k = 0; k < n; ++k) {
      if (plan[k].cd_slot < 0) continue;
      s.regions[k].sites_at = sat;
      s.regions[k].alleles_at = aat;
      sat += static_cast<size_t>(ncand[2 * k]) * sizeof(dv_candidate_site);
      aat += static_cast<size_t>(ncand[2 * k + 1]) * sizeof(dv_candidate_allele);
    }
  }
  at = s.packed_at;
  for (int32_t k = 0; k < n; ++k) {
    if (plan[k].gv_slot < 0) continue;
    s.regions[k].blocks_at = at;
    at += static_cast<size_t>(nblk[k]) * sizeof(dv_gvcf_block);
  }
  return s;
}

// ---- the comparison
long mismatches = 0, cases = 0;

#define SAME(x, y)                                                                                      \
  do {                                                                                                  \
    if (static_cast<long long>(x) != static_cast<long long>(y)) {                                       \
      if (++mismatches <= 20) {                                                                         \
        std::fprintf(stderr, "case %ld: %s = %lld but %s = %lld\n", cases, #x, static_cast<long long>(x), #y, \
                     static_cast<long long>(y));                                                        \
      }                                                                                                 \
    }                                                                                                   \
  } while (0)

void compare(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
             const int32_t* const* keys, const dv_gvcf_options* gv, const dv_candidate_options* co,
             const dv_window_options* wo, bool with_counts, unsigned overflowed, bool one_launch = false) {
  ++cases;
  const bool pos_only = (co && co->positions_only) || (wo && !with_counts);
  std::vector<OldPlan> old;
  const OldTotals t = old_plan(n, reads, options, keys, gv, co, wo, &old);
  const dv::BatchPlan plan = dv::plan_batch(n, reads, options, keys, gv, co, wo, one_launch);
  SAME(plan.regions.size(), old.size());
  SAME(plan.n_batched, t.n_batched);
  {
    // the one-launch kernel's sections, stated a second time: behind everything the image held before, the table of
    // 184-byte descriptors slot by slot, then one word per slot and one more; neither without a batched region
    static_assert(sizeof(dv::CountArgs) == 184, "CountArgs is part of the staging image");
    const bool sections = one_launch && t.n_batched > 0;
    size_t up_bytes = t.up_bytes;
    const size_t args_up = up_bytes;
    if (sections) up_bytes += align16(static_cast<size_t>(t.n_batched) * 184);
    const size_t first_up = up_bytes;
    if (sections) up_bytes += align16((static_cast<size_t>(t.n_batched) + 1) * 4);
    SAME(plan.cnt.one_launch, sections);
    SAME(plan.up_bytes, up_bytes);
    if (sections) {
      SAME(plan.cnt.args_up, args_up);
      SAME(plan.cnt.first_up, first_up);
    }
    long long workgroups = 0;
    int slot = 0;
    for (size_t k = 0; k < old.size(); ++k) {
      SAME(plan.regions[k].count_slot, old[k].batched ? slot : -1);
      if (!old[k].batched) continue;
      ++slot;
      workgroups += (reads[k]->n_reads + 63) / 64;
    }
    SAME(plan.cnt.workgroups, workgroups);
  }
  SAME(plan.cnt_ints, t.cnt_ints);
  SAME(plan.ev_total, t.ev_total);
  SAME(plan.max_cap, t.max_cap);
  SAME(plan.counters_at, 0);
  SAME(plan.counts_at, t.ctr_bytes);
  SAME(plan.res_bytes, t.res_bytes);
  SAME(plan.gv.n, t.n_gv);
  SAME(plan.cd.n, t.n_cd);
  if (gv) {
    SAME(plan.n_blocks_at, t.nblk_off);
    SAME(plan.gv.scratch_ints, t.scr_ints);
    SAME(plan.gv.blocks, t.blk_total);
    SAME(plan.gv.max_len, t.max_len);
    if (t.n_gv) SAME(plan.gv.desc_up, t.desc_up);
  }
  if (co) {
    SAME(plan.n_cand_at, t.ncand_off);
    SAME(plan.cd.scratch_ints, t.cscr_ints);
    if (t.n_cd) SAME(plan.cd.desc_up, t.cdesc_up);
  }
  SAME(plan.win.n, t.n_win);
  if (wo) {
    SAME(plan.n_win_at, t.nwin_off);
    SAME(plan.win.scratch_ints, t.wscr_ints);
    SAME(plan.win.windows, t.win_total);
    SAME(plan.win.mask_words, t.wmask_total);
    if (t.n_win) SAME(plan.win.cand_desc_up, t.wcdesc_up);
    if (t.n_win) SAME(plan.win.desc_up, t.wdesc_up);
  }
  for (size_t k = 0; k < old.size(); ++k) {
    const dv::RegionPlan& p = plan.regions[k];
    const OldPlan& q = old[k];
    SAME(p.batched, q.batched);
    SAME(p.len, q.len);
    if (!q.batched) continue;
    SAME(p.cap, q.cap);
    SAME(p.up.read_pos, q.up[0]);
    SAME(p.up.seq_off, q.up[1]);
    SAME(p.up.cigar_off, q.up[2]);
    SAME(p.up.mapq, q.up[3]);
    SAME(p.up.bases, q.up[4]);
    SAME(p.up.quals, q.up[5]);
    SAME(p.up.cigar, q.up[6]);
    SAME(p.up.ref, q.up[7]);
    SAME(p.mask_words, q.mask_words);
    if (q.mask_words) SAME(p.up.mask, q.up[8]);
    const bool has_keys = (gv || co || wo) && keys && keys[k];
    SAME(p.has_keys, has_keys);
    if (has_keys) SAME(p.up.keys, q.key_up);
    SAME(p.cnt_off, q.cnt_off);
    SAME(p.ev_off, q.ev_off);
    SAME(p.gv.slot, q.gv_slot);
    SAME(p.cd.slot, q.cd_slot);
    if (gv) {
      SAME(p.gv.scratch_off, q.scr_off);
      SAME(p.gv.block_off, q.blk_off);
    }
    if (co) SAME(p.cd.scratch_off, q.cscr_off);
    SAME(p.win.slot, q.win_slot);
    if (wo) {
      SAME(p.win.scratch_off, q.wscr_off);
      SAME(p.win.window_off, q.wwin_off);
      SAME(p.win.mask_off, q.wmask_off);
    }
  }
  // what the first download would bring: event counts within or beyond the first guess, some records everywhere
  std::vector<uint32_t> ctrs(static_cast<size_t>(n) * 4 + 4, 0);
  std::vector<int32_t> nblk(static_cast<size_t>(n) + 1, 0), ncand(static_cast<size_t>(n) * 2 + 2, 0);
  std::vector<int32_t> nwin(static_cast<size_t>(n) + 1, 0);
  for (int32_t k = 0; k < n; ++k) {
    const uint32_t cap = old[k].cap;
    ctrs[4 * k] = (overflowed >> k) & 1 ? cap + 1 + 7 * k : (cap / 3 + 5 * k) % (cap + 1);
    if (k == 1 && !((overflowed >> k) & 1)) ctrs[4 * k] = 0;
    ctrs[4 * k + 1] = 3;
    nblk[k] = 2 + 3 * k;
    ncand[2 * k] = k == 2 ? 0 : 5 + k;
    ncand[2 * k + 1] = 11 - 4 * k;
    nwin[k] = k == 1 ? 0 : 4 - k;
  }
  const bool win_debug = wo && wo->want_debug;
  const OldSecond s = old_second(n, old, ctrs.data(), nblk.data(), ncand.data(), gv != nullptr, co != nullptr, pos_only,
                                 nwin.data(), win_debug, t.cnt_ints, t.wmask_total);
  const dv::SecondImage im = dv::second_image(plan, ctrs.data(), nblk.data(), ncand.data(), pos_only, nwin.data(), win_debug);
  SAME(im.regions.size(), s.regions.size());
  SAME(im.bytes, s.ev_bytes);
  SAME(im.packed_blocks, s.packed_blocks);
  SAME(im.packed_sites, s.packed_sites);
  SAME(im.packed_alleles, s.packed_alleles);
  if (s.packed_blocks) SAME(im.blocks_at, s.packed_at);
  if (s.packed_sites) SAME(im.sites_at, s.sites_at);
  if (s.packed_alleles && !pos_only) SAME(im.alleles_at, s.alleles_at);
  SAME(im.packed_windows, s.packed_windows);
  if (s.packed_windows) SAME(im.windows_at, s.windows_at);
  if (win_debug) {
    SAME(im.scores_at, s.scores_at);
    SAME(im.masks_at, s.masks_at);
  }
  for (size_t k = 0; k < s.regions.size(); ++k) {
    const dv::SecondImage::Region& r = im.regions[k];
    const OldSecond::Region& q = s.regions[k];
    SAME(r.kept, q.kept);
    if (old[k].gv_slot >= 0) {
      SAME(r.n_blocks, nblk[k]);
      SAME(r.blocks_at, q.blocks_at);
    }
    if (old[k].cd_slot >= 0) {
      SAME(r.n_sites, ncand[2 * k]);
      SAME(r.n_alleles, ncand[2 * k + 1]);
      SAME(r.sites_at, q.sites_at);
      if (!pos_only) SAME(r.alleles_at, q.alleles_at);
    }
    if (old[k].win_slot >= 0) {
      SAME(r.n_windows, nwin[k]);
      SAME(r.windows_at, q.windows_at);
    }
    if (!q.kept || pos_only) continue;
    SAME(r.n_events, q.n_ev);
    SAME(r.events_at, q.ev_at);
    if (co) SAME(r.words_at, q.words_at);
  }
}

}  // namespace

int main() {
  const int64_t sizes[6] = {0, 1, 15, 16, 17, 1000};
  const int32_t some_keys[1] = {0};
  dv_gvcf_options gvcf{};
  gvcf.left_padding = 0;
  gvcf.right_padding = 0;
  dv_candidate_options calls{}, positions{};
  positions.positions_only = 1;
  dv_window_options near{}, far{}, debug{};
  near.model_type = far.model_type = debug.model_type = DV_WINDOW_MODEL_ALLELE_COUNT_LINEAR;
  far.min_windows_distance = 80;
  debug.min_windows_distance = 4;
  debug.want_debug = 1;
  struct Mode {
    const dv_gvcf_options* gv;
    const dv_candidate_options* co;
    const dv_window_options* wo;
    bool with_counts;
  };
  const Mode modes[9] = {{nullptr, nullptr, nullptr, true}, {&gvcf, nullptr, nullptr, true}, {nullptr, &calls, nullptr, true},
                         {&gvcf, &calls, nullptr, true}, {nullptr, &positions, nullptr, true},
                         {nullptr, nullptr, &near, false}, {nullptr, nullptr, &far, false}, {nullptr, nullptr, &debug, false},
                         {nullptr, nullptr, &debug, true}};
  for (int n : {0, 1, 3}) {
    for (int combo = 0; combo < 6 * 6 * 6 * 6; ++combo) {
      for (int n_positions = 0; n_positions < 2; ++n_positions) {
        for (int with_keys = 0; with_keys < 2; ++with_keys) {
          dv_batch batches[3];
          dv_allele_counter_options opts[3];
          const dv_batch* reads[3];
          const dv_allele_counter_options* options[3];
          const int32_t* keys[3];
          for (int k = 0; k < n; ++k) {
            // region k takes the combination k * 187 steps on, so that the regions of one batch differ
            const int c = (combo + 187 * k) % (6 * 6 * 6 * 6);
            dv_batch b{};
            b.memory = DV_MEM_HOST;
            b.n_reads = static_cast<int32_t>(sizes[c % 6]);
            b.n_bases = static_cast<uint32_t>(sizes[c / 6 % 6]);
            b.n_cigar = static_cast<uint32_t>(sizes[c / 36 % 6]);
            dv_allele_counter_options o{};
            o.interval_start = 100 + k;
            o.interval_end = o.interval_start + sizes[c / 216 % 6];
            o.n_ref_bases = o.interval_end - o.interval_start + 7;
            o.track_ref_reads = 1;
            o.n_candidate_positions = n_positions;
            batches[k] = b;
            opts[k] = o;
            reads[k] = &batches[k];
            options[k] = &opts[k];
            keys[k] = with_keys && k != 1 ? some_keys : nullptr;      // a batch may mix regions with and without
          }
          for (const Mode& m : modes) {
            for (unsigned overflowed = 0; overflowed < (1u << n); ++overflowed) {
              compare(n, reads, options, with_keys ? keys : nullptr, m.gv, m.co, m.wo, m.with_counts, overflowed);
            }
            compare(n, reads, options, with_keys ? keys : nullptr, m.gv, m.co, m.wo, m.with_counts, 0, true);
          }
        }
      }
    }
  }
  std::printf("%ld cases, %ld mismatches\n", cases, mismatches);
  return mismatches ? 1 : 0;
}
