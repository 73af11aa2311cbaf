// The genotype merge of one site, written once and compiled for both sides: the
// host entry point dv_genotype_sites walks the sites with it, the kernel of genotype.hip gives every site a lane.
// IEEE float32 / float64 operations in a fixed order and nothing else, so both sides agree bit for bit.  No locally
// indexed array: the running minima live in the site's own slice of `predictions`.
#ifndef DV_GENOTYPE_H_
#define DV_GENOTYPE_H_

#include <cmath>
#include <cstdint>

#include "dvhip.h"

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define DV_GT_HD __host__ __device__ inline
#else
#define DV_GT_HD inline
#endif

namespace dv {
namespace gt {

constexpr int kMaxAlts = 32;                                                    // `removed` holds a bit per alt
constexpr int kDeviceMaxAlts = DV_GENOTYPE_DEVICE_MAX_ALTS;
constexpr int kDeviceMaxItems = kDeviceMaxAlts * (kDeviceMaxAlts + 1) / 2;      // alt_allele_combinations of 6 alts

struct Sites {             // one call's tables, all on one side
  const float* probs;      // [N][3]
  const int8_t* item_alts; // [N][2], the second -1 for a single alt
  const int32_t* site_off; // [S + 1]
  const int32_t* n_alts;   // [S]
  double t;                // step 2's threshold; <= 0: no alt is dropped
  int32_t already_rounded; // probs are step 1's results (float32 values): widened as they are
  double* rounded;         // [N][3]
  const int64_t* pred_off; // [S + 1]
  double* predictions;
  int32_t* best;           // [S]
  uint32_t* removed;       // [S]
  uint8_t* status;         // [S]
};

DV_GT_HD int n_genotypes(int alts) { return (alts + 1) * (alts + 2) / 2; }
DV_GT_HD int genotype_index(int a, int b) { return b * (b + 1) / 2 + a; }       // alleles a <= b, VCF order
DV_GT_HD bool fits_device(int alts, int items) { return alts <= kDeviceMaxAlts && items <= kDeviceMaxItems; }
DV_GT_HD int count_bits(uint32_t mask) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(mask);
#else
  return __builtin_popcount(mask);
#endif
}
DV_GT_HD int bits_below(uint32_t mask, int bit) { return count_bits(mask & ((1u << bit) - 1u)); }
DV_GT_HD void take_min(double* slot, double v) {
  if (v < *slot) *slot = v;
}

// Step 1: call_variants.round_gls_batch(p, 10) on one row, widened.  -> the row's sum is off by more than 1e-6
DV_GT_HD bool round_item(const float* p, double* r, bool already_rounded) {
  const float f = 1e10f;
  const float p0 = p[0], p1 = p[1], p2 = p[2];
  const float total = (p0 + p1) + p2;
  if (already_rounded) {
    r[0] = static_cast<double>(p0);
    r[1] = static_cast<double>(p1);
    r[2] = static_cast<double>(p2);
    return fabsf(total - 1.0f) > 1e-6f;
  }
  int lowest = 0;
  float low = p0;
  if (p1 < low) {
    low = p1;
    lowest = 1;
  }
  if (p2 < low) lowest = 2;
  float r0 = rintf(p0 * f) / f, r1 = rintf(p1 * f) / f, r2 = rintf(p2 * f) / f;
  float rest = 0.0f;
  rest = rest + (lowest == 0 ? 0.0f : r0);
  rest = rest + (lowest == 1 ? 0.0f : r1);
  rest = rest + (lowest == 2 ? 0.0f : r2);
  float fix = rintf((1.0f - rest) * f) / f;
  fix = fix > 0.0f ? fix : 0.0f;
  if (lowest == 0) r0 = fix;
  if (lowest == 1) r1 = fix;
  if (lowest == 2) r2 = fix;
  r[0] = static_cast<double>(r0);
  r[1] = static_cast<double>(r1);
  r[2] = static_cast<double>(r2);
  return fabsf(total - 1.0f) > 1e-6f;
}

DV_GT_HD void genotype_site(const Sites& s, int32_t site) {
  const int64_t first = s.site_off[site], last = s.site_off[site + 1];
  const int alts = s.n_alts[site];
  bool bad_sum = false;
  for (int64_t i = first; i < last; ++i) bad_sum |= round_item(s.probs + 3 * i, s.rounded + 3 * i, s.already_rounded != 0);

  // step 2: the alts whose best single-alt item stays below t
  uint32_t removed = 0;
  if (last - first > 1 && s.t > 0.0) {
    bool any = false;
    double best_s = 0.0;
    int best_alt = 0;
    for (int a = 0; a < alts; ++a) {
      bool found = false;
      double s_a = 0.0;
      for (int64_t i = first; i < last; ++i) {
        if (s.item_alts[2 * i] != a || s.item_alts[2 * i + 1] >= 0) continue;
        double v = s.rounded[3 * i + 1] + s.rounded[3 * i + 2];
        v = v < 1.0 ? v : 1.0;
        if (!found || v > s_a) s_a = v;
        found = true;
      }
      if (!found) continue;
      if (s_a < s.t) removed |= 1u << a;
      if (!any || s_a > best_s) {
        best_s = s_a;
        best_alt = a;
      }
      any = true;
    }
    const uint32_t all = alts >= 32 ? 0xffffffffu : (1u << alts) - 1u;
    if (removed == all) removed &= ~(1u << best_alt);
  }

  // step 3: the minima straight into the site's slice
  const int kept = alts - count_bits(removed);
  const int n_valid = n_genotypes(kept), n_slots = n_genotypes(alts);
  double* pred = s.predictions + s.pred_off[site];
  const double inf = __builtin_huge_val();
  for (int g = 0; g < n_valid; ++g) pred[g] = inf;
  for (int g = n_valid; g < n_slots; ++g) pred[g] = 0.0;
  for (int64_t i = first; i < last; ++i) {
    const int x = s.item_alts[2 * i], y = s.item_alts[2 * i + 1];
    if ((removed >> x) & 1u) continue;
    if (y >= 0 && ((removed >> y) & 1u)) continue;
    const double r0 = s.rounded[3 * i], r1 = s.rounded[3 * i + 1], r2 = s.rounded[3 * i + 2];
    const int xa = 1 + x - bits_below(removed, x);
    take_min(pred, r0);
    take_min(pred + genotype_index(0, xa), r1);
    take_min(pred + genotype_index(xa, xa), r2);
    if (y >= 0) {
      const int ya = 1 + y - bits_below(removed, y);
      take_min(pred + genotype_index(0, ya), r1);
      take_min(pred + genotype_index(ya, ya), r2);
      take_min(pred + genotype_index(xa < ya ? xa : ya, xa < ya ? ya : xa), r2);
    }
  }
  bool incomplete = false;
  for (int g = 0; g < n_valid; ++g) incomplete |= pred[g] == inf;
  int best = -1;
  if (!incomplete) {
    if (last - first != 1) {       // a site of one item keeps its rounded values as they are
      double sum = 0.0;
      for (int g = 0; g < n_valid; ++g) sum = sum + pred[g];
      for (int g = 0; g < n_valid; ++g) pred[g] = pred[g] / sum;
    }
    best = 0;
    double best_v = pred[0];
    for (int g = 1; g < n_valid; ++g) {
      const double v = pred[g];
      if (v > best_v) {
        best_v = v;
        best = g;
      }
    }
  }
  s.best[site] = best;
  s.removed[site] = removed;
  s.status[site] = static_cast<uint8_t>(bad_sum ? DV_GENOTYPE_BAD_SUM : incomplete ? DV_GENOTYPE_INCOMPLETE : DV_GENOTYPE_OK);
}

}  // namespace gt
}  // namespace dv

#endif  // DV_GENOTYPE_H_
