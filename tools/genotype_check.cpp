// A stand-alone run of the genotype merge's host code (csrc/genotype.h through dv_genotype_sites, and
// dv_genotype_min_nonref_prob) for AddressSanitizer and UBSan, on the CPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Ideepvariant_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/genotype_check.cpp deepvariant_amd/csrc/genotype.hip deepvariant_amd/csrc/common.hip -o genotype_check
//   ./genotype_check
//
// Seeded sites of 1 to 32 alts with every item combination, partial item lists, empty sites and rows whose sum is off,
// at several thresholds; every result is checked for the invariants the contract gives.  The
// bit-for-bit comparison against the restatement is tests/test_genotype_cpu.py's; this program is about memory and
// undefined behaviour.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dvhip.h"

namespace {

uint64_t state = 0x9e3779b97f4a7c15ull;
double uniform() {       // splitmix64 -> [0, 1)
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return static_cast<double>(z >> 11) / 9007199254740992.0;
}

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "genotype_check: line %d: %s (%s)\n", __LINE__, #cond, dv_last_error()); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

struct Call {
  std::vector<float> probs;
  std::vector<int8_t> item_alts;
  std::vector<int32_t> site_off{0}, n_alts;

  void add_item(int x, int y, bool off_sum) {
    double a = std::pow(uniform(), 4.0), b = std::pow(uniform(), 4.0), c = std::pow(uniform(), 4.0);
    const double total = a + b + c + 1e-300;
    const float p0 = static_cast<float>(a / total), p1 = static_cast<float>(b / total);
    probs.push_back(p0);
    probs.push_back(p1);
    probs.push_back(off_sum ? 1.0f - p0 - p1 + 3e-6f : 1.0f - p0 - p1);
    item_alts.push_back(static_cast<int8_t>(x));
    item_alts.push_back(static_cast<int8_t>(y));
  }
  // every single alt and every pair, each kept with probability `keep`
  void add_site(int alts, double keep, bool off_sum) {
    for (int a = 0; a < alts; ++a) {
      if (uniform() < keep) add_item(a, -1, off_sum && a == 0);
    }
    for (int a = 0; a < alts; ++a) {
      for (int b = a + 1; b < alts; ++b) {
        if (uniform() >= keep) continue;
        const bool swap = uniform() < 0.5;       // a pair in either order
        add_item(swap ? b : a, swap ? a : b, false);
      }
    }
    site_off.push_back(static_cast<int32_t>(item_alts.size() / 2));
    n_alts.push_back(alts);
  }
};

void run(const Call& c, double t, int32_t already_rounded = 0) {
  dv_genotypes* g = nullptr;
  const int32_t n_sites = static_cast<int32_t>(c.n_alts.size());
  const int64_t n_items = static_cast<int64_t>(c.item_alts.size() / 2);
  CHECK(dv_genotype_sites(c.probs.data(), n_items, c.item_alts.data(), n_sites, c.site_off.data(), c.n_alts.data(), t,
                          already_rounded, &g) == DV_OK);
  dv_genotypes_view v;
  CHECK(dv_genotypes_arrays(g, &v) == DV_OK);
  CHECK(v.n_sites == n_sites && v.n_items == n_items && v.pred_off[0] == 0 && v.pred_off[n_sites] == v.n_predictions);
  for (int32_t s = 0; s < n_sites; ++s) {
    const int alts = c.n_alts[s];
    CHECK(v.pred_off[s + 1] - v.pred_off[s] == (alts + 1) * (alts + 2) / 2);
    const int kept = alts - __builtin_popcount(v.removed[s]);
    CHECK(kept >= 1 && (alts == 32 || (v.removed[s] >> alts) == 0));
    const int n_valid = (kept + 1) * (kept + 2) / 2;
    const double* pred = v.predictions + v.pred_off[s];
    CHECK(v.status[s] <= DV_GENOTYPE_INCOMPLETE);
    if (v.status[s] == DV_GENOTYPE_OK) {
      CHECK(v.best[s] >= 0 && v.best[s] < n_valid);
      double sum = 0.0;
      for (int k = 0; k < n_valid; ++k) {
        CHECK((already_rounded || pred[k] >= 0.0) && pred[k] <= pred[v.best[s]]);
        sum += pred[k];
      }
      if (c.site_off[s + 1] - c.site_off[s] > 1) CHECK(std::fabs(sum - 1.0) < 1e-12);
    }
    for (int k = n_valid; k < v.pred_off[s + 1] - v.pred_off[s]; ++k) CHECK(pred[k] == 0.0);
  }
  for (int64_t i = 0; i < n_items * 3; ++i) {
    if (already_rounded) {
      CHECK(v.rounded[i] == static_cast<double>(c.probs[static_cast<size_t>(i)]));     // widened as they are
    } else {
      CHECK(v.rounded[i] >= 0.0 && v.rounded[i] <= 1.0);
    }
  }
  dv_genotypes_free(g);
}

}  // namespace

int main() {
  const double thresholds[] = {0.0, dv_genotype_min_nonref_prob(1.0), dv_genotype_min_nonref_prob(20.0), 1.0, 2.0};
  CHECK(thresholds[1] > 0.2 && thresholds[1] < 0.21 && thresholds[2] > 0.98 && thresholds[2] < 1.0);
  CHECK(dv_genotype_min_nonref_prob(0.0) == 0.0 && std::isinf(dv_genotype_min_nonref_prob(1e9)));
  CHECK(dv_genotype_min_nonref_prob(std::nan("")) == 0.0);
  for (double t : thresholds) {
    Call c;
    run(c, t);                                     // no site
    for (int alts = 1; alts <= 32; ++alts) {
      c.add_site(alts, 1.0, false);
      c.add_site(alts, 0.6, alts % 5 == 0);
      c.add_site(alts, 0.0, false);                // no item
      c.add_site(1, 1.0, false);
    }
    run(c, t);
    if (t == 1.0) run(c, t, 1);
  }
  // what the entry point refuses
  {
    const float p[6] = {0.2f, 0.5f, 0.3f, 0.3f, 0.4f, 0.3f};
    const int32_t n_alts[1] = {2};
    dv_genotypes* g = nullptr;
    const int8_t past[4] = {0, -1, 2, -1};
    const int32_t off[2] = {0, 2}, short_off[2] = {0, 1};
    CHECK(dv_genotype_sites(p, 2, past, 1, off, n_alts, 0.2, 0, &g) == DV_ERR_BAD_INPUT && g == nullptr);
    const int8_t fine[4] = {0, -1, 1, 0};
    CHECK(dv_genotype_sites(p, 2, fine, 1, short_off, n_alts, 0.2, 0, &g) == DV_ERR_BAD_INPUT && g == nullptr);
    CHECK(dv_genotype_sites(nullptr, 2, fine, 1, off, n_alts, 0.2, 0, &g) == DV_ERR_INVALID_ARGUMENT && g == nullptr);
    CHECK(dv_genotype_sites(p, 2, fine, 1, off, n_alts, 0.2, 0, &g) == DV_OK && g != nullptr);
    dv_genotypes_free(g);
    dv_genotypes_free(nullptr);
  }
  std::printf("genotype_check ok\n");
  return 0;
}
