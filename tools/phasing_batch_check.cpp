// phasing_batch_check.cpp -- drives dv_phase_reads_batch's host code (deepvariant_amd/csrc/phasing.h: check, make_plan,
// the checker's loop, Results::hand_out) over empty, odd and out-of-range regions under the host sanitizers.  Every
// table is a heap vector of exactly its size, so a read or write one element past a slice is reported.  For good input
// the batch must equal dv::DirectPhasing run on each region alone; for bad input the status must be the documented one
// and the outputs must keep their sentinel.  Host code only: no HIP call is made and no device is needed.  Not part of
// the library's build:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude -Ideepvariant_amd/csrc \
//       tools/phasing_batch_check.cpp deepvariant_amd/csrc/direct_phasing.cpp -o /tmp/phasing_batch_check \
//       && /tmp/phasing_batch_check
#include <cstdio>
#include <cstdlib>
#include <functional>

#include "phasing.h"

namespace dv {   // dv_internal.h declares it; the library defines it in common.hip
int fail(int status, const std::string&) { return status; }
}  // namespace dv

namespace {

int failures = 0;

void expect(bool ok, const char* what, int line) {
  if (!ok) {
    std::fprintf(stderr, "phasing_batch_check: line %d: %s\n", line, what);
    ++failures;
  }
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

struct Tables {
  std::vector<dv_phasing_region> regions;
  std::vector<dv_phasing_candidate> candidates;
  std::vector<dv_phasing_allele> alleles;
  std::vector<char> bases;
  std::vector<int32_t> reads;
  std::vector<uint8_t> low;
  int64_t n_reads_total = 0;

  // a region of `n_sites` two-allele SNP sites over `n_reads` reads: even reads carry one allele, odd ones the other;
  // with_indel makes the first site a deletion that spans the second
  void add_region(int n_sites, int n_reads, bool with_indel = false, bool empty_alleles = false) {
    dv_phasing_region r{};
    r.candidate_off = static_cast<int32_t>(candidates.size());
    r.allele_off = static_cast<int32_t>(alleles.size());
    r.support_off = static_cast<int64_t>(reads.size());
    r.first_read = n_reads_total;
    r.n_reads = n_reads;
    for (int s = 0; s < n_sites; ++s) {
      const bool indel = with_indel && s == 0;
      dv_phasing_candidate c{100 + 3 * s, 100 + 3 * s + (indel ? 5 : 1), static_cast<int32_t>(alleles.size()), 2};
      for (int k = 0; k < 2; ++k) {
        dv_phasing_allele a{};
        a.bases_off = static_cast<int64_t>(bases.size());
        a.bases_len = indel && k == 1 ? 5 : 1;
        for (int b = 0; b < a.bases_len; ++b) bases.push_back("ACGT"[(s + 2 * k) % 4]);
        a.support_off = static_cast<int64_t>(reads.size());
        if (!empty_alleles) {
          for (int q = k; q < n_reads; q += 2) {
            reads.push_back(q == 4 ? -1 : q);
            low.push_back(q == 6 ? 1 : 0);
          }
        }
        a.n_support = static_cast<int32_t>(reads.size() - a.support_off);
        alleles.push_back(a);
      }
      candidates.push_back(c);
    }
    r.n_candidates = n_sites;
    r.n_alleles = static_cast<int32_t>(alleles.size()) - r.allele_off;
    r.n_support = static_cast<int64_t>(reads.size()) - r.support_off;
    n_reads_total += n_reads;
    regions.push_back(r);
  }

  dv::phasing::Args args() const {
    return dv::phasing::Args{regions.data(), static_cast<int32_t>(regions.size()), candidates.data(),
                             static_cast<int32_t>(candidates.size()), alleles.data(), static_cast<int32_t>(alleles.size()),
                             bases.data(), static_cast<int64_t>(bases.size()), reads.data(), low.data(),
                             static_cast<int64_t>(reads.size()), n_reads_total, 1};
  }
};

struct Outputs {
  std::vector<int32_t> phases, allele_phases;
  std::vector<uint8_t> flags;
  explicit Outputs(const Tables& t) : phases(t.n_reads_total, 77), allele_phases(t.alleles.size(), 77), flags(t.alleles.size(), 77) {}
  bool untouched() const {
    for (int32_t p : phases) if (p != 77) return false;
    for (int32_t p : allele_phases) if (p != 77) return false;
    for (uint8_t f : flags) if (f != 77) return false;
    return true;
  }
};

int run(const Tables& t, Outputs* o, dv_phasing_stats* stats = nullptr) {
  return dv::phasing::run_on_host("check", t.args(), o->phases.data(), o->allele_phases.data(), o->flags.data(), stats);
}

Tables good_tables() {
  Tables t;
  t.add_region(3, 9);
  t.add_region(0, 0);                  // empty
  t.add_region(0, 5);                  // reads without candidates
  t.add_region(4, 131, true);          // bitmaps past two words; an indel shadows its follower
  t.add_region(2, 7, false, true);     // alleles without support
  t.add_region(5, 1);
  t.add_region(2, 0);                  // candidates without reads: every support entry is out of the region
  return t;
}

void check_good() {
  Tables t = good_tables();
  // the last region's support must not name reads it does not have
  const dv_phasing_region& last = t.regions.back();
  for (int64_t s = last.support_off; s < last.support_off + last.n_support; ++s) t.reads[s] = -1;
  Outputs o(t);
  dv_phasing_stats stats{};
  EXPECT(run(t, &o, &stats) == DV_OK);
  EXPECT(stats.regions == static_cast<int64_t>(t.regions.size()) && stats.regions_on_host == 0 && stats.launches == 0);
  EXPECT(stats.sites_in_graphs == 3 + 2 + 2 + 5 + 2 && stats.vertices == 2 * stats.sites_in_graphs);
  const dv::phasing::Args a = t.args();
  for (size_t k = 0; k < t.regions.size(); ++k) {
    std::vector<int32_t> phases(static_cast<size_t>(t.regions[k].n_reads) + 1, 55), allele_phases(t.alleles.size(), 55);
    std::vector<uint8_t> flags(t.alleles.size(), 55);
    EXPECT(dv::phasing::phase_region_on_host("check", a, static_cast<int32_t>(k), phases.data(), allele_phases.data(),
                                             flags.data()) == DV_OK);
    EXPECT(phases.back() == 55);
    for (int32_t q = 0; q < t.regions[k].n_reads; ++q) EXPECT(o.phases[t.regions[k].first_read + q] == phases[q]);
    for (int32_t j = t.regions[k].allele_off; j < t.regions[k].allele_off + t.regions[k].n_alleles; ++j) {
      EXPECT(o.allele_phases[j] == allele_phases[j] && o.flags[j] == flags[j]);
    }
  }
  EXPECT(o.phases[0] != 0 && o.phases[1] != 0 && o.phases[0] != o.phases[1]);     // something was phased
  // optional outputs, and no regions at all with null tables
  std::vector<int32_t> phases(t.n_reads_total, 77);
  EXPECT(dv::phasing::run_on_host("check", a, phases.data(), nullptr, nullptr, nullptr) == DV_OK);
  EXPECT(phases == o.phases);
  const dv::phasing::Args none{nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 0, 1};
  EXPECT(dv::phasing::run_on_host("check", none, nullptr, nullptr, nullptr, &stats) == DV_OK && stats.regions == 0);
}

void check_bad(const char* what, int want, const std::function<void(Tables*)>& change) {
  Tables t = good_tables();
  const dv_phasing_region& last = t.regions.back();
  for (int64_t s = last.support_off; s < last.support_off + last.n_support; ++s) t.reads[s] = -1;
  change(&t);
  Outputs o(t);
  const int rc = run(t, &o);
  if (rc != want || !o.untouched()) {
    std::fprintf(stderr, "phasing_batch_check: %s: status %d (want %d), outputs %s\n", what, rc, want,
                 o.untouched() ? "untouched" : "WRITTEN");
    ++failures;
  }
}

}  // namespace

int main() {
  check_good();
  const int inv = DV_ERR_INVALID_ARGUMENT, bad = DV_ERR_BAD_INPUT;
  check_bad("candidate slice past the table", inv, [](Tables* t) { t->regions[5].n_candidates += 3; });
  check_bad("candidate offset negative", inv, [](Tables* t) { t->regions[0].candidate_off = -1; });
  check_bad("candidate offset past the table", inv, [](Tables* t) { t->regions[2].candidate_off = INT32_MAX; });
  check_bad("allele slice past the table", inv, [](Tables* t) { t->regions[6].n_alleles += 1; });
  check_bad("allele slice too short for its candidates", inv, [](Tables* t) { t->regions[0].n_alleles -= 1; });
  check_bad("support slice past the table", inv, [](Tables* t) { t->regions[6].n_support += 1; });
  check_bad("support offset huge", inv, [](Tables* t) { t->regions[3].support_off = INT64_MAX; });
  check_bad("support count huge", inv, [](Tables* t) { t->regions[3].n_support = INT64_MAX; });
  check_bad("support slice too short for its alleles", inv, [](Tables* t) { t->regions[0].n_support -= 1; });
  check_bad("reads past the total", inv, [](Tables* t) { t->regions[5].n_reads += 1; });
  check_bad("first_read huge", inv, [](Tables* t) { t->regions[1].first_read = INT64_MAX; });
  check_bad("negative n_reads", inv, [](Tables* t) { t->regions[1].n_reads = -1; });
  check_bad("candidate's alleles before its region's", inv, [](Tables* t) { t->candidates[3].allele_off = 0; });
  check_bad("candidate's allele count huge", inv, [](Tables* t) { t->candidates[0].n_alleles = INT32_MAX; });
  check_bad("candidate's allele count negative", inv, [](Tables* t) { t->candidates[0].n_alleles = -1; });
  check_bad("bases past the table", inv, [](Tables* t) { t->alleles.back().bases_len += 1; });
  check_bad("bases offset huge", inv, [](Tables* t) { t->alleles[0].bases_off = INT64_MAX; });
  check_bad("bases length negative", inv, [](Tables* t) { t->alleles[0].bases_len = -1; });
  check_bad("support past the region's slice", inv, [](Tables* t) { t->alleles[5].n_support += 1; });
  check_bad("support count negative", inv, [](Tables* t) { t->alleles[5].n_support = -1; });
  check_bad("support offset huge", inv, [](Tables* t) { t->alleles[5].support_off = INT64_MAX; });
  check_bad("unordered candidates", bad, [](Tables* t) { t->candidates[1].start = t->candidates[0].start; });
  check_bad("read index past the region's reads", bad, [](Tables* t) { t->reads[0] = 9; });
  if (failures) {
    std::fprintf(stderr, "phasing_batch_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("phasing_batch_check: ok\n");
  return 0;
}
