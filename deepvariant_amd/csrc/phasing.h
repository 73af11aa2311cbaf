// Host side of read phasing for a batch of regions (phasing.hip; dv_phase_reads_batch / _device, include/dvhip.h):
// the argument checks, the plan (candidate filter, vertex order, texts' ranks and the device limits, per region) and the
// checker's loop.  Host code only: no HIP call is made here, so tools/phasing_batch_check.cpp drives it without a device.
#ifndef DV_PHASING_H_
#define DV_PHASING_H_

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "direct_phasing.h"
#include "dvhip.h"

namespace dv {
int fail(int status, const std::string& msg);   // dv_internal.h; common.hip defines it

namespace phasing {

constexpr int kMinRefAlleleDepth = 3;            // direct_phasing.cpp
constexpr int kMaxVertices = DV_PHASING_DEVICE_MAX_VERTICES;
constexpr int kMaxReads = DV_PHASING_DEVICE_MAX_READS;

struct Args {
  const dv_phasing_region* regions;
  int32_t n_regions;
  const dv_phasing_candidate* candidates;
  int32_t n_candidates;
  const dv_phasing_allele* alleles;
  int32_t n_alleles;
  const char* bases;
  int64_t n_bases;
  const int32_t* support_reads;
  const uint8_t* support_low_quality;
  int64_t n_support;
  int64_t n_reads_total;
  int32_t min_alleles_to_phase;
};

// What the kernel reads: the graph sites of the regions inside the limits, their vertices in the checker's insertion
// order (REF first, then the alleles by bases) and each vertex's rank among its site's texts.
struct DevRegion {
  int32_t site_off, n_sites;       // into the site table
  int32_t allele_off, n_alleles;   // the region's slice of allele_phases / allele_flags
  int64_t table_off;               // sites before this region's: its place in the per-position score tables
  int64_t phase_off;               // reads of the device regions before it: its place in the downloaded phases
  int32_t n_reads;
  int32_t region;                  // index into the call's regions
};
struct DevSite {
  int32_t vertex_off, n_vertices;
};
struct DevVertex {
  int64_t support_off;
  int32_t n_support;
  int32_t allele;                  // absolute index into the allele table
  int32_t rank;                    // of its text ("REF" or the bases) among the site's, as strings
  int32_t reserved;
};

struct Plan {
  std::vector<DevRegion> regions;
  std::vector<DevSite> sites;
  std::vector<DevVertex> vertices;
  std::vector<int32_t> host_regions;   // outside the limits
  int64_t device_reads = 0;
  int64_t candidates_in_regions = 0;
  dv_phasing_stats stats = {0, 0, 0, 0, 0, 0};
};

inline std::string allele_text(const Args& a, const dv_phasing_allele& al) {
  return al.is_ref ? std::string("REF") : std::string(a.bases + al.bases_off, static_cast<size_t>(al.bases_len));
}

// Null pointers, negative counts, slices outside their tables (DV_ERR_INVALID_ARGUMENT, all regions first); then
// unordered candidates and read indices past n_reads (DV_ERR_BAD_INPUT, the smallest such region).
inline int check(const std::string& who, const Args& a, const int32_t* read_phases) {
  if (a.n_regions < 0 || a.n_candidates < 0 || a.n_alleles < 0 || a.n_bases < 0 || a.n_support < 0 || a.n_reads_total < 0 ||
      (a.n_regions > 0 && !a.regions) || (a.n_candidates > 0 && !a.candidates) || (a.n_alleles > 0 && !a.alleles) ||
      (a.n_bases > 0 && !a.bases) || (a.n_support > 0 && (!a.support_reads || !a.support_low_quality)) ||
      (a.n_reads_total > 0 && !read_phases)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, who + ": null pointer or negative count");
  }
  for (int32_t k = 0; k < a.n_regions; ++k) {
    const dv_phasing_region& r = a.regions[k];
    const std::string where = who + ": region " + std::to_string(k) + ": ";
    if (r.candidate_off < 0 || r.n_candidates < 0 || static_cast<int64_t>(r.candidate_off) + r.n_candidates > a.n_candidates ||
        r.allele_off < 0 || r.n_alleles < 0 || static_cast<int64_t>(r.allele_off) + r.n_alleles > a.n_alleles ||
        r.support_off < 0 || r.n_support < 0 || r.support_off > a.n_support || r.n_support > a.n_support - r.support_off ||
        r.n_reads < 0 || r.first_read < 0 || r.first_read > a.n_reads_total || r.n_reads > a.n_reads_total - r.first_read) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, where + "slice outside its table");
    }
    for (int32_t i = r.candidate_off; i < r.candidate_off + r.n_candidates; ++i) {
      const dv_phasing_candidate& c = a.candidates[i];
      if (c.allele_off < r.allele_off || c.n_alleles < 0 ||
          static_cast<int64_t>(c.allele_off) + c.n_alleles > static_cast<int64_t>(r.allele_off) + r.n_alleles) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, where + "candidate allele range outside the region's alleles");
      }
      for (int32_t j = c.allele_off; j < c.allele_off + c.n_alleles; ++j) {
        const dv_phasing_allele& al = a.alleles[j];
        if (al.bases_off < 0 || al.bases_len < 0 || al.bases_off > a.n_bases || al.bases_len > a.n_bases - al.bases_off ||
            al.support_off < r.support_off || al.n_support < 0 ||
            al.support_off - r.support_off > r.n_support - al.n_support) {
          return dv::fail(DV_ERR_INVALID_ARGUMENT, where + "allele range outside its table");
        }
      }
    }
  }
  for (int32_t k = 0; k < a.n_regions; ++k) {
    const dv_phasing_region& r = a.regions[k];
    const std::string where = who + ": region " + std::to_string(k) + ": ";
    for (int32_t i = r.candidate_off; i < r.candidate_off + r.n_candidates; ++i) {
      const dv_phasing_candidate& c = a.candidates[i];
      if (i > r.candidate_off && !(a.candidates[i - 1].start < c.start)) {
        return dv::fail(DV_ERR_BAD_INPUT,
                        where + "Check failed: candidates[i - 1].variant().start() < candidate.variant().start()");
      }
      for (int32_t j = c.allele_off; j < c.allele_off + c.n_alleles; ++j) {
        const dv_phasing_allele& al = a.alleles[j];
        for (int64_t s = al.support_off; s < al.support_off + al.n_support; ++s) {
          if (a.support_reads[s] >= r.n_reads) return dv::fail(DV_ERR_BAD_INPUT, where + "read index out of range");
        }
      }
    }
  }
  return DV_OK;
}

// The candidate filter and the vertex order of direct_phasing.cpp (candidate_filter, build) on the arrays, and which
// regions the kernel takes.  `a` has passed check().
inline void make_plan(const Args& a, Plan* p) {
  std::vector<int64_t> stamp;      // per read: the last graph site (numbered over the call, from 1) that listed it
  int64_t site_id = 0;
  std::vector<int32_t> alts, by_text;
  std::vector<std::string> texts;
  p->stats.regions = a.n_regions;
  for (int32_t k = 0; k < a.n_regions; ++k) {
    const dv_phasing_region& r = a.regions[k];
    p->candidates_in_regions += r.n_candidates;
    const size_t sites_before = p->sites.size(), vertices_before = p->vertices.size();
    bool inside = r.n_reads <= kMaxReads;
    if (stamp.size() < static_cast<size_t>(r.n_reads)) stamp.resize(static_cast<size_t>(r.n_reads), 0);
    int64_t indel_end = 0;
    for (int32_t i = r.candidate_off; i < r.candidate_off + r.n_candidates; ++i) {
      const dv_phasing_candidate& c = a.candidates[i];
      const dv_phasing_allele* al = a.alleles + c.allele_off;
      int called = 0, ref_support = 0;
      for (int32_t j = 0; j < c.n_alleles; ++j) {
        if (al[j].is_ref) {
          ref_support = al[j].n_support;
        } else {
          ++called;
        }
      }
      if (called <= 1 && ref_support < kMinRefAlleleDepth) continue;
      bool substitutions = true;
      for (int32_t j = 0; j < c.n_alleles && substitutions; ++j) {
        if (al[j].is_ref) continue;
        if (c.end <= indel_end || static_cast<int64_t>(al[j].bases_len) != c.end - c.start) {
          if (indel_end < c.end) indel_end = c.end;
          substitutions = false;
        }
      }
      if (!substitutions) continue;
      // AddCandidate: the reference vertex (>= 3 support entries, low quality ones included), then alleles by bases
      DevSite site{static_cast<int32_t>(p->vertices.size()), 0};
      alts.clear();
      auto add = [&](int32_t j) {
        p->vertices.push_back(DevVertex{al[j].support_off, al[j].n_support, c.allele_off + j, 0, 0});
        ++site.n_vertices;
      };
      for (int32_t j = 0; j < c.n_alleles; ++j) {
        if (!al[j].is_ref) {
          alts.push_back(j);
        } else if (al[j].n_support >= kMinRefAlleleDepth) {
          add(j);
        }
      }
      texts.assign(static_cast<size_t>(c.n_alleles), std::string());
      for (int32_t j = 0; j < c.n_alleles; ++j) texts[j] = allele_text(a, al[j]);
      std::stable_sort(alts.begin(), alts.end(), [&](int32_t x, int32_t y) { return texts[x] < texts[y]; });
      for (int32_t j : alts) add(j);
      // compare_vertex_pair_by_bases compares the texts as strings: their ranks within the site stand for them
      DevVertex* verts = p->vertices.data() + site.vertex_off;
      by_text.resize(static_cast<size_t>(site.n_vertices));
      for (int32_t v = 0; v < site.n_vertices; ++v) by_text[v] = v;
      auto text_of = [&](int32_t v) -> const std::string& { return texts[verts[v].allele - c.allele_off]; };
      std::stable_sort(by_text.begin(), by_text.end(), [&](int32_t x, int32_t y) { return text_of(x) < text_of(y); });
      for (int32_t q = 0; q < site.n_vertices; ++q) {
        verts[by_text[q]].rank = q;
        if (q > 0 && text_of(by_text[q]) == text_of(by_text[q - 1])) inside = false;   // texts must be distinct
      }
      if (site.n_vertices > kMaxVertices) inside = false;
      // a read under two entries of one site makes edges within the site: the checker's business
      ++site_id;
      for (int32_t v = 0; v < site.n_vertices && inside; ++v) {
        for (int64_t s = verts[v].support_off; s < verts[v].support_off + verts[v].n_support; ++s) {
          const int32_t read = a.support_reads[s];
          if (read < 0 || a.support_low_quality[s]) continue;
          if (stamp[read] == site_id) {
            inside = false;
            break;
          }
          stamp[read] = site_id;
        }
      }
      p->sites.push_back(site);
    }
    p->stats.sites_in_graphs += static_cast<int64_t>(p->sites.size() - sites_before);
    p->stats.vertices += static_cast<int64_t>(p->vertices.size() - vertices_before);
    if (inside) {
      p->regions.push_back(DevRegion{static_cast<int32_t>(sites_before), static_cast<int32_t>(p->sites.size() - sites_before),
                                     r.allele_off, r.n_alleles, static_cast<int64_t>(sites_before), p->device_reads,
                                     r.n_reads, k});
      p->device_reads += r.n_reads;
    } else {
      p->sites.resize(sites_before);
      p->vertices.resize(vertices_before);
      p->host_regions.push_back(k);
      ++p->stats.regions_on_host;
    }
  }
}

// The checker on one region, as dv_phase_reads feeds it.  read_phases: the region's n_reads entries; allele_phases /
// allele_flags (either may be null): the whole tables, written at the region's candidates' alleles.
inline int phase_region_on_host(const std::string& who, const Args& a, int32_t k, int32_t* read_phases,
                                int32_t* allele_phases, uint8_t* allele_flags) {
  const dv_phasing_region& r = a.regions[k];
  std::vector<PhasingCandidate> cs(static_cast<size_t>(r.n_candidates));
  for (int32_t i = 0; i < r.n_candidates; ++i) {
    const dv_phasing_candidate& c = a.candidates[r.candidate_off + i];
    cs[i].start = c.start;
    cs[i].end = c.end;
    for (int32_t j = c.allele_off; j < c.allele_off + c.n_alleles; ++j) {
      const dv_phasing_allele& al = a.alleles[j];
      PhasingAllele pa;
      pa.bases.assign(a.bases + al.bases_off, static_cast<size_t>(al.bases_len));
      pa.is_ref = al.is_ref != 0;
      for (int64_t s = al.support_off; s < al.support_off + al.n_support; ++s) {
        pa.support.push_back(PhasingReadSupport{a.support_reads[s], a.support_low_quality[s] != 0});
      }
      cs[i].alleles.push_back(std::move(pa));
    }
  }
  DirectPhasing phasing(a.min_alleles_to_phase);
  std::vector<int> phases;
  std::string error;
  if (!phasing.phase_reads(cs, r.n_reads, &phases, &error)) {
    return dv::fail(DV_ERR_BAD_INPUT, who + ": region " + std::to_string(k) + ": " + error);
  }
  for (int32_t q = 0; q < r.n_reads; ++q) read_phases[q] = phases[q];
  for (int32_t i = 0; i < r.n_candidates; ++i) {
    const auto& per_allele = phasing.allele_phases()[i];
    for (size_t j = 0; j < per_allele.size(); ++j) {
      const int32_t at = a.candidates[r.candidate_off + i].allele_off + static_cast<int32_t>(j);
      if (allele_phases) allele_phases[at] = per_allele[j].in_graph ? per_allele[j].phase : -1;
      if (allele_flags) allele_flags[at] = per_allele[j].is_first_in_block ? 1 : 0;
    }
  }
  return DV_OK;
}

// A call's results before they are handed out: an error exit leaves the caller's arrays untouched.
struct Results {
  std::vector<int32_t> read_phases;    // regions' reads, concatenated in region order
  std::vector<int64_t> read_off;       // [n_regions + 1]
  std::vector<int32_t> allele_phases;  // whole table; only the regions' candidates' alleles are handed out
  std::vector<uint8_t> allele_flags;
  explicit Results(const Args& a) : read_off(static_cast<size_t>(a.n_regions) + 1, 0), allele_phases(a.n_alleles, 0),
                                    allele_flags(a.n_alleles, 0) {
    for (int32_t k = 0; k < a.n_regions; ++k) read_off[k + 1] = read_off[k] + a.regions[k].n_reads;
    read_phases.assign(static_cast<size_t>(read_off[a.n_regions]), 0);
  }
  void hand_out(const Args& a, int32_t* out_reads, int32_t* out_allele_phases, uint8_t* out_allele_flags) const {
    for (int32_t k = 0; k < a.n_regions; ++k) {
      const dv_phasing_region& r = a.regions[k];
      std::copy(read_phases.begin() + read_off[k], read_phases.begin() + read_off[k + 1], out_reads + r.first_read);
      for (int32_t i = r.candidate_off; i < r.candidate_off + r.n_candidates; ++i) {
        const dv_phasing_candidate& c = a.candidates[i];
        for (int32_t j = c.allele_off; j < c.allele_off + c.n_alleles; ++j) {
          if (out_allele_phases) out_allele_phases[j] = allele_phases[j];
          if (out_allele_flags) out_allele_flags[j] = allele_flags[j];
        }
      }
    }
  }
};

// dv_phase_reads_batch's body.
inline int run_on_host(const std::string& who, const Args& a, int32_t* read_phases, int32_t* allele_phases,
                       uint8_t* allele_flags, dv_phasing_stats* stats) {
  if (int rc = check(who, a, read_phases)) return rc;
  Plan plan;
  make_plan(a, &plan);
  Results res(a);
  for (int32_t k = 0; k < a.n_regions; ++k) {
    if (int rc = phase_region_on_host(who, a, k, res.read_phases.data() + res.read_off[k], res.allele_phases.data(),
                                      res.allele_flags.data())) {
      return rc;
    }
  }
  res.hand_out(a, read_phases, allele_phases, allele_flags);
  if (stats) *stats = plan.stats;
  return DV_OK;
}

}  // namespace phasing
}  // namespace dv

#endif  // DV_PHASING_H_
