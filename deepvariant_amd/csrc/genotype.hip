// genotype.hip -- postprocess_variants' merge of each site's genotype calls: dv_genotype_sites
// (host code), dv_genotype_sites_device and dv_genotype_min_nonref_prob (include/dvhip.h).
//
// The rule is genotype.h, compiled for both sides.  Device: one launch, one lane per site -- most sites have one alt
// and one item, and the item and genotype loops of a lane are bounded by the device limit (6 alts, 21 items, 28
// genotypes).  A lane rounds its items into `rounded`, finds the alts to drop with two doubles compared (the phred
// threshold arrives as the probability t, see dv_genotype_min_nonref_prob), and keeps the running minima in its own
// slice of `predictions`, which it then normalises in place.  The probabilities are read where the classifier left
// them (probs_memory); one staged upload carries the other tables, one download brings every result home, and the
// stream is waited for once.  Sites above the limit are merged by the host code inside the call and counted.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_round_trip.h"
#include "genotype.h"

static_assert(sizeof(dv_genotype_device_stats) == 32, "dv_genotype_device_stats layout");
static_assert(sizeof(dv_genotypes_view) == 72, "dv_genotypes_view layout");

struct dv_genotypes {
  int64_t n_items = 0;
  std::vector<double> rounded, predictions;
  std::vector<int64_t> pred_off;
  std::vector<int32_t> best;
  std::vector<uint32_t> removed;
  std::vector<uint8_t> status;
};

namespace {

namespace gt = dv::gt;

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void genotype_sites_kernel(gt::Sites s, int32_t n_sites) {
  const int32_t site = static_cast<int32_t>(blockIdx.x) * kThreads + static_cast<int32_t>(threadIdx.x);
  if (site >= n_sites) return;
  if (!gt::fits_device(s.n_alts[site], s.site_off[site + 1] - s.site_off[site])) return;     // the host's
  gt::genotype_site(s, site);
}

dv_genotype_device_stats& last_stats() {
  static thread_local dv_genotype_device_stats stats;
  return stats;
}

// The arguments, checked; allocates the result with pred_off filled in.
int parse(const char* who, const float* probs, int64_t n_items, const int8_t* item_alts, int32_t n_sites,
          const int32_t* site_off, const int32_t* n_alts, dv_genotypes** out, std::unique_ptr<dv_genotypes>* res) {
  const std::string name(who);
  if (out) *out = nullptr;
  if (!out || n_items < 0 || n_sites < 0 || !site_off || (n_items > 0 && (!probs || !item_alts)) || (n_sites > 0 && !n_alts)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer or negative count");
  }
  if (n_items > 0x7fffffff) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": more than 2^31 - 1 items in one call");
  if (site_off[0] != 0 || site_off[n_sites] != n_items) {
    return dv::fail(DV_ERR_BAD_INPUT, name + ": site_off must run from 0 to n_items");
  }
  auto r = std::make_unique<dv_genotypes>();
  r->pred_off.assign(1, 0);
  for (int32_t s = 0; s < n_sites; ++s) {
    if (site_off[s + 1] < site_off[s]) {
      return dv::fail(DV_ERR_BAD_INPUT, name + ": site_off descends at site " + std::to_string(s));
    }
    const int alts = n_alts[s];
    if (alts < 1 || alts > gt::kMaxAlts) {
      return dv::fail(DV_ERR_BAD_INPUT, name + ": site " + std::to_string(s) + ": n_alts must be 1..32");
    }
    for (int64_t i = site_off[s]; i < site_off[s + 1]; ++i) {
      const int x = item_alts[2 * i], y = item_alts[2 * i + 1];
      if (x < 0 || x >= alts || y < -1 || y >= alts || y == x) {
        return dv::fail(DV_ERR_BAD_INPUT, name + ": item " + std::to_string(i) +
                                              ": one or two distinct alt indices below the site's n_alts are expected");
      }
    }
    r->pred_off.push_back(r->pred_off.back() + gt::n_genotypes(alts));
  }
  r->n_items = n_items;
  r->rounded.assign(static_cast<size_t>(n_items) * 3, 0.0);
  r->predictions.assign(static_cast<size_t>(r->pred_off.back()), 0.0);
  r->best.assign(static_cast<size_t>(n_sites), 0);
  r->removed.assign(static_cast<size_t>(n_sites), 0);
  r->status.assign(static_cast<size_t>(n_sites), 0);
  *res = std::move(r);
  return DV_OK;
}

gt::Sites host_sites(const float* probs, const int8_t* item_alts, const int32_t* site_off, const int32_t* n_alts,
                     double t, int32_t already_rounded, dv_genotypes* r) {
  gt::Sites s;
  s.probs = probs;
  s.item_alts = item_alts;
  s.site_off = site_off;
  s.n_alts = n_alts;
  s.t = t;
  s.already_rounded = already_rounded;
  s.rounded = r->rounded.data();
  s.pred_off = r->pred_off.data();
  s.predictions = r->predictions.data();
  s.best = r->best.data();
  s.removed = r->removed.data();
  s.status = r->status.data();
  return s;
}

int sites_on_device(const float* probs, int32_t probs_memory, int64_t n_items, const int8_t* item_alts, int32_t n_sites,
                    const int32_t* site_off, const int32_t* n_alts, double t, void* stream, dv_genotypes* r) {
  dv_genotype_device_stats& stats = last_stats();
  stats.sites = n_sites;
  std::vector<int32_t> on_host;
  int64_t host_items = 0;
  for (int32_t s = 0; s < n_sites; ++s) {
    if (gt::fits_device(n_alts[s], site_off[s + 1] - site_off[s])) continue;
    on_host.push_back(s);
    host_items += site_off[s + 1] - site_off[s];
  }
  stats.sites_on_host = static_cast<int64_t>(on_host.size());
  const bool launch = static_cast<int64_t>(on_host.size()) < n_sites;
  const bool probs_on_device = probs_memory == DV_MEM_DEVICE;
  const bool fetch = probs_on_device && host_items > 0;      // the host's sites need their probabilities at home
  const size_t n = static_cast<size_t>(n_items), ns = static_cast<size_t>(n_sites);
  const size_t n_pred = static_cast<size_t>(r->pred_off.back());

  dv::Layout up;
  const size_t u_probs = up.add(probs_on_device ? 0 : n * 3 * sizeof(float));
  const size_t u_alts = up.add(n * 2);
  const size_t u_site_off = up.add((ns + 1) * sizeof(int32_t));
  const size_t u_n_alts = up.add(ns * sizeof(int32_t));
  const size_t u_pred_off = up.add((ns + 1) * sizeof(int64_t));
  dv::Layout down;
  const size_t d_rounded = down.add(n * 3 * sizeof(double));
  const size_t d_pred = down.add(n_pred * sizeof(double));
  const size_t d_best = down.add(ns * sizeof(int32_t));
  const size_t d_removed = down.add(ns * sizeof(uint32_t));
  const size_t d_status = down.add_last(ns);

  static thread_local dv::RoundTrip rt;
  std::vector<float> fetched;
  if (launch || fetch) {
    if (int rc = rt.begin("dv_genotype_sites_device: no HIP device (dv_genotype_sites is the host code)", stream,
                          launch ? up.bytes() : 0, launch ? down.bytes() : 0, 0)) {
      return rc;
    }
  }
  if (launch) {
    if (!probs_on_device && n > 0) std::memcpy(rt.host_up<float>(u_probs), probs, n * 3 * sizeof(float));
    if (n > 0) std::memcpy(rt.host_up<int8_t>(u_alts), item_alts, n * 2);
    std::memcpy(rt.host_up<int32_t>(u_site_off), site_off, (ns + 1) * sizeof(int32_t));
    std::memcpy(rt.host_up<int32_t>(u_n_alts), n_alts, ns * sizeof(int32_t));
    std::memcpy(rt.host_up<int64_t>(u_pred_off), r->pred_off.data(), (ns + 1) * sizeof(int64_t));
    if (int rc = rt.upload(up.bytes())) return rc;
    gt::Sites s;
    s.probs = probs_on_device ? probs : rt.dev_up<const float>(u_probs);
    s.item_alts = rt.dev_up<const int8_t>(u_alts);
    s.site_off = rt.dev_up<const int32_t>(u_site_off);
    s.n_alts = rt.dev_up<const int32_t>(u_n_alts);
    s.t = t;
    s.already_rounded = 0;
    s.rounded = rt.dev_down<double>(d_rounded);
    s.pred_off = rt.dev_up<const int64_t>(u_pred_off);
    s.predictions = rt.dev_down<double>(d_pred);
    s.best = rt.dev_down<int32_t>(d_best);
    s.removed = rt.dev_down<uint32_t>(d_removed);
    s.status = rt.dev_down<uint8_t>(d_status);
    {
      dv::ProfileScope prof(dv::kProfOther, rt.stream());
      const unsigned groups = static_cast<unsigned>((ns + kThreads - 1) / kThreads);
      hipLaunchKernelGGL(genotype_sites_kernel, dim3(groups), dim3(kThreads), 0, rt.stream(), s, n_sites);
      DV_HIP_CHECK(hipGetLastError());
      ++stats.launches;
    }
  }
  if (fetch) {
    fetched.assign(n * 3, 0.0f);
    for (int32_t s : on_host) {
      const size_t a = static_cast<size_t>(site_off[s]) * 3;
      const size_t bytes = (static_cast<size_t>(site_off[s + 1]) * 3 - a) * sizeof(float);
      if (bytes == 0) continue;
      DV_HIP_CHECK(hipMemcpyAsync(fetched.data() + a, probs + a, bytes, hipMemcpyDeviceToHost, rt.stream()));
      stats.bytes_down += static_cast<int64_t>(bytes);
    }
  }
  if (launch) {
    if (int rc = rt.finish(down.bytes())) return rc;
    stats.bytes_down += static_cast<int64_t>(down.bytes());
    if (n > 0) std::memcpy(r->rounded.data(), rt.host_down<double>(d_rounded), n * 3 * sizeof(double));
    if (n_pred > 0) std::memcpy(r->predictions.data(), rt.host_down<double>(d_pred), n_pred * sizeof(double));
    std::memcpy(r->best.data(), rt.host_down<int32_t>(d_best), ns * sizeof(int32_t));
    std::memcpy(r->removed.data(), rt.host_down<uint32_t>(d_removed), ns * sizeof(uint32_t));
    std::memcpy(r->status.data(), rt.host_down<uint8_t>(d_status), ns);
  } else if (fetch) {
    DV_HIP_CHECK(hipStreamSynchronize(rt.stream()));
  }
  // the sites above the limit: the host code, over whatever the download left in their slices
  const gt::Sites h = host_sites(fetch ? fetched.data() : probs, item_alts, site_off, n_alts, t, 0, r);
  for (int32_t s : on_host) gt::genotype_site(h, s);
  return DV_OK;
}

// Python's round(x, 7) of a finite double: the nearest decimal with 7 places to the double's exact value, as a double.
double round7(double x) {
  char text[512];
  std::snprintf(text, sizeof text, "%.7f", x);
  return std::strtod(text, nullptr);
}

bool qual_reaches(double t, double qual_filter) {
  const double max_confidence = 1.0 - 1e-15;
  const double p = t < 1.0 ? t : 1.0;
  const double phred = -10.0 * std::log10(1.0 - (p < max_confidence ? p : max_confidence));
  return round7(phred) >= qual_filter;
}

double from_bits(uint64_t b) {
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}

}  // namespace

extern "C" {

int dv_genotype_sites(const float* probs, int64_t n_items, const int8_t* item_alts, int32_t n_sites,
                      const int32_t* site_off, const int32_t* n_alts, double t, int32_t already_rounded,
                      dv_genotypes** out) {
  return dv::guarded("dv_genotype_sites", [&]() -> int {
    std::unique_ptr<dv_genotypes> res;
    if (int rc = parse("dv_genotype_sites", probs, n_items, item_alts, n_sites, site_off, n_alts, out, &res)) return rc;
    const gt::Sites s = host_sites(probs, item_alts, site_off, n_alts, t, already_rounded, res.get());
    for (int32_t site = 0; site < n_sites; ++site) gt::genotype_site(s, site);
    *out = res.release();
    return DV_OK;
  });
}

int dv_genotype_sites_device(const float* probs, int32_t probs_memory, int64_t n_items, const int8_t* item_alts,
                             int32_t n_sites, const int32_t* site_off, const int32_t* n_alts, double t,
                             dv_genotypes** out, void* stream) {
  return dv::guarded("dv_genotype_sites_device", [&]() -> int {
    last_stats() = dv_genotype_device_stats();
    if (probs_memory != DV_MEM_HOST && probs_memory != DV_MEM_DEVICE) {
      if (out) *out = nullptr;
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_genotype_sites_device: probs_memory must be a dv_memory");
    }
    std::unique_ptr<dv_genotypes> res;
    // item_alts, site_off and n_alts are host arrays: everything but the probabilities is checked before any device work
    if (int rc = parse("dv_genotype_sites_device", probs, n_items, item_alts, n_sites, site_off, n_alts, out, &res)) {
      return rc;
    }
    if (n_sites > 0) {
      if (int rc = sites_on_device(probs, probs_memory, n_items, item_alts, n_sites, site_off, n_alts, t, stream, res.get())) {
        return rc;
      }
    }
    *out = res.release();
    return DV_OK;
  });
}

int dv_genotypes_arrays(const dv_genotypes* g, dv_genotypes_view* out) {
  if (!g || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_genotypes_arrays: null");
  out->n_sites = static_cast<int32_t>(g->best.size());
  out->reserved = 0;
  out->n_items = g->n_items;
  out->n_predictions = static_cast<int64_t>(g->predictions.size());
  out->rounded = g->rounded.data();
  out->pred_off = g->pred_off.data();
  out->predictions = g->predictions.data();
  out->best = g->best.data();
  out->removed = g->removed.data();
  out->status = g->status.data();
  return DV_OK;
}

void dv_genotypes_free(dv_genotypes* g) { delete g; }

double dv_genotype_min_nonref_prob(double qual_filter) {
  if (!(qual_filter > 0.0)) return 0.0;
  uint64_t lo = 0, hi;                       // doubles in [0, 1] order as their bit patterns do
  const double one = 1.0;
  std::memcpy(&hi, &one, sizeof hi);
  if (!qual_reaches(1.0, qual_filter)) return __builtin_huge_val();
  while (hi - lo > 1) {                      // qual_reaches(lo) is false, qual_reaches(hi) is true
    const uint64_t mid = lo + (hi - lo) / 2;
    if (qual_reaches(from_bits(mid), qual_filter)) {
      hi = mid;
    } else {
      lo = mid;
    }
  }
  return from_bits(hi);
}

int dv_genotype_device_last_stats(dv_genotype_device_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_genotype_device_last_stats: null");
  *out = last_stats();
  return DV_OK;
}

}  // extern "C"
