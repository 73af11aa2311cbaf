// Candidates + the reads of a batch of regions -> the item / list arrays of a dv_batch, on the device, with read
// support given by ROW key instead of by name: dv_pack_regions_device and its accessors, include/dvhip.h.
//
// The contract is dv_pack_region's (region_packer.cpp, which stays the checker), restated without strings.
// Query.  A read is in a candidate's list iff end + buffer > read_pos && start - buffer < read_end; the picked
// reads stand in ascending row order whether or not the region's rows are sorted by position.
// Support.  read_key[r] is equal for two rows of one region iff their "<fragment_name>/<read_number>" keys are
// equal.  A candidate has n_support entries (support_key, support_alt).  For a picked read first_alt is the
// smallest support_alt among the candidate's entries with the read's key and group the largest; with no such
// entry first_alt = 255 and group = n_alts.  An entry whose key matches no read is ignored.
// Items.  Candidates with ref_idx < 0 are skipped; the others give one item per combination mask, whose list is
// the picked reads; list_code = 0 for first_alt == 255, 1 if bit first_alt of the mask is set, else 2; list_group =
// group; item_image_start = start - (width - 1) / 2; item_height = pileup_height; item_out_off = item *
// example_bytes.  Items are numbered across the batch in region order then candidate order, list_read is the row
// in the concatenated table.
//
// Host plan (O(reads + support entries)): per region whether read_pos ascends and the largest reference span;
// every candidate's support entries sorted by (key, alt) -- one stable sort over (candidate, key, alt) for the
// batch; item_candidate / item_combo, which need no device.  One upload.
// pack_count_kernel, one workgroup per candidate: in a sorted region the rows that can overlap are
// [first row with pos >= q0 - max_span + 1, first row with pos >= q1) -- two binary searches, the host's bound --
// in an unsorted region the whole slice; lanes stride over the range and test the predicate; the number picked
// is left per candidate.
// pack_scan_kernel, one workgroup: exclusive scans in candidate order of picked * n_combos (64-bit) and of
// n_combos, and the largest list; the three totals are all that comes home (one small download, one
// synchronisation), and they decide the limits before anything is emitted.
// pack_emit_kernel, one workgroup per candidate: repeats the walk and compacts order-preserving (ballot + lane
// prefix per wave, the waves' counts through LDS, a running base per chunk); per picked read two binary searches
// of its key in the candidate's sorted support (start of the run: first_alt; end: group); the list is written
// once per combination with that mask's codes, and the first lanes write the item records.
// Placement is a pure function of the input; there are no atomics.  Every index is inside its array by
// construction: rows inside the region's slice (checked on the host), list positions below the scanned total
// (the emit walk is the count walk), support positions inside the candidate's slice (checked on the host).
//
// dv_pack_draws_device fills the same handle for items whose list is GIVEN -- a row range of a trimmed or
// alt-aligned table -- so only the support rule is left: the host plan sorts the support the same way and lays the
// lists out (prefix sum of the draws' n_rows), pack_draws_kernel runs one wave per draw.  One upload, one allocation,
// one launch, no download and no synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_round_trip.h"

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kScanThreads = 1024;

struct Region {          // as the kernels take a region
  int32_t read_first, n_reads;
  int32_t sorted;        // read_pos ascends over the slice
  int32_t pad;
  int64_t max_span;      // max(1, largest read_end - read_pos)
};

struct Cand {            // as the kernels take a candidate
  int64_t start, end;
  int32_t region;
  int32_t n_alts;
  int32_t ref_idx;
  uint32_t first_combo, n_combos;     // n_combos = 0 for a skipped candidate
  uint32_t first_support, n_support;  // slice of the SORTED support arrays
  int32_t index;                      // of the caller's cands
};

struct Totals {          // the download
  unsigned long long n_list;
  long long n_items;
  uint32_t max_list_len;
  uint32_t pad;
};

struct Inputs {          // device pointers into the upload
  const Region* regions;
  const Cand* cands;
  const int32_t* read_pos;
  const int64_t* read_end;
  const int32_t* read_key;
  const uint32_t* combo_masks;
  const int32_t* support_key;
  const uint8_t* support_alt;
  int32_t n_cands;
  int32_t buffer;
};

struct Outputs {         // device pointers into the handle's allocation
  int32_t* item_variant_start;
  int32_t* item_image_start;
  uint32_t* item_ref_idx;
  uint32_t* item_list_off;
  uint16_t* item_height;
  uint64_t* item_out_off;
  float* item_mean_coverage;
  uint32_t* list_read;
  uint8_t* list_code;
  uint8_t* list_group;
};

struct EmitOptions {
  int32_t half_width;
  int32_t pileup_height;
  uint64_t example_bytes;
  float mean_coverage;
  uint32_t n_items, n_list;
};

// The rows of the candidate's region that can overlap [q0, q1): [*lo, *hi) of the concatenated table.
__device__ __forceinline__ void row_range(const Inputs& in, const Region& rg, long long q0, long long q1, int32_t* lo,
                                          int32_t* hi) {
  const int32_t first = rg.read_first, n = rg.n_reads;
  if (!rg.sorted) {
    *lo = first;
    *hi = first + n;
    return;
  }
  const int32_t* pos = in.read_pos + first;
  const long long from = q0 - rg.max_span + 1;
  int32_t a = 0, b = n;              // first row with pos >= from
  while (a < b) {
    const int32_t m = a + ((b - a) >> 1);
    if (pos[m] < from) a = m + 1; else b = m;
  }
  const int32_t l = a;
  b = n;                             // first row at or after it with pos >= q1
  while (a < b) {
    const int32_t m = a + ((b - a) >> 1);
    if (pos[m] < q1) a = m + 1; else b = m;
  }
  *lo = first + l;
  *hi = first + a;
}

__device__ __forceinline__ bool overlaps(const Inputs& in, int32_t row, long long q0, long long q1) {
  return q1 > in.read_pos[row] && q0 < in.read_end[row];
}

// Pass 1: the number of reads each candidate picks.
__global__ __launch_bounds__(kThreads) void pack_count_kernel(Inputs in, uint32_t* picked) {
  __shared__ uint32_t wave_count[kWaves];
  const int32_t c = static_cast<int32_t>(blockIdx.x);
  const Cand cd = in.cands[c];
  if (cd.n_combos == 0) {            // skipped, or no combination: no item reads its list
    if (threadIdx.x == 0) picked[c] = 0;
    return;
  }
  const Region rg = in.regions[cd.region];
  const long long q0 = cd.start - in.buffer, q1 = cd.end + in.buffer;
  int32_t lo, hi;
  row_range(in, rg, q0, q1, &lo, &hi);
  uint32_t count = 0;
  for (int32_t row = lo + static_cast<int32_t>(threadIdx.x); row < hi; row += kThreads) count += overlaps(in, row, q0, q1);
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) count += __shfl_xor(count, d, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) wave_count[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (int w = 0; w < kWaves; ++w) total += wave_count[w];
    picked[c] = total;
  }
}

__device__ __forceinline__ unsigned long long wave_inclusive_scan(unsigned long long v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned long long up = __shfl_up(v, d, kWave);
    if (lane >= d) v += up;
  }
  return v;
}

// Pass 2: where every candidate's lists and items start, by one workgroup.
__global__ __launch_bounds__(kScanThreads) void pack_scan_kernel(Inputs in, const uint32_t* picked,
                                                                 unsigned long long* list_base, long long* item_base,
                                                                 Totals* totals) {
  __shared__ unsigned long long wave_list[kScanThreads / kWave], wave_items[kScanThreads / kWave];
  __shared__ uint32_t wave_max[kScanThreads / kWave];
  __shared__ unsigned long long carry_list, carry_items;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  if (tid == 0) carry_list = carry_items = 0;
  uint32_t longest = 0;
  __syncthreads();
  for (int32_t base = 0; base < in.n_cands; base += kScanThreads) {
    const int32_t c = base + tid;
    unsigned long long entries = 0, items = 0;
    if (c < in.n_cands) {
      items = in.cands[c].n_combos;
      entries = static_cast<unsigned long long>(picked[c]) * items;
      if (items && picked[c] > longest) longest = picked[c];
    }
    const unsigned long long list_incl = wave_inclusive_scan(entries, lane), items_incl = wave_inclusive_scan(items, lane);
    if (lane == kWave - 1) {
      wave_list[wave] = list_incl;
      wave_items[wave] = items_incl;
    }
    __syncthreads();
    unsigned long long before_list = carry_list, before_items = carry_items;
    for (int w = 0; w < wave; ++w) {
      before_list += wave_list[w];
      before_items += wave_items[w];
    }
    if (c < in.n_cands) {
      list_base[c] = before_list + list_incl - entries;
      item_base[c] = static_cast<long long>(before_items + items_incl - items);
    }
    __syncthreads();
    if (tid == kScanThreads - 1) {
      carry_list = before_list + list_incl;
      carry_items = before_items + items_incl;
    }
    __syncthreads();
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const uint32_t other = __shfl_xor(longest, d, kWave);
    longest = other > longest ? other : longest;
  }
  if (lane == 0) wave_max[wave] = longest;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kScanThreads / kWave; ++w) longest = wave_max[w] > longest ? wave_max[w] : longest;
    totals->n_list = carry_list;
    totals->n_items = static_cast<long long>(carry_items);
    totals->max_list_len = longest;
    totals->pad = 0;
  }
}

// A read's place in a candidate's support, sorted by (key, alt): the start of its key's run gives first_alt, the
// end group; both are left alone when no entry has the key.  ns > 0.
__device__ __forceinline__ void support_of(const int32_t* skey, const uint8_t* salt, int32_t ns, int32_t key,
                                           uint32_t* first_alt, uint32_t* group) {
  int32_t a = 0, b = ns;            // first entry with key >= the read's
  while (a < b) {
    const int32_t m = a + ((b - a) >> 1);
    if (skey[m] < key) a = m + 1; else b = m;
  }
  if (a < ns && skey[a] == key) {
    *first_alt = salt[a];           // entries of one key ascend by alt
    int32_t e = a + 1;
    b = ns;                         // first entry with key > the read's
    while (e < b) {
      const int32_t m = e + ((b - e) >> 1);
      if (skey[m] <= key) e = m + 1; else b = m;
    }
    *group = salt[e - 1];
  }
}

// Pass 3: the lists and item records, at the places pass 2 gave them.
__global__ __launch_bounds__(kThreads) void pack_emit_kernel(Inputs in, const uint32_t* picked,
                                                             const unsigned long long* list_base,
                                                             const long long* item_base, EmitOptions eo, Outputs o) {
  __shared__ uint32_t wave_count[kWaves];
  const int32_t c = static_cast<int32_t>(blockIdx.x);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  if (c == 0 && tid == 0) o.item_list_off[eo.n_items] = eo.n_list;
  const Cand cd = in.cands[c];
  if (cd.n_combos == 0) return;
  const uint32_t n_picked = picked[c];
  const uint32_t at = static_cast<uint32_t>(list_base[c]);      // the totals fit: the host checked them
  const uint32_t item0 = static_cast<uint32_t>(item_base[c]);
  for (uint32_t k = tid; k < cd.n_combos; k += kThreads) {
    const uint32_t item = item0 + k;
    o.item_variant_start[item] = static_cast<int32_t>(cd.start);
    o.item_image_start[item] = static_cast<int32_t>(cd.start - eo.half_width);
    o.item_ref_idx[item] = static_cast<uint32_t>(cd.ref_idx);
    o.item_list_off[item] = at + k * n_picked;
    o.item_height[item] = static_cast<uint16_t>(eo.pileup_height);
    o.item_out_off[item] = static_cast<uint64_t>(item) * eo.example_bytes;
    o.item_mean_coverage[item] = eo.mean_coverage;
  }
  if (n_picked == 0) return;
  const Region rg = in.regions[cd.region];
  const long long q0 = cd.start - in.buffer, q1 = cd.end + in.buffer;
  int32_t lo, hi;
  row_range(in, rg, q0, q1, &lo, &hi);
  const int32_t* skey = in.support_key + cd.first_support;
  const uint8_t* salt = in.support_alt + cd.first_support;
  const int32_t ns = static_cast<int32_t>(cd.n_support);
  uint32_t running = 0;                                         // picked in the chunks before this one
  for (int32_t chunk = lo; chunk < hi; chunk += kThreads) {     // the trip count is the workgroup's
    const int32_t row = chunk + tid;
    const bool pick = row < hi && overlaps(in, row, q0, q1);
    const unsigned long long ballot = __ballot(pick);
    if (lane == 0) wave_count[wave] = static_cast<uint32_t>(__popcll(ballot));
    __syncthreads();
    uint32_t before = running, in_chunk = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) before += wave_count[w];
      in_chunk += wave_count[w];
    }
    __syncthreads();
    running += in_chunk;
    if (!pick) continue;
    const uint32_t j = before + static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
    if (j >= n_picked) continue;      // cannot happen: the count walk is this walk
    uint32_t first_alt = 255, group = static_cast<uint32_t>(cd.n_alts);
    if (ns > 0) support_of(skey, salt, ns, in.read_key[row], &first_alt, &group);
    for (uint32_t k = 0; k < cd.n_combos; ++k) {
      const uint32_t mask = in.combo_masks[cd.first_combo + k];
      const uint32_t p = at + k * n_picked + j;
      o.list_read[p] = static_cast<uint32_t>(row);
      o.list_code[p] = first_alt == 255 ? 0 : ((mask >> first_alt) & 1u) ? 1 : 2;
      o.list_group[p] = static_cast<uint8_t>(group);
    }
  }
}

// ---- dv_pack_draws_device: items whose list is a given row range (trimmed and alt-aligned regions).  There is no
// query, so every size is the host's: item_list_off is the prefix sum of the draws' n_rows and travels with them.
struct Draw {              // as the kernel takes a draw: the caller's record, its candidate's support, its list's place
  int32_t row_first, n_rows;
  uint32_t list_off;
  uint32_t mask;
  uint32_t first_support, n_support;  // slice of the SORTED support arrays
  int32_t n_alts;
  int32_t variant_start, image_start;
  uint32_t ref_idx;
  uint64_t out_off;
  float mean_coverage;
  uint32_t height;
};

struct DrawInputs {        // device pointers into the upload
  const Draw* draws;
  const int32_t* rows_key;           // nullptr: a row is its own key
  const int32_t* support_key;
  const uint8_t* support_alt;
  uint32_t n_draws, n_list;
};

// One wave per draw, four to a workgroup: lanes stride over the draw's rows; lane 0 copies the item record.  Every
// index is inside its array by construction: rows inside the table and support slices inside their arrays (checked on
// the host), list positions below n_list (the host's prefix sum of the same n_rows).
__global__ __launch_bounds__(kThreads) void pack_draws_kernel(DrawInputs in, Outputs o) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t d = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (d >= in.n_draws) return;       // the wave's
  const Draw dr = in.draws[d];
  if (lane == 0) {
    o.item_variant_start[d] = dr.variant_start;
    o.item_image_start[d] = dr.image_start;
    o.item_ref_idx[d] = dr.ref_idx;
    o.item_list_off[d] = dr.list_off;
    o.item_height[d] = static_cast<uint16_t>(dr.height);
    o.item_out_off[d] = dr.out_off;
    o.item_mean_coverage[d] = dr.mean_coverage;
    if (d == 0) o.item_list_off[in.n_draws] = in.n_list;
  }
  const int32_t* skey = in.support_key + dr.first_support;
  const uint8_t* salt = in.support_alt + dr.first_support;
  const int32_t ns = static_cast<int32_t>(dr.n_support);
  for (int32_t i = lane; i < dr.n_rows; i += kWave) {
    const int32_t row = dr.row_first + i;
    uint32_t first_alt = 255, group = static_cast<uint32_t>(dr.n_alts);
    if (ns > 0) support_of(skey, salt, ns, in.rows_key ? in.rows_key[row] : row, &first_alt, &group);
    const uint32_t p = dr.list_off + static_cast<uint32_t>(i);
    o.list_read[p] = static_cast<uint32_t>(row);
    o.list_code[p] = first_alt == 255 ? 0 : ((dr.mask >> first_alt) & 1u) ? 1 : 2;
    o.list_group[p] = static_cast<uint8_t>(group);
  }
}

dv_pack_draws_stats& last_draws_stats() {
  static thread_local dv_pack_draws_stats stats;
  return stats;
}

dv_pack_device_stats& last_stats() {
  static thread_local dv_pack_device_stats stats;
  return stats;
}

// Sections of the handle's one device allocation (and of its host copy).
struct Sections {
  size_t ivs, iis, iri, ilo, ih, ioo, imc, lr, lc, lg, bytes;
  Sections(size_t n_items, size_t n_list) {
    dv::Layout l;
    ivs = l.add(n_items * sizeof(int32_t));
    iis = l.add(n_items * sizeof(int32_t));
    iri = l.add(n_items * sizeof(uint32_t));
    ilo = l.add((n_items + 1) * sizeof(uint32_t));
    ih = l.add(n_items * sizeof(uint16_t));
    ioo = l.add(n_items * sizeof(uint64_t));
    imc = l.add(n_items * sizeof(float));
    lr = l.add(n_list * sizeof(uint32_t));
    lc = l.add(n_list);
    lg = l.add(n_list);
    bytes = l.bytes();
  }
};

}  // namespace

struct dv_packed_regions {
  std::vector<int32_t> item_candidate;
  std::vector<uint32_t> item_combo;
  uint32_t n_list = 0, max_list_len = 0;
  void* device = nullptr;            // the arrays, laid out by Sections
  int device_id = -1;
  hipEvent_t emitted = nullptr;      // recorded behind the emit kernel
  std::vector<uint8_t> host;         // the download, made once
  bool downloaded = false;
  ~dv_packed_regions() {
    if (emitted) (void)hipEventDestroy(emitted);
    if (device) (void)hipFree(device);
  }
};

namespace {

// A support entry of the host plans, and the order the kernels search them in: by candidate, then (key, alt).
struct Entry {
  int32_t cand, key;
  uint8_t alt;
};

void sort_support(std::vector<Entry>* entries) {
  std::stable_sort(entries->begin(), entries->end(), [](const Entry& a, const Entry& b) {
    if (a.cand != b.cand) return a.cand < b.cand;
    if (a.key != b.key) return a.key < b.key;
    return a.alt < b.alt;
  });
}

// The call's arguments, checked, in the form the kernels take them.
struct Plan {
  std::vector<Region> regions;
  std::vector<Cand> cands;
  std::vector<int32_t> support_key;
  std::vector<uint8_t> support_alt;
  std::vector<int32_t> item_candidate;
  std::vector<uint32_t> item_combo;
  int64_t unsorted = 0;
};

int parse(int32_t n_regions, const dv_pack_region_slice* regions, const dv_pack_rows* rows,
          const dv_pack_regions_options* opt, const dv_pack_candidate* cands, const uint32_t* combo_masks,
          const int32_t* support_key, const uint8_t* support_alt, Plan* plan) {
  const std::string who = "dv_pack_regions_device: ";
  if (!rows || !opt || n_regions < 0 || (n_regions > 0 && !regions) || rows->n_reads < 0 || opt->n_candidates < 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "null pointer or negative count");
  }
  if (opt->width < 3 || opt->pileup_height <= 0) return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "width < 3 or pileup_height <= 0");
  if (rows->n_reads > 0 && (!rows->read_pos || !rows->read_end)) return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "null read_pos or read_end");
  if ((opt->n_candidates > 0 && !cands) || (opt->n_combo_masks > 0 && !combo_masks) ||
      (opt->n_support > 0 && (!support_key || !support_alt))) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "null candidate, combination or support array");
  }
  int64_t next_cand = 0;
  plan->regions.resize(static_cast<size_t>(n_regions));
  plan->cands.resize(static_cast<size_t>(opt->n_candidates));
  for (int32_t k = 0; k < n_regions; ++k) {
    const dv_pack_region_slice& s = regions[k];
    if (s.read_first < 0 || s.n_reads < 0 || static_cast<int64_t>(s.read_first) + s.n_reads > rows->n_reads) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "region " + std::to_string(k) + ": rows outside the table");
    }
    if (s.n_cands < 0 || s.cand_first != next_cand || next_cand + s.n_cands > opt->n_candidates) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "region " + std::to_string(k) + ": candidate slices must follow each other inside cands");
    }
    next_cand += s.n_cands;
    Region& rg = plan->regions[k];
    rg = Region{s.read_first, s.n_reads, 1, 0, 1};
    for (int32_t r = s.read_first; r < s.read_first + s.n_reads; ++r) {
      if (r > s.read_first && rows->read_pos[r] < rows->read_pos[r - 1]) rg.sorted = 0;
      rg.max_span = std::max<int64_t>(rg.max_span, rows->read_end[r] - rows->read_pos[r]);
    }
    if (s.n_cands > 0 && !rg.sorted) ++plan->unsorted;
    for (int32_t ci = s.cand_first; ci < s.cand_first + s.n_cands; ++ci) plan->cands[ci].region = k;
  }
  if (next_cand != opt->n_candidates) return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "the regions' candidate slices do not cover cands");
  // support entries of the candidates that give items, as (candidate, key, alt): one stable sort for the batch
  std::vector<Entry> entries;
  for (int32_t ci = 0; ci < opt->n_candidates; ++ci) {
    const dv_pack_candidate& c = cands[ci];
    Cand& cd = plan->cands[ci];
    cd.start = c.start;
    cd.end = c.end;
    cd.n_alts = c.n_alts;
    cd.ref_idx = c.ref_idx;
    cd.first_combo = c.first_combo;
    cd.n_combos = 0;
    cd.first_support = cd.n_support = 0;
    cd.index = ci;
    if (c.ref_idx < 0) continue;         // no reference window: skipped, as the reference does
    if (c.n_alts < 0 || c.n_alts > 32) return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "n_alts out of range");
    if (static_cast<uint64_t>(c.first_combo) + c.n_combos > opt->n_combo_masks) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "candidate " + std::to_string(ci) + ": combinations outside combo_masks");
    }
    if (static_cast<uint64_t>(c.first_support) + c.n_support > opt->n_support) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "candidate " + std::to_string(ci) + ": support entries outside the support arrays");
    }
    if (c.start < INT32_MIN || c.start > INT32_MAX) return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "variant start outside int32");
    cd.n_combos = c.n_combos;
    for (uint32_t j = c.first_support; j < c.first_support + c.n_support; ++j) {
      if (support_alt[j] >= c.n_alts) return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "support_alt out of range");
      if (c.n_combos) entries.push_back(Entry{ci, support_key[j], support_alt[j]});
    }
    for (uint32_t k = 0; k < c.n_combos; ++k) {
      plan->item_candidate.push_back(ci);
      plan->item_combo.push_back(combo_masks[c.first_combo + k]);
    }
  }
  if (entries.size() > UINT32_MAX) return dv::fail(DV_ERR_BAD_INPUT, who + "more than 2^32 - 1 support entries");
  sort_support(&entries);
  plan->support_key.resize(entries.size());
  plan->support_alt.resize(entries.size());
  for (size_t j = 0; j < entries.size(); ++j) {
    plan->support_key[j] = entries[j].key;
    plan->support_alt[j] = entries[j].alt;
    Cand& cd = plan->cands[entries[j].cand];
    if (cd.n_support++ == 0) cd.first_support = static_cast<uint32_t>(j);
  }
  return DV_OK;
}

int pack_on_device(const Plan& plan, const dv_pack_rows* rows, const dv_pack_regions_options* opt,
                   const uint32_t* combo_masks, void* stream_in, dv_packed_regions* res, dv_pack_device_stats* stats) {
  const size_t n_reads = static_cast<size_t>(rows->n_reads), n_regions = plan.regions.size(), n_cands = plan.cands.size();
  const size_t n_masks = opt->n_combo_masks, n_sup = plan.support_key.size();
  dv::Layout up, down, work;
  // upload image: regions | candidates | read_pos | read_end | read_key | combination masks | support keys | support alts
  const size_t u_regions = up.add(n_regions * sizeof(Region));
  const size_t u_cands = up.add(n_cands * sizeof(Cand));
  const size_t u_end = up.add(n_reads * sizeof(int64_t));
  const size_t u_pos = up.add(n_reads * sizeof(int32_t));
  const size_t u_key = up.add(n_reads * sizeof(int32_t));
  const size_t u_masks = up.add(n_masks * sizeof(uint32_t));
  const size_t u_skey = up.add(n_sup * sizeof(int32_t));
  const size_t u_salt = up.add(n_sup);
  const size_t d_totals = down.add(sizeof(Totals));
  // device-only work space: picked | list_base | item_base per candidate
  const size_t k_base = work.add(n_cands * sizeof(unsigned long long));
  const size_t k_item = work.add(n_cands * sizeof(long long));
  const size_t k_picked = work.add(n_cands * sizeof(uint32_t));
  static thread_local dv::RoundTrip rt;
  // the emit kernel of this thread's previous call reads the staging that this call refills: it has to be over
  // (it is, unless the caller never waited for its stream)
  static thread_local hipEvent_t previous_emit = nullptr;
  if (previous_emit) (void)hipEventSynchronize(previous_emit);
  if (int rc = rt.begin("dv_pack_regions_device: no HIP device (dv_pack_region is the host code)", stream_in, up.bytes(),
                        down.bytes(), work.bytes())) {
    return rc;
  }
  std::memcpy(rt.host_up<Region>(u_regions), plan.regions.data(), n_regions * sizeof(Region));
  std::memcpy(rt.host_up<Cand>(u_cands), plan.cands.data(), n_cands * sizeof(Cand));
  if (n_reads) {
    std::memcpy(rt.host_up<int64_t>(u_end), rows->read_end, n_reads * sizeof(int64_t));
    std::memcpy(rt.host_up<int32_t>(u_pos), rows->read_pos, n_reads * sizeof(int32_t));
    int32_t* key = rt.host_up<int32_t>(u_key);
    if (rows->read_key) {
      std::memcpy(key, rows->read_key, n_reads * sizeof(int32_t));
    } else {
      for (size_t r = 0; r < n_reads; ++r) key[r] = static_cast<int32_t>(r);
    }
  }
  if (n_masks) std::memcpy(rt.host_up<uint32_t>(u_masks), combo_masks, n_masks * sizeof(uint32_t));
  if (n_sup) {
    std::memcpy(rt.host_up<int32_t>(u_skey), plan.support_key.data(), n_sup * sizeof(int32_t));
    std::memcpy(rt.host_up<uint8_t>(u_salt), plan.support_alt.data(), n_sup);
  }
  Inputs in;
  in.regions = rt.dev_up<const Region>(u_regions);
  in.cands = rt.dev_up<const Cand>(u_cands);
  in.read_pos = rt.dev_up<const int32_t>(u_pos);
  in.read_end = rt.dev_up<const int64_t>(u_end);
  in.read_key = rt.dev_up<const int32_t>(u_key);
  in.combo_masks = rt.dev_up<const uint32_t>(u_masks);
  in.support_key = rt.dev_up<const int32_t>(u_skey);
  in.support_alt = rt.dev_up<const uint8_t>(u_salt);
  in.n_cands = static_cast<int32_t>(n_cands);
  in.buffer = opt->read_overlap_buffer_bp;
  uint8_t* d_work = static_cast<uint8_t*>(rt.d_scratch.ptr);
  uint32_t* d_picked = reinterpret_cast<uint32_t*>(d_work + k_picked);
  unsigned long long* d_list_base = reinterpret_cast<unsigned long long*>(d_work + k_base);
  long long* d_item_base = reinterpret_cast<long long*>(d_work + k_item);
  hipStream_t stream = rt.stream();
  const unsigned blocks = static_cast<unsigned>(n_cands);
  if (int rc = rt.upload(up.bytes())) return rc;
  {
    dv::ProfileScope prof(dv::kProfOther, stream);
    hipLaunchKernelGGL(pack_count_kernel, dim3(blocks), dim3(kThreads), 0, stream, in, d_picked);
    DV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, in, d_picked, d_list_base, d_item_base,
                       rt.dev_down<Totals>(d_totals));
    DV_HIP_CHECK(hipGetLastError());
  }
  if (int rc = rt.finish(down.bytes())) return rc;
  stats->launches += 2;
  const Totals totals = *rt.host_down<Totals>(d_totals);
  if (totals.n_items != static_cast<long long>(plan.item_candidate.size())) {
    return dv::fail(DV_ERR_HIP, "dv_pack_regions_device: the device's item count differs from the plan's");
  }
  if (totals.n_list > UINT32_MAX) {
    return dv::fail(DV_ERR_BAD_INPUT, "dv_pack_regions_device: " + std::to_string(totals.n_list) +
                                          " list entries, more than 2^32 - 1; pass fewer regions");
  }
  const size_t n_items = static_cast<size_t>(totals.n_items), n_list = static_cast<size_t>(totals.n_list);
  const Sections s(n_items, n_list);
  DV_HIP_CHECK(hipGetDevice(&res->device_id));
  DV_HIP_CHECK(hipMalloc(&res->device, s.bytes));
  DV_HIP_CHECK(hipEventCreateWithFlags(&res->emitted, hipEventDisableTiming));
  uint8_t* base = static_cast<uint8_t*>(res->device);
  Outputs o;
  o.item_variant_start = reinterpret_cast<int32_t*>(base + s.ivs);
  o.item_image_start = reinterpret_cast<int32_t*>(base + s.iis);
  o.item_ref_idx = reinterpret_cast<uint32_t*>(base + s.iri);
  o.item_list_off = reinterpret_cast<uint32_t*>(base + s.ilo);
  o.item_height = reinterpret_cast<uint16_t*>(base + s.ih);
  o.item_out_off = reinterpret_cast<uint64_t*>(base + s.ioo);
  o.item_mean_coverage = reinterpret_cast<float*>(base + s.imc);
  o.list_read = reinterpret_cast<uint32_t*>(base + s.lr);
  o.list_code = base + s.lc;
  o.list_group = base + s.lg;
  EmitOptions eo;
  eo.half_width = (opt->width - 1) / 2;
  eo.pileup_height = opt->pileup_height;
  eo.example_bytes = opt->example_bytes;
  eo.mean_coverage = opt->mean_coverage;
  eo.n_items = static_cast<uint32_t>(n_items);
  eo.n_list = static_cast<uint32_t>(n_list);
  {
    dv::ProfileScope prof(dv::kProfOther, stream);
    hipLaunchKernelGGL(pack_emit_kernel, dim3(blocks), dim3(kThreads), 0, stream, in, d_picked, d_list_base, d_item_base,
                       eo, o);
    DV_HIP_CHECK(hipGetLastError());
  }
  stats->launches += 1;
  DV_HIP_CHECK(hipEventRecord(res->emitted, stream));
  if (!previous_emit) DV_HIP_CHECK(hipEventCreateWithFlags(&previous_emit, hipEventDisableTiming));
  DV_HIP_CHECK(hipEventRecord(previous_emit, stream));
  if (!stream_in) DV_HIP_CHECK(hipStreamSynchronize(stream));   // nobody else can order work behind the library's stream
  res->n_list = static_cast<uint32_t>(n_list);
  res->max_list_len = totals.max_list_len;
  stats->items = static_cast<int64_t>(n_items);
  stats->list_entries = static_cast<int64_t>(n_list);
  return DV_OK;
}

// dv_pack_draws_device's arguments, checked, in the form the kernel takes them.
struct DrawPlan {
  std::vector<Draw> draws;
  std::vector<int32_t> support_key;
  std::vector<uint8_t> support_alt;
  uint64_t n_list = 0;
  uint32_t max_list_len = 0;
};

int parse_draws(int32_t n_rows, const dv_pack_draw* draws, int64_t n_draws,
                const dv_pack_candidate* cands, int32_t n_cands, const int32_t* support_key, const uint8_t* support_alt,
                uint32_t n_support, DrawPlan* plan) {
  const std::string who = "dv_pack_draws_device: ";
  if (n_rows < 0 || n_draws < 0 || n_cands < 0 || (n_draws > 0 && !draws) || (n_cands > 0 && !cands) ||
      (n_support > 0 && (!support_key || !support_alt))) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, who + "null pointer with a non-zero count, or a negative count");
  }
  if (n_draws > INT32_MAX) return dv::fail(DV_ERR_BAD_INPUT, who + "more than 2^31 - 1 draws; pass fewer regions");
  for (int32_t ci = 0; ci < n_cands; ++ci) {
    const dv_pack_candidate& c = cands[ci];
    const std::string which = who + "candidate " + std::to_string(ci) + ": ";
    if (c.n_alts < 0 || c.n_alts > 32) return dv::fail(DV_ERR_INVALID_ARGUMENT, which + "n_alts out of range");
    if (static_cast<uint64_t>(c.first_support) + c.n_support > n_support) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, which + "support entries outside the support arrays");
    }
    for (uint32_t j = c.first_support; j < c.first_support + c.n_support; ++j) {
      if (support_alt[j] >= c.n_alts) return dv::fail(DV_ERR_INVALID_ARGUMENT, which + "support_alt out of range");
    }
  }
  std::vector<uint8_t> drawn(static_cast<size_t>(n_cands), 0);
  for (int64_t d = 0; d < n_draws; ++d) {
    const dv_pack_draw& w = draws[d];
    const std::string which = who + "draw " + std::to_string(d) + ": ";
    if (w.row_first < 0 || w.n_rows < 0 || static_cast<int64_t>(w.row_first) + w.n_rows > n_rows) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, which + "rows outside the table");
    }
    if (w.cand < 0 || w.cand >= n_cands) return dv::fail(DV_ERR_INVALID_ARGUMENT, which + "candidate outside cands");
    if (w.height == 0) return dv::fail(DV_ERR_INVALID_ARGUMENT, which + "height 0");
    const int32_t n_alts = cands[w.cand].n_alts;
    if (n_alts < 32 && (w.combo_mask >> n_alts) != 0) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, which + "combo_mask names an alt the candidate does not have");
    }
    drawn[w.cand] = 1;
    plan->n_list += static_cast<uint64_t>(w.n_rows);
    plan->max_list_len = std::max(plan->max_list_len, static_cast<uint32_t>(w.n_rows));
  }
  if (plan->n_list > UINT32_MAX) {
    return dv::fail(DV_ERR_BAD_INPUT, who + std::to_string(plan->n_list) + " list entries, more than 2^32 - 1; pass fewer regions");
  }
  // support entries of the candidates that are drawn, sorted as the regions' plan sorts them
  std::vector<Entry> entries;
  for (int32_t ci = 0; ci < n_cands; ++ci) {
    if (!drawn[ci]) continue;
    const dv_pack_candidate& c = cands[ci];
    for (uint32_t j = c.first_support; j < c.first_support + c.n_support; ++j) {
      entries.push_back(Entry{ci, support_key[j], support_alt[j]});
    }
  }
  sort_support(&entries);
  std::vector<uint32_t> first(static_cast<size_t>(n_cands), 0), count(static_cast<size_t>(n_cands), 0);
  plan->support_key.resize(entries.size());
  plan->support_alt.resize(entries.size());
  for (size_t j = 0; j < entries.size(); ++j) {
    plan->support_key[j] = entries[j].key;
    plan->support_alt[j] = entries[j].alt;
    if (count[entries[j].cand]++ == 0) first[entries[j].cand] = static_cast<uint32_t>(j);
  }
  plan->draws.resize(static_cast<size_t>(n_draws));
  uint32_t at = 0;
  for (int64_t d = 0; d < n_draws; ++d) {
    const dv_pack_draw& w = draws[d];
    Draw& dr = plan->draws[static_cast<size_t>(d)];
    dr.row_first = w.row_first;
    dr.n_rows = w.n_rows;
    dr.list_off = at;
    dr.mask = w.combo_mask;
    dr.first_support = first[w.cand];
    dr.n_support = count[w.cand];
    dr.n_alts = cands[w.cand].n_alts;
    dr.variant_start = w.variant_start;
    dr.image_start = w.image_start;
    dr.ref_idx = w.ref_idx;
    dr.out_off = w.out_off;
    dr.mean_coverage = w.mean_coverage;
    dr.height = w.height;
    at += static_cast<uint32_t>(w.n_rows);
  }
  return DV_OK;
}

int pack_draws_on_device(const DrawPlan& plan, const int32_t* rows_key, int32_t n_rows, void* stream_in,
                         dv_packed_regions* res, dv_pack_draws_stats* stats) {
  const size_t n_draws = plan.draws.size(), n_sup = plan.support_key.size(), n_list = static_cast<size_t>(plan.n_list);
  const size_t n_keys = rows_key ? static_cast<size_t>(n_rows) : 0;
  dv::Layout up;
  // upload image: draws | row keys | support keys | support alts
  const size_t u_draws = up.add(n_draws * sizeof(Draw));
  const size_t u_key = up.add(n_keys * sizeof(int32_t));
  const size_t u_skey = up.add(n_sup * sizeof(int32_t));
  const size_t u_salt = up.add(n_sup);
  static thread_local dv::RoundTrip rt;
  // as in pack_on_device: the kernel of this thread's previous call reads the staging that this call refills
  static thread_local hipEvent_t previous_pack = nullptr;
  if (previous_pack) (void)hipEventSynchronize(previous_pack);
  if (int rc = rt.begin("dv_pack_draws_device: no HIP device", stream_in, up.bytes(), 0, 0)) return rc;
  std::memcpy(rt.host_up<Draw>(u_draws), plan.draws.data(), n_draws * sizeof(Draw));
  if (n_keys) std::memcpy(rt.host_up<int32_t>(u_key), rows_key, n_keys * sizeof(int32_t));
  if (n_sup) {
    std::memcpy(rt.host_up<int32_t>(u_skey), plan.support_key.data(), n_sup * sizeof(int32_t));
    std::memcpy(rt.host_up<uint8_t>(u_salt), plan.support_alt.data(), n_sup);
  }
  DrawInputs in;
  in.draws = rt.dev_up<const Draw>(u_draws);
  in.rows_key = n_keys ? rt.dev_up<const int32_t>(u_key) : nullptr;
  in.support_key = rt.dev_up<const int32_t>(u_skey);
  in.support_alt = rt.dev_up<const uint8_t>(u_salt);
  in.n_draws = static_cast<uint32_t>(n_draws);
  in.n_list = static_cast<uint32_t>(n_list);
  hipStream_t stream = rt.stream();
  const Sections s(n_draws, n_list);
  DV_HIP_CHECK(hipGetDevice(&res->device_id));
  DV_HIP_CHECK(hipMalloc(&res->device, s.bytes));
  DV_HIP_CHECK(hipEventCreateWithFlags(&res->emitted, hipEventDisableTiming));
  uint8_t* base = static_cast<uint8_t*>(res->device);
  Outputs o;
  o.item_variant_start = reinterpret_cast<int32_t*>(base + s.ivs);
  o.item_image_start = reinterpret_cast<int32_t*>(base + s.iis);
  o.item_ref_idx = reinterpret_cast<uint32_t*>(base + s.iri);
  o.item_list_off = reinterpret_cast<uint32_t*>(base + s.ilo);
  o.item_height = reinterpret_cast<uint16_t*>(base + s.ih);
  o.item_out_off = reinterpret_cast<uint64_t*>(base + s.ioo);
  o.item_mean_coverage = reinterpret_cast<float*>(base + s.imc);
  o.list_read = reinterpret_cast<uint32_t*>(base + s.lr);
  o.list_code = base + s.lc;
  o.list_group = base + s.lg;
  if (int rc = rt.upload(up.bytes())) return rc;
  {
    dv::ProfileScope prof(dv::kProfOther, stream);
    const unsigned blocks = static_cast<unsigned>((n_draws + kWaves - 1) / kWaves);
    hipLaunchKernelGGL(pack_draws_kernel, dim3(blocks), dim3(kThreads), 0, stream, in, o);
    DV_HIP_CHECK(hipGetLastError());
  }
  stats->launches += 1;
  DV_HIP_CHECK(hipEventRecord(res->emitted, stream));
  if (!previous_pack) DV_HIP_CHECK(hipEventCreateWithFlags(&previous_pack, hipEventDisableTiming));
  DV_HIP_CHECK(hipEventRecord(previous_pack, stream));
  if (!stream_in) DV_HIP_CHECK(hipStreamSynchronize(stream));   // nobody else can order work behind the library's stream
  return DV_OK;
}

}  // namespace

extern "C" {

int dv_pack_regions_device(int32_t n_regions, const dv_pack_region_slice* regions, const dv_pack_rows* rows,
                           const dv_pack_regions_options* opt, const dv_pack_candidate* cands,
                           const uint32_t* combo_masks, const int32_t* support_key, const uint8_t* support_alt,
                           void* stream, dv_packed_regions** out) {
  return dv::guarded("dv_pack_regions_device", [&]() -> int {
    last_stats() = dv_pack_device_stats{0, 0, 0, 0, 0, 0};
    if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_pack_regions_device: null out");
    *out = nullptr;
    Plan plan;
    if (int rc = parse(n_regions, regions, rows, opt, cands, combo_masks, support_key, support_alt, &plan)) return rc;
    auto res = std::make_unique<dv_packed_regions>();
    res->item_candidate = plan.item_candidate;
    res->item_combo = plan.item_combo;
    dv_pack_device_stats& stats = last_stats();
    stats.regions = n_regions;
    stats.candidates = opt->n_candidates;
    stats.regions_unsorted = plan.unsorted;
    if (plan.item_candidate.size() > static_cast<size_t>(INT32_MAX)) {
      return dv::fail(DV_ERR_BAD_INPUT, "dv_pack_regions_device: more than 2^31 - 1 items; pass fewer regions");
    }
    if (!plan.item_candidate.empty()) {      // otherwise nothing to launch
      if (int rc = pack_on_device(plan, rows, opt, combo_masks, stream, res.get(), &stats)) return rc;
    }
    *out = res.release();
    return DV_OK;
  });
}

int dv_pack_draws_device(const int32_t* rows_key, int32_t n_rows, const dv_pack_draw* draws, int64_t n_draws,
                         const dv_pack_candidate* cands, int32_t n_cands, const int32_t* support_key,
                         const uint8_t* support_alt, uint32_t n_support, void* stream, dv_packed_regions** out) {
  return dv::guarded("dv_pack_draws_device", [&]() -> int {
    last_draws_stats() = dv_pack_draws_stats{0, 0, 0, 0};
    if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_pack_draws_device: null out");
    *out = nullptr;
    DrawPlan plan;
    if (int rc = parse_draws(n_rows, draws, n_draws, cands, n_cands, support_key, support_alt, n_support, &plan)) return rc;
    auto res = std::make_unique<dv_packed_regions>();      // frees its allocation and event on every error exit
    res->item_candidate.resize(plan.draws.size());
    res->item_combo.resize(plan.draws.size());
    for (size_t d = 0; d < plan.draws.size(); ++d) {
      res->item_candidate[d] = draws[d].cand;
      res->item_combo[d] = draws[d].combo_mask;
    }
    dv_pack_draws_stats& stats = last_draws_stats();
    stats.draws = n_draws;
    stats.candidates = n_cands;
    stats.list_entries = static_cast<int64_t>(plan.n_list);
    if (!plan.draws.empty()) {               // otherwise nothing to launch
      if (int rc = pack_draws_on_device(plan, rows_key, n_rows, stream, res.get(), &stats)) return rc;
    }
    res->n_list = static_cast<uint32_t>(plan.n_list);
    res->max_list_len = plan.max_list_len;
    *out = res.release();
    return DV_OK;
  });
}

int dv_pack_draws_device_last_stats(dv_pack_draws_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_pack_draws_device_last_stats: null");
  *out = last_draws_stats();
  return DV_OK;
}

int dv_packed_regions_fill_batch(const dv_packed_regions* p, int use_groups, dv_batch* b) {
  if (!p || !b) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_packed_regions_fill_batch: null");
  if (b->memory != DV_MEM_DEVICE) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_packed_regions_fill_batch: the batch must be in device memory");
  const size_t n_items = p->item_candidate.size();
  b->n_items = static_cast<int32_t>(n_items);
  b->n_list = p->n_list;
  b->max_list_len = p->max_list_len;
  b->item_blank_mask = nullptr;
  const uint8_t* base = static_cast<const uint8_t*>(p->device);
  if (!base) {
    b->item_variant_start = b->item_image_start = nullptr;
    b->item_ref_idx = b->item_list_off = nullptr;
    b->item_height = nullptr;
    b->item_out_off = nullptr;
    b->item_mean_coverage = nullptr;
    b->list_read = nullptr;
    b->list_code = b->list_group = nullptr;
    return DV_OK;
  }
  const Sections s(n_items, p->n_list);
  b->item_variant_start = reinterpret_cast<const int32_t*>(base + s.ivs);
  b->item_image_start = reinterpret_cast<const int32_t*>(base + s.iis);
  b->item_ref_idx = reinterpret_cast<const uint32_t*>(base + s.iri);
  b->item_list_off = reinterpret_cast<const uint32_t*>(base + s.ilo);
  b->item_height = reinterpret_cast<const uint16_t*>(base + s.ih);
  b->item_out_off = reinterpret_cast<const uint64_t*>(base + s.ioo);
  b->item_mean_coverage = reinterpret_cast<const float*>(base + s.imc);
  b->list_read = reinterpret_cast<const uint32_t*>(base + s.lr);
  b->list_code = base + s.lc;
  b->list_group = use_groups ? base + s.lg : nullptr;
  return DV_OK;
}

int dv_packed_regions_download(dv_packed_regions* p, dv_packed_regions_view* out) {
  if (!p || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_packed_regions_download: null");
  const size_t n_items = p->item_candidate.size();
  const Sections s(n_items, p->n_list);
  if (!p->downloaded) {
    p->host.assign(s.bytes, 0);      // an empty handle: item_list_off = {0}
    if (p->device) {
      DV_HIP_CHECK(hipEventSynchronize(p->emitted));
      DV_HIP_CHECK(hipMemcpy(p->host.data(), p->device, s.bytes, hipMemcpyDeviceToHost));
    }
    p->downloaded = true;
  }
  const uint8_t* base = p->host.data();
  out->n_items = static_cast<int32_t>(n_items);
  out->n_list = p->n_list;
  out->max_list_len = p->max_list_len;
  out->item_variant_start = reinterpret_cast<const int32_t*>(base + s.ivs);
  out->item_image_start = reinterpret_cast<const int32_t*>(base + s.iis);
  out->item_ref_idx = reinterpret_cast<const uint32_t*>(base + s.iri);
  out->item_list_off = reinterpret_cast<const uint32_t*>(base + s.ilo);
  out->item_height = reinterpret_cast<const uint16_t*>(base + s.ih);
  out->item_out_off = reinterpret_cast<const uint64_t*>(base + s.ioo);
  out->item_mean_coverage = reinterpret_cast<const float*>(base + s.imc);
  out->item_candidate = p->item_candidate.data();
  out->item_combo = p->item_combo.data();
  out->list_read = reinterpret_cast<const uint32_t*>(base + s.lr);
  out->list_code = base + s.lc;
  out->list_group = base + s.lg;
  return DV_OK;
}

int dv_packed_regions_items(const dv_packed_regions* p, const int32_t** item_candidate, const uint32_t** item_combo) {
  if (!p) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_packed_regions_items: null");
  if (item_candidate) *item_candidate = p->item_candidate.data();
  if (item_combo) *item_combo = p->item_combo.data();
  return static_cast<int>(p->item_candidate.size());
}

void dv_packed_regions_free(dv_packed_regions* p) { delete p; }

int dv_pack_regions_device_last_stats(dv_pack_device_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_pack_regions_device_last_stats: null");
  *out = last_stats();
  return DV_OK;
}

}  // extern "C"
