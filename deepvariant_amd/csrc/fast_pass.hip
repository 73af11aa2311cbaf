// fast_pass.hip -- the fast pass of FastPassAligner (fast_pass_aligner.cpp: build_index +
// fast_align_reads_to_haplotype) for every (window, haplotype) of a batch in one kernel launch, and the C
// entry points dv_fast_pass_batch / dv_fast_pass_batch_device.
//
// Contract: include/dvhip.h, "the fast pass over many windows in one call".  The host code walks the haplotype,
// looks every k-mer up in a hash map of the reads' k-mers, tries the read at the start the hit implies and stops at
// the first position no read covers.  Its result does not depend on that order: a (read, start) is tried exactly when
// some k-mer of the read equals the haplotype's k-mer on a diagonal that names the start, the first such hit in the
// walk -- the smallest (i, off) -- decides ties between equal scores (a later start replaces the read's alignment
// only with a strictly larger score) and where the coverage the hole test sees begins, and a position's coverage is
// final by the time the walk tests it, because every start that covers position i is discovered at a position <= i.
// The walk tests a position for coverage only after its k-mer was found in the index.
// So the k-mer index is not needed here: lanes compare bytes along diagonals.
//
// Shape: one workgroup of four waves per (window, haplotype); the haplotype's bytes and a bitmap of its covered
// positions live in LDS; the waves take the window's reads in turn.  Per read the lanes own the diagonals
// d = start = 0 .. n - L, 64 at a time, and step along the read: the read's byte is wave-uniform (a 64-byte register
// chunk, readlane), the haplotype's byte is hap[d + p].  A lane keeps the current run of equal bytes -- the first time
// it reaches k is the diagonal's first seed, off = p - k + 1 -- and the mismatch count with 'N' as a wildcard; the
// chunk stops as soon as every lane is past M mismatches, which on unrelated sequence is after a few bytes.  Start 0
// is also named by seeds on the negative diagonals (the host clamps i - off at 0): they are walked only when
// start 0 is within M mismatches, for the smallest (i, off) alone.  An accepted start ORs [key.i, start + L) into
// the bitmap (LDS atomics); the lanes' (score, key, start) are reduced with __shfl_xor, largest score then smallest
// key, and lane 0 stores the read's row.  After a barrier the workgroup applies the hole rule: the host tests a
// position only where the haplotype's k-mer is in its index, so the uncovered positions of the tested range -- usually
// none -- are compared against every k-mer of every read longer than k, 64 positions per wave at a time, until one is
// found.  Thread 0 stores the haplotype's score and discarded flag.
//
// Host side: one upload image, one launch, one download image per call; their layouts and the calling thread's
// buffers and stream are device_round_trip.h's (Layout, RoundTrip).
#include <algorithm>
#include <cctype>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

#include "device_round_trip.h"
#include "fast_pass_aligner.h"
#include "fast_pass_device.h"

static_assert(sizeof(dv_fast_pass_stats) == 40, "dv_fast_pass_stats layout");
static_assert(sizeof(dv_fast_pass_window) == 32, "dv_fast_pass_window layout");

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kCap = dv::kFastPassMaxHaplotype;
constexpr int kNoKey = INT_MAX;
static_assert(kCap % 32 == 0 && kCap <= (1 << 15), "a discovery key is (i << 16) | off in a positive int");

struct Item {            // one (window, haplotype) of the launch
  int32_t hap_off, n;    // its bytes in the table
  int32_t first_read, n_reads;   // the window's reads in the read offset table
  int32_t first_row;     // its reads' rows in the output
  int32_t lo, hi;        // the hole rule tests positions [lo, hi)
  int32_t is_ref;
};

struct Params {
  int k, max_mismatches, match, mismatch;
};

__device__ void cover_range(uint32_t* cover, int a, int b) {   // [a, b), a < b
  for (int w = a >> 5; w <= (b - 1) >> 5; ++w) {
    const int lo = max(a - w * 32, 0), hi = min(b - w * 32, 32);
    const uint32_t below_hi = hi == 32 ? 0xffffffffu : (1u << hi) - 1u;
    atomicOr(&cover[w], below_hi & ~((1u << lo) - 1u));
  }
}

// wave-uniform: this wave has found a hole, or some wave of the workgroup has said so
__device__ bool found_any(const int* hole, bool found) {
  return __any(found) || *reinterpret_cast<const volatile int*>(hole) != 0;
}

__global__ __launch_bounds__(kThreads) void fast_pass_kernel(const uint8_t* __restrict__ bytes,
                                                             const int32_t* __restrict__ read_off,
                                                             const Item* __restrict__ items, const Params prm,
                                                             int2* __restrict__ rows, int2* __restrict__ hap_out) {
  __shared__ uint8_t hap[kCap];
  __shared__ uint32_t cover[kCap / 32];
  __shared__ int total, hole;
  const Item it = items[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = it.n, k = prm.k, M = prm.max_mismatches;
  for (int x = tid; x < n; x += kThreads) hap[x] = bytes[it.hap_off + x];
  for (int x = tid; x < (n + 31) / 32; x += kThreads) cover[x] = 0;
  if (tid == 0) {
    total = 0;
    hole = 0;
  }
  __syncthreads();

  for (int r = wave; r < it.n_reads; r += kWaves) {
    const int r0 = __builtin_amdgcn_readfirstlane(read_off[it.first_read + r]);
    const int L = __builtin_amdgcn_readfirstlane(read_off[it.first_read + r + 1]) - r0;
    const uint8_t* rp = bytes + r0;
    int2* row = rows + it.first_row + r;
    if (L <= k || L > n) {
      if (lane == 0) *row = make_int2(-1, 0);
      continue;
    }
    int best_score = 0, best_key = kNoKey, best_s = -1;
    int mm0 = M + 1, key0 = kNoKey;            // start 0: decided after the negative diagonals
    const int n_starts = n - L + 1;
    for (int base = 0; base < n_starts; base += 64) {
      const int d = base + lane;
      const bool active = d < n_starts;
      const uint8_t* hp = hap + (active ? d : 0);
      int run = 0, off = -1, chunk = 0;
      int mm = active ? 0 : M + 1;
      for (int p = 0; p < L; ++p) {
        if ((p & 63) == 0) chunk = p + lane < L ? rp[p + lane] : 0;
        const int rb = __builtin_amdgcn_readlane(chunk, p & 63);
        const int hb = hp[p];
        const bool eq = hb == rb;
        run = eq ? run + 1 : 0;
        if (run == k && off < 0) off = p - k + 1;
        mm += (!eq && hb != 'N' && rb != 'N') ? 1 : 0;
        if ((p & 7) == 7 && !__any(mm <= M)) break;     // nobody can be accepted any more
      }
      if (base == 0) {
        mm0 = __shfl(mm, 0);
        const int off0 = __shfl(off, 0);
        key0 = off0 >= 0 ? ((off0 << 16) | off0) : kNoKey;
      }
      if (active && d > 0 && off >= 0 && mm <= M) {
        const int i = d + off;
        cover_range(cover, i, d + L);
        const int score = (L - mm) * prm.match - mm * prm.mismatch;
        const int key = (i << 16) | off;
        if (score > best_score || (score == best_score && best_s >= 0 && key < best_key)) {
          best_score = score;
          best_key = key;
          best_s = d;
        }
      }
    }
    if (mm0 <= M) {
      // seeds on the negative diagonals -j: H[i] against R[i + j]
      int kmin = key0;
      const int n_neg = L - k;
      for (int base = 0; base < n_neg; base += 64) {
        const int j = base + lane + 1;
        const bool active = j <= n_neg;
        int run = 0, found = kNoKey, chunk = 0;
        for (int p = 0; p < L; ++p) {
          if ((p & 63) == 0) chunk = p + lane < L ? rp[p + lane] : 0;
          const int rb = __builtin_amdgcn_readlane(chunk, p & 63);
          const int h = p - j;
          const bool valid = active && h >= 0;
          const int hb = hap[valid ? h : 0];
          run = valid && hb == rb ? run + 1 : 0;
          if (run == k && found == kNoKey) found = ((h - k + 1) << 16) | (p - k + 1);
        }
        kmin = min(kmin, found);
      }
      for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, __shfl_xor(kmin, o));
      if (kmin != kNoKey && lane == 0) {
        cover_range(cover, kmin >> 16, L);
        const int score = (L - mm0) * prm.match - mm0 * prm.mismatch;
        if (score > best_score || (score == best_score && best_s >= 0 && kmin < best_key)) {
          best_score = score;
          best_key = kmin;
          best_s = 0;
        }
      }
    }
    // largest score, then smallest discovery key
    for (int o = 32; o > 0; o >>= 1) {
      const int os = __shfl_xor(best_score, o), ok = __shfl_xor(best_key, o), op = __shfl_xor(best_s, o);
      if (os > best_score || (os == best_score && ok < best_key)) {
        best_score = os;
        best_key = ok;
        best_s = op;
      }
    }
    if (lane == 0) {
      *row = make_int2(best_s, best_s >= 0 ? best_score : 0);
      if (best_s >= 0) atomicAdd(&total, best_score);
    }
  }
  __syncthreads();
  // The hole rule.  The host tests a position only where the haplotype's k-mer is in its index, i.e. occurs in some
  // read longer than k (any such read: one longer than the haplotype is indexed too).  Lanes own the uncovered
  // positions of [lo, hi), 64 at a time, and every (read, offset) is compared against all of them at once: the
  // read's bytes are wave-uniform, the comparison goes on while some lane still matches.
  if (!it.is_ref) {
    for (int base = it.lo + 64 * wave; base < it.hi; base += 64 * kWaves) {
      const int i = base + lane;
      const bool open = i < it.hi && ((cover[i >> 5] >> (i & 31)) & 1u) == 0;
      if (!__any(open)) continue;
      const uint8_t* hp = hap + (open ? i : 0);      // i + k <= n for every tested position
      bool found = false;
      for (int r = 0; r < it.n_reads && !found_any(&hole, found); ++r) {
        const int r0 = __builtin_amdgcn_readfirstlane(read_off[it.first_read + r]);
        const int L = __builtin_amdgcn_readfirstlane(read_off[it.first_read + r + 1]) - r0;
        if (L <= k) continue;
        const uint8_t* rp = bytes + r0;
        for (int off = 0; off + k <= L; ++off) {
          bool same = open;
          for (int q = 0; q < k && __any(same); ++q) same = same && hp[q] == rp[off + q];
          found = found || same;
        }
      }
      if (found) hole = 1;
    }
  }
  __syncthreads();
  if (tid == 0) hap_out[blockIdx.x] = make_int2(hole ? 0 : total, hole);
}

// the positions [lo, hi) the hole rule tests, with the host's unsigned arithmetic: a suffix longer than the
// haplotype wraps and excludes nothing
void hole_range(int n, int k, int prefix, int suffix, int* lo, int* hi) {
  const int end = suffix > n ? n : n - suffix;
  *lo = std::max(prefix, 0);
  *hi = std::max(*lo, std::min(end, n - k + 1));
}

void host_haplotypes(const dv::FastPassWindow& w, const dv::FastPassScoring& sc, const std::vector<size_t>& which,
                     size_t first_haplotype, dv::FastPassResults* out) {
  if (which.empty()) return;
  dv::FastPassAligner a;
  dv::AlignerOptions ao;
  ao.kmer_size = sc.kmer_size;
  ao.max_num_of_mismatches = sc.max_num_of_mismatches;
  ao.match = sc.match;
  ao.mismatch = sc.mismatch;
  std::string error;
  (void)a.set_options(ao, &error);        // resolved values of a class that accepted them
  a.set_ref_prefix_len(w.ref_prefix_len);
  a.set_ref_suffix_len(w.ref_suffix_len);
  std::vector<std::string> reads;
  reads.reserve(w.reads.size());
  for (std::string_view r : w.reads) reads.emplace_back(r);
  a.set_reads(reads);
  a.build_index();
  if (w.has_reference) a.set_reference(std::string(w.reference));
  std::vector<dv::ReadAlignment> ra(reads.size());
  for (size_t h : which) {
    for (dv::ReadAlignment& x : ra) x.reset();
    int score = 0;
    bool discarded = false;
    const std::string_view hap = w.haplotypes[h];
    // without a reference the class's own is empty: only an empty haplotype equals it, and that one has no positions
    a.fast_align_reads_to_haplotype(hap, &score, &ra, &discarded);
    const size_t g = first_haplotype + h;
    out->haplotype_score[g] = score;
    out->haplotype_discarded[g] = discarded ? 1 : 0;
    for (size_t r = 0; r < ra.size(); ++r) {
      const size_t row = static_cast<size_t>(out->first_row[g]) + r;
      const bool placed = score != 0 && ra[r].position != dv::ReadAlignment::kNotAligned;
      out->read_position[row] = placed ? ra[r].position : -1;
      out->read_score[row] = placed ? ra[r].score : 0;
    }
  }
}

void size_results(const std::vector<dv::FastPassWindow>& windows, dv::FastPassResults* out) {
  out->first_row.assign(1, 0);
  for (const dv::FastPassWindow& w : windows) {
    for (size_t h = 0; h < w.haplotypes.size(); ++h) {
      out->first_row.push_back(out->first_row.back() + static_cast<int64_t>(w.reads.size()));
    }
  }
  const size_t n_haps = out->first_row.size() - 1, n_rows = static_cast<size_t>(out->first_row.back());
  out->haplotype_score.assign(n_haps, 0);
  out->haplotype_discarded.assign(n_haps, 0);
  out->read_position.assign(n_rows, -1);
  out->read_score.assign(n_rows, 0);
}

}  // namespace

namespace dv {

FastPassStats& last_fast_pass_stats() {
  static thread_local FastPassStats stats;
  return stats;
}

bool device_fast_pass_enabled() { return env_switch("DV_REALIGN_DEVICE_FASTPASS", false); }

void fast_pass_on_host(const std::vector<FastPassWindow>& windows, const FastPassScoring& sc, FastPassResults* out) {
  size_results(windows, out);
  size_t first = 0;
  for (const FastPassWindow& w : windows) {
    std::vector<size_t> all(w.haplotypes.size());
    for (size_t h = 0; h < all.size(); ++h) all[h] = h;
    host_haplotypes(w, sc, all, first, out);
    first += w.haplotypes.size();
  }
}

int fast_pass_on_device(const std::vector<FastPassWindow>& windows, const FastPassScoring& sc, void* stream_in,
                        FastPassResults* out, FastPassStats* stats) {
  size_results(windows, out);
  const bool scoring_fits = sc.match >= 0 && sc.mismatch >= 0 && sc.match <= kFastPassMaxScoring &&
                            sc.mismatch <= kFastPassMaxScoring && sc.kmer_size >= 1 && sc.max_num_of_mismatches >= 0;
  // upload image: items | read offsets | bytes (the reads of every window with device work, then the haplotypes)
  std::vector<Item> items;
  std::vector<size_t> item_haplotype;                 // the call's haplotype of each item
  std::vector<std::string_view> item_bytes;
  std::vector<int32_t> read_off(1, 0);
  std::vector<std::string_view> pieces;               // the byte table, in order
  std::vector<std::vector<size_t>> on_host(windows.size());
  int64_t n_bytes = 0, n_rows = 0, cells = 0, pairs = 0, host_count = 0, n_haps = 0;
  size_t first = 0;
  for (size_t wi = 0; wi < windows.size(); ++wi) {
    const FastPassWindow& w = windows[wi];
    int32_t first_read = -1;
    for (size_t h = 0; h < w.haplotypes.size(); ++h) {
      ++n_haps;
      const std::string_view hap = w.haplotypes[h];
      if (!scoring_fits || hap.size() > static_cast<size_t>(kCap)) {
        on_host[wi].push_back(h);
        ++host_count;
        continue;
      }
      if (first_read < 0) {
        first_read = static_cast<int32_t>(read_off.size() - 1);
        for (std::string_view r : w.reads) {
          pieces.push_back(r);
          n_bytes += static_cast<int64_t>(r.size());
          read_off.push_back(static_cast<int32_t>(n_bytes));
        }
      }
      Item it;
      it.hap_off = 0;        // set once the reads are all in
      it.n = static_cast<int32_t>(hap.size());
      it.first_read = first_read;
      it.n_reads = static_cast<int32_t>(w.reads.size());
      it.first_row = static_cast<int32_t>(n_rows);
      hole_range(it.n, sc.kmer_size, w.ref_prefix_len, w.ref_suffix_len, &it.lo, &it.hi);
      it.is_ref = w.has_reference && hap == w.reference ? 1 : 0;
      items.push_back(it);
      item_haplotype.push_back(first + h);
      item_bytes.push_back(hap);
      n_rows += it.n_reads;
      for (std::string_view r : w.reads) {
        const int64_t len = static_cast<int64_t>(r.size());
        if (len > sc.kmer_size && len <= it.n) {
          ++pairs;
          cells += (it.n - sc.kmer_size + 1) * len;
        }
      }
      if (n_bytes >= (int64_t{1} << 30) || n_rows >= (int64_t{1} << 30)) {
        return fail(DV_ERR_INVALID_ARGUMENT, "fast pass: more than 1 GiB of sequence or 2^30 rows in one call");
      }
    }
    first += w.haplotypes.size();
  }
  // the haplotypes follow the reads in the table
  for (size_t x = 0; x < items.size(); ++x) {
    pieces.push_back(item_bytes[x]);
    items[x].hap_off = static_cast<int32_t>(n_bytes);
    n_bytes += items[x].n;
    if (n_bytes >= (int64_t{1} << 30)) {
      return fail(DV_ERR_INVALID_ARGUMENT, "fast pass: more than 1 GiB of sequence in one call");
    }
  }
  if (stats) {
    stats->haplotypes += n_haps;
    stats->haplotypes_on_host += host_count;
    stats->pairs += pairs;
    stats->cells += cells;
  }
  if (!items.empty()) {
    // the heaviest haplotypes first: early workgroups start first
    std::vector<size_t> order(items.size());
    for (size_t x = 0; x < order.size(); ++x) order[x] = x;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      return static_cast<int64_t>(items[a].n) * items[a].n_reads > static_cast<int64_t>(items[b].n) * items[b].n_reads;
    });
    const size_t n_items = items.size();
    Layout up, down;
    const size_t o_items = up.add(n_items * sizeof(Item));
    const size_t o_off = up.add(read_off.size() * sizeof(int32_t));
    const size_t o_bytes = up.add(static_cast<size_t>(n_bytes));
    // download image: a row per (item, read) | a (score, discarded) per item
    const size_t o_rows = down.add(static_cast<size_t>(n_rows) * sizeof(int2));
    const size_t o_haps = down.add_last(n_items * sizeof(int2));
    static thread_local RoundTrip rt;
    if (int rc = rt.begin("fast pass: no HIP device (the device route has no CPU fallback)", stream_in, up.bytes(),
                          down.bytes(), 0)) {
      return rc;
    }
    Item* up_items = rt.host_up<Item>(o_items);
    for (size_t x = 0; x < n_items; ++x) up_items[x] = items[order[x]];
    std::memcpy(rt.host_up<int32_t>(o_off), read_off.data(), read_off.size() * sizeof(int32_t));
    uint8_t* at = rt.host_up<uint8_t>(o_bytes);
    for (std::string_view p : pieces) {
      std::memcpy(at, p.data(), p.size());
      at += p.size();
    }
    if (int rc = rt.upload(up.bytes())) return rc;
    {
      ProfileScope prof(kProfOther, rt.stream());
      const Params prm{sc.kmer_size, sc.max_num_of_mismatches, sc.match, sc.mismatch};
      hipLaunchKernelGGL(fast_pass_kernel, dim3(static_cast<unsigned>(n_items)), dim3(kThreads), 0, rt.stream(),
                         rt.dev_up<const uint8_t>(o_bytes), rt.dev_up<const int32_t>(o_off),
                         rt.dev_up<const Item>(o_items), prm, rt.dev_down<int2>(o_rows), rt.dev_down<int2>(o_haps));
      DV_HIP_CHECK(hipGetLastError());
    }
    if (int rc = rt.finish(down.bytes())) return rc;
    if (stats) stats->launches += 1;
    const int2* rows = rt.host_down<int2>(o_rows);
    const int2* haps = rt.host_down<int2>(o_haps);
    for (size_t x = 0; x < n_items; ++x) {
      const Item& it = items[order[x]];
      const size_t g = item_haplotype[order[x]];
      const bool discarded = haps[x].y != 0;
      const int score = discarded ? 0 : haps[x].x;
      out->haplotype_score[g] = score;
      out->haplotype_discarded[g] = discarded ? 1 : 0;
      if (score == 0) continue;         // the rows stay reset, as fast_align_reads_to_haplotypes leaves them
      for (int32_t r = 0; r < it.n_reads; ++r) {
        const int2 v = rows[it.first_row + r];
        const size_t row = static_cast<size_t>(out->first_row[g]) + r;
        out->read_position[row] = v.x;
        out->read_score[row] = v.x >= 0 ? v.y : 0;
      }
    }
  }
  first = 0;
  for (size_t wi = 0; wi < windows.size(); ++wi) {
    host_haplotypes(windows[wi], sc, on_host[wi], first, out);
    first += windows[wi].haplotypes.size();
  }
  return DV_OK;
}

}  // namespace dv

namespace {

struct Batch {           // a call's arguments as windows; `upper` backs the reads
  std::string upper;
  std::vector<dv::FastPassWindow> windows;
  dv::FastPassScoring scoring;
  size_t n_haplotypes = 0;
};

int parse(const char* who, int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
          const dv_fast_pass_window* windows, const dv_aligner_options* o, const int32_t* haplotype_score,
          const int32_t* haplotype_discarded, const int32_t* read_position, const int32_t* read_score, Batch* b) {
  const std::string name(who);
  if (n_seqs < 0 || n_windows < 0 || (n_seqs > 0 && !seq_off) || (n_windows > 0 && !windows)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer or negative count");
  }
  if (int rc = dv::check_sequence_table(name, n_seqs, seq_off)) return rc;
  if (n_seqs > 0 && seq_off[n_seqs] > seq_off[0] && !bytes) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null bytes");
  dv::AlignerOptions ao;
  if (o) {
    ao.match = o->match;
    ao.mismatch = o->mismatch;
    ao.kmer_size = o->kmer_size;
    ao.max_num_of_mismatches = o->max_num_of_mismatches;
  }
  dv::FastPassAligner resolved;
  std::string error;
  if (!resolved.set_options(ao, &error)) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": " + error);
  b->scoring = dv::FastPassScoring{resolved.kmer_size(), resolved.max_num_of_mismatches(), resolved.match(),
                                   resolved.mismatch()};
  int64_t n_rows = 0;
  for (int32_t w = 0; w < n_windows; ++w) {
    const dv_fast_pass_window& win = windows[w];
    if (win.n_reads < 0 || win.n_haplotypes < 0 || win.first_read < 0 || win.first_haplotype < 0 ||
        static_cast<int64_t>(win.first_read) + win.n_reads > n_seqs ||
        static_cast<int64_t>(win.first_haplotype) + win.n_haplotypes > n_seqs || win.reference < -1 ||
        win.reference >= n_seqs || win.ref_prefix_len < 0 || win.ref_suffix_len < 0) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": a window's range, reference or padding is out of range");
    }
    for (int32_t h = 0; h < win.n_haplotypes; ++h) {
      if (seq_off[win.first_haplotype + h + 1] - seq_off[win.first_haplotype + h] >= 0xffff) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, "haplotypes are limited to 65534 bases (16-bit read offsets)");
      }
    }
    b->n_haplotypes += static_cast<size_t>(win.n_haplotypes);
    n_rows += static_cast<int64_t>(win.n_haplotypes) * win.n_reads;
  }
  if ((b->n_haplotypes > 0 && (!haplotype_score || !haplotype_discarded)) ||
      (n_rows > 0 && (!read_position || !read_score))) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null output array");
  }
  if (b->n_haplotypes == 0) return DV_OK;
  const int64_t base = seq_off[0];
  b->upper.assign(bytes + base, static_cast<size_t>(seq_off[n_seqs] - base));
  for (char& c : b->upper) c = static_cast<char>(std::toupper(static_cast<unsigned char>(c)));
  auto view = [&](const char* from, int32_t s) {
    return std::string_view(from + (seq_off[s] - base), static_cast<size_t>(seq_off[s + 1] - seq_off[s]));
  };
  for (int32_t w = 0; w < n_windows; ++w) {
    const dv_fast_pass_window& win = windows[w];
    dv::FastPassWindow fw;
    for (int32_t r = 0; r < win.n_reads; ++r) fw.reads.push_back(view(b->upper.data(), win.first_read + r));
    for (int32_t h = 0; h < win.n_haplotypes; ++h) fw.haplotypes.push_back(view(bytes + base, win.first_haplotype + h));
    fw.has_reference = win.reference >= 0;
    if (fw.has_reference) fw.reference = view(bytes + base, win.reference);
    fw.ref_prefix_len = win.ref_prefix_len;
    fw.ref_suffix_len = win.ref_suffix_len;
    b->windows.push_back(std::move(fw));
  }
  return DV_OK;
}

void copy_out(const dv::FastPassResults& res, int32_t* haplotype_score, int32_t* haplotype_discarded,
              int32_t* read_position, int32_t* read_score) {
  const size_t n_haps = res.haplotype_score.size(), n_rows = res.read_position.size();
  if (n_haps) {
    std::memcpy(haplotype_score, res.haplotype_score.data(), n_haps * sizeof(int32_t));
    std::memcpy(haplotype_discarded, res.haplotype_discarded.data(), n_haps * sizeof(int32_t));
  }
  if (n_rows) {
    std::memcpy(read_position, res.read_position.data(), n_rows * sizeof(int32_t));
    std::memcpy(read_score, res.read_score.data(), n_rows * sizeof(int32_t));
  }
}

}  // namespace

extern "C" {

int dv_fast_pass_batch(int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
                       const dv_fast_pass_window* windows, const dv_aligner_options* options, void* /*stream*/,
                       int32_t* haplotype_score, int32_t* haplotype_discarded, int32_t* read_position,
                       int32_t* read_score) {
  return dv::guarded("dv_fast_pass_batch", [&]() -> int {
    Batch b;
    if (int rc = parse("dv_fast_pass_batch", n_seqs, bytes, seq_off, n_windows, windows, options, haplotype_score,
                       haplotype_discarded, read_position, read_score, &b)) {
      return rc;
    }
    if (b.n_haplotypes == 0) return DV_OK;
    dv::FastPassResults res;
    dv::fast_pass_on_host(b.windows, b.scoring, &res);
    copy_out(res, haplotype_score, haplotype_discarded, read_position, read_score);
    return DV_OK;
  });
}

int dv_fast_pass_batch_device(int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
                              const dv_fast_pass_window* windows, const dv_aligner_options* options, void* stream,
                              int32_t* haplotype_score, int32_t* haplotype_discarded, int32_t* read_position,
                              int32_t* read_score) {
  return dv::guarded("dv_fast_pass_batch_device", [&]() -> int {
    dv::last_fast_pass_stats() = dv::FastPassStats();
    Batch b;
    if (int rc = parse("dv_fast_pass_batch_device", n_seqs, bytes, seq_off, n_windows, windows, options,
                       haplotype_score, haplotype_discarded, read_position, read_score, &b)) {
      return rc;
    }
    if (b.n_haplotypes == 0) return DV_OK;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
      return dv::fail(DV_ERR_NO_DEVICE, "dv_fast_pass_batch_device: no HIP device (dv_fast_pass_batch is the host code)");
    }
    dv::FastPassResults res;
    if (int rc = dv::fast_pass_on_device(b.windows, b.scoring, stream, &res, &dv::last_fast_pass_stats())) return rc;
    copy_out(res, haplotype_score, haplotype_discarded, read_position, read_score);
    return DV_OK;
  });
}

int dv_fast_pass_device_last_stats(dv_fast_pass_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_fast_pass_device_last_stats: null");
  const dv::FastPassStats& s = dv::last_fast_pass_stats();
  out->haplotypes = s.haplotypes;
  out->haplotypes_on_host = s.haplotypes_on_host;
  out->pairs = s.pairs;
  out->cells = s.cells;
  out->launches = s.launches;
  return DV_OK;
}

}  // extern "C"
