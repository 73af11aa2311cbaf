// Window trimming of reads on a packed read table: dv_trim_reads_batch (host code) and
// dv_trim_reads_batch_device (three kernels), include/dvhip.h.
//
// The contract -- TrimCigar / TrimRead / TrimReads (deepvariant/alt_aligned_pileup_lib.cc:91-248), restated in
// Python by alt_aligned_pileup_lib.trim_cigar / trim_read / trim_reads, which stay the checker -- in closed form.
//
// Inputs per pair.  A read at `pos` with packed CIGAR words w[0..n): operation w & 15 (nucleus' numbering), length
// w >> 4; operations 1, 3, 4, 8, 9 (M D N = X) advance the reference, 1, 2, 5, 8, 9 (M I S = X) the read.  For a
// window [r0, r1):
//   T = max(r0 - pos, 0)          reference bases to drop in front
//   C = r1 - max(r0, pos)         reference bases to cover at most
//   R[k], Q[k]                    reference / read bases consumed before operation k
// Errors (for the whole call, never a dropped read): C <= 0 (the reference's CHECK_GT), and
// read_trim + new_len > the read's sequence length.  The smallest offending (window, row) is reported.
// First kept operation a.  T == 0: a = 0, nothing is cut, leading S / I stay.  Otherwise a is the first k with
// R[k+1] > T or R[k] == T (the predicate is monotone in k); the operations before it are dropped whole, I / S among
// them, and their read bases count into read_trim.  R[a] < T: operation a is cut by T - R[a], its length becomes
// R[a+1] - T, and read_trim = Q[a] + (T - R[a] if it advances the read, else 0).  R[a] == T (an I sitting exactly
// where the prefix ends, say): kept whole, read_trim = Q[a].  No such a: the CIGAR is empty, read_trim = Q[n].
// Last kept operation b.  An operation k >= a is kept whole while R[k+1] - T <= C, so operations that do not
// advance the reference always fit (I / S after an exact fit are kept).  b is the first k >= a with
// R[k+1] - T > C (monotone again; b advances the reference); it is emitted with length C - (max(R[b], T) - T),
// which MAY BE 0, and the CIGAR ends there.  No such b: every remaining operation is kept.  When a == b the
// length is b's (= C).
// Outputs per kept read.  new_len = the kept lengths that advance the read; span = those that advance the
// reference; position r0 if T != 0, else pos; end = position + span.
// Filter.  The pair is kept iff span >= min_overlap and new_len > 0.
// Reads of a window.  Rows with q1 > read_pos && q0 < read_end, in row order; the table may be unsorted.  The same
// read appears once per window that keeps it; the output is ordered by (window, row).
//
// Kernels.  One wave per pair that passes the overlap test (the host lists the pairs while it fills the upload).
// The lanes take the CIGAR 64 operations at a time: a wave prefix sum of both advances, carried from chunk to
// chunk, then a and b from ballots over the two monotone predicates; the chunk loop ends at b.  Pass 1 (count)
// leaves a PairResult per pair; pass 2, one workgroup, is the exclusive scan of kept rows and words over the
// pairs in order; pass 3 (emit) writes each kept pair's row and copies its operations, lane 0 and the last lane
// patching the two cut lengths.  Placement is a pure function of the input (no atomics decide it); the one atomic
// is the minimum over the offending pairs for the error report.
//
// Host side: one upload image, the three launches, one download image per call; the layouts of the images and of
// the device-only work space, and the calling thread's buffers and stream, are device_round_trip.h's (Layout,
// RoundTrip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_round_trip.h"
#include "trim_reads.h"

namespace {

using dv::trim::Pair;
using dv::trim::PairResult;

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kScanThreads = 1024;
// one call's staging: pairs and the CIGAR operations they could write
constexpr int64_t kMaxPairs = int64_t{1} << 28;
constexpr int64_t kMaxWords = int64_t{1} << 28;

struct Header {          // the download's first bytes
  unsigned long long error;   // kNoError, or (pair << 2) | kind of the smallest offending pair
  int32_t n_rows, n_words;
};

struct Tables {          // device pointers into the upload
  const int32_t* read_pos;
  const uint32_t* seq_len;
  const uint32_t* cigar_off;
  const uint32_t* cigar;
  const dv_trim_window* windows;
  const Pair* pairs;
  const int32_t* window_pair_off;   // [n_windows + 1]
  int32_t n_pairs, n_windows;
};

struct Outputs {         // device pointers into the download; row arrays hold n_pairs entries, words `bound`
  Header* header;
  int32_t* window_row_off;
  int32_t *src_row, *pos, *end, *read_trim, *new_len;
  uint32_t* cigar_off;
  uint32_t* cigar;
};

__device__ __forceinline__ long long wave_inclusive_scan(long long v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const long long up = __shfl_up(v, d, kWave);
    if (lane >= d) v += up;
  }
  return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}

// Pass 1: the closed form for one pair per wave.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void trim_count_kernel(Tables t, PairResult* results,
                                                                           unsigned long long* error) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long pair = static_cast<long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (pair >= t.n_pairs) return;                       // the whole wave
  const Pair pr = t.pairs[pair];
  const dv_trim_window win = t.windows[pr.window];
  const long long pos = t.read_pos[pr.row];
  const long long T = win.r0 > pos ? win.r0 - pos : 0;
  const long long C = win.r1 - (win.r0 > pos ? win.r0 : pos);
  PairResult res{0, -1, 0, 0, 0, -1, -1, 0};
  if (C <= 0) {
    if (lane == 0) {
      atomicMin(error, (static_cast<unsigned long long>(pair) << 2) | dv::trim::kErrCover);
      results[pair] = res;
    }
    return;
  }
  const uint32_t c0 = t.cigar_off[pr.row];
  const uint32_t n = t.cigar_off[pr.row + 1] - c0;
  long long r_carry = 0, q_carry = 0;      // R / Q at the chunk's first operation
  long long read_trim = 0;
  long long q_kept = 0, r_kept = 0;        // per lane; summed over the wave at the end
  int a = -1, b = -1, len_a = -1, len_b = -1;
  for (uint32_t base = 0; base < n; base += kWave) {
    const uint32_t k = base + lane;
    const bool valid = k < n;
    const uint32_t word = valid ? t.cigar[c0 + k] : 0u;
    const uint32_t op = word & 15u;
    const long long length = word >> 4;
    const bool on_ref = valid && ((dv::trim::kRefAdvancing >> op) & 1u);
    const bool on_read = valid && ((dv::trim::kReadAdvancing >> op) & 1u);
    const long long ra = on_ref ? length : 0, qa = on_read ? length : 0;
    const long long r_incl = wave_inclusive_scan(ra, lane), q_incl = wave_inclusive_scan(qa, lane);
    const long long r1 = r_carry + r_incl, r0 = r1 - ra;     // R[k+1], R[k]
    const long long q0 = q_carry + q_incl - qa;              // Q[k]
    if (a < 0) {
      const unsigned long long m = __ballot(valid && (T == 0 || r1 > T || r0 == T));
      if (m) {
        const int la = __ffsll(static_cast<long long>(m)) - 1;
        a = static_cast<int>(base) + la;
        const long long r0a = __shfl(r0, la, kWave), r1a = __shfl(r1, la, kWave), q0a = __shfl(q0, la, kWave);
        const int read_a = __shfl(static_cast<int>(on_read), la, kWave);
        read_trim = q0a;
        if (r0a < T) {                       // T > 0 and the prefix ends inside operation a
          len_a = static_cast<int>(r1a - T);
          if (read_a) read_trim += T - r0a;
        }
      }
    }
    if (a >= 0) {
      const bool in = valid && static_cast<long long>(k) >= a;
      const unsigned long long mb = __ballot(in && r1 - T > C);
      const int lb = mb ? __ffsll(static_cast<long long>(mb)) - 1 : kWave;
      long long emitted = length;
      if (static_cast<long long>(k) == a && len_a >= 0) emitted = len_a;
      if (lane == lb) emitted = C - ((r0 > T ? r0 : T) - T);
      if (in && lane <= lb) {
        if (on_read) q_kept += emitted;
        if (on_ref) r_kept += emitted;
      }
      if (mb) {
        b = static_cast<int>(base) + lb;
        len_b = static_cast<int>(__shfl(emitted, lb, kWave));
        break;
      }
    }
    r_carry += __shfl(r_incl, kWave - 1, kWave);
    q_carry += __shfl(q_incl, kWave - 1, kWave);
  }
  if (a < 0) read_trim = q_carry;            // everything fell into the trimmed prefix
  const long long new_len = wave_sum(q_kept), span = wave_sum(r_kept);
  if (lane != 0) return;
  const long long seq_len = t.seq_len[pr.row];
  if (read_trim + new_len > seq_len) {
    atomicMin(error, (static_cast<unsigned long long>(pair) << 2) | dv::trim::kErrLength);
    results[pair] = res;                     // not kept: the call fails
    return;
  }
  res.first = a;
  res.n_words = a < 0 ? 0 : (b >= 0 ? b - a + 1 : static_cast<int>(n) - a);
  res.read_trim = static_cast<int32_t>(read_trim);
  res.new_len = static_cast<int32_t>(new_len);
  res.len_first = len_a;
  res.len_last = len_b;
  res.span = static_cast<int32_t>(span);
  res.kept = span >= win.min_overlap && new_len > 0;
  results[pair] = res;
}

// Pass 2: exclusive scan of (kept, kept ? n_words : 0) over the pairs in order, by one workgroup; the windows'
// row ranges and the totals fall out of it.
__global__ __launch_bounds__(kScanThreads) void trim_scan_kernel(Tables t, const PairResult* results,
                                                                 const unsigned long long* error, int32_t* row_of,
                                                                 uint32_t* word_of, Outputs o) {
  __shared__ int32_t wave_rows[kScanThreads / kWave], wave_words[kScanThreads / kWave];
  __shared__ int32_t carry_rows, carry_words;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  if (tid == 0) carry_rows = carry_words = 0;
  __syncthreads();
  for (int32_t base = 0; base < t.n_pairs; base += kScanThreads) {
    const int32_t p = base + tid;
    int32_t rows = 0, words = 0;
    if (p < t.n_pairs && results[p].kept) {
      rows = 1;
      words = results[p].n_words;
    }
    const int32_t rows_incl = static_cast<int32_t>(wave_inclusive_scan(rows, lane));
    const int32_t words_incl = static_cast<int32_t>(wave_inclusive_scan(words, lane));
    if (lane == kWave - 1) {
      wave_rows[wave] = rows_incl;
      wave_words[wave] = words_incl;
    }
    __syncthreads();
    int32_t before_rows = carry_rows, before_words = carry_words;
    for (int w = 0; w < wave; ++w) {
      before_rows += wave_rows[w];
      before_words += wave_words[w];
    }
    if (p < t.n_pairs) {
      row_of[p] = before_rows + rows_incl - rows;
      word_of[p] = static_cast<uint32_t>(before_words + words_incl - words);
    }
    __syncthreads();
    if (tid == kScanThreads - 1) {
      carry_rows = before_rows + rows_incl;
      carry_words = before_words + words_incl;
    }
    __syncthreads();
  }
  if (tid == 0) {
    row_of[t.n_pairs] = carry_rows;
    word_of[t.n_pairs] = static_cast<uint32_t>(carry_words);
    o.header->error = *error;
    o.header->n_rows = carry_rows;
    o.header->n_words = carry_words;
    o.cigar_off[carry_rows] = static_cast<uint32_t>(carry_words);
  }
  __syncthreads();
  for (int32_t w = tid; w <= t.n_windows; w += kScanThreads) o.window_row_off[w] = row_of[t.window_pair_off[w]];
}

// Pass 3: each kept pair's row and operations, at the places pass 2 gave them.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void trim_emit_kernel(Tables t, const PairResult* results,
                                                                          const int32_t* row_of,
                                                                          const uint32_t* word_of, Outputs o) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long pair = static_cast<long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (pair >= t.n_pairs) return;
  const PairResult res = results[pair];
  if (!res.kept) return;
  const Pair pr = t.pairs[pair];
  const int32_t row = row_of[pair];
  const uint32_t at = word_of[pair];
  if (lane == 0) {
    const dv_trim_window win = t.windows[pr.window];
    const long long pos = t.read_pos[pr.row];
    const int32_t new_pos = static_cast<int32_t>(win.r0 > pos ? win.r0 : pos);
    o.src_row[row] = pr.row;
    o.pos[row] = new_pos;
    o.end[row] = new_pos + res.span;
    o.read_trim[row] = res.read_trim;
    o.new_len[row] = res.new_len;
    o.cigar_off[row] = at;
  }
  const uint32_t from = t.cigar_off[pr.row] + static_cast<uint32_t>(res.first);
  for (int32_t i = lane; i < res.n_words; i += kWave) {
    uint32_t word = t.cigar[from + i];
    if (i == 0 && res.len_first >= 0) word = (static_cast<uint32_t>(res.len_first) << 4) | (word & 15u);
    if (i == res.n_words - 1 && res.len_last >= 0) word = (static_cast<uint32_t>(res.len_last) << 4) | (word & 15u);
    o.cigar[at + i] = word;
  }
}

dv_trim_stats& last_stats() {
  static thread_local dv_trim_stats stats;
  return stats;
}

}  // namespace

struct dv_trimmed_reads {
  std::vector<int32_t> window_row_off, src_row, pos, end, read_trim, new_len;
  std::vector<uint32_t> cigar_off, cigar;
};

namespace {

// The call's arguments, checked, and the pairs that pass the overlap test in (window, row) order.
struct Call {
  const dv_batch* reads = nullptr;
  std::vector<int32_t> end;               // read_end as the kernels take it
  std::vector<Pair> pairs;
  std::vector<int32_t> window_pair_off;   // [n_windows + 1]
  int64_t words = 0;                      // operations of the pairs' reads: what they could write at most
};

int parse(const char* who, const dv_batch* reads, const int64_t* read_end, int32_t n_windows,
          const dv_trim_window* windows, dv_trimmed_reads** out, Call* c) {
  const std::string name(who);
  if (out) *out = nullptr;
  if (!out || !reads || n_windows < 0 || (n_windows > 0 && !windows) || reads->n_reads < 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer or negative count");
  }
  if (reads->memory != DV_MEM_HOST) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": the read table must be in host memory");
  const int32_t n = reads->n_reads;
  if (n > 0 && (!reads->read_pos || !reads->read_seq_off || !reads->read_cigar_off || !read_end)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null read_pos, read_seq_off, read_cigar_off or read_end");
  }
  if (n > 0) {
    for (int32_t r = 0; r < n; ++r) {
      if (reads->read_seq_off[r + 1] < reads->read_seq_off[r] || reads->read_cigar_off[r + 1] < reads->read_cigar_off[r]) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": offsets must ascend");
      }
      if (read_end[r] < INT32_MIN || read_end[r] > INT32_MAX) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": read_end outside int32");
      }
    }
    if (reads->read_cigar_off[n] > reads->n_cigar || reads->read_seq_off[n] > reads->n_bases) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": offsets run past n_cigar / n_bases");
    }
    if (reads->read_cigar_off[n] > reads->read_cigar_off[0] && !reads->cigar) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null cigar");
    }
  }
  for (int32_t w = 0; w < n_windows; ++w) {
    if (windows[w].r0 < INT32_MIN || windows[w].r0 > INT32_MAX || windows[w].r1 < INT32_MIN || windows[w].r1 > INT32_MAX) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": window " + std::to_string(w) + " lies outside int32");
    }
  }
  c->reads = reads;
  c->end.resize(static_cast<size_t>(n));
  for (int32_t r = 0; r < n; ++r) c->end[r] = static_cast<int32_t>(read_end[r]);
  c->window_pair_off.assign(1, 0);
  for (int32_t w = 0; w < n_windows; ++w) {
    const int64_t q0 = windows[w].q0, q1 = windows[w].q1;
    for (int32_t r = 0; r < n; ++r) {
      if (q1 > reads->read_pos[r] && q0 < c->end[r]) {
        c->pairs.push_back(Pair{w, r});
        c->words += reads->read_cigar_off[r + 1] - reads->read_cigar_off[r];
      }
    }
    if (static_cast<int64_t>(c->pairs.size()) >= kMaxPairs || c->words >= kMaxWords) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": more than 2^28 (window, read) pairs or CIGAR operations "
                                                      "among them in one call; pass fewer windows");
    }
    c->window_pair_off.push_back(static_cast<int32_t>(c->pairs.size()));
  }
  return DV_OK;
}

int pair_error(const char* who, const Call& c, const dv_trim_window* windows, unsigned long long error) {
  const Pair pr = c.pairs[static_cast<size_t>(error >> 2)];
  const dv_trim_window& w = windows[pr.window];
  const std::string where = std::string(who) + ": window " + std::to_string(pr.window) + " [" + std::to_string(w.r0) +
                            ", " + std::to_string(w.r1) + "), row " + std::to_string(pr.row) + ": ";
  if ((error & 3) == dv::trim::kErrCover) return dv::fail(DV_ERR_BAD_INPUT, where + "Check failed: ref_length > 0");
  return dv::fail(DV_ERR_BAD_INPUT, where + "Check failed: read_trim + new_read_length <= aligned_sequence.size()");
}

int trim_on_host(const Call& c, int32_t n_windows, const dv_trim_window* windows, dv_trimmed_reads* res) {
  const dv_batch& b = *c.reads;
  res->window_row_off.assign(1, 0);
  res->cigar_off.assign(1, 0);
  for (int32_t w = 0; w < n_windows; ++w) {
    const dv_trim_window& win = windows[w];
    for (int32_t p = c.window_pair_off[w]; p < c.window_pair_off[w + 1]; ++p) {
      const int32_t row = c.pairs[p].row;
      const int64_t pos = b.read_pos[row];
      const int64_t T = std::max<int64_t>(win.r0 - pos, 0), C = win.r1 - std::max<int64_t>(win.r0, pos);
      if (C <= 0) return pair_error("dv_trim_reads_batch", c, windows, (static_cast<unsigned long long>(p) << 2) | dv::trim::kErrCover);
      const uint32_t c0 = b.read_cigar_off[row], n = b.read_cigar_off[row + 1] - c0;
      PairResult r;
      if (dv::trim::trim_serial(n ? b.cigar + c0 : nullptr, n, T, C, b.read_seq_off[row + 1] - b.read_seq_off[row],
                                win.min_overlap, &r)) {
        return pair_error("dv_trim_reads_batch", c, windows, (static_cast<unsigned long long>(p) << 2) | dv::trim::kErrLength);
      }
      if (!r.kept) continue;
      const int32_t new_pos = static_cast<int32_t>(T != 0 ? win.r0 : pos);
      res->src_row.push_back(row);
      res->pos.push_back(new_pos);
      res->end.push_back(new_pos + r.span);
      res->read_trim.push_back(r.read_trim);
      res->new_len.push_back(r.new_len);
      for (int32_t i = 0; i < r.n_words; ++i) {
        uint32_t word = b.cigar[c0 + r.first + i];
        if (i == 0 && r.len_first >= 0) word = (static_cast<uint32_t>(r.len_first) << 4) | (word & 15u);
        if (i == r.n_words - 1 && r.len_last >= 0) word = (static_cast<uint32_t>(r.len_last) << 4) | (word & 15u);
        res->cigar.push_back(word);
      }
      res->cigar_off.push_back(static_cast<uint32_t>(res->cigar.size()));
    }
    res->window_row_off.push_back(static_cast<int32_t>(res->src_row.size()));
  }
  return DV_OK;
}

int trim_on_device(const Call& c, int32_t n_windows, const dv_trim_window* windows, void* stream_in,
                   dv_trimmed_reads* res, dv_trim_stats* stats) {
  const dv_batch& b = *c.reads;
  const size_t n_reads = static_cast<size_t>(b.n_reads), n_pairs = c.pairs.size(), n_win = static_cast<size_t>(n_windows);
  const size_t n_cigar = b.read_cigar_off[n_reads], bound = static_cast<size_t>(c.words);
  dv::Layout up, down, work;
  // upload image: error word | windows | window pair offsets | pairs | read_pos | seq_len | cigar_off | cigar
  const size_t u_error = up.add(sizeof(unsigned long long));
  const size_t u_windows = up.add(n_win * sizeof(dv_trim_window));
  const size_t u_wpo = up.add((n_win + 1) * sizeof(int32_t));
  const size_t u_pairs = up.add(n_pairs * sizeof(Pair));
  const size_t u_pos = up.add(n_reads * sizeof(int32_t));
  const size_t u_len = up.add(n_reads * sizeof(uint32_t));
  const size_t u_coff = up.add((n_reads + 1) * sizeof(uint32_t));
  const size_t u_cigar = up.add(n_cigar * sizeof(uint32_t));
  // download image: header | window row offsets | five row arrays | cigar_off | words, each for the most there can be
  const size_t d_header = down.add(sizeof(Header));
  const size_t d_wro = down.add((n_win + 1) * sizeof(int32_t));
  size_t d_rows[5];     // src_row, pos, end, read_trim, new_len
  for (size_t& at : d_rows) at = down.add(n_pairs * sizeof(int32_t));
  const size_t d_coff = down.add((n_pairs + 1) * sizeof(uint32_t));
  const size_t d_words = down.add(bound * sizeof(uint32_t));
  // device-only work space: PairResult per pair | row_of | word_of
  const size_t k_results = work.add(n_pairs * sizeof(PairResult));
  const size_t k_row = work.add((n_pairs + 1) * sizeof(int32_t));
  const size_t k_word = work.add((n_pairs + 1) * sizeof(uint32_t));
  static_assert(sizeof(Header) <= 16 && sizeof(unsigned long long) <= 16, "the two first sections take 16 bytes each");
  static thread_local dv::RoundTrip rt;     // its scratch: the work space
  if (int rc = rt.begin("dv_trim_reads_batch_device: no HIP device (dv_trim_reads_batch is the host code)", stream_in,
                        up.bytes(), down.bytes(), work.bytes())) {
    return rc;
  }
  *rt.host_up<unsigned long long>(u_error) = dv::trim::kNoError;
  if (n_win) std::memcpy(rt.host_up<dv_trim_window>(u_windows), windows, n_win * sizeof(dv_trim_window));
  std::memcpy(rt.host_up<int32_t>(u_wpo), c.window_pair_off.data(), (n_win + 1) * sizeof(int32_t));
  std::memcpy(rt.host_up<Pair>(u_pairs), c.pairs.data(), n_pairs * sizeof(Pair));
  std::memcpy(rt.host_up<int32_t>(u_pos), b.read_pos, n_reads * sizeof(int32_t));
  uint32_t* seq_len = rt.host_up<uint32_t>(u_len);
  for (size_t r = 0; r < n_reads; ++r) seq_len[r] = b.read_seq_off[r + 1] - b.read_seq_off[r];
  std::memcpy(rt.host_up<uint32_t>(u_coff), b.read_cigar_off, (n_reads + 1) * sizeof(uint32_t));
  if (n_cigar) std::memcpy(rt.host_up<uint32_t>(u_cigar), b.cigar, n_cigar * sizeof(uint32_t));
  Tables t;
  t.read_pos = rt.dev_up<const int32_t>(u_pos);
  t.seq_len = rt.dev_up<const uint32_t>(u_len);
  t.cigar_off = rt.dev_up<const uint32_t>(u_coff);
  t.cigar = rt.dev_up<const uint32_t>(u_cigar);
  t.windows = rt.dev_up<const dv_trim_window>(u_windows);
  t.pairs = rt.dev_up<const Pair>(u_pairs);
  t.window_pair_off = rt.dev_up<const int32_t>(u_wpo);
  t.n_pairs = static_cast<int32_t>(n_pairs);
  t.n_windows = n_windows;
  Outputs o;
  o.header = rt.dev_down<Header>(d_header);
  o.window_row_off = rt.dev_down<int32_t>(d_wro);
  o.src_row = rt.dev_down<int32_t>(d_rows[0]);
  o.pos = rt.dev_down<int32_t>(d_rows[1]);
  o.end = rt.dev_down<int32_t>(d_rows[2]);
  o.read_trim = rt.dev_down<int32_t>(d_rows[3]);
  o.new_len = rt.dev_down<int32_t>(d_rows[4]);
  o.cigar_off = rt.dev_down<uint32_t>(d_coff);
  o.cigar = rt.dev_down<uint32_t>(d_words);
  unsigned long long* d_error = rt.dev_up<unsigned long long>(u_error);
  uint8_t* d_work = static_cast<uint8_t*>(rt.d_scratch.ptr);
  PairResult* d_results = reinterpret_cast<PairResult*>(d_work + k_results);
  int32_t* d_row_of = reinterpret_cast<int32_t*>(d_work + k_row);
  uint32_t* d_word_of = reinterpret_cast<uint32_t*>(d_work + k_word);
  const unsigned blocks = static_cast<unsigned>((n_pairs + kWavesPerBlock - 1) / kWavesPerBlock);
  hipStream_t stream = rt.stream();
  if (int rc = rt.upload(up.bytes())) return rc;
  {
    dv::ProfileScope prof(dv::kProfOther, stream);
    hipLaunchKernelGGL(trim_count_kernel, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, stream, t, d_results, d_error);
    DV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(trim_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, t, d_results, d_error, d_row_of,
                       d_word_of, o);
    DV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(trim_emit_kernel, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, stream, t, d_results, d_row_of,
                       d_word_of, o);
    DV_HIP_CHECK(hipGetLastError());
  }
  if (int rc = rt.finish(down.bytes())) return rc;
  stats->launches += 3;
  const Header header = *rt.host_down<Header>(d_header);
  if (header.error != dv::trim::kNoError) return pair_error("dv_trim_reads_batch_device", c, windows, header.error);
  const size_t n_rows = static_cast<size_t>(header.n_rows), n_words = static_cast<size_t>(header.n_words);
  if (n_rows > n_pairs || n_words > bound) return dv::fail(DV_ERR_HIP, "dv_trim_reads_batch_device: totals past their bounds");
  auto rows_of = [&](size_t k) { return rt.host_down<int32_t>(d_rows[k]); };
  const int32_t* wro = rt.host_down<int32_t>(d_wro);
  res->window_row_off.assign(wro, wro + n_win + 1);
  res->src_row.assign(rows_of(0), rows_of(0) + n_rows);
  res->pos.assign(rows_of(1), rows_of(1) + n_rows);
  res->end.assign(rows_of(2), rows_of(2) + n_rows);
  res->read_trim.assign(rows_of(3), rows_of(3) + n_rows);
  res->new_len.assign(rows_of(4), rows_of(4) + n_rows);
  const uint32_t* coff = rt.host_down<uint32_t>(d_coff);
  res->cigar_off.assign(coff, coff + n_rows + 1);
  const uint32_t* words = rt.host_down<uint32_t>(d_words);
  res->cigar.assign(words, words + n_words);
  stats->pairs_kept += static_cast<int64_t>(n_rows);
  stats->words_written += static_cast<int64_t>(n_words);
  return DV_OK;
}

int run(const char* who, bool on_device, const dv_batch* reads, const int64_t* read_end, int32_t n_windows,
        const dv_trim_window* windows, dv_trimmed_reads** out, void* stream) {
  return dv::guarded(who, [&]() -> int {
    if (on_device) last_stats() = dv_trim_stats{0, 0, 0, 0, 0};
    Call c;
    if (int rc = parse(who, reads, read_end, n_windows, windows, out, &c)) return rc;
    auto res = std::make_unique<dv_trimmed_reads>();
    int rc = DV_OK;
    if (!on_device) {
      rc = trim_on_host(c, n_windows, windows, res.get());
    } else if (c.pairs.empty()) {          // nothing to launch
      res->window_row_off.assign(static_cast<size_t>(n_windows) + 1, 0);
      res->cigar_off.assign(1, 0);
    } else {
      last_stats().pairs_tested = static_cast<int64_t>(c.pairs.size());
      last_stats().words_read = c.words;
      rc = trim_on_device(c, n_windows, windows, stream, res.get(), &last_stats());
    }
    if (rc) return rc;
    *out = res.release();
    return DV_OK;
  });
}

}  // namespace

extern "C" {

int dv_trim_reads_batch(const dv_batch* reads, const int64_t* read_end, int32_t n_windows,
                        const dv_trim_window* windows, dv_trimmed_reads** out) {
  return run("dv_trim_reads_batch", false, reads, read_end, n_windows, windows, out, nullptr);
}

int dv_trim_reads_batch_device(const dv_batch* reads, const int64_t* read_end, int32_t n_windows,
                               const dv_trim_window* windows, dv_trimmed_reads** out, void* stream) {
  return run("dv_trim_reads_batch_device", true, reads, read_end, n_windows, windows, out, stream);
}

int dv_trimmed_reads_arrays(const dv_trimmed_reads* t, dv_trimmed_reads_view* out) {
  if (!t || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_trimmed_reads_arrays: null");
  out->n_windows = static_cast<int32_t>(t->window_row_off.size()) - 1;
  out->n_rows = static_cast<int32_t>(t->src_row.size());
  out->n_words = static_cast<int64_t>(t->cigar.size());
  out->window_row_off = t->window_row_off.data();
  out->src_row = t->src_row.data();
  out->pos = t->pos.data();
  out->end = t->end.data();
  out->read_trim = t->read_trim.data();
  out->new_len = t->new_len.data();
  out->cigar_off = t->cigar_off.data();
  out->cigar = t->cigar.data();
  return DV_OK;
}

void dv_trimmed_reads_free(dv_trimmed_reads* t) { delete t; }

int dv_trim_device_last_stats(dv_trim_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_trim_device_last_stats: null");
  *out = last_stats();
  return DV_OK;
}

}  // extern "C"
