// local_align.hip -- the sweeps of the local aligner (local_align.h) on the device, its banded
// trace-back behind them in the same launch, and the C entry point that aligns a list of pairs
// with them.
//
// Contract: per pair the values of LocalAligner::sweep forward and of the reverse sweep of
// LocalAligner::finish.  score = the maximum of H over the matrix, ref_end = the first reference
// column holding it, q_end = the smallest query index holding it in that column; the reverse
// pass runs on the reversed prefixes ref[0..ref_end], q[0..q_end] and reports the first column,
// in walking order, that reaches `score`, and the smallest row in it.  The reverse maximum
// cannot exceed `score` (its matrix is a sub-matrix of the forward one), so the host's rule --
// the first column whose maximum exceeds every earlier one, stop at the target -- is "global
// maximum, then smallest column, then smallest row" in both passes.  int32 throughout.
//
// Shape: one wave per pair, four waves per workgroup, one launch for the whole list.  Lane l
// owns the query rows [l*S, (l+1)*S), S = ceil(|q| / 64) rounded up to a bucket the kernel is
// instantiated for; at step t it computes reference column t - l, so the wave walks the matrix
// as a skewed front.  H of the previous column, E and the query codes of a lane's rows stay in
// registers.  Per step two values move from lane l-1 to lane l: H of its last row packed with
// the column's reference base, and F leaving its last row -- the vertical gap is carried in the
// host's serial order.  Lane 0 takes its reference bases from a 64-base register chunk that
// the wave reloads every 64 steps.
//
// Cells outside the matrix (rows past |q| in the last lanes, columns before 0 and past |ref| at
// the two ends of the skew) are computed with codes that match nothing.  Before the matrix they
// keep H = 0 and E, F <= 0, which is the host's initial state as far as H can tell (a
// non-positive E or F never wins max(., 0)).  Past it, a cell's value comes from a real cell
// that is earlier in (column, row) order, minus non-negative penalties: it can tie that cell but
// never beat it, and ties go to the earlier cell.  Columns outside the matrix are not recorded
// at all.
//
// Each lane keeps (max, column, row) of its own cells with a strict >, visiting them in
// (column, row) order; the lanes' triples are reduced lexicographically at the end.  Inside a
// column the lane's maximum and its smallest row come from one integer max over keys
// (H << 5) | (31 - row): H <= 127 * 2048 < 2^18.
//
// The reverse pass stops early: once some lane has reached the target in column c, every lane
// has passed column c after step c + 63, and no later column can matter.
//
// The trace-back (trace_back below) runs in the same wave right after the sweeps, for a pair that
// holds an alignment: LocalAligner::banded_cigar on ref[ref_begin..ref_end] x q[q_begin..q_end],
// bit for bit -- the band |ref_len - q_len| + 1 that doubles until `best` (kept across the
// doublings) reaches the score, the same zeroes at the band's edges, the same tie rules, the walk
// from the bottom-right cell in state 2.  Lane k owns the band diagonal k = j - i + band and
// computes cell (i, k) at step t = 2i + k, so lanes of t's parity work in a step: lane k - 1
// holds the left neighbour (H and the running F) and lane k + 1 the upper one (H and E) from step
// t - 1, the diagonal neighbour is the lane's own H from step t - 2.  The bases travel with those
// moves: the query base of row i enters at lane 0 and goes up the lanes with H, the reference base
// of column j enters at lane 2 * band -- at step 2j, rows before the matrix included -- and goes
// down them; both entries read base t / 2 of a 64-base register chunk.  One direction byte per
// cell (dH in bits 0-2, "E opened" in bit 3, "F opened" in bit 4) goes to the pair's scratch
// area, row t of 32 bytes, byte k / 2: one contiguous store per step.  The walk is wave-uniform:
// it loads 32 rows (1 KiB, 16 bytes per lane) at a time and picks its cells out of the registers
// with readlane; a step moves t back by one or two, so the blocks are visited once, in order.
// Lane 0 writes the runs as they close, last run first.  A pair that cannot be finished here
// (band > 31, more than 64 runs, no scratch area, or where banded_cigar itself gives up) is
// flagged not traced and the host's banded_cigar does it: the host never reads a partial list.
//
// Host side: one upload image, one launch, one download per call; the image's layout and the calling
// thread's buffers, scratch (the direction bytes) and stream are device_round_trip.h's (Layout, RoundTrip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "device_round_trip.h"
#include "local_align_device.h"

static_assert(sizeof(dv_realign_device_stats) == 32, "dv_realign_device_stats layout");
static_assert(sizeof(dv_realign_traceback_stats) == 32, "dv_realign_traceback_stats layout");

namespace {

constexpr int kWavesPerGroup = 4;
constexpr int kRefNothing = 6, kQueryNothing = 5;   // codes that match nothing, not even each other
constexpr int kRowBuckets[] = {1, 2, 3, 4, 8, 16, 24, 32};
static_assert(64 * 32 == dv::kDeviceAlignMaxQuery, "the widest bucket holds the longest query");

constexpr int kMaxBand = DV_LOCAL_ALIGN_DEVICE_MAX_BAND;
constexpr int kMaxRuns = DV_LOCAL_ALIGN_DEVICE_MAX_RUNS;
static_assert(2 * kMaxBand + 1 <= 63, "one band diagonal per lane");
static_assert(kMaxRuns < (1 << 16), "the run count shares a word with the band");
// words per pair in the download: the six corner values alone, or with the trace-back
// [6] traced, [7] runs | band << 16, [8 ..) the runs, (length << 2) | 0 M / 1 I / 2 D, last run first
constexpr int kCornerWords = 6, kTraceHeaderWords = 8, kTraceWords = kTraceHeaderWords + kMaxRuns;
// direction bytes: 32 per step, steps 0 .. 2 * (q_len - 1) + 2 * band, in blocks of 32 steps
constexpr size_t kAreaUnit = 1024;
constexpr size_t kScratchBudget = size_t{256} << 20;   // per call; pairs past it are traced back on the host

struct SweepItem {     // one pair of the launch
  int32_t ref, query;  // indices into the sequence table
  int32_t rows;        // query rows per lane: one of kRowBuckets
  int32_t pair;        // the caller's pair (host side only)
  int32_t area;        // its direction bytes start at scratch + area * kAreaUnit; -1: no trace-back
};

size_t area_units(size_t query_len) {   // for any sub-problem of the query and any band <= kMaxBand
  const size_t steps = 2 * (query_len - 1) + 2 * kMaxBand + 1;
  return (steps + 31) / 32;
}

struct Scoring {
  int match, mismatch, gap_open, gap_extend;
};

struct Best {
  int score, column, row;
};

// One pass over `columns` reference bases (ref[0], ref[step], ...) x `n` query bases, S rows
// per lane.  target > 0: the pass may stop once the target has been reached (reverse pass).
template <int S>
__device__ Best sweep(const uint8_t* __restrict__ ref, int ref_step, int columns,
                                      const uint8_t* __restrict__ q, int q_step, int n, int target,
                                      const Scoring sc, int lane) {
  int h_prev[S], e[S], qcode[S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int row = lane * S + j;
    const int c = row < n ? q[row * q_step] : kQueryNothing;
    qcode[j] = c < 4 ? c : kQueryNothing;
    h_prev[j] = 0;
    e[j] = 0;
  }
  const int miss = -sc.mismatch;
  Best best{0, -1, -1};
  int out_hr = kRefNothing;   // (H of the last row << 3) | reference code: what the next lane receives
  int out_f = 0;
  int diag_in = 0;            // H of the previous lane's last row, one column back
  int chunk = kRefNothing;
  int last_step = columns + 62;   // lane 63 reaches the last column
  bool found = false;
  for (int t = 0; t <= last_step; ++t) {
    if ((t & 63) == 0) {
      const int c = t + lane;
      const int code = c < columns ? ref[c * ref_step] : kRefNothing;
      chunk = code < 4 ? code : kRefNothing;
    }
    int in_hr = __shfl_up(out_hr, 1);
    int f = __shfl_up(out_f, 1);
    const int first = __builtin_amdgcn_readlane(chunk, t & 63);
    if (lane == 0) {
      in_hr = first;
      f = 0;
    }
    const int r = in_hr & 7;
    int diag = diag_in;
    diag_in = in_hr >> 3;
    int key = 0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      int h = diag + (r == qcode[j] ? sc.match : miss);
      const int ej = e[j];
      h = max(max(h, ej), max(f, 0));
      diag = h_prev[j];
      h_prev[j] = h;
      key = max(key, (h << 5) | (31 - j));
      const int open = h - sc.gap_open;
      e[j] = max(ej - sc.gap_extend, open);
      f = max(f - sc.gap_extend, open);
    }
    out_hr = (h_prev[S - 1] << 3) | r;
    out_f = f;
    const int column = t - lane;
    const int column_best = key >> 5;
    if (column_best > best.score && static_cast<unsigned>(column) < static_cast<unsigned>(columns)) {
      best.score = column_best;
      best.column = column;
      best.row = lane * S + 31 - (key & 31);
    }
    if (target > 0 && !found && __any(best.score == target)) {
      found = true;
      int c = best.score == target ? best.column : columns;
      for (int off = 32; off > 0; off >>= 1) c = min(c, __shfl_xor(c, off));
      last_step = min(last_step, __builtin_amdgcn_readfirstlane(c) + 63);
    }
  }
  // maximum, then smallest column, then smallest row
  for (int off = 32; off > 0; off >>= 1) {
    const int os = __shfl_xor(best.score, off), oc = __shfl_xor(best.column, off), orow = __shfl_xor(best.row, off);
    const bool take = os > best.score ||
                      (os == best.score && (oc < best.column || (oc == best.column && orow < best.row)));
    if (take) {
      best.score = os;
      best.column = oc;
      best.row = orow;
    }
  }
  best.score = __builtin_amdgcn_readfirstlane(best.score);
  best.column = __builtin_amdgcn_readfirstlane(best.column);
  best.row = __builtin_amdgcn_readfirstlane(best.row);
  return best;
}

struct Corners {   // wave-uniform
  int score, ref_end, q_end, rev_score, ref_begin, q_begin;
};

template <int S>
__device__ Corners align_pair(const uint8_t* __restrict__ codes, const int32_t* __restrict__ seq_off,
                              const SweepItem item, const Scoring sc, int lane) {
  const uint8_t* ref = codes + seq_off[item.ref];
  const int columns = seq_off[item.ref + 1] - seq_off[item.ref];
  const uint8_t* q = codes + seq_off[item.query];
  const int n = seq_off[item.query + 1] - seq_off[item.query];
  // both passes through one copy of the loop: forward, then the reversed prefixes
  Best fwd{0, -1, -1}, rev{0, 0, 0};
  const uint8_t* pass_ref = ref;
  const uint8_t* pass_q = q;
  int step = 1, pass_columns = columns, pass_n = n, target = -1;
#pragma nounroll
  for (int pass = 0; pass < 2; ++pass) {
    const Best b = sweep<S>(pass_ref, step, pass_columns, pass_q, step, pass_n, target, sc, lane);
    if (pass == 1) {
      rev = b;
      break;
    }
    fwd = b;
    if (b.score <= 0) break;
    pass_ref = ref + b.column;
    pass_q = q + b.row;
    step = -1;
    pass_columns = b.column + 1;
    pass_n = b.row + 1;
    target = b.score;
  }
  return Corners{fwd.score, fwd.column, fwd.row, rev.score, fwd.score > 0 ? fwd.column - rev.column : -1,
                 fwd.score > 0 ? fwd.row - rev.row : -1};
}

__device__ int wave_max(int v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return __builtin_amdgcn_readfirstlane(v);
}

// LocalAligner::banded_cigar for ref[0..rl) x q[0..ql) and `target`; see the top of the file.
// -> the number of runs written to `runs` (last run first), 0: not traced.  *final_band as the host reports it.
__device__ int trace_back(const uint8_t* __restrict__ ref, int rl, const uint8_t* __restrict__ q, int ql, int target,
                          const Scoring sc, int lane, uint8_t* area, uint32_t* __restrict__ runs, int* final_band) {
  const int miss = -sc.mismatch;
  int band = abs(rl - ql) + 1;
  int best = 0;
  for (;;) {
    if (band > kMaxBand) return 0;
    const int last_lane = 2 * band;
    const int last_step = 2 * (ql - 1) + last_lane;
    int out_l = kQueryNothing, out_u = kQueryNothing;   // (H << 3) | base: to the lane above / below
    int out_e = 0, out_f = 0, h_own = 0, lane_best = 0;
    int q_chunk = kQueryNothing, r_chunk = kQueryNothing;
    for (int t = 0; t <= last_step; ++t) {
      const int m = t >> 1;
      if ((t & 127) == 0) {
        const int c = m + lane;
        q_chunk = c < ql ? q[c] : kQueryNothing;
        r_chunk = c < rl ? ref[c] : kQueryNothing;
      }
      const int in_l = __shfl_up(out_l, 1), in_f = __shfl_up(out_f, 1);
      const int in_u = __shfl_down(out_u, 1), in_e = __shfl_down(out_e, 1);
      const int q_first = __builtin_amdgcn_readlane(q_chunk, m & 63);
      const int r_last = __builtin_amdgcn_readlane(r_chunk, m & 63);
      const int i = (t - lane) >> 1, j = i + lane - band;
      const bool active = ((t - lane) & 1) == 0 && lane <= last_lane;
      const int qc = lane == 0 ? q_first : (in_l & 7);
      const int rc = lane == last_lane ? r_last : (in_u & 7);
      const bool up = i > 0 && lane < last_lane, left = lane > 0 && j > 0;
      int t1 = (up ? in_u >> 3 : 0) - sc.gap_open, t2 = (up ? in_e : 0) - sc.gap_extend;
      const int e = max(t1, t2), e_opened = t1 > t2;
      t1 = (left ? in_l >> 3 : 0) - sc.gap_open;
      t2 = (left ? in_f : 0) - sc.gap_extend;
      const int f = max(t1, t2), f_opened = t1 > t2;
      const int e1 = max(e, 0), f1 = max(f, 0);
      t1 = max(e1, f1);
      t2 = (i > 0 && j > 0 ? h_own : 0) + (qc == rc && qc < 4 ? sc.match : miss);
      const int h = max(t1, t2);
      const int dh = t1 <= t2 ? 1 : (e1 > f1 ? 2 + e_opened : 4 + f_opened);
      if (active) {
        h_own = h;
        out_l = (h << 3) | qc;
        out_u = (h << 3) | rc;
        out_e = e;
        out_f = f;
        if (i >= 0 && i < ql && j >= 0 && j < rl) {
          lane_best = max(lane_best, h);
          area[t * 32 + (lane >> 1)] = static_cast<uint8_t>(dh | (e_opened << 3) | (f_opened << 4));
        }
      }
    }
    best = max(best, wave_max(lane_best));
    if (best >= target) break;
    if (band > 2 * (rl + ql)) return 0;   // the host gives up here too
    band *= 2;
  }
  *final_band = band;
  __threadfence_block();   // the wave reads its own lanes' stores below
  // the walk: everything from here on is wave-uniform
  int i = ql - 1, j = rl - 1, state = 2, run = 0, op = 0, prev_op = 0, n = 0, loaded = -1;
  uint4 w = make_uint4(0, 0, 0, 0);
  while (i > 0) {
    const int k = j - i + band;
    if (j < 0 || k < 0 || k > 2 * band) return 0;   // left the band
    const int t = 2 * i + k, block = t >> 5, half = k >> 1;
    if (block != loaded) {
      w = *reinterpret_cast<const uint4*>(area + static_cast<size_t>(block) * kAreaUnit + lane * 16);
      loaded = block;
    }
    const int part = (half & 15) >> 2;
    const uint32_t word = part == 0 ? w.x : part == 1 ? w.y : part == 2 ? w.z : w.w;
    const uint32_t cell = __builtin_amdgcn_readlane(word, ((t & 31) << 1) | (half >> 4)) >> ((half & 3) * 8);
    const int d = state == 2 ? (cell & 7) : state == 0 ? 2 + ((cell >> 3) & 1) : 4 + ((cell >> 4) & 1);
    switch (d) {
      case 1: --i; --j; state = 2; op = 0; break;
      case 2: --i; state = 0; op = 1; break;
      case 3: --i; state = 2; op = 1; break;
      case 4: --j; state = 1; op = 2; break;
      case 5: --j; state = 2; op = 2; break;
      default: return 0;
    }
    if (op == prev_op) {
      ++run;
    } else {
      if (run > 0) {
        if (n >= kMaxRuns) return 0;
        if (lane == 0) runs[n] = (static_cast<uint32_t>(run) << 2) | prev_op;
        ++n;
      }
      prev_op = op;
      run = 1;
    }
  }
  // the first cell of the alignment is a match
  if (op != 0) {
    if (n >= kMaxRuns) return 0;
    if (lane == 0) runs[n] = (static_cast<uint32_t>(run) << 2) | op;
    ++n;
    run = 0;
  }
  if (n >= kMaxRuns) return 0;
  if (lane == 0) runs[n] = (static_cast<uint32_t>(run + 1) << 2);
  return n + 1;
}

__global__ __launch_bounds__(64 * kWavesPerGroup) void local_align_sweeps(
    const uint8_t* __restrict__ codes, const int32_t* __restrict__ seq_off, const SweepItem* __restrict__ items,
    int n_items, const Scoring sc, int32_t* __restrict__ out, int out_words, uint8_t* scratch) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
  if (w >= n_items) return;   // a whole wave leaves; nothing below synchronises the workgroup
  const SweepItem item = items[w];
  int32_t* o = out + static_cast<size_t>(w) * out_words;
  Corners c;
  switch (item.rows) {
    case 1: c = align_pair<1>(codes, seq_off, item, sc, lane); break;
    case 2: c = align_pair<2>(codes, seq_off, item, sc, lane); break;
    case 3: c = align_pair<3>(codes, seq_off, item, sc, lane); break;
    case 4: c = align_pair<4>(codes, seq_off, item, sc, lane); break;
    case 8: c = align_pair<8>(codes, seq_off, item, sc, lane); break;
    case 16: c = align_pair<16>(codes, seq_off, item, sc, lane); break;
    case 24: c = align_pair<24>(codes, seq_off, item, sc, lane); break;
    default: c = align_pair<32>(codes, seq_off, item, sc, lane); break;
  }
  if (lane == 0) {
    o[0] = c.score;
    o[1] = c.ref_end;
    o[2] = c.q_end;
    o[3] = c.rev_score;
    o[4] = c.ref_begin;
    o[5] = c.q_begin;
  }
  if (out_words < kTraceWords) return;
  int n_runs = 0, band = 0;
  // the area holds any sub-problem of the query: corners outside the sequences would not fit it
  const int columns = seq_off[item.ref + 1] - seq_off[item.ref], n = seq_off[item.query + 1] - seq_off[item.query];
  const bool inside = c.ref_begin >= 0 && c.ref_begin <= c.ref_end && c.ref_end < columns && c.q_begin >= 0 &&
                      c.q_begin <= c.q_end && c.q_end < n;
  if (item.area >= 0 && c.score > 0 && c.rev_score == c.score && inside) {
    n_runs = trace_back(codes + seq_off[item.ref] + c.ref_begin, c.ref_end - c.ref_begin + 1,
                        codes + seq_off[item.query] + c.q_begin, c.q_end - c.q_begin + 1, c.score, sc, lane,
                        scratch + static_cast<size_t>(item.area) * kAreaUnit,
                        reinterpret_cast<uint32_t*>(o + kTraceHeaderWords), &band);
  }
  if (lane == 0) {
    o[6] = n_runs > 0;
    o[7] = n_runs | (band << 16);
  }
}

int rows_bucket(size_t query_len) {
  const int need = static_cast<int>((query_len + 63) / 64);
  for (int b : kRowBuckets) {
    if (b >= need) return b;
  }
  return kRowBuckets[sizeof(kRowBuckets) / sizeof(kRowBuckets[0]) - 1];
}

}  // namespace

namespace dv {

int sweep_pairs_on_device(const std::vector<const CodedSequence*>& sequences, const std::vector<int32_t>& pair_ref,
                          const std::vector<int32_t>& pair_query, int match, int mismatch, int gap_open,
                          int gap_extend, void* stream_in, std::vector<SweepCorners>* corners,
                          std::vector<uint8_t>* route, DeviceAlignStats* stats, DeviceRuns* traced,
                          ResidentSweep* keep) {
  const size_t n_pairs = pair_ref.size();
  if (keep) {
    *keep = ResidentSweep();
    keep->item_of_pair.assign(n_pairs, -1);
    keep->traced.assign(n_pairs, 0);
  }
  corners->assign(n_pairs, SweepCorners());
  route->assign(n_pairs, kRouteHost);
  TracebackStats& tb = last_traceback_stats();
  tb = TracebackStats();
  const bool trace = traced && (keep || device_traceback_enabled());
  if (traced) {
    traced->traced.assign(n_pairs, 0);
    traced->band.assign(n_pairs, 0);
    traced->first.assign(n_pairs, 0);
    traced->count.assign(n_pairs, 0);
    traced->words.clear();
  }
  const bool scoring_fits = match >= 0 && mismatch >= 0 && gap_open >= 0 && gap_extend >= 0 &&
                            match <= kDeviceAlignMaxScoringValue && mismatch <= kDeviceAlignMaxScoringValue &&
                            gap_open <= kDeviceAlignMaxScoringValue && gap_extend <= kDeviceAlignMaxScoringValue;
  // the sequences the device pairs use, each uploaded once
  std::vector<int32_t> slot(sequences.size(), -1);
  std::vector<int32_t> used;
  std::vector<SweepItem> items;
  int64_t cells = 0, on_host = 0;
  size_t n_codes = 0;
  for (size_t k = 0; k < n_pairs; ++k) {
    const size_t m = sequences[pair_ref[k]]->size(), n = sequences[pair_query[k]]->size();
    if (m == 0 || n == 0) {
      (*route)[k] = kRouteEmpty;
      continue;
    }
    if (!scoring_fits || !device_align_fits(m, n)) {
      ++on_host;
      continue;
    }
    (*route)[k] = kRouteDevice;
    for (int32_t s : {pair_ref[k], pair_query[k]}) {
      if (slot[s] < 0) {
        slot[s] = static_cast<int32_t>(used.size());
        used.push_back(s);
        n_codes += sequences[s]->size();
      }
    }
    items.push_back(SweepItem{slot[pair_ref[k]], slot[pair_query[k]], rows_bucket(n), static_cast<int32_t>(k), -1});
    cells += static_cast<int64_t>(m) * static_cast<int64_t>(n);
  }
  if (stats) {
    stats->pairs += static_cast<int64_t>(n_pairs);
    stats->pairs_on_host += on_host;
    stats->cells += cells;
  }
  if (items.empty()) return DV_OK;
  if (n_codes >= (size_t{1} << 31) || items.size() >= (size_t{1} << 28)) {
    return fail(DV_ERR_INVALID_ARGUMENT, "local aligner: more than 2 GiB of sequence in one call");
  }
  // the longest sweeps first: a wave takes the item of its index, and early workgroups start first
  std::stable_sort(items.begin(), items.end(), [&](const SweepItem& a, const SweepItem& b) {
    const int64_t ca = static_cast<int64_t>(a.rows) * static_cast<int64_t>(sequences[used[a.ref]]->size());
    const int64_t cb = static_cast<int64_t>(b.rows) * static_cast<int64_t>(sequences[used[b.ref]]->size());
    return ca > cb;
  });

  // the direction bytes of the trace-back: an area per pair, sized for the whole query, while the budget lasts
  size_t scratch_units = 0;
  if (trace) {
    for (SweepItem& item : items) {
      const size_t units = area_units(sequences[used[item.query]]->size());
      if ((scratch_units + units) * kAreaUnit > kScratchBudget) continue;
      item.area = static_cast<int32_t>(scratch_units);
      scratch_units += units;
    }
  }

  // upload image: items | sequence offsets | codes
  const size_t n_items = items.size();
  Layout up;
  const size_t o_items = up.add(n_items * sizeof(SweepItem));
  const size_t o_off = up.add((used.size() + 1) * sizeof(int32_t));
  const size_t o_codes = up.add(n_codes);
  // download image: out_words per pair
  const size_t out_words = trace ? kTraceWords : kCornerWords;
  const size_t down_bytes = n_items * out_words * sizeof(int32_t);
  static thread_local RoundTrip rt;     // its scratch: the trace-back's direction bytes
  if (int rc = rt.begin("local aligner: no HIP device (the device route has no CPU fallback)", stream_in, up.bytes(),
                        down_bytes, scratch_units * kAreaUnit)) {
    return rc;
  }
  std::memcpy(rt.host_up<SweepItem>(o_items), items.data(), n_items * sizeof(SweepItem));
  int32_t* off = rt.host_up<int32_t>(o_off);
  uint8_t* codes = rt.host_up<uint8_t>(o_codes);
  int32_t at = 0;
  for (size_t u = 0; u < used.size(); ++u) {
    const CodedSequence& s = *sequences[used[u]];
    off[u] = at;
    std::memcpy(codes + at, s.data(), s.size());
    at += static_cast<int32_t>(s.size());
  }
  off[used.size()] = at;

  if (int rc = rt.upload(up.bytes())) return rc;
  {
    ProfileScope prof(kProfOther, rt.stream());
    const Scoring sc{match, mismatch, gap_open, gap_extend};
    const unsigned groups = static_cast<unsigned>((n_items + kWavesPerGroup - 1) / kWavesPerGroup);
    hipLaunchKernelGGL(local_align_sweeps, dim3(groups), dim3(64 * kWavesPerGroup), 0, rt.stream(),
                       rt.dev_up<const uint8_t>(o_codes), rt.dev_up<const int32_t>(o_off),
                       rt.dev_up<const SweepItem>(o_items), static_cast<int>(n_items), sc, rt.dev_down<int32_t>(0),
                       static_cast<int>(out_words), static_cast<uint8_t*>(rt.d_scratch.ptr));
    DV_HIP_CHECK(hipGetLastError());
  }
  // the words a pair's row holds on the host: all of them, or with `keep` the header alone, rows packed
  const size_t host_words = keep ? kTraceHeaderWords : out_words;
  if (keep) {
    DV_HIP_CHECK(hipMemcpy2DAsync(rt.down.ptr, host_words * sizeof(int32_t), rt.d_down.ptr, out_words * sizeof(int32_t),
                                  host_words * sizeof(int32_t), n_items, hipMemcpyDeviceToHost, rt.stream()));
    DV_HIP_CHECK(hipStreamSynchronize(rt.stream()));
    keep->d_out = rt.dev_down<const int32_t>(0);
    keep->out_words = static_cast<int32_t>(out_words);
    keep->n_items = static_cast<int32_t>(n_items);
    keep->d_items = rt.dev_up<const SweepItem>(o_items);
    keep->d_seq_off = rt.dev_up<const int32_t>(o_off);
    keep->d_codes = rt.dev_up<const uint8_t>(o_codes);
    keep->stream = rt.stream();
    keep->bytes_down = static_cast<int64_t>(n_items * host_words * sizeof(int32_t));
  } else if (int rc = rt.finish(down_bytes)) {
    return rc;
  }
  if (stats) stats->launches += 1;
  const int32_t* res = rt.host_down<int32_t>(0);
  for (size_t w = 0; w < n_items; ++w) {
    const int32_t* r = res + w * host_words;
    const size_t k = static_cast<size_t>(items[w].pair);
    if (keep) keep->item_of_pair[k] = static_cast<int32_t>(w);
    SweepCorners& c = (*corners)[k];
    c.score = r[0];
    c.ref_end = r[1];
    c.query_end = r[2];
    c.reverse_score = r[3];
    c.ref_begin = r[4];
    c.query_begin = r[5];
    if (c.score <= 0 || c.reverse_score != c.score) continue;   // no alignment: nothing to trace back
    const int32_t n_runs = trace ? r[7] & 0xffff : 0, band = trace ? r[7] >> 16 : 0;
    if (!trace || r[6] != 1 || n_runs < 1 || n_runs > kMaxRuns || band < 1 || band > kMaxBand) {
      ++tb.traced_on_host;
      continue;
    }
    ++tb.traced_on_device;
    tb.band_cells += static_cast<int64_t>(c.query_end - c.query_begin + 1) * (2 * band + 1);
    tb.widest_band = std::max<int64_t>(tb.widest_band, band);
    if (keep) {                // the runs stay on the device
      keep->traced[k] = 1;
      continue;
    }
    traced->traced[k] = 1;
    traced->band[k] = band;
    traced->first[k] = static_cast<int32_t>(traced->words.size());
    traced->count[k] = n_runs;
    for (int32_t x = n_runs; x-- > 0;) traced->words.push_back(static_cast<uint32_t>(r[kTraceHeaderWords + x]));   // the kernel wrote the last run first
  }
  return DV_OK;
}

TracebackStats& last_traceback_stats() {
  static thread_local TracebackStats stats;
  return stats;
}

bool device_traceback_enabled() { return env_switch("DV_REALIGN_DEVICE_TRACEBACK", kTracebackByDefault); }

bool complete_on_device_route(const LocalAligner& aligner, const CodedSequence& ref, const CodedSequence& q,
                              const SweepCorners& corners, const DeviceRuns* traced, size_t k, LocalAlignment* out) {
  if (!traced || !traced->traced[k]) return aligner.complete(ref, q, corners, out);
  CigarRuns runs(static_cast<size_t>(traced->count[k]));
  for (size_t x = 0; x < runs.size(); ++x) {
    const uint32_t word = traced->words[static_cast<size_t>(traced->first[k]) + x];
    runs[x] = {"MID"[word & 3], static_cast<int>(word >> 2)};
  }
  aligner.complete_with_runs(ref, q, corners, runs, traced->band[k], out);
  return true;
}

}  // namespace dv

namespace {

thread_local dv::DeviceAlignStats g_last_stats;

void fill_alignment(const dv::LocalAlignment& r, bool ok, dv_local_alignment* out) {
  out->score = ok ? r.score : -1;
  out->ref_begin = r.ref_begin;
  out->ref_end = r.ref_end;
  out->query_begin = r.query_begin;
  out->query_end = r.query_end;
  out->mismatches = r.mismatches;
  out->cigar[0] = '\0';
}

}  // namespace

extern "C" {

int dv_local_align_pairs_device(int32_t n_seqs, const char* bases, const int64_t* seq_off, int32_t n_pairs,
                                const int32_t* pair_ref, const int32_t* pair_query, int32_t match, int32_t mismatch,
                                int32_t gap_open, int32_t gap_extend, dv_local_alignment* out, void* stream) {
  return dv::guarded("dv_local_align_pairs_device", [&]() -> int {
    g_last_stats = dv::DeviceAlignStats();
    dv::last_traceback_stats() = dv::TracebackStats();
    if (n_seqs < 0 || n_pairs < 0 || (n_seqs > 0 && !seq_off) || (n_pairs > 0 && (!pair_ref || !pair_query || !out))) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_local_align_pairs_device: null pointer or negative count");
    }
    if (match <= 0 || mismatch < 0 || gap_open < 0 || gap_extend < 0 || match > dv::kDeviceAlignMaxScoringValue ||
        mismatch > dv::kDeviceAlignMaxScoringValue || gap_open > dv::kDeviceAlignMaxScoringValue ||
        gap_extend > dv::kDeviceAlignMaxScoringValue) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT,
                      "dv_local_align_pairs_device: match must be in [1, 127], the penalties in [0, 127]");
    }
    if (int rc = dv::check_sequence_table("dv_local_align_pairs_device", n_seqs, seq_off)) return rc;
    if (n_seqs > 0 && seq_off[n_seqs] > seq_off[0] && !bases) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_local_align_pairs_device: null bases");
    }
    for (int32_t k = 0; k < n_pairs; ++k) {
      if (pair_ref[k] < 0 || pair_ref[k] >= n_seqs || pair_query[k] < 0 || pair_query[k] >= n_seqs) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_local_align_pairs_device: sequence index out of range");
      }
    }
    if (n_pairs == 0) return DV_OK;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
      return dv::fail(DV_ERR_NO_DEVICE, "dv_local_align_pairs_device: no HIP device (there is no CPU fallback)");
    }
    std::vector<dv::CodedSequence> coded(n_seqs);
    std::vector<const dv::CodedSequence*> seqs(n_seqs);
    for (int32_t s = 0; s < n_seqs; ++s) {
      coded[s] = dv::encode_sequence(std::string(bases + seq_off[s], static_cast<size_t>(seq_off[s + 1] - seq_off[s])));
      seqs[s] = &coded[s];
    }
    const std::vector<int32_t> refs(pair_ref, pair_ref + n_pairs), queries(pair_query, pair_query + n_pairs);
    std::vector<dv::SweepCorners> corners;
    std::vector<uint8_t> route;
    dv::DeviceRuns traced;
    if (int rc = dv::sweep_pairs_on_device(seqs, refs, queries, match, mismatch, gap_open, gap_extend, stream,
                                           &corners, &route, &g_last_stats, &traced)) {
      return rc;
    }
    const dv::LocalAligner aligner(match, mismatch, gap_open, gap_extend);
    for (int32_t k = 0; k < n_pairs; ++k) {
      const dv::CodedSequence& ref = *seqs[refs[k]];
      const dv::CodedSequence& q = *seqs[queries[k]];
      dv::LocalAlignment r;
      bool ok = false;
      if (route[k] == dv::kRouteDevice) {
        ok = dv::complete_on_device_route(aligner, ref, q, corners[k], &traced, static_cast<size_t>(k), &r);
      } else if (route[k] == dv::kRouteHost) {
        std::vector<dv::LocalAlignment> one;
        std::vector<char> one_ok;
        aligner.align_pairs({&ref}, {&q}, &one, &one_ok);
        r = one[0];
        ok = one_ok[0] != 0;
      }
      fill_alignment(r, ok, &out[k]);
      if (ok) {
        if (r.cigar.size() >= sizeof(out[k].cigar)) {
          return dv::fail(DV_ERR_INVALID_ARGUMENT, "text buffer too small");
        }
        std::memcpy(out[k].cigar, r.cigar.c_str(), r.cigar.size() + 1);
      }
    }
    return DV_OK;
  });
}

int dv_local_align_device_last_stats(dv_realign_device_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_local_align_device_last_stats: null");
  out->pairs = g_last_stats.pairs;
  out->pairs_on_host = g_last_stats.pairs_on_host;
  out->cells = g_last_stats.cells;
  out->launches = g_last_stats.launches;
  return DV_OK;
}

int dv_local_align_device_last_traceback_stats(dv_realign_traceback_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_local_align_device_last_traceback_stats: null");
  const dv::TracebackStats& tb = dv::last_traceback_stats();
  out->traced_on_device = tb.traced_on_device;
  out->traced_on_host = tb.traced_on_host;
  out->band_cells = tb.band_cells;
  out->widest_band = tb.widest_band;
  return DV_OK;
}

}  // extern "C"
