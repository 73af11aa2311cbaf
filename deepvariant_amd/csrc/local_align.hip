// local_align.hip -- the sweeps of the local aligner (local_align.h) on the device, and the C
// entry point that aligns a list of pairs with them.
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
#include <algorithm>
#include <cstring>
#include <numeric>

#include "dv_internal.h"
#include "local_align_device.h"

static_assert(sizeof(dv_realign_device_stats) == 32, "dv_realign_device_stats layout");

namespace {

constexpr int kWavesPerGroup = 4;
constexpr int kRefNothing = 6, kQueryNothing = 5;   // codes that match nothing, not even each other
constexpr int kRowBuckets[] = {1, 2, 3, 4, 8, 16, 24, 32};
static_assert(64 * 32 == dv::kDeviceAlignMaxQuery, "the widest bucket holds the longest query");

struct SweepItem {     // one pair of the launch
  int32_t ref, query;  // indices into the sequence table
  int32_t rows;        // query rows per lane: one of kRowBuckets
  int32_t pair;        // the caller's pair (host side only)
};

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

template <int S>
__device__ void align_pair(const uint8_t* __restrict__ codes, const int32_t* __restrict__ seq_off,
                                        const SweepItem item, const Scoring sc, int lane, int32_t* __restrict__ out) {
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
  if (lane == 0) {
    out[0] = fwd.score;
    out[1] = fwd.column;
    out[2] = fwd.row;
    out[3] = rev.score;
    out[4] = fwd.score > 0 ? fwd.column - rev.column : -1;
    out[5] = fwd.score > 0 ? fwd.row - rev.row : -1;
  }
}

__global__ __launch_bounds__(64 * kWavesPerGroup) void local_align_sweeps(
    const uint8_t* __restrict__ codes, const int32_t* __restrict__ seq_off, const SweepItem* __restrict__ items,
    int n_items, const Scoring sc, int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
  if (w >= n_items) return;   // a whole wave leaves; nothing below synchronises the workgroup
  const SweepItem item = items[w];
  int32_t* o = out + static_cast<size_t>(w) * 6;
  switch (item.rows) {
    case 1: align_pair<1>(codes, seq_off, item, sc, lane, o); break;
    case 2: align_pair<2>(codes, seq_off, item, sc, lane, o); break;
    case 3: align_pair<3>(codes, seq_off, item, sc, lane, o); break;
    case 4: align_pair<4>(codes, seq_off, item, sc, lane, o); break;
    case 8: align_pair<8>(codes, seq_off, item, sc, lane, o); break;
    case 16: align_pair<16>(codes, seq_off, item, sc, lane, o); break;
    case 24: align_pair<24>(codes, seq_off, item, sc, lane, o); break;
    default: align_pair<32>(codes, seq_off, item, sc, lane, o); break;
  }
}

// Grow-only pinned staging, one per host thread and direction.
struct PinnedStage {
  uint8_t* ptr = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return DV_OK;
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    cap = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 1u << 16);
    if (hipHostMalloc(reinterpret_cast<void**>(&ptr), want, hipHostMallocDefault) != hipSuccess) {
      ptr = nullptr;
      return dv::fail(DV_ERR_OUT_OF_MEMORY, "hipHostMalloc (local aligner staging)");
    }
    cap = want;
    return DV_OK;
  }
};

struct ThreadState {
  PinnedStage up, down;
  dv::DeviceBuffer d_up, d_down;
  hipStream_t stream = nullptr;   // the library's own, for callers that pass none
  int stream_device = -1;
};

size_t align16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

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
                          std::vector<uint8_t>* route, DeviceAlignStats* stats) {
  const size_t n_pairs = pair_ref.size();
  corners->assign(n_pairs, SweepCorners());
  route->assign(n_pairs, kRouteHost);
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
    items.push_back(SweepItem{slot[pair_ref[k]], slot[pair_query[k]], rows_bucket(n), static_cast<int32_t>(k)});
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

  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    return fail(DV_ERR_NO_DEVICE, "local aligner: no HIP device (the device route has no CPU fallback)");
  }
  // the call may come from a thread that has not used the device yet (RealignJob.start on an executor)
  int device = 0;
  DV_HIP_CHECK(hipGetDevice(&device));
  DV_HIP_CHECK(hipSetDevice(device));
  static thread_local ThreadState ts;
  hipStream_t stream = static_cast<hipStream_t>(stream_in);
  if (!stream) {
    if (ts.stream && ts.stream_device != device) {
      (void)hipStreamDestroy(ts.stream);
      ts.stream = nullptr;
    }
    if (!ts.stream) {
      DV_HIP_CHECK(hipStreamCreateWithFlags(&ts.stream, hipStreamNonBlocking));
      ts.stream_device = device;
    }
    stream = ts.stream;
  }

  // upload image: items | sequence offsets | codes
  const size_t n_items = items.size();
  const size_t o_items = 0;
  const size_t o_off = align16(n_items * sizeof(SweepItem));
  const size_t o_codes = o_off + align16((used.size() + 1) * sizeof(int32_t));
  const size_t up_bytes = o_codes + align16(n_codes);
  const size_t down_bytes = n_items * 6 * sizeof(int32_t);
  if (int rc = ts.up.reserve(up_bytes)) return rc;
  if (int rc = ts.down.reserve(down_bytes)) return rc;
  if (int rc = ts.d_up.reserve_on_current_device(up_bytes)) return rc;
  if (int rc = ts.d_down.reserve_on_current_device(down_bytes)) return rc;
  std::memcpy(ts.up.ptr + o_items, items.data(), n_items * sizeof(SweepItem));
  int32_t* off = reinterpret_cast<int32_t*>(ts.up.ptr + o_off);
  uint8_t* codes = ts.up.ptr + o_codes;
  int32_t at = 0;
  for (size_t u = 0; u < used.size(); ++u) {
    const CodedSequence& s = *sequences[used[u]];
    off[u] = at;
    std::memcpy(codes + at, s.data(), s.size());
    at += static_cast<int32_t>(s.size());
  }
  off[used.size()] = at;

  uint8_t* d_up = static_cast<uint8_t*>(ts.d_up.ptr);
  DV_HIP_CHECK(hipMemcpyAsync(d_up, ts.up.ptr, up_bytes, hipMemcpyHostToDevice, stream));
  {
    ProfileScope prof(kProfOther, stream);
    const Scoring sc{match, mismatch, gap_open, gap_extend};
    const unsigned groups = static_cast<unsigned>((n_items + kWavesPerGroup - 1) / kWavesPerGroup);
    hipLaunchKernelGGL(local_align_sweeps, dim3(groups), dim3(64 * kWavesPerGroup), 0, stream, d_up + o_codes,
                       reinterpret_cast<const int32_t*>(d_up + o_off),
                       reinterpret_cast<const SweepItem*>(d_up + o_items), static_cast<int>(n_items), sc,
                       static_cast<int32_t*>(ts.d_down.ptr));
    DV_HIP_CHECK(hipGetLastError());
  }
  DV_HIP_CHECK(hipMemcpyAsync(ts.down.ptr, ts.d_down.ptr, down_bytes, hipMemcpyDeviceToHost, stream));
  DV_HIP_CHECK(hipStreamSynchronize(stream));
  if (stats) stats->launches += 1;
  const int32_t* res = reinterpret_cast<const int32_t*>(ts.down.ptr);
  for (size_t w = 0; w < n_items; ++w) {
    SweepCorners& c = (*corners)[items[w].pair];
    c.score = res[w * 6 + 0];
    c.ref_end = res[w * 6 + 1];
    c.query_end = res[w * 6 + 2];
    c.reverse_score = res[w * 6 + 3];
    c.ref_begin = res[w * 6 + 4];
    c.query_begin = res[w * 6 + 5];
  }
  return DV_OK;
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
  try {
    g_last_stats = dv::DeviceAlignStats();
    if (n_seqs < 0 || n_pairs < 0 || (n_seqs > 0 && !seq_off) || (n_pairs > 0 && (!pair_ref || !pair_query || !out))) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_local_align_pairs_device: null pointer or negative count");
    }
    if (match <= 0 || mismatch < 0 || gap_open < 0 || gap_extend < 0 || match > dv::kDeviceAlignMaxScoringValue ||
        mismatch > dv::kDeviceAlignMaxScoringValue || gap_open > dv::kDeviceAlignMaxScoringValue ||
        gap_extend > dv::kDeviceAlignMaxScoringValue) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT,
                      "dv_local_align_pairs_device: match must be in [1, 127], the penalties in [0, 127]");
    }
    for (int32_t s = 0; s < n_seqs; ++s) {
      if (seq_off[s] < 0 || seq_off[s + 1] < seq_off[s]) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_local_align_pairs_device: sequence offsets must ascend from >= 0");
      }
    }
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
    if (int rc = dv::sweep_pairs_on_device(seqs, refs, queries, match, mismatch, gap_open, gap_extend, stream,
                                           &corners, &route, &g_last_stats)) {
      return rc;
    }
    const dv::LocalAligner aligner(match, mismatch, gap_open, gap_extend);
    for (int32_t k = 0; k < n_pairs; ++k) {
      const dv::CodedSequence& ref = *seqs[refs[k]];
      const dv::CodedSequence& q = *seqs[queries[k]];
      dv::LocalAlignment r;
      bool ok = false;
      if (route[k] == dv::kRouteDevice) {
        ok = aligner.complete(ref, q, corners[k], &r);
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
  } catch (const std::bad_alloc&) {
    return dv::fail(DV_ERR_OUT_OF_MEMORY, "dv_local_align_pairs_device: out of host memory");
  } catch (const std::exception& e) {
    return dv::fail(DV_ERR_BAD_INPUT, std::string("dv_local_align_pairs_device: ") + e.what());
  }
}

int dv_local_align_device_last_stats(dv_realign_device_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_local_align_device_last_stats: null");
  out->pairs = g_last_stats.pairs;
  out->pairs_on_host = g_last_stats.pairs_on_host;
  out->cells = g_last_stats.cells;
  out->launches = g_last_stats.launches;
  return DV_OK;
}

}  // extern "C"
