// The realigner's alignments finished on the device: dv_align_windows_batch (host code),
// dv_align_windows_batch_device (fast pass, sweeps + trace-back, finish kernels) and finish_windows_on_device, the
// finish step alone for dv_realign_regions_device (include/dvhip.h, realign_finish_device.h).
//
// The contract is FastPassAligner::finish_alignments as it stands in fast_pass_aligner.cpp -- apply_haplotype_alignments,
// positions_map, apply_read_alignments, realign_reads_to_reference with best_read_alignment,
// calculate_read_to_ref_alignment, merge_cigar_op and is_alignment_normalized -- which stays the checker and the host
// entry point's code.  realign_finish.h is that code restated without text, compiled for both sides.  Per window:
//
// Haplotypes.  A haplotype byte-equal to the reference has the CIGAR "<n>=" at 0 and is the reference.  Any other one
// has the result of its Smith-Waterman against the reference: with a score > 0 reached by the reverse pass, the CIGAR
// [q_begin S] runs [n - 1 - q_end S] at ref_pos = ref_begin, and it is the reference when that is one '=' token over
// the whole haplotype (corners 0 .. n - 1, one M run of n, no differing 0..4 code: 'N' equals 'N' here); otherwise an
// empty CIGAR, an all-zero map and ref_pos 0.
// Order.  realign_reads_to_reference sorts the haplotype alignments by haplotype_score with std::sort, which is not
// stable; best_read_alignment walks the sorted list, so the order of tied haplotypes decides results.  The host
// computes the permutation with the same call over (score, index) records and uploads it (fin::sorted_order).
// Reads.  A read the fast pass placed holds, per haplotype with a score != 0, "<L>=" at its row's position with the
// row's score.  An unplaced read holds, per target haplotype (haplotype_score != 0, or the reference under
// force_alignment), its Smith-Waterman result when that holds an alignment and score >= uint16_t(score_threshold) (or
// the target is forced): [q_begin S] runs [L - 1 - q_end S] at uint16_t(ref_begin).  The best haplotype is the first
// of the sorted list with the largest score > 0, unless a later one with that score is not the reference.  None:
// status 2 under force_alignment, else 0.
// Merge.  position >= n: status 0.  shift = positions_map[position] (S lowers the shift and then fills, D raises it, I
// fills and lowers it per base, unreached positions keep 0).  The haplotype CIGAR is trimmed on the left by `position`
// haplotype bases (M, S, I consume them, D does not; a D left in front is dropped; nothing left: status 0).  Then
// the base-by-base walk of calculate_read_to_ref_alignment, token by token -- an M run counts as the '=' / 'X' tokens
// the coded sequences split it into, because a read whose token ends exactly where the haplotype ends goes on with
// whole operations while one cut inside a token is cleared -- with the priority S, D, I, M, I against D cancelling,
// and a one-base match pushed to the front of both queues when the haplotype side was the D.
// Normalisation.  is_alignment_normalized on raw bytes (the reference as handed over, the read upper-cased) at
// offset = int(ref_pos + position + shift); a negative offset counts as normalised; only without normalize_reads.
// Result.  Status 1, position = ref_start + offset, the merged words; an empty CIGAR is status 0.
//
// Device.  One lane per haplotype (its state), then one lane per (window, read): pick + count (finish_read without
// output: status, position, words), scan (one workgroup, steps of 1,024 reads carrying a running total), write
// (finish_read again at the scanned offset).  The pairs' words are read where the sweep kernel left them; one staged
// upload carries the windows, haplotypes, permutation, reads, pair indices, fast-pass rows and raw bytes.  The words
// are downloaded by a bounded guess, because an exact size would need a synchronisation between the count and the
// write pass: the device holds room for 64 words per read of the call, and the one download beside the statuses,
// positions and offsets takes the first 4 words per read of it (a realigned read's CIGAR is one to three words as a
// rule; 64 per read would be several times what the parent route downloads for its pairs).  A call with more words
// fetches the rest in a second download; one whose words do not fit the room at all (the write pass never stores past
// it) runs again with the exact room.  DV_REALIGN_FINISH_ROOM=<words per read>, read at each call, sets the room
// (default 64): tests lower it to walk the second run.  Placement is a pure function of the input; no atomics, no workgroup waits
// for another.
#include <hip/hip_runtime.h>

#include <cctype>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_round_trip.h"
#include "fast_pass_device.h"
#include "realign_finish.h"
#include "realign_finish_device.h"
#include "realign_finish_stage.h"

static_assert(sizeof(dv_realign_finish_stats) == 48, "dv_realign_finish_stats layout");
static_assert(sizeof(dv_align_window) == 40, "dv_align_window layout");
static_assert(dv::fin::kPairMaxRuns == DV_LOCAL_ALIGN_DEVICE_MAX_RUNS, "the rule's run bound is the kernel's");

namespace {

namespace fin = dv::fin;

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kGuessWordsPerRead = 64;      // room on the device, unless DV_REALIGN_FINISH_ROOM says otherwise
constexpr int kDownloadWordsPerRead = 4;    // of it in the first download

struct Header {          // the download's first bytes
  int64_t n_words;
  int64_t reserved;
};

struct Outputs {         // device pointers into the download
  Header* header;
  fin::ReadOut* reads;   // [n_reads]
  uint32_t* cigar_off;   // [n_reads + 1]
  uint32_t* cigar;
  uint32_t word_room;    // the words `cigar` holds
};

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t up = __shfl_up(v, d, kWave);
    if (lane >= d) v += up;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void finish_haps_kernel(fin::Batch b, fin::HapState* states) {
  const int g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= b.n_haps) return;
  states[g] = fin::hap_state(b, g);
}

// Pass 1: the best haplotype and the merge walked once, nothing written but status, position and word count.
__global__ __launch_bounds__(kThreads) void finish_count_kernel(fin::Batch b, const fin::HapState* states, Outputs o) {
  const int d = blockIdx.x * kThreads + threadIdx.x;
  if (d >= b.n_reads) return;
  int cancelled = 0;
  o.reads[d] = fin::finish_read(b, states, d, nullptr, &cancelled);
}

// Pass 2: exclusive scan of the word counts over the reads in order, by one workgroup, 1,024 reads per step.
__global__ __launch_bounds__(kScanThreads) void finish_scan_kernel(int32_t n_reads, Outputs o) {
  __shared__ uint32_t wave_words[kScanThreads / kWave];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int32_t base = 0; base < n_reads; base += kScanThreads) {
    const int32_t p = base + tid;
    const uint32_t words = p < n_reads ? static_cast<uint32_t>(o.reads[p].n_words) : 0u;
    const uint32_t incl = wave_inclusive_scan(words, lane);
    if (lane == kWave - 1) wave_words[wave] = incl;
    __syncthreads();
    uint32_t before = carry;
    for (int w = 0; w < wave; ++w) before += wave_words[w];
    if (p < n_reads) o.cigar_off[p] = before + incl - words;
    __syncthreads();
    if (tid == kScanThreads - 1) carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) {
    o.cigar_off[n_reads] = carry;
    o.header->n_words = carry;
    o.header->reserved = 0;
  }
}

// Pass 3: the words of every status-1 read, at the place pass 2 gave them.
__global__ __launch_bounds__(kThreads) void finish_write_kernel(fin::Batch b, const fin::HapState* states, Outputs o) {
  const int d = blockIdx.x * kThreads + threadIdx.x;
  if (d >= b.n_reads) return;
  const fin::ReadOut c = o.reads[d];
  if (c.status != 1 || c.n_words <= 0) return;
  const uint32_t at = o.cigar_off[d];
  if (static_cast<unsigned long long>(at) + static_cast<unsigned long long>(c.n_words) > o.word_room) return;
  int cancelled = 0;
  fin::finish_read(b, states, d, o.cigar + at, &cancelled);
}

}  // namespace

namespace dv {

FinishStats& last_finish_stats() {
  static thread_local FinishStats stats;
  return stats;
}

bool device_finish_enabled() { return env_switch("DV_REALIGN_DEVICE_FINISH", false); }

bool window_finishes_on_device(size_t first_pair, size_t n_pairs, const std::vector<uint8_t>& route,
                               const std::vector<SweepCorners>& corners, const ResidentSweep& sweep) {
  for (size_t k = first_pair; k < first_pair + n_pairs; ++k) {
    if (route[k] != kRouteDevice || sweep.item_of_pair[k] < 0) return false;
    const SweepCorners& c = corners[k];
    if (c.score > 0 && c.reverse_score == c.score && !sweep.traced[k]) return false;
  }
  return true;
}

int finish_windows_on_device(const std::vector<FinishWindow>& windows, const ResidentSweep& sweep,
                             bool force_alignment, bool normalize_reads, FinishStats* stats) {
  if (windows.empty()) return DV_OK;
  fin::Staged staged;
  for (const FinishWindow& w : windows) {
    fin::stage_window(*w.aligner, *w.pairs, sweep.item_of_pair.data() + w.first_pair,
                      static_cast<int64_t>(w.aligner->ref_start()), &staged);
    if (!staged.fits()) return fail(DV_ERR_INVALID_ARGUMENT, "finish: more than 1 GiB of tables in one call; pass fewer windows");
  }
  const size_t n_windows = staged.windows.size(), n_haps = staged.haps.size(), n_reads = staged.reads.size();
  for (const FinishWindow& w : windows) w.out->assign(w.pairs->n_input_reads, RealignedRead());
  if (n_reads == 0) return DV_OK;

  Layout up;
  const size_t o_windows = up.add(n_windows * sizeof(fin::Window));
  const size_t o_haps = up.add(n_haps * sizeof(fin::Hap));
  const size_t o_perm = up.add(n_haps * sizeof(int32_t));
  const size_t o_reads = up.add(n_reads * sizeof(fin::Read));
  const size_t o_items = up.add(staged.read_item.size() * sizeof(int32_t));
  const size_t o_row_pos = up.add(staged.row_position.size() * sizeof(int32_t));
  const size_t o_row_score = up.add(staged.row_score.size() * sizeof(int32_t));
  const size_t o_bytes = up.add(staged.bytes.size());
  static thread_local RoundTrip rt;     // its scratch: the haplotypes' states
  size_t room_per_read = kGuessWordsPerRead;
  if (const char* v = getenv("DV_REALIGN_FINISH_ROOM")) {
    const int asked = std::atoi(v);
    if (asked >= 1 && asked <= kGuessWordsPerRead) room_per_read = static_cast<size_t>(asked);
  }
  // the kernels hold the room and every offset in 32 bits
  if (n_reads * kGuessWordsPerRead >= (size_t{1} << 32)) {
    return fail(DV_ERR_INVALID_ARGUMENT, "finish: more than 2^26 reads in one call; pass fewer windows");
  }
  size_t word_room = n_reads * room_per_read;
  for (int attempt = 0; attempt < 2; ++attempt) {
    Layout down;
    const size_t o_header = down.add(sizeof(Header));
    const size_t o_out = down.add(n_reads * sizeof(fin::ReadOut));
    const size_t o_off = down.add((n_reads + 1) * sizeof(uint32_t));
    const size_t o_words = down.add_last(word_room * sizeof(uint32_t));
    if (int rc = rt.begin("finish: no HIP device (the device route has no CPU fallback)", sweep.stream, up.bytes(),
                          down.bytes(), std::max<size_t>(n_haps, 1) * sizeof(fin::HapState))) {
      return rc;
    }
    std::memcpy(rt.host_up<fin::Window>(o_windows), staged.windows.data(), n_windows * sizeof(fin::Window));
    std::memcpy(rt.host_up<fin::Hap>(o_haps), staged.haps.data(), n_haps * sizeof(fin::Hap));
    std::memcpy(rt.host_up<int32_t>(o_perm), staged.perm.data(), n_haps * sizeof(int32_t));
    std::memcpy(rt.host_up<fin::Read>(o_reads), staged.reads.data(), n_reads * sizeof(fin::Read));
    std::memcpy(rt.host_up<int32_t>(o_items), staged.read_item.data(), staged.read_item.size() * sizeof(int32_t));
    std::memcpy(rt.host_up<int32_t>(o_row_pos), staged.row_position.data(), staged.row_position.size() * sizeof(int32_t));
    std::memcpy(rt.host_up<int32_t>(o_row_score), staged.row_score.data(), staged.row_score.size() * sizeof(int32_t));
    std::memcpy(rt.host_up<uint8_t>(o_bytes), staged.bytes.data(), staged.bytes.size());
    if (int rc = rt.upload(up.bytes())) return rc;

    fin::Batch b;
    b.windows = rt.dev_up<const fin::Window>(o_windows);
    b.haps = rt.dev_up<const fin::Hap>(o_haps);
    b.perm = rt.dev_up<const int32_t>(o_perm);
    b.reads = rt.dev_up<const fin::Read>(o_reads);
    b.read_item = rt.dev_up<const int32_t>(o_items);
    b.row_position = rt.dev_up<const int32_t>(o_row_pos);
    b.row_score = rt.dev_up<const int32_t>(o_row_score);
    b.bytes = rt.dev_up<const uint8_t>(o_bytes);
    b.sweep.out = sweep.d_out;
    b.sweep.out_words = sweep.out_words;
    b.sweep.n_items = sweep.n_items;
    b.sweep.items = static_cast<const fin::SweepItemView*>(sweep.d_items);
    b.sweep.seq_off = sweep.d_seq_off;
    b.sweep.codes = sweep.d_codes;
    b.n_windows = static_cast<int32_t>(n_windows);
    b.n_haps = static_cast<int32_t>(n_haps);
    b.n_reads = static_cast<int32_t>(n_reads);
    b.force_alignment = force_alignment ? 1 : 0;
    b.normalize_reads = normalize_reads ? 1 : 0;
    Outputs o;
    o.header = rt.dev_down<Header>(o_header);
    o.reads = rt.dev_down<fin::ReadOut>(o_out);
    o.cigar_off = rt.dev_down<uint32_t>(o_off);
    o.cigar = rt.dev_down<uint32_t>(o_words);
    o.word_room = static_cast<uint32_t>(word_room);
    fin::HapState* states = static_cast<fin::HapState*>(rt.d_scratch.ptr);
    {
      ProfileScope prof(kProfOther, rt.stream());
      const unsigned hap_groups = static_cast<unsigned>((n_haps + kThreads - 1) / kThreads);
      const unsigned read_groups = static_cast<unsigned>((n_reads + kThreads - 1) / kThreads);
      if (hap_groups > 0) {
        hipLaunchKernelGGL(finish_haps_kernel, dim3(hap_groups), dim3(kThreads), 0, rt.stream(), b, states);
        DV_HIP_CHECK(hipGetLastError());
      }
      hipLaunchKernelGGL(finish_count_kernel, dim3(read_groups), dim3(kThreads), 0, rt.stream(), b, states, o);
      DV_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(finish_scan_kernel, dim3(1), dim3(kScanThreads), 0, rt.stream(), b.n_reads, o);
      DV_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(finish_write_kernel, dim3(read_groups), dim3(kThreads), 0, rt.stream(), b, states, o);
      DV_HIP_CHECK(hipGetLastError());
      if (stats) stats->launches += 3 + (hap_groups > 0 ? 1 : 0);
    }
    const size_t first_words = std::min(word_room, n_reads * kDownloadWordsPerRead);
    const size_t first_bytes = o_words + first_words * sizeof(uint32_t);
    if (int rc = rt.finish(first_bytes)) return rc;
    if (stats) stats->bytes_down += static_cast<int64_t>(first_bytes);
    const Header* header = rt.host_down<Header>(o_header);
    // nothing below is sized or indexed by a value the device returned without a range check
    if (header->n_words < 0 || header->n_words > static_cast<int64_t>(n_reads) * (int64_t{1} << 16)) {
      return fail(DV_ERR_HIP, "finish: the device returned an impossible word count");
    }
    if (static_cast<size_t>(header->n_words) > word_room) {
      if (attempt == 1) return fail(DV_ERR_HIP, "finish: the device's word count changed between two runs");
      word_room = static_cast<size_t>(header->n_words);
      if (word_room >= (size_t{1} << 32)) return fail(DV_ERR_INVALID_ARGUMENT, "finish: more than 2^32 CIGAR words in one call");
      continue;
    }
    const size_t n_words = static_cast<size_t>(header->n_words);
    if (n_words > first_words) {         // the rest of the words
      const size_t rest = (n_words - first_words) * sizeof(uint32_t);
      DV_HIP_CHECK(hipMemcpyAsync(rt.down.ptr + first_bytes, static_cast<const uint8_t*>(rt.d_down.ptr) + first_bytes, rest,
                                  hipMemcpyDeviceToHost, rt.stream()));
      DV_HIP_CHECK(hipStreamSynchronize(rt.stream()));
      if (stats) stats->bytes_down += static_cast<int64_t>(rest);
    }
    const fin::ReadOut* outs = rt.host_down<fin::ReadOut>(o_out);
    const uint32_t* off = rt.host_down<uint32_t>(o_off);
    const uint32_t* words = rt.host_down<uint32_t>(o_words);
    size_t d = 0;
    for (const FinishWindow& w : windows) {
      for (RealignedRead& r : *w.out) {
        const fin::ReadOut& ro = outs[d];
        const size_t a = off[d], e = off[d + 1];
        ++d;
        if (ro.status < 0 || ro.status > 2 || a > e || e > n_words || (ro.status == 1) != (e > a) ||
            static_cast<size_t>(ro.n_words) != e - a) {
          return fail(DV_ERR_HIP, "finish: the device returned an inconsistent read");
        }
        r.status = ro.status;
        if (ro.status != 1) continue;
        r.position = ro.position;
        r.cigar.resize(e - a);
        for (size_t x = a; x < e; ++x) r.cigar[x - a] = CigarOp{static_cast<int>(words[x] & 15u), static_cast<int>(words[x] >> 4)};
      }
    }
    if (stats) {
      stats->reads += static_cast<int64_t>(n_reads);
      stats->cigar_words += static_cast<int64_t>(n_words);
    }
    return DV_OK;
  }
  return DV_OK;
}

}  // namespace dv

// ---------------------------------------------------------------- the C entry points
struct dv_aligned_windows {
  std::vector<int32_t> window_read_off, status;
  std::vector<int64_t> position;
  std::vector<uint32_t> cigar_off, cigar;
};

namespace {

struct Call {            // the arguments, checked
  int32_t n_windows = 0;
  const dv_align_window* windows = nullptr;
  const char* bytes = nullptr;
  const int64_t* seq_off = nullptr;
  dv::AlignerOptions options;
  bool normalize_reads = false;

  std::string sequence(int32_t s) const {
    return std::string(bytes + seq_off[s], static_cast<size_t>(seq_off[s + 1] - seq_off[s]));
  }
  void set_up(const dv_align_window& w, dv::FastPassAligner* a) const {
    std::string error;
    a->set_options(options, &error);   // checked by parse()
    a->set_normalize_reads(normalize_reads);
    a->set_ref_prefix_len(w.ref_prefix_len);
    a->set_ref_suffix_len(w.ref_suffix_len);
    a->set_reference(sequence(w.reference));
    a->set_ref_start(static_cast<uint64_t>(w.ref_start));
    std::vector<std::string> haplotypes;
    for (int32_t h = 0; h < w.n_haplotypes; ++h) haplotypes.push_back(sequence(w.first_haplotype + h));
    a->set_haplotypes(haplotypes);
  }
  std::vector<std::string> reads_of(const dv_align_window& w) const {
    std::vector<std::string> out;
    for (int32_t r = 0; r < w.n_reads; ++r) out.push_back(sequence(w.first_read + r));
    return out;
  }
};

int parse(const char* who, int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
          const dv_align_window* windows, const dv_aligner_options* o, dv_aligned_windows** out, Call* c) {
  const std::string name(who);
  if (out) *out = nullptr;
  if (!out || !o || n_seqs < 0 || n_windows < 0 || (n_seqs > 0 && !seq_off) || (n_windows > 0 && !windows)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer or negative count");
  }
  if (int rc = dv::check_sequence_table(name, n_seqs, seq_off)) return rc;
  if (n_seqs > 0 && seq_off[n_seqs] > seq_off[0] && !bytes) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null bytes");
  c->options.match = o->match;
  c->options.mismatch = o->mismatch;
  c->options.gap_open = o->gap_open;
  c->options.gap_extend = o->gap_extend;
  c->options.kmer_size = o->kmer_size;
  c->options.read_size = o->read_size;
  c->options.max_num_of_mismatches = o->max_num_of_mismatches;
  c->options.similarity_threshold = o->realignment_similarity_threshold;
  c->options.force_alignment = o->force_alignment != 0;
  c->normalize_reads = o->normalize_reads != 0;
  dv::FastPassAligner resolved;
  std::string error;
  if (!resolved.set_options(c->options, &error)) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": " + error);
  resolved.init_local_aligner();
  const dv::LocalAligner& la = resolved.local_aligner();
  if (la.match() > dv::kDeviceAlignMaxScoringValue || la.mismatch() > dv::kDeviceAlignMaxScoringValue ||
      la.gap_open() > dv::kDeviceAlignMaxScoringValue || la.gap_extend() > dv::kDeviceAlignMaxScoringValue) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": scoring values are limited to 127 (the aligner's int8_t matrix)");
  }
  int64_t reads = 0;
  for (int32_t w = 0; w < n_windows; ++w) {
    const dv_align_window& win = windows[w];
    if (win.n_reads < 0 || win.n_haplotypes < 0 || win.first_read < 0 || win.first_haplotype < 0 ||
        static_cast<int64_t>(win.first_read) + win.n_reads > n_seqs ||
        static_cast<int64_t>(win.first_haplotype) + win.n_haplotypes > n_seqs || win.reference < 0 ||
        win.reference >= n_seqs || win.ref_prefix_len < 0 || win.ref_suffix_len < 0 || win.ref_start < 0) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": window " + std::to_string(w) +
                                                   ": range, reference, padding or ref_start out of range");
    }
    for (int32_t h = 0; h < win.n_haplotypes; ++h) {
      if (seq_off[win.first_haplotype + h + 1] - seq_off[win.first_haplotype + h] >= 0xffff) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, "haplotypes are limited to 65534 bases (16-bit read offsets)");
      }
    }
    reads += win.n_reads;
    if (reads >= (int64_t{1} << 28)) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": more than 2^28 reads in one call");
  }
  c->n_windows = n_windows;
  c->windows = windows;
  c->bytes = bytes;
  c->seq_off = seq_off;
  return DV_OK;
}

void append(const std::vector<dv::RealignedRead>& reads, dv_aligned_windows* res) {
  for (const dv::RealignedRead& r : reads) {
    res->status.push_back(r.status);
    res->position.push_back(r.status == 1 ? r.position : 0);
    if (r.status == 1) {
      for (const dv::CigarOp& op : r.cigar) {
        res->cigar.push_back((static_cast<uint32_t>(op.length) << 4) | static_cast<uint32_t>(op.op));
      }
    }
    res->cigar_off.push_back(static_cast<uint32_t>(res->cigar.size()));
  }
  res->window_read_off.push_back(static_cast<int32_t>(res->status.size()));
}

int align_on_device(const Call& c, void* stream, dv_aligned_windows* res) {
  dv::FinishStats& stats = dv::last_finish_stats();
  struct Win {
    std::unique_ptr<dv::FastPassAligner> aligner;
    dv::AlignmentPairs pairs;
    size_t first_pair = 0, first_haplotype = 0;
    std::vector<dv::RealignedRead> aligned;
  };
  std::vector<Win> wins(static_cast<size_t>(c.n_windows));
  // the fast pass of every (window, haplotype) in one launch
  std::vector<dv::FastPassWindow> fast_windows;
  size_t n_haplotypes = 0;
  const dv::FastPassAligner* any = nullptr;
  for (int32_t w = 0; w < c.n_windows; ++w) {
    const dv_align_window& win = c.windows[w];
    if (win.n_reads == 0) continue;
    Win& x = wins[static_cast<size_t>(w)];
    x.aligner = std::make_unique<dv::FastPassAligner>();
    c.set_up(win, x.aligner.get());
    x.aligner->begin_alignments(c.reads_of(win));
    any = x.aligner.get();
    fast_windows.push_back(dv::fast_pass_window_of(*any));
    x.first_haplotype = n_haplotypes;
    n_haplotypes += any->haplotypes().size();
  }
  if (!any) return DV_OK;
  dv::FastPassResults fast;
  fast.first_row.assign(1, 0);
  if (n_haplotypes > 0) {
    if (int rc = dv::fast_pass_on_device(fast_windows, dv::fast_pass_scoring_of(*any), stream, &fast, nullptr)) return rc;
  }
  // the pairs of every window through one sweep + trace-back launch whose result stays on the device
  std::vector<const dv::CodedSequence*> sequences;
  std::vector<int32_t> pair_ref, pair_query;
  for (Win& x : wins) {
    if (!x.aligner) continue;
    const size_t h = x.first_haplotype;
    const size_t row = static_cast<size_t>(fast.first_row[h]);
    x.aligner->install_fast_pass(fast.haplotype_score.data() + h, fast.haplotype_discarded.data() + h,
                                 fast.read_position.data() + row, fast.read_score.data() + row);
    x.aligner->collect_alignments(x.aligner->reads().size(), &x.pairs);
    const int32_t base = static_cast<int32_t>(sequences.size());
    for (const dv::CodedSequence& s : x.pairs.sequences) sequences.push_back(&s);
    x.first_pair = pair_ref.size();
    for (size_t k = 0; k < x.pairs.pair_ref.size(); ++k) {
      pair_ref.push_back(base + x.pairs.pair_ref[k]);
      pair_query.push_back(base + x.pairs.pair_query[k]);
    }
  }
  const dv::LocalAligner& scoring = any->local_aligner();
  std::vector<dv::SweepCorners> corners;
  std::vector<uint8_t> route;
  dv::DeviceRuns traced;
  dv::ResidentSweep sweep;
  if (!pair_ref.empty()) {
    if (int rc = dv::sweep_pairs_on_device(sequences, pair_ref, pair_query, scoring.match(), scoring.mismatch(),
                                           scoring.gap_open(), scoring.gap_extend(), stream, &corners, &route, nullptr,
                                           &traced, &sweep)) {
      return rc;
    }
    stats.bytes_down += sweep.bytes_down;
  }
  // the windows inside the limits on the device, the others as the host route finishes them
  std::vector<dv::FinishWindow> on_device;
  for (Win& x : wins) {
    if (!x.aligner) continue;
    ++stats.windows;
    const size_t n_pairs = x.pairs.pair_ref.size();
    if (dv::window_finishes_on_device(x.first_pair, n_pairs, route, corners, sweep)) {
      on_device.push_back(dv::FinishWindow{x.aligner.get(), &x.pairs, x.first_pair, &x.aligned});
      continue;
    }
    ++stats.windows_on_host;
    std::vector<dv::LocalAlignment> results(n_pairs);
    std::vector<char> ok(n_pairs, 0);
    for (size_t k = 0; k < n_pairs; ++k) {
      const dv::CodedSequence& ref = *sequences[pair_ref[x.first_pair + k]];
      const dv::CodedSequence& q = *sequences[pair_query[x.first_pair + k]];
      if (route[x.first_pair + k] == dv::kRouteDevice) {
        ok[k] = scoring.complete(ref, q, corners[x.first_pair + k], &results[k]);
      } else if (route[x.first_pair + k] == dv::kRouteHost) {
        std::vector<dv::LocalAlignment> one;
        std::vector<char> one_ok;
        scoring.align_pairs({&ref}, {&q}, &one, &one_ok);
        results[k] = std::move(one[0]);
        ok[k] = one_ok[0];
      }
    }
    x.aligned = x.aligner->finish_alignments(x.pairs, results.data(), ok.data());
  }
  if (!sweep.stream) sweep.stream = stream;     // no pair was swept: the caller's stream
  if (int rc = dv::finish_windows_on_device(on_device, sweep, c.options.force_alignment, c.normalize_reads, &stats)) {
    return rc;
  }
  for (Win& x : wins) append(x.aligned, res);
  return DV_OK;
}

}  // namespace

extern "C" {

int dv_align_windows_batch(int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
                           const dv_align_window* windows, const dv_aligner_options* options,
                           dv_aligned_windows** out) {
  return dv::guarded("dv_align_windows_batch", [&]() -> int {
    Call c;
    if (int rc = parse("dv_align_windows_batch", n_seqs, bytes, seq_off, n_windows, windows, options, out, &c)) return rc;
    auto res = std::make_unique<dv_aligned_windows>();
    res->window_read_off.assign(1, 0);
    res->cigar_off.assign(1, 0);
    for (int32_t w = 0; w < n_windows; ++w) {
      std::vector<dv::RealignedRead> aligned;
      if (windows[w].n_reads > 0) {
        dv::FastPassAligner a;
        c.set_up(windows[w], &a);
        aligned = a.align_reads(c.reads_of(windows[w]));
      }
      append(aligned, res.get());
    }
    *out = res.release();
    return DV_OK;
  });
}

int dv_align_windows_batch_device(int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
                                  const dv_align_window* windows, const dv_aligner_options* options,
                                  dv_aligned_windows** out, void* stream) {
  return dv::guarded("dv_align_windows_batch_device", [&]() -> int {
    dv::last_finish_stats() = dv::FinishStats();
    Call c;
    if (int rc = parse("dv_align_windows_batch_device", n_seqs, bytes, seq_off, n_windows, windows, options, out, &c)) {
      return rc;
    }
    auto res = std::make_unique<dv_aligned_windows>();
    res->window_read_off.assign(1, 0);
    res->cigar_off.assign(1, 0);
    int64_t reads = 0;
    for (int32_t w = 0; w < n_windows; ++w) reads += windows[w].n_reads;
    if (reads > 0) {
      int count = 0;
      if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        return dv::fail(DV_ERR_NO_DEVICE,
                        "dv_align_windows_batch_device: no HIP device (dv_align_windows_batch is the host code)");
      }
      if (int rc = align_on_device(c, stream, res.get())) return rc;
    } else {
      for (int32_t w = 0; w < n_windows; ++w) res->window_read_off.push_back(0);
    }
    *out = res.release();
    return DV_OK;
  });
}

int dv_aligned_windows_arrays(const dv_aligned_windows* a, dv_aligned_windows_view* out) {
  if (!a || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_aligned_windows_arrays: null");
  out->n_windows = static_cast<int32_t>(a->window_read_off.size() - 1);
  out->n_reads = static_cast<int32_t>(a->status.size());
  out->n_words = static_cast<int64_t>(a->cigar.size());
  out->window_read_off = a->window_read_off.data();
  out->status = a->status.data();
  out->position = a->position.data();
  out->cigar_off = a->cigar_off.data();
  out->cigar = a->cigar.data();
  return DV_OK;
}

void dv_aligned_windows_free(dv_aligned_windows* a) { delete a; }

int dv_realign_finish_sorted_order(int32_t n, const int32_t* scores, int32_t* order_records, int32_t* order_objects) {
  return dv::guarded("dv_realign_finish_sorted_order", [&]() -> int {
    if (n < 0 || (n > 0 && (!scores || !order_records || !order_objects))) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_realign_finish_sorted_order: null pointer or negative count");
    }
    dv::fin::sorted_order(scores, n, order_records);
    std::vector<dv::HaplotypeAlignment> real(static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i) {
      real[static_cast<size_t>(i)].haplotype_index = static_cast<size_t>(i);
      real[static_cast<size_t>(i)].haplotype_score = scores[i];
      real[static_cast<size_t>(i)].reads.resize(2);
    }
    std::sort(real.begin(), real.end(), [](const dv::HaplotypeAlignment& a, const dv::HaplotypeAlignment& b) {
      return a.haplotype_score < b.haplotype_score;
    });
    for (int32_t i = 0; i < n; ++i) order_objects[i] = static_cast<int32_t>(real[static_cast<size_t>(i)].haplotype_index);
    return DV_OK;
  });
}

int dv_realign_finish_last_stats(dv_realign_finish_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_realign_finish_last_stats: null");
  const dv::FinishStats& s = dv::last_finish_stats();
  out->windows = s.windows;
  out->windows_on_host = s.windows_on_host;
  out->reads = s.reads;
  out->cigar_words = s.cigar_words;
  out->launches = s.launches;
  out->bytes_down = s.bytes_down;
  return DV_OK;
}

}  // extern "C"
