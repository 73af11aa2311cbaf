// Alt-aligned realignment of trimmed reads on a packed read table: dv_alt_align_batch (host code) and
// dv_alt_align_batch_device (fast pass, sweeps and three finish kernels), include/dvhip.h.
//
// The contract -- RealignReadsToHaplotype (deepvariant/alt_aligned_pileup_lib.cc:278-313): per (candidate, sample, alt
// allele) a FastPassAligner with ONE haplotype that IS its reference (the target), force_alignment, no padding -- is
// FastPassAligner::align_reads, which stays the checker and the host entry point's code.  In that special case the
// haplotype is never discarded, its CIGAR to the reference is "<n>=" (every position maps with shift 0), and the
// score threshold decides nothing, so for pair (item t, read R of L bytes, upper-cased; target T of n bytes):
//
// Choice.  The fast pass' position p >= 0 gives the read-to-haplotype alignment "<L>=" at p.  Otherwise the local
// aligner's result with score > 0 gives p = uint16_t(ref_begin) and its CIGAR, soft clips included, one run per
// token ('=' and 'X' stay separate runs of M).  Otherwise status 2.
// Merge (calculate_read_to_ref_alignment against "<n>=").  p >= n: status 0 (nothing of the haplotype is left).  A
// leading S is merged as it is and takes no haplotype base.  Then run by run against the n - p matches: I is merged
// whole; S, D and M are merged for min(run, haplotype bases left) and take that many.  Once the haplotype is used
// up the runs not yet started are merged whole, and what is left of a started run is merged if it is S and clears
// the CIGAR (status 0) otherwise; so do runs that remain when the read-consuming lengths have reached L.
// merge_cigar_op, run-wise: lengths of S / I / M are capped by L - (read bases merged so far), nothing is merged once
// that is 0; an I arriving on a D (or a D on an I) cancels base by base, each cancelled base a match added to the M
// in front of the indel or planted there; otherwise equal kinds add up and others are appended.  Only the last two
// operations are ever touched, so the kernels stream: two held operations, every older one final.
// Normalisation (is_alignment_normalized at reference offset p), evaluated as operations become final: an I whose
// last read base equals T[ref_i - 1], or a D whose last target base equals R[read_i - 1], or one that runs past its
// sequence, is not normalised: status 0 unless normalize_reads.
// Result.  Status 1, position = ref_start + p, the merged words; an empty CIGAR is status 0.
// alt_align.h's finish_pair() is that text as code, compiled for both sides.
//
// Device route.  Plan on the host from the arrays alone.  Stage A: one FastPassWindow per item through
// fast_pass_on_device.  Stage B: every unplaced read against its item's target through sweep_pairs_on_device;
// complete_on_device_route writes the text CIGAR (from the device's runs where it traced the pair back), whose
// tokens become the run words.  Stage C, the kernels below, one lane per pair: count (finish_pair without output:
// status, position, words), scan (one workgroup: exclusive scan of the word counts), emit (finish_pair again, writing
// at the scanned offset).  Placement is a pure function of the input; there are no atomics.  An item whose target
// does not fit the fast pass kernel runs through FastPassAligner inside the call.
#include <hip/hip_runtime.h>

#include <cctype>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#include "alt_align.h"
#include "device_round_trip.h"
#include "fast_pass_aligner.h"
#include "fast_pass_device.h"
#include "local_align_device.h"

namespace {

using dv::alt::PairCount;
using dv::alt::PairIn;

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxPairs = int64_t{1} << 28;
constexpr int64_t kMaxBytes = int64_t{1} << 30;

struct Header {          // the download's first bytes
  int64_t n_words;
  int64_t reserved;
};

struct Inputs {          // device pointers into the upload
  const PairIn* pairs;
  const int64_t* ref_start;   // per pair
  const uint32_t* runs;
  const uint8_t* bytes;
  int32_t n_pairs, normalize_reads;
  uint32_t word_bound;        // the words the download holds
};

struct Outputs {         // device pointers into the download
  Header* header;
  int32_t* status;
  int64_t* position;
  uint32_t* cigar_off;        // [n_pairs + 1]
  uint32_t* cigar;
};

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t up = __shfl_up(v, d, kWave);
    if (lane >= d) v += up;
  }
  return v;
}

// Pass 1: the closed form per pair, nothing written but the pair's status, position and word count.
__global__ __launch_bounds__(kThreads) void alt_finish_count_kernel(Inputs in, PairCount* counts, Outputs o) {
  const long long d = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (d >= in.n_pairs) return;
  const PairIn pr = in.pairs[d];
  int32_t n_words = 0;
  const int status = dv::alt::finish_pair(pr, in.bytes, in.runs, in.normalize_reads != 0, nullptr, &n_words);
  counts[d] = PairCount{status, n_words};
  o.status[d] = status;
  o.position[d] = status == 1 ? in.ref_start[d] + pr.p : 0;
}

// Pass 2: exclusive scan of the word counts over the pairs in order, by one workgroup.
__global__ __launch_bounds__(kScanThreads) void alt_finish_scan_kernel(Inputs in, const PairCount* counts, Outputs o) {
  __shared__ uint32_t wave_words[kScanThreads / kWave];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int32_t base = 0; base < in.n_pairs; base += kScanThreads) {
    const int32_t p = base + tid;
    const uint32_t words = p < in.n_pairs ? static_cast<uint32_t>(counts[p].n_words) : 0u;
    const uint32_t incl = wave_inclusive_scan(words, lane);
    if (lane == kWave - 1) wave_words[wave] = incl;
    __syncthreads();
    uint32_t before = carry;
    for (int w = 0; w < wave; ++w) before += wave_words[w];
    if (p < in.n_pairs) o.cigar_off[p] = before + incl - words;
    __syncthreads();
    if (tid == kScanThreads - 1) carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) {
    o.cigar_off[in.n_pairs] = carry;
    o.header->n_words = carry;
    o.header->reserved = 0;
  }
}

// Pass 3: the words of every status-1 pair, at the place pass 2 gave them.
__global__ __launch_bounds__(kThreads) void alt_finish_emit_kernel(Inputs in, const PairCount* counts, Outputs o) {
  const long long d = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (d >= in.n_pairs) return;
  const PairCount c = counts[d];
  if (c.status != 1 || c.n_words <= 0) return;
  const uint32_t at = o.cigar_off[d];
  if (static_cast<unsigned long long>(at) + static_cast<unsigned long long>(c.n_words) > in.word_bound) return;
  int32_t n_words = 0;
  dv::alt::finish_pair(in.pairs[d], in.bytes, in.runs, in.normalize_reads != 0, o.cigar + at, &n_words);
}

dv_alt_align_stats& last_stats() {
  static thread_local dv_alt_align_stats stats;
  return stats;
}

}  // namespace

struct dv_alt_aligned {
  std::vector<int32_t> item_pair_off, status;
  std::vector<int64_t> position;
  std::vector<uint32_t> cigar_off, cigar;
};

namespace {

// The call's arguments, checked.
struct Call {
  const dv_batch* reads = nullptr;
  int32_t n_items = 0;
  const dv_alt_align_item* items = nullptr;
  const char* target_bytes = nullptr;
  const int64_t* target_off = nullptr;
  dv::AlignerOptions options;          // read_size is the item's
  bool normalize_reads = false;
  dv::FastPassScoring scoring{0, 0, 0, 0};
  int gap_open = 0, gap_extend = 0;
  std::vector<int32_t> item_pair_off;  // [n_items + 1]

  std::string_view target(int32_t s) const {
    return std::string_view(target_bytes + target_off[s], static_cast<size_t>(target_off[s + 1] - target_off[s]));
  }
  std::string read(int32_t row) const {
    const uint32_t a = reads->read_seq_off[row], b = reads->read_seq_off[row + 1];
    return std::string(reinterpret_cast<const char*>(reads->bases) + a, b - a);
  }
  void set_up(const dv_alt_align_item& item, dv::FastPassAligner* a) const {
    dv::AlignerOptions o = options;
    o.read_size = item.read_size;
    std::string error;
    a->set_options(o, &error);         // checked by parse()
    a->set_normalize_reads(normalize_reads);
    const std::string t(target(item.target));
    a->set_reference(t);
    a->set_ref_start(static_cast<uint64_t>(item.ref_start));
    a->set_haplotypes({t});
  }
  std::vector<std::string> reads_of(const dv_alt_align_item& item) const {
    std::vector<std::string> out;
    out.reserve(static_cast<size_t>(item.n_rows));
    for (int32_t r = 0; r < item.n_rows; ++r) out.push_back(read(item.first_row + r));
    return out;
  }
};

int parse(const char* who, const dv_batch* reads, int32_t n_items, const dv_alt_align_item* items, int32_t n_targets,
          const char* target_bytes, const int64_t* target_off, const dv_aligner_options* o, dv_alt_aligned** out,
          Call* c) {
  const std::string name(who);
  if (out) *out = nullptr;
  if (!out || !reads || !o || n_items < 0 || n_targets < 0 || (n_items > 0 && !items) || (n_targets > 0 && !target_off) ||
      reads->n_reads < 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null pointer or negative count");
  }
  if (reads->memory != DV_MEM_HOST) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": the read table must be in host memory");
  const int32_t n = reads->n_reads;
  if (n > 0) {
    if (!reads->read_seq_off) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null read_seq_off");
    for (int32_t r = 0; r < n; ++r) {
      if (reads->read_seq_off[r + 1] < reads->read_seq_off[r]) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": offsets must ascend");
      }
    }
    if (reads->read_seq_off[n] > reads->n_bases) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": offsets run past n_bases");
    if (reads->read_seq_off[n] > reads->read_seq_off[0] && !reads->bases) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null bases");
  }
  if (int rc = dv::check_sequence_table(name, n_targets, target_off)) return rc;
  if (n_targets > 0 && target_off[n_targets] > target_off[0] && !target_bytes) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null target_bytes");
  }
  if (o->force_alignment != 1 || o->ref_prefix_len != 0 || o->ref_suffix_len != 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": force_alignment must be 1, ref_prefix_len and ref_suffix_len 0");
  }
  c->options.match = o->match;
  c->options.mismatch = o->mismatch;
  c->options.gap_open = o->gap_open;
  c->options.gap_extend = o->gap_extend;
  c->options.kmer_size = o->kmer_size;
  c->options.max_num_of_mismatches = o->max_num_of_mismatches;
  c->options.similarity_threshold = o->realignment_similarity_threshold;
  c->options.force_alignment = true;
  c->normalize_reads = o->normalize_reads != 0;
  dv::FastPassAligner resolved;
  std::string error;
  if (!resolved.set_options(c->options, &error)) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": " + error);
  resolved.init_local_aligner();
  c->scoring = dv::fast_pass_scoring_of(resolved);
  c->gap_open = resolved.local_aligner().gap_open();
  c->gap_extend = resolved.local_aligner().gap_extend();
  if (c->scoring.match > dv::kDeviceAlignMaxScoringValue || c->scoring.mismatch > dv::kDeviceAlignMaxScoringValue ||
      c->gap_open > dv::kDeviceAlignMaxScoringValue || c->gap_extend > dv::kDeviceAlignMaxScoringValue) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": scoring values are limited to 127 (the aligner's int8_t matrix)");
  }
  int64_t pairs = 0;
  c->item_pair_off.assign(1, 0);
  for (int32_t t = 0; t < n_items; ++t) {
    const dv_alt_align_item& it = items[t];
    if (it.first_row < 0 || it.n_rows < 0 || static_cast<int64_t>(it.first_row) + it.n_rows > n || it.target < 0 ||
        it.target >= n_targets || it.ref_start < 0 || it.read_size < 0) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": item " + std::to_string(t) +
                                                   ": row range, target, ref_start or read_size out of range");
    }
    pairs += it.n_rows;
    if (pairs >= kMaxPairs) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": more than 2^28 pairs in one call; pass fewer items");
    c->item_pair_off.push_back(static_cast<int32_t>(pairs));
  }
  c->reads = reads;
  c->n_items = n_items;
  c->items = items;
  c->target_bytes = target_bytes;
  c->target_off = target_off;
  return DV_OK;
}

// One pair's result while the call is assembled.
struct PairOut {
  int32_t status = 0;
  int64_t position = 0;
  std::vector<uint32_t> words;
};

void take(const dv::RealignedRead& r, PairOut* out) {
  out->status = r.status;
  out->position = r.status == 1 ? r.position : 0;
  out->words.clear();
  if (r.status != 1) return;
  for (const dv::CigarOp& op : r.cigar) {
    out->words.push_back((static_cast<uint32_t>(op.length) << 4) | static_cast<uint32_t>(op.op));
  }
}

void append(const PairOut& p, dv_alt_aligned* res) {
  res->status.push_back(p.status);
  res->position.push_back(p.position);
  res->cigar.insert(res->cigar.end(), p.words.begin(), p.words.end());
  res->cigar_off.push_back(static_cast<uint32_t>(res->cigar.size()));
}

int align_on_host(const Call& c, dv_alt_aligned* res) {
  res->item_pair_off = c.item_pair_off;
  res->cigar_off.assign(1, 0);
  for (int32_t t = 0; t < c.n_items; ++t) {
    const dv_alt_align_item& item = c.items[t];
    if (item.n_rows == 0) continue;
    dv::FastPassAligner a;
    c.set_up(item, &a);
    const std::vector<dv::RealignedRead> out = a.align_reads(c.reads_of(item));
    for (const dv::RealignedRead& r : out) {
      PairOut p;
      take(r, &p);
      append(p, res);
    }
  }
  return DV_OK;
}

// An item outside the device's limits, inside the device call: align_reads in its phases, so that the pairs the
// fast pass placed can be counted.
void item_on_host(const Call& c, const dv_alt_align_item& item, PairOut* out, dv_alt_align_stats* stats) {
  dv::FastPassAligner a;
  c.set_up(item, &a);
  a.begin_alignments(c.reads_of(item));
  dv::FastPassResults fast;
  dv::fast_pass_on_host({dv::fast_pass_window_of(a)}, dv::fast_pass_scoring_of(a), &fast);
  a.install_fast_pass(fast.haplotype_score.data(), fast.haplotype_discarded.data(), fast.read_position.data(),
                      fast.read_score.data());
  dv::AlignmentPairs pairs;
  a.collect_alignments(static_cast<size_t>(item.n_rows), &pairs);
  std::vector<dv::LocalAlignment> results;
  std::vector<char> ok;
  a.align_pairs_on_host(pairs, 0, pairs.pair_ref.size(), &results, &ok);
  const int64_t swept = static_cast<int64_t>(pairs.pair_ref.size() - pairs.n_haplotype_pairs);
  stats->pairs_swept += swept;
  stats->pairs_swept_on_host += swept;
  stats->pairs_fast += item.n_rows - swept;
  const std::vector<dv::RealignedRead> res = a.finish_alignments(pairs, results.data(), ok.data());
  for (int32_t r = 0; r < item.n_rows; ++r) take(res[static_cast<size_t>(r)], &out[r]);
}

int align_on_device(const Call& c, void* stream_in, dv_alt_aligned* res, dv_alt_align_stats* stats) {
  const dv_batch& b = *c.reads;
  const size_t n_pairs = static_cast<size_t>(c.item_pair_off.back());
  // the reads, upper-cased once
  const uint32_t base0 = b.read_seq_off[0];
  std::string upper;
  if (b.read_seq_off[b.n_reads] > base0) {
    upper.assign(reinterpret_cast<const char*>(b.bases) + base0, b.read_seq_off[b.n_reads] - base0);
  }
  for (char& ch : upper) ch = static_cast<char>(std::toupper(static_cast<unsigned char>(ch)));
  auto read_view = [&](int32_t row) {
    return std::string_view(upper.data() + (b.read_seq_off[row] - base0), b.read_seq_off[row + 1] - b.read_seq_off[row]);
  };
  std::vector<PairOut> host_out(n_pairs);      // used by the pairs of items on the host
  std::vector<int32_t> device_index(n_pairs, -1);

  // ---- plan: which items the device takes
  std::vector<int32_t> dev_items;
  std::vector<dv::FastPassWindow> windows;
  for (int32_t t = 0; t < c.n_items; ++t) {
    const dv_alt_align_item& item = c.items[t];
    if (item.n_rows == 0) continue;
    const std::string_view target = c.target(item.target);
    if (target.empty() || target.size() > static_cast<size_t>(dv::kFastPassMaxHaplotype) || target.size() >= 0xffff) {
      ++stats->items_on_host;
      item_on_host(c, item, &host_out[static_cast<size_t>(c.item_pair_off[t])], stats);
      continue;
    }
    dv::FastPassWindow w;
    w.reads.reserve(static_cast<size_t>(item.n_rows));
    for (int32_t r = 0; r < item.n_rows; ++r) w.reads.push_back(read_view(item.first_row + r));
    w.haplotypes.push_back(target);
    w.reference = target;
    dev_items.push_back(t);
    windows.push_back(std::move(w));
  }

  std::vector<PairIn> pairs;
  std::vector<int64_t> pair_ref_start;
  std::vector<uint32_t> run_words;
  int64_t word_bound = 0;
  if (!dev_items.empty()) {
    // ---- stage A: the fast pass
    dv::FastPassResults fast;
    dv::FastPassStats fp_stats;
    if (int rc = dv::fast_pass_on_device(windows, c.scoring, stream_in, &fast, &fp_stats)) return rc;
    stats->launches += fp_stats.launches;

    // the byte table of the finish kernels: the upper-cased reads, then each device item's target
    int64_t n_bytes = static_cast<int64_t>(upper.size());
    std::vector<int32_t> item_target_off(dev_items.size());
    for (size_t x = 0; x < dev_items.size(); ++x) {
      item_target_off[x] = static_cast<int32_t>(n_bytes);
      n_bytes += static_cast<int64_t>(windows[x].reference.size());
      if (n_bytes >= kMaxBytes) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_alt_align_batch_device: more than 1 GiB of sequence in one call; pass fewer items");
    }

    // ---- stage B: the sweeps of the reads the fast pass did not place
    std::vector<dv::CodedSequence> coded;
    std::vector<int32_t> row_sequence(static_cast<size_t>(b.n_reads), -1);
    std::vector<int32_t> sweep_ref, sweep_query, sweep_pair;   // sweep k -> device pair
    coded.reserve(dev_items.size() + static_cast<size_t>(b.n_reads));
    for (size_t x = 0; x < dev_items.size(); ++x) {
      const int32_t t = dev_items[x];
      const dv_alt_align_item& item = c.items[t];
      const std::string_view target = windows[x].reference;
      const bool any_placed = fast.haplotype_score[x] != 0;
      int32_t target_sequence = -1;
      for (int32_t r = 0; r < item.n_rows; ++r) {
        const int32_t row = item.first_row + r;
        const size_t fast_row = static_cast<size_t>(fast.first_row[x]) + static_cast<size_t>(r);
        const std::string_view read = windows[x].reads[static_cast<size_t>(r)];
        PairIn pr;
        pr.target_off = item_target_off[x];
        pr.target_len = static_cast<int32_t>(target.size());
        pr.read_off = static_cast<int32_t>(b.read_seq_off[row] - base0);
        pr.read_len = static_cast<int32_t>(read.size());
        pr.kind = dv::alt::kKindNone;
        pr.p = 0;
        pr.run_off = 0;
        pr.n_runs = 0;
        if (any_placed && fast.read_position[fast_row] >= 0 && fast.read_score[fast_row] > 0) {
          pr.kind = dv::alt::kKindFast;
          pr.p = fast.read_position[fast_row];
          ++stats->pairs_fast;
        } else {
          if (target_sequence < 0) {
            target_sequence = static_cast<int32_t>(coded.size());
            coded.push_back(dv::encode_sequence(std::string(target)));
          }
          if (row_sequence[static_cast<size_t>(row)] < 0) {
            row_sequence[static_cast<size_t>(row)] = static_cast<int32_t>(coded.size());
            coded.push_back(dv::encode_sequence(std::string(read)));
          }
          sweep_ref.push_back(target_sequence);
          sweep_query.push_back(row_sequence[static_cast<size_t>(row)]);
          sweep_pair.push_back(static_cast<int32_t>(pairs.size()));
          ++stats->pairs_swept;
        }
        device_index[static_cast<size_t>(c.item_pair_off[t]) + static_cast<size_t>(r)] = static_cast<int32_t>(pairs.size());
        pairs.push_back(pr);
        pair_ref_start.push_back(item.ref_start);
      }
    }
    if (!sweep_pair.empty()) {
      std::vector<const dv::CodedSequence*> sequences(coded.size());
      for (size_t s = 0; s < coded.size(); ++s) sequences[s] = &coded[s];
      std::vector<dv::SweepCorners> corners;
      std::vector<uint8_t> route;
      dv::DeviceRuns traced;
      dv::DeviceAlignStats sweep_stats;
      if (int rc = dv::sweep_pairs_on_device(sequences, sweep_ref, sweep_query, c.scoring.match, c.scoring.mismatch,
                                             c.gap_open, c.gap_extend, stream_in, &corners, &route, &sweep_stats,
                                             &traced)) {
        return rc;
      }
      stats->launches += sweep_stats.launches;
      stats->pairs_swept_on_host += sweep_stats.pairs_on_host;
      stats->pairs_traced_on_host += dv::last_traceback_stats().traced_on_host;
      const dv::LocalAligner aligner(c.scoring.match, c.scoring.mismatch, c.gap_open, c.gap_extend);
      for (size_t k = 0; k < sweep_pair.size(); ++k) {
        const dv::CodedSequence& ref = coded[static_cast<size_t>(sweep_ref[k])];
        const dv::CodedSequence& q = coded[static_cast<size_t>(sweep_query[k])];
        dv::LocalAlignment r;
        bool ok = false;
        if (route[k] == dv::kRouteDevice) {
          ok = dv::complete_on_device_route(aligner, ref, q, corners[k], &traced, k, &r);
        } else if (route[k] == dv::kRouteHost) {
          std::vector<dv::LocalAlignment> one;
          std::vector<char> one_ok;
          aligner.align_pairs({&ref}, {&q}, &one, &one_ok);
          r = one[0];
          ok = one_ok[0] != 0;
        }
        if (!ok || r.score <= 0) continue;     // status 2
        PairIn& pr = pairs[static_cast<size_t>(sweep_pair[k])];
        pr.kind = dv::alt::kKindSw;
        pr.p = static_cast<uint16_t>(r.ref_begin);
        pr.run_off = static_cast<int32_t>(run_words.size());
        for (const dv::CigarOp& op : dv::parse_cigar(r.cigar)) {
          run_words.push_back((static_cast<uint32_t>(op.length) << 4) | static_cast<uint32_t>(op.op));
        }
        pr.n_runs = static_cast<int32_t>(run_words.size()) - pr.run_off;
      }
    }
    // a merge call leaves two operations at most, and a pair makes one call per run and one more
    for (const PairIn& pr : pairs) {
      word_bound += pr.kind == dv::alt::kKindFast ? 1 : pr.kind == dv::alt::kKindSw ? 2 * pr.n_runs + 4 : 0;
    }
    if (word_bound >= (int64_t{1} << 31) || run_words.size() >= (size_t{1} << 31)) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_alt_align_batch_device: more than 2^31 CIGAR words in one call; pass fewer items");
    }

    // ---- stage C: finish every pair
    const size_t nd = pairs.size(), bound = static_cast<size_t>(word_bound);
    dv::Layout up, down, work;
    const size_t u_pairs = up.add(nd * sizeof(PairIn));
    const size_t u_start = up.add(nd * sizeof(int64_t));
    const size_t u_runs = up.add(run_words.size() * sizeof(uint32_t));
    const size_t u_bytes = up.add(static_cast<size_t>(n_bytes));
    const size_t d_header = down.add(sizeof(Header));
    const size_t d_status = down.add(nd * sizeof(int32_t));
    const size_t d_position = down.add(nd * sizeof(int64_t));
    const size_t d_coff = down.add((nd + 1) * sizeof(uint32_t));
    const size_t d_words = down.add(bound * sizeof(uint32_t));
    const size_t k_counts = work.add(nd * sizeof(PairCount));
    static thread_local dv::RoundTrip rt;     // its scratch: the PairCount per pair
    if (int rc = rt.begin("dv_alt_align_batch_device: no HIP device (dv_alt_align_batch is the host code)", stream_in,
                          up.bytes(), down.bytes(), work.bytes())) {
      return rc;
    }
    std::memcpy(rt.host_up<PairIn>(u_pairs), pairs.data(), nd * sizeof(PairIn));
    std::memcpy(rt.host_up<int64_t>(u_start), pair_ref_start.data(), nd * sizeof(int64_t));
    if (!run_words.empty()) std::memcpy(rt.host_up<uint32_t>(u_runs), run_words.data(), run_words.size() * sizeof(uint32_t));
    uint8_t* bytes = rt.host_up<uint8_t>(u_bytes);
    if (!upper.empty()) std::memcpy(bytes, upper.data(), upper.size());
    for (size_t x = 0; x < dev_items.size(); ++x) {
      const std::string_view target = windows[x].reference;
      if (!target.empty()) std::memcpy(bytes + item_target_off[x], target.data(), target.size());
    }
    Inputs in;
    in.pairs = rt.dev_up<const PairIn>(u_pairs);
    in.ref_start = rt.dev_up<const int64_t>(u_start);
    in.runs = rt.dev_up<const uint32_t>(u_runs);
    in.bytes = rt.dev_up<const uint8_t>(u_bytes);
    in.n_pairs = static_cast<int32_t>(nd);
    in.normalize_reads = c.normalize_reads ? 1 : 0;
    in.word_bound = static_cast<uint32_t>(bound);
    Outputs o;
    o.header = rt.dev_down<Header>(d_header);
    o.status = rt.dev_down<int32_t>(d_status);
    o.position = rt.dev_down<int64_t>(d_position);
    o.cigar_off = rt.dev_down<uint32_t>(d_coff);
    o.cigar = rt.dev_down<uint32_t>(d_words);
    PairCount* d_counts = reinterpret_cast<PairCount*>(static_cast<uint8_t*>(rt.d_scratch.ptr) + k_counts);
    const unsigned blocks = static_cast<unsigned>((nd + kThreads - 1) / kThreads);
    hipStream_t stream = rt.stream();
    if (int rc = rt.upload(up.bytes())) return rc;
    {
      dv::ProfileScope prof(dv::kProfOther, stream);
      hipLaunchKernelGGL(alt_finish_count_kernel, dim3(blocks), dim3(kThreads), 0, stream, in, d_counts, o);
      DV_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(alt_finish_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, in, d_counts, o);
      DV_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(alt_finish_emit_kernel, dim3(blocks), dim3(kThreads), 0, stream, in, d_counts, o);
      DV_HIP_CHECK(hipGetLastError());
    }
    if (int rc = rt.finish(down.bytes())) return rc;
    stats->launches += 3;
    const Header header = *rt.host_down<Header>(d_header);
    if (header.n_words < 0 || static_cast<size_t>(header.n_words) > bound) {
      return dv::fail(DV_ERR_HIP, "dv_alt_align_batch_device: totals past their bounds");
    }
    // ---- the call's arrays: the device's pairs and the host items' pairs, in pair order
    const int32_t* status = rt.host_down<int32_t>(d_status);
    const int64_t* position = rt.host_down<int64_t>(d_position);
    const uint32_t* coff = rt.host_down<uint32_t>(d_coff);
    const uint32_t* words = rt.host_down<uint32_t>(d_words);
    res->item_pair_off = c.item_pair_off;
    res->cigar_off.assign(1, 0);
    res->status.reserve(n_pairs);
    res->position.reserve(n_pairs);
    res->cigar_off.reserve(n_pairs + 1);
    res->cigar.reserve(static_cast<size_t>(header.n_words));
    for (size_t g = 0; g < n_pairs; ++g) {
      const int32_t d = device_index[g];
      if (d < 0) {
        append(host_out[g], res);
        continue;
      }
      if (coff[d + 1] < coff[d] || coff[d + 1] > header.n_words) {
        return dv::fail(DV_ERR_HIP, "dv_alt_align_batch_device: word offsets out of order");
      }
      res->status.push_back(status[d]);
      res->position.push_back(position[d]);
      res->cigar.insert(res->cigar.end(), words + coff[d], words + coff[d + 1]);
      res->cigar_off.push_back(static_cast<uint32_t>(res->cigar.size()));
    }
  } else {
    res->item_pair_off = c.item_pair_off;
    res->cigar_off.assign(1, 0);
    for (size_t g = 0; g < n_pairs; ++g) append(host_out[g], res);
  }
  for (int32_t s : res->status) {
    if (s == 0) ++stats->status0;
    if (s == 1) ++stats->status1;
    if (s == 2) ++stats->status2;
  }
  stats->words_written = static_cast<int64_t>(res->cigar.size());
  return DV_OK;
}

int run(const char* who, bool on_device, const dv_batch* reads, int32_t n_items, const dv_alt_align_item* items,
        int32_t n_targets, const char* target_bytes, const int64_t* target_off, const dv_aligner_options* options,
        dv_alt_aligned** out, void* stream) {
  return dv::guarded(who, [&]() -> int {
    if (on_device) last_stats() = dv_alt_align_stats{};
    Call c;
    if (int rc = parse(who, reads, n_items, items, n_targets, target_bytes, target_off, options, out, &c)) return rc;
    auto res = std::make_unique<dv_alt_aligned>();
    int rc = DV_OK;
    if (!on_device) {
      rc = align_on_host(c, res.get());
    } else if (c.item_pair_off.back() == 0) {        // nothing to launch
      res->item_pair_off = c.item_pair_off;
      res->cigar_off.assign(1, 0);
      last_stats().items = n_items;
    } else {
      int count = 0;
      if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        return dv::fail(DV_ERR_NO_DEVICE, std::string(who) + ": no HIP device (dv_alt_align_batch is the host code)");
      }
      last_stats().items = n_items;
      last_stats().pairs = c.item_pair_off.back();
      rc = align_on_device(c, stream, res.get(), &last_stats());
    }
    if (rc) return rc;
    *out = res.release();
    return DV_OK;
  });
}

}  // namespace

extern "C" {

int dv_alt_align_batch(const dv_batch* reads, int32_t n_items, const dv_alt_align_item* items, int32_t n_targets,
                       const char* target_bytes, const int64_t* target_off, const dv_aligner_options* options,
                       dv_alt_aligned** out) {
  return run("dv_alt_align_batch", false, reads, n_items, items, n_targets, target_bytes, target_off, options, out,
             nullptr);
}

int dv_alt_align_batch_device(const dv_batch* reads, int32_t n_items, const dv_alt_align_item* items,
                              int32_t n_targets, const char* target_bytes, const int64_t* target_off,
                              const dv_aligner_options* options, dv_alt_aligned** out, void* stream) {
  return run("dv_alt_align_batch_device", true, reads, n_items, items, n_targets, target_bytes, target_off, options,
             out, stream);
}

int dv_alt_aligned_arrays(const dv_alt_aligned* a, dv_alt_aligned_view* out) {
  if (!a || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_alt_aligned_arrays: null");
  out->n_items = static_cast<int32_t>(a->item_pair_off.size()) - 1;
  out->n_pairs = static_cast<int32_t>(a->status.size());
  out->n_words = static_cast<int64_t>(a->cigar.size());
  out->item_pair_off = a->item_pair_off.data();
  out->status = a->status.data();
  out->position = a->position.data();
  out->cigar_off = a->cigar_off.data();
  out->cigar = a->cigar.data();
  return DV_OK;
}

void dv_alt_aligned_free(dv_alt_aligned* a) { delete a; }

int dv_alt_align_device_last_stats(dv_alt_align_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_alt_align_device_last_stats: null");
  *out = last_stats();
  return DV_OK;
}

}  // extern "C"
