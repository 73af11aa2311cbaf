// Alt-aligned realignment on a packed read table (dv_alt_align_batch / dv_alt_align_batch_device, include/dvhip.h):
// what alt_align.hip's host code and its finish kernels share.  The contract is written out at the top of
// alt_align.hip; finish_pair() below is the closed form of FastPassAligner::finish_alignments for one pair of the
// special case (one haplotype that is the reference, force_alignment), written once for the host and the device.
#ifndef DV_ALT_ALIGN_H_
#define DV_ALT_ALIGN_H_

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DV_ALT_HD __host__ __device__ __forceinline__
#else
#define DV_ALT_HD inline
#endif

namespace dv {
namespace alt {

// nucleus CigarUnit::Operation, the four the aligner writes
constexpr int kM = 1, kI = 2, kD = 3, kS = 5;

// how a pair reached the finish step
constexpr int kKindNone = 0;   // no alignment at all: status 2
constexpr int kKindFast = 1;   // the fast pass placed it: read-to-haplotype is "<L>=" at `p`
constexpr int kKindSw = 2;     // Smith-Waterman with score > 0: its runs (soft clips included) at `p` = uint16(ref_begin)

struct PairIn {        // one (item, read) pair of the device route, in item order, then row order
  int32_t target_off, target_len;   // the item's target in the byte table
  int32_t read_off, read_len;       // the read, upper-cased, in the byte table
  int32_t kind, p;
  int32_t run_off, n_runs;          // kKindSw: its (length << 4 | op) runs
};

struct PairCount {     // what the count pass leaves per pair
  int32_t status;      // 0 / 1 / 2 as dv_realigned_read
  int32_t n_words;     // words of the merged CIGAR, status 1 only
};

// The merged CIGAR under construction.  merge_cigar_op only ever looks at the last operation and the one in front
// of it, and the one in front is only ever touched when the last one is an indel, so two held operations and a
// stream of finished ones restate the vector: `a` in front of `b`, `held` of them in use.  A finished operation goes
// through is_alignment_normalized's step and, when `out` is set, into the output.
struct Merger {
  int a_op = 0, a_len = 0, b_op = 0, b_len = 0, held = 0;
  int aligned = 0;                 // AlignedLength: every length but the deletions'
  int read_len = 0;
  int n_out = 0;
  uint32_t* out = nullptr;
  // is_alignment_normalized, walked as operations finish
  const uint8_t* target = nullptr;
  const uint8_t* read = nullptr;
  int target_len = 0;
  int ref_i = 0, read_i = 0;
  bool normalized = true;

  DV_ALT_HD void finish_op(int op, int len) {
    if (out) out[n_out] = (static_cast<uint32_t>(len) << 4) | static_cast<uint32_t>(op);
    ++n_out;
    if (op == kS) {
      read_i += len;
      return;
    }
    if (op != kM) {
      uint8_t last = 0;
      if (op == kD) {
        if (ref_i + len > target_len) {
          normalized = false;
          return;
        }
        if (len > 0) last = target[ref_i + len - 1];
      } else {
        if (read_i + len > read_len) {
          normalized = false;
          return;
        }
        if (len > 0) last = read[read_i + len - 1];
      }
      if ((ref_i > 0 && op == kI && ref_i - 1 < target_len && last == target[ref_i - 1]) ||
          (read_i > 0 && op == kD && read_i - 1 < read_len && last == read[read_i - 1])) {
        normalized = false;
      }
    }
    if (op != kI) ref_i += len;
    if (op != kD) read_i += len;
  }

  DV_ALT_HD void push(int op, int len) {
    if (held == 2) finish_op(a_op, a_len);
    if (held >= 1) {
      a_op = b_op;
      a_len = b_len;
    }
    b_op = op;
    b_len = len;
    if (held < 2) ++held;
  }

  // merge_cigar_op for a run.  !whole: what `len` calls with length 1 leave (the base-by-base walk against the
  // haplotype).  whole: ONE call with length `len` (the runs past the haplotype's end), which differs where an
  // insertion meets a deletion: a single call cancels a single base and drops the rest of its length.
  DV_ALT_HD void merge(int op, int len, bool whole = false) {
    const int last_op = held ? b_op : 0;
    const int new_len = op != kD ? (len < read_len - aligned ? len : read_len - aligned) : len;
    if (new_len <= 0 || aligned == read_len) return;
    if ((op == kI && last_op == kD) || (op == kD && last_op == kI)) {
      // an insertion beside a deletion: base by base they cancel into matches planted in front of the indel
      const int c = whole ? 1 : (new_len < b_len ? new_len : b_len);
      if (held == 2 && a_op == kM) {
        a_len += c;
      } else {
        if (held == 2) finish_op(a_op, a_len);
        a_op = kM;
        a_len = c;
        held = 2;
      }
      if (op == kI) aligned += c;          // D -> M adds read bases; I -> M keeps them
      b_len -= c;
      const int rest = whole ? 0 : new_len - c;
      if (b_len == 0) {                    // the indel is used up: the planted match is the last operation
        b_op = a_op;
        b_len = a_len;
        held = 1;
        if (rest > 0) {
          push(op, rest);
          if (op != kD) aligned += rest;
        }
      }
    } else if (op == last_op) {
      b_len += new_len;
      if (op != kD) aligned += new_len;
    } else {
      push(op, new_len);
      if (op != kD) aligned += new_len;
    }
  }

  DV_ALT_HD void flush() {
    if (held == 2) finish_op(a_op, a_len);
    if (held >= 1) finish_op(b_op, b_len);
    held = 0;
  }
};

// One pair: calculate_read_to_ref_alignment against a haplotype CIGAR of one match run of target_len, then
// is_alignment_normalized at offset p.  `bytes` is the table both offsets of `pr` point into, `runs` the run words.
// -> status; *n_words = the words of the merged CIGAR (written to `out` when it is set), status 1 only.
DV_ALT_HD int finish_pair(const PairIn& pr, const uint8_t* bytes, const uint32_t* runs, bool normalize_reads,
                          uint32_t* out, int32_t* n_words) {
  *n_words = 0;
  if (pr.kind == kKindNone) return 2;
  const int n = pr.target_len, L = pr.read_len, p = pr.p;
  if (p >= n) return 0;                    // the position lies outside the map / nothing of the haplotype is left
  Merger m;
  m.read_len = L;
  m.out = out;
  m.target = bytes + pr.target_off;
  m.read = bytes + pr.read_off;
  m.target_len = n;
  m.ref_i = p;
  const int n_runs = pr.kind == kKindFast ? 1 : pr.n_runs;
  const uint32_t* w = runs + pr.run_off;
  auto run_op = [&](int i) { return pr.kind == kKindFast ? kM : static_cast<int>(w[i] & 15u); };
  auto run_len = [&](int i) { return pr.kind == kKindFast ? L : static_cast<int>(w[i] >> 4); };
  int i = 0;
  if (n_runs > 0 && run_op(0) == kS) {     // the leading soft clip takes no haplotype bases
    m.merge(kS, run_len(0));
    i = 1;
  }
  int cr_op = 0, cr_len = 0, ch_len = 0;
  bool hap_run_waits = true;               // the one run of n - p matches, not fetched yet
  while ((i < n_runs || hap_run_waits) && m.aligned < L) {
    if (i < n_runs && !hap_run_waits && ch_len == 0) {   // past the haplotype: the read's operations as they are
      m.merge(run_op(i), run_len(i), true);
      ++i;
      continue;
    }
    if (i >= n_runs && cr_len == 0 && hap_run_waits) break;   // the read is used up
    if (cr_len == 0) {
      cr_op = run_op(i);
      cr_len = run_len(i);
      ++i;
    }
    if (ch_len == 0) {
      if (!hap_run_waits) break;
      ch_len = n - p;
      hap_run_waits = false;
    }
    if (cr_len > 0 && ch_len > 0) {        // against a match: S / D / I / M keep their kind; only I leaves the haplotype alone
      if (cr_op == kI) {
        m.merge(kI, cr_len);
        cr_len = 0;
      } else {
        const int t = cr_len < ch_len ? cr_len : ch_len;
        m.merge(cr_op, t);
        cr_len -= t;
        ch_len -= t;
      }
    }
  }
  if (cr_len > 0 && cr_op == kS) {         // the soft-clipped tail past the haplotype
    m.merge(kS, cr_len);
    cr_len = 0;
  }
  const bool cleared = i < n_runs || cr_len > 0;   // the read runs past the haplotype
  m.flush();
  if (cleared || m.n_out == 0) return 0;
  if (!normalize_reads && !m.normalized) return 0;
  *n_words = m.n_out;
  return 1;
}

}  // namespace alt
}  // namespace dv

#endif  // DV_ALT_ALIGN_H_
