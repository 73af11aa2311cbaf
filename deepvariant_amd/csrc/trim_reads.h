// Window trimming of reads (TrimCigar / TrimRead / TrimReads, deepvariant/alt_aligned_pileup_lib.cc:91-248) on a
// packed read table: what trim_reads.hip's host code and its kernels share.  The contract is written out at the
// top of trim_reads.hip.
#ifndef DV_TRIM_READS_H_
#define DV_TRIM_READS_H_

#include <cstdint>

namespace dv {
namespace trim {

// nucleus CigarUnit::Operation: M=1 I=2 D=3 N=4 S=5 H=6 P=7 '='=8 X=9.  Bit `op` of each mask.
constexpr uint32_t kRefAdvancing = (1u << 1) | (1u << 3) | (1u << 4) | (1u << 8) | (1u << 9);
constexpr uint32_t kReadAdvancing = (1u << 1) | (1u << 2) | (1u << 5) | (1u << 8) | (1u << 9);

// error kinds of a pair, in the order the reference checks them
constexpr int kErrCover = 1;    // C <= 0: CHECK_GT(ref_length, 0)
constexpr int kErrLength = 2;   // read_trim + new_len > the read's sequence
constexpr unsigned long long kNoError = ~0ull;

struct Pair {        // one (window, read) that passed the overlap test
  int32_t window, row;
};

// What the count pass leaves per pair for the emit pass.
struct PairResult {
  int32_t kept;        // passes the filter: span >= min_overlap && new_len > 0
  int32_t first;       // a: the first kept operation
  int32_t n_words;     // operations of the trimmed CIGAR (a .. b, or a .. the end)
  int32_t read_trim;   // read bases in front of the kept part
  int32_t new_len;     // read bases of the kept part
  int32_t len_first;   // the cut length of operation a, or -1: whole
  int32_t len_last;    // the length operation b is emitted with (may be 0), or -1: there is no b
  int32_t span;        // reference bases of the trimmed CIGAR
};

// TrimCigar operation by operation, as alt_aligned_pileup_lib.trim_cigar walks it: the host entry point's code and
// the check of the kernels' closed form.  -> 0, or kErrLength.
inline int trim_serial(const uint32_t* w, uint32_t n, int64_t T, int64_t C, int64_t seq_len, int32_t min_overlap,
                       PairResult* out) {
  int64_t trim_remaining = T, cover_remaining = C, read_start = 0, new_len = 0, span = 0;
  PairResult r{0, -1, 0, 0, 0, -1, -1, 0};
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t op = w[k] & 15u;
    int64_t length = w[k] >> 4;
    const bool on_ref = (kRefAdvancing >> op) & 1u, on_read = (kReadAdvancing >> op) & 1u;
    int64_t ref_step = on_ref ? length : 0;
    bool cut = false;
    if (trim_remaining > 0) {
      if (ref_step <= trim_remaining) {
        trim_remaining -= ref_step;
        read_start += on_read ? length : 0;
        continue;
      }
      ref_step -= trim_remaining;
      read_start += on_read ? trim_remaining : 0;
      length = ref_step;
      trim_remaining = 0;
      cut = true;
    }
    if (r.first < 0) {
      r.first = static_cast<int32_t>(k);
      if (cut) r.len_first = static_cast<int32_t>(length);
    }
    ++r.n_words;
    if (ref_step <= cover_remaining) {
      cover_remaining -= ref_step;
      new_len += on_read ? length : 0;
      span += on_ref ? length : 0;
    } else {
      length = cover_remaining;
      r.len_last = static_cast<int32_t>(length);
      new_len += on_read ? length : 0;
      span += length;
      break;
    }
  }
  *out = r;
  if (read_start + new_len > seq_len) return kErrLength;
  out->read_trim = static_cast<int32_t>(read_start);
  out->new_len = static_cast<int32_t>(new_len);
  out->span = static_cast<int32_t>(span);
  out->kept = span >= min_overlap && new_len > 0;
  return 0;
}

}  // namespace trim
}  // namespace dv

#endif  // DV_TRIM_READS_H_
