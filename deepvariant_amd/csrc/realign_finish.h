// The last step of FastPassAligner::align_reads -- finish_alignments: apply_haplotype_alignments, positions_map,
// apply_read_alignments, realign_reads_to_reference -- for the general case (several haplotypes, a haplotype ->
// reference CIGAR with indels and soft clips, the best haplotype per read), written once for the host and the device.
// alt_align.h holds the special case (one haplotype that is the reference); its Merger is the output side here too.
// The rule works on what the device route holds before any text exists: the sweep kernel's words per pair (corners,
// traced flag, M/I/D runs, last run first), raw bytes (the reference as handed over, the reads upper-cased), the coded
// sequences, the fast pass' rows and the order std::sort gave the haplotypes.  No strings, no allocation; every loop
// is bounded by the read length plus the run counts.  The contract is written out at the top of realign_finish.hip.
#ifndef DV_REALIGN_FINISH_H_
#define DV_REALIGN_FINISH_H_

#include <cstdint>

#include <algorithm>
#include <vector>

#include "alt_align.h"

namespace dv {
namespace fin {

using alt::kD;
using alt::kI;
using alt::kM;
using alt::kS;

constexpr int kPairCornerWords = 6;      // score, ref_end, q_end, reverse score, ref_begin, q_begin
constexpr int kPairHeaderWords = 8;      // + [6] traced, [7] runs | band << 16; the runs follow
constexpr int kPairMaxRuns = 64;         // DV_LOCAL_ALIGN_DEVICE_MAX_RUNS

struct SweepItemView {     // local_align.hip's SweepItem
  int32_t ref, query;      // slots of the sweep's sequence table
  int32_t rows, pair, area;
};

struct Sweep {             // the sweep call's buffers, where it left them
  const int32_t* out = nullptr;          // out_words per item
  int32_t out_words = 0;
  int32_t n_items = 0;
  const SweepItemView* items = nullptr;
  const int32_t* seq_off = nullptr;      // [slots + 1] into codes
  const uint8_t* codes = nullptr;        // the aligner's 0..4 codes
};

struct Window {
  int64_t ref_start;                // FastPassAligner::set_ref_start
  int32_t ref_off, ref_len;         // the reference as handed over, in `bytes`
  int32_t first_hap, n_haps;        // its haplotypes: Hap / HapState / perm [first_hap, first_hap + n_haps)
  int32_t first_read, n_reads;      // its reads: Read and the outputs [first_read, first_read + n_reads)
  int32_t first_row;                // fast pass row of (haplotype h, read r): first_row + h * n_reads + r
  int32_t first_read_item;          // read_item[first_read_item + u * n_targets + t]: sweep item of (unplaced u, target t)
  int32_t n_targets;
  int32_t threshold;                // uint16_t(score_threshold)
};

struct Hap {               // in haplotype order (the order of alignments_ before the sort)
  int32_t window;
  int32_t len;
  int32_t score;           // haplotype_score as install_fast_pass leaves it
  int32_t item;            // sweep item of its haplotype -> reference pair; -1: none
  int32_t same_as_ref;     // byte-equal to the window's reference: no Smith-Waterman, "<len>=" at 0
  int32_t target;          // its index among the window's read targets; -1: not one
};

struct Read {
  int32_t window;
  int32_t off, len;        // upper-cased, in `bytes`
  int32_t unplaced;        // its index among the window's unplaced reads; -1: the fast pass placed it (or no targets)
};

struct HapState {          // what apply_haplotype_alignments leaves, minus the text
  int32_t valid;           // holds a CIGAR
  int32_t is_reference;
  int32_t ref_pos;
  int32_t reserved;
};

struct Batch {
  const Window* windows = nullptr;
  const Hap* haps = nullptr;
  const int32_t* perm = nullptr;          // per window: sorted place -> haplotype (local index)
  const Read* reads = nullptr;
  const int32_t* read_item = nullptr;
  const int32_t* row_position = nullptr;  // the fast pass' rows; -1: not aligned
  const int32_t* row_score = nullptr;
  const uint8_t* bytes = nullptr;
  Sweep sweep;
  int32_t n_windows = 0, n_haps = 0, n_reads = 0;
  int32_t force_alignment = 0, normalize_reads = 0;
};

struct ReadOut {           // per read, between the passes
  int32_t status, n_words;
  int64_t position;
};

// An alignment's operations: the soft clip in front, the M/I/D runs, the soft clip behind.  The text form splits an
// M run into '=' and 'X' tokens, and the merge can tell: where the haplotype ends exactly between two tokens of the
// read, the rest of the read is merged as whole operations; inside a token it clears the CIGAR.  So a Queue (below)
// walks an M run in the pieces the coded sequences give it; the map and the run counts need the runs alone.
// `whole` > 0: one token "<n>=".
struct Ops {
  int lead = 0, tail = 0, n_runs = 0, whole = 0;
  const uint32_t* runs = nullptr;   // (length << 2) | 0 M / 1 I / 2 D, the LAST run first
  const uint8_t* rc = nullptr;      // the codes of the pair's reference from ref_begin on, of its query from q_begin on:
  const uint8_t* qc = nullptr;      // equal codes are '=', others 'X' (describe_runs)

  DV_ALT_HD int size() const { return whole > 0 ? 1 : (lead > 0) + n_runs + (tail > 0); }
  DV_ALT_HD void get(int i, int* op, int* len) const {
    if (whole > 0) {
      *op = kM;
      *len = whole;
      return;
    }
    if (lead > 0) {
      if (i == 0) {
        *op = kS;
        *len = lead;
        return;
      }
      --i;
    }
    if (i < n_runs) {
      const uint32_t w = runs[n_runs - 1 - i];
      const int k = static_cast<int>(w & 3u);
      *op = k == 0 ? kM : k == 1 ? kI : kD;
      *len = static_cast<int>(w >> 2);
      return;
    }
    *op = kS;
    *len = tail;
  }
};

// The words of a sweep item, or null.
DV_ALT_HD const int32_t* pair_words(const Sweep& s, int item) {
  if (item < 0 || item >= s.n_items) return nullptr;
  return s.out + static_cast<int64_t>(item) * s.out_words;
}

// ok && score > 0 with the runs at hand.  Nothing the words say is trusted past this test: the run count lies inside
// the kernel's own bound, the corners inside the item's two sequences, and the runs cover exactly the span between the
// corners, so that walking them indexes neither sequence out of bounds.
DV_ALT_HD bool pair_aligned(const Sweep& s, int item) {
  const int32_t* o = pair_words(s, item);
  if (!o || s.out_words < kPairHeaderWords + kPairMaxRuns) return false;
  const int n_runs = o[7] & 0xffff;
  if (!(o[0] > 0 && o[3] == o[0] && o[6] == 1 && n_runs >= 1 && n_runs <= kPairMaxRuns)) return false;
  const SweepItemView& it = s.items[item];
  const int ref_n = s.seq_off[it.ref + 1] - s.seq_off[it.ref], q_n = s.seq_off[it.query + 1] - s.seq_off[it.query];
  if (o[4] < 0 || o[4] > o[1] || o[1] >= ref_n || o[5] < 0 || o[5] > o[2] || o[2] >= q_n) return false;
  int on_ref = 0, on_query = 0;
  for (int i = 0; i < n_runs; ++i) {
    const uint32_t w = static_cast<uint32_t>(o[kPairHeaderWords + i]);
    const int k = static_cast<int>(w & 3u), len = static_cast<int>(w >> 2);
    if (k > 2 || len <= 0 || len > ref_n + q_n) return false;
    if (k != 1) on_ref += len;
    if (k != 2) on_query += len;
  }
  return on_ref == o[1] - o[4] + 1 && on_query == o[2] - o[5] + 1;
}

// The operations of an aligned pair (pair_aligned holds for it).
DV_ALT_HD Ops pair_ops(const Sweep& s, int item, int query_len) {
  const int32_t* o = pair_words(s, item);
  Ops ops;
  ops.lead = o[5];
  ops.tail = query_len - 1 - o[2];
  if (ops.tail < 0) ops.tail = 0;
  ops.n_runs = o[7] & 0xffff;
  ops.runs = reinterpret_cast<const uint32_t*>(o + kPairHeaderWords);
  ops.rc = s.codes + s.seq_off[s.items[item].ref] + o[4];
  ops.qc = s.codes + s.seq_off[s.items[item].query] + o[5];
  return ops;
}

// apply_haplotype_alignments for one haplotype.  is_reference: byte-equal to the reference, or an alignment that is
// one '=' run over the whole haplotype -- corners 0 .. n - 1, one M run of n, no differing code.
DV_ALT_HD HapState hap_state(const Batch& b, int g) {
  HapState st{0, 0, 0, 0};
  const Hap& h = b.haps[g];
  if (h.same_as_ref) {
    st.valid = 1;
    st.is_reference = 1;
    return st;
  }
  const int32_t* o = pair_words(b.sweep, h.item);
  if (!pair_aligned(b.sweep, h.item)) return st;        // empty CIGAR, all-zero map, ref_pos 0
  st.valid = 1;
  st.ref_pos = o[4];
  const int n = h.len;
  const int n_runs = o[7] & 0xffff;
  if (o[5] != 0 || o[2] != n - 1 || n_runs != 1) return st;
  const uint32_t w = static_cast<uint32_t>(o[kPairHeaderWords]);
  if ((w & 3u) != 0 || static_cast<int>(w >> 2) != n) return st;
  const SweepItemView& it = b.sweep.items[h.item];
  const int ref_at = b.sweep.seq_off[it.ref], ref_n = b.sweep.seq_off[it.ref + 1] - ref_at;
  const int hap_at = b.sweep.seq_off[it.query], hap_n = b.sweep.seq_off[it.query + 1] - hap_at;
  if (hap_n != n || o[4] + n > ref_n) return st;
  const uint8_t* rc = b.sweep.codes + ref_at + o[4];
  const uint8_t* hc = b.sweep.codes + hap_at;
  for (int i = 0; i < n; ++i) {
    if (rc[i] != hc[i]) return st;
  }
  st.is_reference = 1;
  return st;
}

DV_ALT_HD Ops hap_ops(const Batch& b, int g, const HapState& st) {
  Ops ops;
  const Hap& h = b.haps[g];
  if (h.same_as_ref) {
    ops.whole = h.len;
  } else if (st.valid) {
    ops = pair_ops(b.sweep, h.item, h.len);
  }
  return ops;
}

// positions_map(cigar, size)[p]: S lowers the shift and then fills, D raises it, I fills and lowers it per base;
// a position the CIGAR does not reach keeps 0.
DV_ALT_HD int map_value(const Ops& ops, int p) {
  int shift = 0, pos = 0;
  const int n = ops.size();
  for (int i = 0; i < n; ++i) {
    int op, len;
    ops.get(i, &op, &len);
    if (op == kD) {
      shift += len;
      continue;
    }
    if (op == kS) shift -= len;
    if (p < pos + len) return op == kI ? shift - (p - pos) : shift;
    pos += len;
    if (op == kI) shift -= len;
  }
  return 0;
}

// A queue of tokens as calculate_read_to_ref_alignment's deques: the tokens from run `next` on -- an M run in its
// '=' / 'X' pieces --, the first one at `first_len` when the left trim cut it, and in front of them `pushed` one-base
// matches.
struct Queue {
  const Ops* ops = nullptr;
  int next = 0, n = 0, first_len = -1, pushed = 0;
  int ri = 0, qi = 0;        // code positions of the run `next`
  int within = 0;            // bases of it that earlier pieces took
  int piece = 0;             // the token front() found

  DV_ALT_HD bool empty() const { return pushed == 0 && next >= n; }
  DV_ALT_HD void front(int* op, int* len) {
    if (pushed > 0) {
      *op = kM;
      *len = 1;
      return;
    }
    ops->get(next, op, len);
    piece = *len;
    if (*op == kM && ops->whole == 0 && ops->rc) {
      const uint8_t* rc = ops->rc + ri + within;
      const uint8_t* qc = ops->qc + qi + within;
      const int left = *len - within;
      const bool eq = rc[0] == qc[0];
      int k = 1;
      while (k < left && (rc[k] == qc[k]) == eq) ++k;
      piece = k;
      *len = k;
    }
    if (first_len >= 0) *len = first_len;
  }
  // behind front()
  DV_ALT_HD void pop() {
    if (pushed > 0) {
      --pushed;
      return;
    }
    first_len = -1;
    int op, len;
    ops->get(next, &op, &len);
    if (op == kM) {
      within += piece;
      if (within < len) return;
    }
    if (op == kM || op == kD) ri += len;
    if (op == kM || op == kI) qi += len;
    within = 0;
    ++next;
  }
};

// LeftTrimHaplotypeToRefAlignment up to the read's position: M, S and I consume haplotype bases, D does not; a D
// left at the front is dropped; nothing left is a failure.
DV_ALT_HD bool left_trim(Queue* h2r, int hap_pos) {
  int cur = 0;
  while (cur != hap_pos) {
    if (h2r->empty()) return false;
    int op, len;
    h2r->front(&op, &len);
    if (op == kM || op == kS || op == kI) {
      if (len + cur > hap_pos) {
        h2r->first_len = len - (hap_pos - cur);     // pushed back at what is left of it
        cur = hap_pos;
        continue;
      }
      cur += len;
    }
    h2r->pop();
  }
  if (!h2r->empty()) {
    int op, len;
    h2r->front(&op, &len);
    if (op == kD) h2r->pop();
  }
  return !h2r->empty();
}

// merge_one: the operation of the pair with the highest priority, S, D, I, M, as one base.
DV_ALT_HD int merged_kind(int a, int b) {
  if (a == kS || b == kS) return kS;
  if (a == kD || b == kD) return kD;
  if (a == kI || b == kI) return kI;
  if (a == kM || b == kM) return kM;
  return 0;
}

// calculate_read_to_ref_alignment behind the left trim.  -> cleared (the read runs past the haplotype).
// *cancelled counts the I/D bases that cancelled.
DV_ALT_HD bool merge_walk(Queue r2h, Queue h2r, alt::Merger* m, int* cancelled) {
  const int L = m->read_len;
  int op, len;
  if (!r2h.empty()) {
    r2h.front(&op, &len);
    if (op == kS) {
      m->merge(kS, len, true);
      r2h.pop();
    }
  }
  int cr_op = 0, cr_len = 0, ch_op = 0, ch_len = 0;
  while ((!r2h.empty() || !h2r.empty()) && m->aligned < L) {
    if (!r2h.empty() && h2r.empty() && ch_len == 0) {      // past the haplotype: the read's operations as they are
      r2h.front(&op, &len);
      m->merge(op, len, true);
      r2h.pop();
      continue;
    }
    if (r2h.empty() && cr_len == 0 && !h2r.empty()) break;   // the read is used up
    if (cr_len == 0) {
      r2h.front(&cr_op, &cr_len);
      r2h.pop();
    }
    if (ch_len == 0) {
      if (h2r.empty()) break;
      h2r.front(&ch_op, &ch_len);
      h2r.pop();
    }
    while (cr_len > 0 && ch_len > 0) {
      if ((cr_op == kD && ch_op == kI) || (cr_op == kI && ch_op == kD)) {
        --ch_len;
        --cr_len;
        ++*cancelled;
        if (ch_op == kD) {          // a read insertion filling a haplotype deletion is a match, taken up once the
          ++h2r.pushed;             // current operations have run out
          ++r2h.pushed;
        }
        continue;
      }
      const int k = merged_kind(cr_op, ch_op);
      if (k) m->merge(k, 1);
      if (cr_op == kI) {
        --cr_len;
      } else if (ch_op == kD) {
        --ch_len;
      } else {
        --ch_len;
        --cr_len;
      }
    }
  }
  if (cr_len > 0 && cr_op == kS) {
    for (; cr_len > 0; --cr_len) m->merge(kS, 1);
  }
  return !r2h.empty() || cr_len > 0;
}

// The score read r (local) holds on haplotype g after apply_read_alignments; *item: the sweep item behind it, or -1
// for the fast pass' "<L>=", *position its place on the haplotype.
DV_ALT_HD int read_score_on(const Batch& b, const HapState* states, const Window& w, int g, int r, int* item,
                            int* position) {
  const Hap& h = b.haps[g];
  const Read& rd = b.reads[w.first_read + r];
  *item = -1;
  *position = -1;
  if (rd.unplaced >= 0) {
    if (h.target < 0) return 0;
    const bool forced = b.force_alignment && states[g].is_reference;
    if (h.score == 0 && !forced) return 0;
    const int it = b.read_item[w.first_read_item + rd.unplaced * w.n_targets + h.target];
    const int32_t* o = pair_words(b.sweep, it);
    if (!pair_aligned(b.sweep, it)) return 0;
    if (o[0] < w.threshold && !forced) return 0;
    *item = it;
    *position = static_cast<int>(static_cast<uint16_t>(o[4]));
    return o[0];
  }
  if (h.score == 0) return 0;
  const int row = w.first_row + (g - w.first_hap) * w.n_reads + r;
  if (b.row_position[row] < 0) return 0;
  *position = static_cast<int>(static_cast<uint16_t>(b.row_position[row]));
  return b.row_score[row];
}

// realign_reads_to_reference for read d of the batch: best_read_alignment over the sorted haplotypes (among equal
// scores the first, unless a later one is not the reference), the map's shift, the left trim, the merge, the
// normalization at ref_pos + position + shift.  The words go to `out` when it is set.
DV_ALT_HD ReadOut finish_read(const Batch& b, const HapState* states, int d, uint32_t* out, int* cancelled) {
  ReadOut res{0, 0, 0};
  const Read& rd = b.reads[d];
  const Window& w = b.windows[rd.window];
  const int r = d - w.first_read;
  int best = 0, best_g = -1, best_item = -1, best_pos = -1;
  for (int x = 0; x < w.n_haps; ++x) {
    const int g = w.first_hap + b.perm[w.first_hap + x];
    int item, pos;
    const int s = read_score_on(b, states, w, g, r, &item, &pos);
    if (s > best || (best > 0 && s == best && !states[g].is_reference)) {
      best = s;
      best_g = g;
      best_item = item;
      best_pos = pos;
    }
  }
  if (best_g < 0) {
    res.status = b.force_alignment ? 2 : 0;
    return res;
  }
  const Hap& h = b.haps[best_g];
  const HapState& st = states[best_g];
  const int p = best_pos;
  if (p >= h.len) return res;                      // outside the map
  const Ops h_ops = hap_ops(b, best_g, st);
  Ops r_ops;
  if (best_item < 0) {
    r_ops.whole = rd.len;
  } else {
    r_ops = pair_ops(b.sweep, best_item, rd.len);
  }
  const int shift = map_value(h_ops, p);
  const int64_t offset = static_cast<int64_t>(st.ref_pos) + p + shift;
  Queue h2r, r2h;
  h2r.ops = &h_ops;
  h2r.n = h_ops.size();
  r2h.ops = &r_ops;
  r2h.n = r_ops.size();
  if (!left_trim(&h2r, p)) return res;
  alt::Merger m;
  m.read_len = rd.len;
  m.out = out;
  m.read = b.bytes + rd.off;
  const int at = static_cast<int>(offset);
  if (at >= 0) {                                   // a negative offset counts as normalized: nothing is looked at
    m.target = b.bytes + w.ref_off;
    m.target_len = w.ref_len;
    m.ref_i = at;
  }
  const bool cleared = merge_walk(r2h, h2r, &m, cancelled);
  m.flush();
  if (cleared || m.n_out == 0) return res;
  if (!b.normalize_reads && at >= 0 && !m.normalized) return res;
  res.status = 1;
  res.n_words = m.n_out;
  res.position = w.ref_start + offset;
  return res;
}

// Host only.  The order realign_reads_to_reference's std::sort gives n haplotype alignments: the same call and comparator over
// (score, index) records.  libstdc++'s moves depend on the comparison results alone, so the permutation is the same.
inline void sorted_order(const int32_t* scores, int n, int32_t* perm) {
  struct Rec {
    int32_t score, index;
  };
  std::vector<Rec> v(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) v[static_cast<size_t>(i)] = Rec{scores[i], i};
  std::sort(v.begin(), v.end(), [](const Rec& a, const Rec& b) { return a.score < b.score; });
  for (int i = 0; i < n; ++i) perm[i] = v[static_cast<size_t>(i)].index;
}

}  // namespace fin
}  // namespace dv

#endif  // DV_REALIGN_FINISH_H_
