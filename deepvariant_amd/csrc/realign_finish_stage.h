// Host side of realign_finish.h: what one window adds to a batch's staged tables, from the aligner as
// collect_alignments leaves it.  Shared by realign_finish.hip and tools/realign_finish_check.cpp.
#ifndef DV_REALIGN_FINISH_STAGE_H_
#define DV_REALIGN_FINISH_STAGE_H_

#include <cstdint>
#include <string>
#include <vector>

#include "fast_pass_aligner.h"
#include "realign_finish.h"

namespace dv {
namespace fin {

struct Staged {            // the tables of a batch, in the order realign_finish.h reads them
  std::vector<Window> windows;
  std::vector<Hap> haps;
  std::vector<int32_t> perm;
  std::vector<Read> reads;
  std::vector<int32_t> read_item, row_position, row_score;
  std::string bytes;

  void clear() { *this = Staged(); }
  bool fits() const {      // offsets are int32_t
    const size_t limit = size_t{1} << 30;
    return bytes.size() < limit && row_position.size() < limit && read_item.size() < limit && reads.size() < limit;
  }
  Batch view(const Sweep& sweep, bool force_alignment, bool normalize_reads) const {
    Batch b;
    b.windows = windows.data();
    b.haps = haps.data();
    b.perm = perm.data();
    b.reads = reads.data();
    b.read_item = read_item.data();
    b.row_position = row_position.data();
    b.row_score = row_score.data();
    b.bytes = reinterpret_cast<const uint8_t*>(bytes.data());
    b.sweep = sweep;
    b.n_windows = static_cast<int32_t>(windows.size());
    b.n_haps = static_cast<int32_t>(haps.size());
    b.n_reads = static_cast<int32_t>(reads.size());
    b.force_alignment = force_alignment ? 1 : 0;
    b.normalize_reads = normalize_reads ? 1 : 0;
    return b;
  }
};

// Appends the window of `aligner` (after collect_alignments; alignments_ still in haplotype order) with its `pairs`.
// item_of_pair[k]: the sweep item of the window's pair k, -1: none.
inline void stage_window(const FastPassAligner& aligner, const AlignmentPairs& pairs, const int32_t* item_of_pair,
                         int64_t ref_start, Staged* s) {
  const std::vector<HaplotypeAlignment>& has = aligner.haplotype_alignments();
  const std::vector<std::string>& reads = aligner.reads();
  const size_t n_reads = pairs.n_input_reads, n_haps = has.size();
  Window w;
  w.ref_start = ref_start;
  w.ref_off = static_cast<int32_t>(s->bytes.size());
  w.ref_len = static_cast<int32_t>(aligner.reference().size());
  s->bytes += aligner.reference();
  w.first_hap = static_cast<int32_t>(s->haps.size());
  w.n_haps = static_cast<int32_t>(n_haps);
  w.first_read = static_cast<int32_t>(s->reads.size());
  w.n_reads = static_cast<int32_t>(n_reads);
  w.first_row = static_cast<int32_t>(s->row_position.size());
  w.first_read_item = static_cast<int32_t>(s->read_item.size());
  w.n_targets = static_cast<int32_t>(pairs.read_targets.size());
  w.threshold = static_cast<int32_t>(static_cast<uint16_t>(aligner.score_threshold()));
  const int32_t window = static_cast<int32_t>(s->windows.size());
  s->windows.push_back(w);

  std::vector<int32_t> scores(n_haps);
  for (size_t a = 0; a < n_haps; ++a) {
    const HaplotypeAlignment& ha = has[a];
    Hap h;
    h.window = window;
    h.len = static_cast<int32_t>(aligner.haplotypes()[ha.haplotype_index].size());
    h.score = ha.haplotype_score;
    h.item = -1;
    h.same_as_ref = ha.is_reference ? 1 : 0;     // so far set by collect_haplotype_pairs alone: byte-equal
    h.target = -1;
    s->haps.push_back(h);
    scores[a] = ha.haplotype_score;
    for (size_t r = 0; r < n_reads; ++r) {
      const ReadAlignment& ra = ha.reads[r];
      s->row_position.push_back(ra.position == ReadAlignment::kNotAligned ? -1 : static_cast<int32_t>(ra.position));
      s->row_score.push_back(ra.score);
    }
  }
  for (size_t k = 0; k < pairs.haplotype_todo.size(); ++k) {
    s->haps[static_cast<size_t>(w.first_hap) + pairs.haplotype_todo[k]].item = item_of_pair[k];
  }
  for (size_t t = 0; t < pairs.read_targets.size(); ++t) {
    s->haps[static_cast<size_t>(w.first_hap) + pairs.read_targets[t]].target = static_cast<int32_t>(t);
  }
  s->perm.resize(s->perm.size() + n_haps);
  sorted_order(scores.data(), static_cast<int>(n_haps), s->perm.data() + w.first_hap);
  for (size_t r = 0; r < n_reads; ++r) {
    Read rd;
    rd.window = window;
    rd.off = static_cast<int32_t>(s->bytes.size());
    rd.len = static_cast<int32_t>(reads[r].size());
    rd.unplaced = -1;
    s->bytes += reads[r];
    s->reads.push_back(rd);
  }
  for (size_t u = 0; u < pairs.unplaced_reads.size(); ++u) {
    s->reads[static_cast<size_t>(w.first_read) + pairs.unplaced_reads[u]].unplaced = static_cast<int32_t>(u);
  }
  const size_t n_read_pairs = pairs.unplaced_reads.size() * pairs.read_targets.size();
  for (size_t k = 0; k < n_read_pairs; ++k) s->read_item.push_back(item_of_pair[pairs.n_haplotype_pairs + k]);
}

}  // namespace fin
}  // namespace dv

#endif  // DV_REALIGN_FINISH_STAGE_H_
