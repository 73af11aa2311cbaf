// A stand-alone run of the gVCF merge's host code (csrc/gvcf_merge.h through dv_gvcf_merge) for AddressSanitizer and
// UBSan, on the CPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Ideepvariant_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/gvcf_merge_check.cpp deepvariant_amd/csrc/gvcf_merge.hip deepvariant_amd/csrc/common.hip -o gvcf_merge_check
//   ./gvcf_merge_check
//
// Seeded layouts of one to four groups (gaps between blocks, nested and identical variants, variants in gaps and past
// both ends, empty groups), each compared with a plain sequential loop written here -- two streams and `lessthan`, as
// DESIGN.md section 22 states the rule -- and the inputs the entry point refuses.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "dvhip.h"

namespace {

uint64_t state = 0x9e3779b97f4a7c15ull;
uint64_t next() {        // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
int64_t below(int64_t n) { return static_cast<int64_t>(next() % static_cast<uint64_t>(n)); }

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "gvcf_merge_check: line %d: %s (%s)\n", __LINE__, #cond, dv_last_error()); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

using Span = std::pair<int64_t, int64_t>;

struct Call {
  std::vector<int64_t> block_off{0}, var_off{0}, block_start, block_end, var_start, var_end;

  void add_group(int64_t n_blocks, int64_t n_variants, int64_t max_len) {
    int64_t at = below(20);
    for (int64_t b = 0; b < n_blocks; ++b) {
      if (below(3) == 0) at += 1 + below(15);      // a gap
      const int64_t len = 1 + below(max_len);
      block_start.push_back(at);
      block_end.push_back(at + len);
      at += len;
    }
    std::vector<Span> v;
    for (int64_t j = 0; j < n_variants; ++j) {
      if (!v.empty() && below(8) == 0) {
        v.push_back(v[static_cast<size_t>(below(static_cast<int64_t>(v.size())))]);       // identical
        continue;
      }
      const int64_t s = below(at + 30);
      v.emplace_back(s, s + 1 + (below(4) == 0 ? below(4 * max_len) : below(3)));
    }
    std::sort(v.begin(), v.end());
    for (const Span& x : v) {
      var_start.push_back(x.first);
      var_end.push_back(x.second);
    }
    block_off.push_back(static_cast<int64_t>(block_start.size()));
    var_off.push_back(static_cast<int64_t>(var_start.size()));
  }
  int32_t groups() const { return static_cast<int32_t>(block_off.size()) - 1; }
  int run(dv_gvcf_merged** out) const {
    return dv_gvcf_merge(groups(), block_off.data(), var_off.data(), block_start.data(), block_end.data(),
                         var_start.data(), var_end.data(), out);
  }
};

struct Expected {
  std::vector<int64_t> piece_start, piece_end, piece_slot, var_slot;
  std::vector<int32_t> piece_block;
};

// merge_variants_and_nonvariants, group by group: two streams and lessthan.
Expected sequential(const Call& c) {
  Expected e;
  e.var_slot.assign(c.var_start.size(), -1);
  int64_t slot = 0;
  for (int32_t g = 0; g < c.groups(); ++g) {
    int64_t bi = c.block_off[g], vi = c.var_off[g];
    const int64_t b1 = c.block_off[g + 1], v1 = c.var_off[g + 1];
    bool have_block = bi < b1;
    Span block = have_block ? Span(c.block_start[bi], c.block_end[bi]) : Span(0, 0);
    auto next_block = [&]() {
      ++bi;
      have_block = bi < b1;
      if (have_block) block = Span(c.block_start[bi], c.block_end[bi]);
    };
    auto piece = [&](int64_t s, int64_t end) {
      e.piece_start.push_back(s);
      e.piece_end.push_back(end);
      e.piece_block.push_back(static_cast<int32_t>(bi));
      e.piece_slot.push_back(slot++);
    };
    while (have_block || vi < v1) {
      const bool have_variant = vi < v1;
      const Span variant = have_variant ? Span(c.var_start[vi], c.var_end[vi]) : Span(0, 0);
      if (have_variant && (!have_block || variant.second <= block.first)) {
        e.var_slot[static_cast<size_t>(vi++)] = slot++;
      } else if (have_block && (!have_variant || block.second <= variant.first)) {
        piece(block.first, block.second);
        next_block();
      } else {
        if (block.first < variant.first) piece(block.first, variant.first);
        if (block.second > variant.second) {
          block.first = variant.second;
        } else {
          next_block();
        }
      }
    }
  }
  return e;
}

void compare(const Call& c) {
  dv_gvcf_merged* m = nullptr;
  CHECK(c.run(&m) == DV_OK && m != nullptr);
  dv_gvcf_merged_view v;
  CHECK(dv_gvcf_merged_arrays(m, &v) == DV_OK);
  const Expected e = sequential(c);
  CHECK(v.n_pieces == static_cast<int64_t>(e.piece_start.size()) && v.n_variants == static_cast<int64_t>(e.var_slot.size()));
  CHECK(v.n_pieces <= static_cast<int64_t>(c.block_start.size() + c.var_start.size()));
  for (int64_t k = 0; k < v.n_pieces; ++k) {
    const size_t i = static_cast<size_t>(k);
    CHECK(v.piece_start[k] == e.piece_start[i] && v.piece_end[k] == e.piece_end[i] && v.piece_block[k] == e.piece_block[i] &&
          v.piece_slot[k] == e.piece_slot[i]);
  }
  for (int64_t j = 0; j < v.n_variants; ++j) CHECK(v.var_slot[j] == e.var_slot[static_cast<size_t>(j)]);
  dv_gvcf_merged_free(m);
}

void refused(const std::vector<int64_t>& block_off, const std::vector<int64_t>& var_off, const std::vector<int64_t>& bs,
             const std::vector<int64_t>& be, const std::vector<int64_t>& vs, const std::vector<int64_t>& ve) {
  dv_gvcf_merged* m = reinterpret_cast<dv_gvcf_merged*>(1);
  CHECK(dv_gvcf_merge(static_cast<int32_t>(block_off.size()) - 1, block_off.data(), var_off.data(), bs.data(), be.data(),
                      vs.data(), ve.data(), &m) == DV_ERR_BAD_INPUT);
  CHECK(m == nullptr);
}

}  // namespace

int main() {
  int64_t layouts = 0;
  for (int round = 0; round < 40000; ++round) {
    Call c;
    const int groups = 1 + static_cast<int>(below(4));
    for (int g = 0; g < groups; ++g) {
      const bool empty = below(6) == 0;
      c.add_group(empty ? 0 : below(7), empty || below(6) == 0 ? 0 : below(7), 1 + below(12));
    }
    compare(c);
    ++layouts;
  }
  for (int round = 0; round < 20; ++round) {        // long groups: the bisections past a handful of records
    Call c;
    c.add_group(2000 + below(3000), below(1500), 40);
    c.add_group(0, 0, 1);
    c.add_group(below(3000), 500 + below(1500), 25);
    compare(c);
    ++layouts;
  }
  {
    Call none;                                        // one group without records, and no group at all
    none.add_group(0, 0, 1);
    compare(none);
    const int64_t zero[1] = {0};
    dv_gvcf_merged* m = nullptr;
    CHECK(dv_gvcf_merge(0, zero, zero, nullptr, nullptr, nullptr, nullptr, &m) == DV_OK && m != nullptr);
    dv_gvcf_merged_view v;
    CHECK(dv_gvcf_merged_arrays(m, &v) == DV_OK && v.n_pieces == 0 && v.n_variants == 0);
    dv_gvcf_merged_free(m);
    dv_gvcf_merged_free(nullptr);
  }
  // what the entry point refuses
  refused({0, 2}, {0, 0}, {10, 0}, {20, 5}, {}, {});            // blocks unsorted
  refused({0, 2}, {0, 0}, {0, 9}, {10, 20}, {}, {});            // blocks overlap
  refused({0, 0}, {0, 2}, {}, {}, {5, 4}, {6, 9});              // variant starts descend
  refused({0, 0}, {0, 2}, {}, {}, {5, 5}, {9, 6});              // the same start, ends descend
  refused({0, 1}, {0, 0}, {5}, {5}, {}, {});                    // an empty block
  refused({0, 0}, {0, 1}, {}, {}, {7}, {6});                    // an empty variant
  refused({0, 2, 1, 2}, {0, 0, 0, 0}, {0, 10}, {5, 20}, {}, {});     // offsets descend
  refused({1, 2}, {0, 0}, {0, 10}, {5, 20}, {}, {});            // offsets do not start at 0
  {
    const int64_t off[2] = {0, 1}, zero[2] = {0, 0}, s[1] = {0}, e[1] = {5};
    dv_gvcf_merged* m = nullptr;
    CHECK(dv_gvcf_merge(1, off, zero, nullptr, e, nullptr, nullptr, &m) == DV_ERR_INVALID_ARGUMENT && m == nullptr);
    CHECK(dv_gvcf_merge(-1, off, zero, s, e, nullptr, nullptr, &m) == DV_ERR_INVALID_ARGUMENT && m == nullptr);
    CHECK(dv_gvcf_merge(1, off, zero, s, e, nullptr, nullptr, nullptr) == DV_ERR_INVALID_ARGUMENT);
    dv_gvcf_merge_stats stats;
    CHECK(dv_gvcf_merge_last_stats(&stats) == DV_OK && dv_gvcf_merge_scan_chunk() > 0);
  }
  std::printf("gvcf_merge_check ok: %lld layouts\n", static_cast<long long>(layouts));
  return 0;
}
