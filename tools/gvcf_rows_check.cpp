// A stand-alone run of the gVCF rows' host code (csrc/gvcf_rows.h through dv_gvcf_rows) for AddressSanitizer and UBSan,
// on the CPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Ideepvariant_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/gvcf_rows_check.cpp deepvariant_amd/csrc/gvcf_rows.hip deepvariant_amd/csrc/common.hip -o gvcf_rows_check
//   ./gvcf_rows_check
//
// Seeded layouts of one to four groups (gaps between blocks, nested and identical variants, empty groups), each compared
// byte for byte with a loop written here: the sequential merge of DESIGN.md section 22, two streams and `lessthan`,
// printing every row with snprintf.  Then the number edges, calls without records and the inputs the entry point refuses.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
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
      std::fprintf(stderr, "gvcf_rows_check: line %d: %s (%s)\n", __LINE__, #cond, dv_last_error()); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

using Span = std::pair<int64_t, int64_t>;

char base_at(int64_t position) { return "ACGT"[static_cast<uint64_t>(position) % 4]; }

struct Call {
  std::vector<int64_t> block_off{0}, var_off{0}, var_start, var_end, var_text_off{0}, name_off{0};
  std::vector<dv_gvcf_block> blocks;
  std::vector<uint8_t> var_end_base;
  std::string var_text, names;
  int32_t med_dp = -1;

  void add_block(int64_t start, int64_t end) {
    dv_gvcf_block b;
    std::memset(&b, 0, sizeof b);
    b.start = start;
    b.end = end;
    for (double& gl : b.likelihoods) gl = -static_cast<double>(below(4000)) / 80.0;     // many exact halves of -10 GL
    b.gq = static_cast<int32_t>(below(120)) - 5;
    b.min_dp = static_cast<int32_t>(below(3) == 0 ? below(2000000000) : below(300));
    b.med_dp = below(3) == 0 ? -1 : static_cast<int32_t>(below(500));
    b.ref_base = 'N';
    b.has_valid_gl = static_cast<uint8_t>(below(2));
    blocks.push_back(b);
  }
  void add_variant(int64_t start, int64_t end) {
    var_start.push_back(start);
    var_end.push_back(end);
    var_end_base.push_back(static_cast<uint8_t>(base_at(end)));
    var_text += "v" + std::to_string(var_start.size()) + std::string(static_cast<size_t>(below(below(40) == 0 ? 6000 : 60)), 'x') + "\n";
    var_text_off.push_back(static_cast<int64_t>(var_text.size()));
  }
  void end_group() {
    names += std::string(static_cast<size_t>(1 + below(12)), static_cast<char>('a' + below(26)));
    name_off.push_back(static_cast<int64_t>(names.size()));
    block_off.push_back(static_cast<int64_t>(blocks.size()));
    var_off.push_back(static_cast<int64_t>(var_start.size()));
  }
  void add_group(int64_t n_blocks, int64_t n_variants, int64_t max_len, int64_t origin) {
    int64_t at = origin + below(20);
    for (int64_t b = 0; b < n_blocks; ++b) {
      if (below(3) == 0) at += 1 + below(15);      // a gap
      const int64_t len = 1 + below(max_len);
      add_block(at, at + len);
      at += len;
    }
    std::vector<Span> v;
    for (int64_t j = 0; j < n_variants; ++j) {
      if (!v.empty() && below(8) == 0) {
        v.push_back(v[static_cast<size_t>(below(static_cast<int64_t>(v.size())))]);       // identical
        continue;
      }
      const int64_t s = origin + below(at - origin + 30);
      v.emplace_back(s, s + 1 + (below(4) == 0 ? below(4 * max_len) : below(3)));
    }
    std::sort(v.begin(), v.end());
    for (const Span& x : v) add_variant(x.first, x.second);
    end_group();
  }
  dv_gvcf_rows_input input(int32_t want_row_off) const {
    dv_gvcf_rows_input in;
    std::memset(&in, 0, sizeof in);
    in.n_groups = static_cast<int32_t>(block_off.size()) - 1;
    in.med_dp = med_dp;
    in.want_row_off = want_row_off;
    in.block_off = block_off.data();
    in.var_off = var_off.data();
    in.blocks = blocks.data();
    in.var_start = var_start.data();
    in.var_end = var_end.data();
    in.var_end_base = var_end_base.data();
    in.var_text_off = var_text_off.data();
    in.var_text = var_text.data();
    in.name_off = name_off.data();
    in.names = names.data();
    return in;
  }
};

// One block row as the Python formatter prints it.
std::string row(const std::string& name, int64_t start, int64_t end, char base, const dv_gvcf_block& b, bool med_dp) {
  long long pl[3];
  for (int k = 0; k < 3; ++k) pl[k] = static_cast<long long>(std::nearbyint(-10.0 * b.likelihoods[k]));
  const long long low = std::min(pl[0], std::min(pl[1], pl[2]));
  char med[16] = ".";
  if (b.med_dp >= 0) std::snprintf(med, sizeof med, "%d", b.med_dp);
  char text[512];
  if (med_dp) {
    std::snprintf(text, sizeof text, "\t%" PRId64 "\t.\t%c\t<*>\t0\t.\tEND=%" PRId64 "\tGT:GQ:MIN_DP:MED_DP:PL\t%s:%d:%d:%s:%lld,%lld,%lld\n",
                  start + 1, base, end, b.has_valid_gl ? "0/0" : "./.", b.gq, b.min_dp, med, pl[0] - low, pl[1] - low, pl[2] - low);
  } else {
    std::snprintf(text, sizeof text, "\t%" PRId64 "\t.\t%c\t<*>\t0\t.\tEND=%" PRId64 "\tGT:GQ:MIN_DP:PL\t%s:%d:%d:%lld,%lld,%lld\n",
                  start + 1, base, end, b.has_valid_gl ? "0/0" : "./.", b.gq, b.min_dp, pl[0] - low, pl[1] - low, pl[2] - low);
  }
  return name + text;
}

// merge_variants_and_nonvariants, group by group: two streams and lessthan, printing as it goes.
std::vector<std::string> sequential(const Call& c, bool med_dp, int64_t* n_pieces) {
  std::vector<std::string> rows;
  *n_pieces = 0;
  for (size_t g = 0; g + 1 < c.block_off.size(); ++g) {
    const std::string name = c.names.substr(static_cast<size_t>(c.name_off[g]), static_cast<size_t>(c.name_off[g + 1] - c.name_off[g]));
    int64_t bi = c.block_off[g], vi = c.var_off[g];
    const int64_t b1 = c.block_off[g + 1], v1 = c.var_off[g + 1];
    bool have_block = bi < b1, moved = false;
    Span block = have_block ? Span(c.blocks[bi].start, c.blocks[bi].end) : Span(0, 0);
    auto next_block = [&]() {
      ++bi;
      have_block = bi < b1;
      moved = false;
      if (have_block) block = Span(c.blocks[bi].start, c.blocks[bi].end);
    };
    auto piece = [&](int64_t s, int64_t end) {
      rows.push_back(row(name, s, end, moved ? base_at(s) : static_cast<char>(c.blocks[bi].ref_base), c.blocks[bi], med_dp));
      ++*n_pieces;
    };
    while (have_block || vi < v1) {
      const bool have_variant = vi < v1;
      const Span variant = have_variant ? Span(c.var_start[vi], c.var_end[vi]) : Span(0, 0);
      if (have_variant && (!have_block || variant.second <= block.first)) {
        rows.push_back(c.var_text.substr(static_cast<size_t>(c.var_text_off[vi]),
                                         static_cast<size_t>(c.var_text_off[vi + 1] - c.var_text_off[vi])));
        ++vi;
      } else if (have_block && (!have_variant || block.second <= variant.first)) {
        piece(block.first, block.second);
        next_block();
      } else {
        if (block.first < variant.first) piece(block.first, variant.first);
        if (block.second > variant.second) {
          block.first = variant.second;
          moved = true;
        } else {
          next_block();
        }
      }
    }
  }
  return rows;
}

void compare(const Call& c) {
  const dv_gvcf_rows_input in = c.input(1);
  dv_gvcf_text* t = nullptr;
  CHECK(dv_gvcf_rows(&in, &t) == DV_OK && t != nullptr);
  dv_gvcf_text_view v;
  CHECK(dv_gvcf_text_arrays(t, &v) == DV_OK && v.row_off != nullptr);
  bool any = false;
  for (const dv_gvcf_block& b : c.blocks) any = any || b.med_dp >= 0;
  const bool med_dp = c.med_dp < 0 ? any : c.med_dp != 0;
  CHECK((v.med_dp != 0) == med_dp);
  int64_t n_pieces = 0;
  const std::vector<std::string> rows = sequential(c, med_dp, &n_pieces);
  CHECK(v.n_rows == static_cast<int64_t>(rows.size()) && v.n_pieces == n_pieces);
  CHECK(v.row_off[0] == 0 && v.row_off[v.n_rows] == v.n_bytes);
  for (int64_t k = 0; k < v.n_rows; ++k) {
    const std::string& want = rows[static_cast<size_t>(k)];
    CHECK(v.row_off[k + 1] - v.row_off[k] == static_cast<int64_t>(want.size()));
    CHECK(std::memcmp(v.text + v.row_off[k], want.data(), want.size()) == 0);
  }
  dv_gvcf_text_free(t);
  // without row_off: the same bytes
  const dv_gvcf_rows_input plain = c.input(0);
  CHECK(dv_gvcf_rows(&plain, &t) == DV_OK);
  dv_gvcf_text_view w;
  CHECK(dv_gvcf_text_arrays(t, &w) == DV_OK && w.row_off == nullptr && w.n_bytes == v.n_bytes);
  dv_gvcf_text_free(t);
}

void refused(const Call& c, int status = DV_ERR_BAD_INPUT) {
  const dv_gvcf_rows_input in = c.input(1);
  dv_gvcf_text* t = reinterpret_cast<dv_gvcf_text*>(1);
  CHECK(dv_gvcf_rows(&in, &t) == status);
  CHECK(t == nullptr);
}

Call one_block(int64_t start, int64_t end) {
  Call c;
  c.add_block(start, end);
  c.end_group();
  return c;
}

Call cut_block() {            // [0, 30) cut by the variant [12, 15)
  Call c;
  c.add_block(0, 30);
  c.add_variant(12, 15);
  c.end_group();
  return c;
}

}  // namespace

int main() {
  int64_t layouts = 0;
  for (int round = 0; round < 20000; ++round) {
    Call c;
    c.med_dp = static_cast<int32_t>(below(3)) - 1;
    const int groups = 1 + static_cast<int>(below(4));
    for (int g = 0; g < groups; ++g) {
      const bool empty = below(6) == 0;
      const int64_t origin = below(5) == 0 ? 999999990 + below(20) : 0;       // starts and ends across a digit count
      c.add_group(empty ? 0 : below(7), empty || below(6) == 0 ? 0 : below(7), 1 + below(12), origin);
    }
    compare(c);
    ++layouts;
  }
  for (int round = 0; round < 10; ++round) {         // long groups
    Call c;
    c.add_group(2000 + below(3000), below(1500), 40, 0);
    c.add_group(0, 0, 1, 0);
    c.add_group(below(3000), 500 + below(1500), 25, 4000000000ll);
    compare(c);
    ++layouts;
  }
  // the number edges
  for (int64_t start : {0ll, 8ll, 9ll, 98ll, 99ll, 999999998ll, 999999999ll, 2147483648ll, 999999999999ll, -12ll, -1ll}) {
    compare(one_block(start, start + 1));
    compare(one_block(start, start + 2));
  }
  compare(one_block(std::numeric_limits<int64_t>::min() + 1, std::numeric_limits<int64_t>::max()));
  for (int32_t value : {0, 9, 10, 99, 100, 2147483647, -7, std::numeric_limits<int32_t>::min()}) {
    Call c = one_block(5, 50);
    c.blocks[0].gq = value;
    compare(c);
    c.blocks[0].min_dp = value;
    c.blocks[0].med_dp = value;
    compare(c);
  }
  for (double gl : {-0.05, -0.15, -0.25, -1.25, 3000.75, 0.0, -0.0, -9.0e14, 9.0e14}) {
    Call c = one_block(5, 50);
    c.blocks[0].likelihoods[0] = gl;
    compare(c);
    c.blocks[0].likelihoods[2] = gl;
    compare(c);
  }
  {
    Call none;                                        // one group without records, and no group at all
    none.end_group();
    compare(none);
    Call nothing;
    compare(nothing);
    dv_gvcf_text_free(nullptr);
  }
  // what the entry point refuses
  {
    Call c = cut_block();
    compare(c);
    c.var_end_base[0] = 0x7f;
    refused(c);
    c.var_end_base[0] = 'A';
    c.var_end[0] = 30;                                // the end is no piece's start: its base is not read
    c.var_end_base[0] = 0;
    compare(c);
  }
  { Call c = cut_block(); c.blocks[0].ref_base = ' '; refused(c); }
  { Call c = cut_block(); c.blocks[0].likelihoods[1] = std::nan(""); refused(c); }
  { Call c = cut_block(); c.blocks[0].likelihoods[1] = -std::numeric_limits<double>::infinity(); refused(c); }
  { Call c = cut_block(); c.blocks[0].likelihoods[1] = 9007199254740992.0 / 10; refused(c); }
  { Call c = cut_block(); c.var_text_off[0] = 1; refused(c); }
  { Call c = cut_block(); c.var_text_off[1] = 0; refused(c); }
  { Call c = cut_block(); c.var_text_off[1] -= 1; refused(c); }
  { Call c = cut_block(); c.name_off[0] = c.name_off[1] + 1; refused(c); }
  { Call c = cut_block(); c.blocks[0].end = 0; refused(c); }
  { Call c = cut_block(); c.var_end[0] = 12; refused(c); }
  { Call c = cut_block(); c.block_off[0] = 1; refused(c); }
  { Call c = cut_block(); c.med_dp = 2; refused(c, DV_ERR_INVALID_ARGUMENT); }
  {
    const Call c = cut_block();
    dv_gvcf_rows_input in = c.input(1);
    dv_gvcf_text* t = nullptr;
    CHECK(dv_gvcf_rows(&in, nullptr) == DV_ERR_INVALID_ARGUMENT && dv_gvcf_rows(nullptr, &t) == DV_ERR_INVALID_ARGUMENT);
    in.blocks = nullptr;
    CHECK(dv_gvcf_rows(&in, &t) == DV_ERR_INVALID_ARGUMENT && t == nullptr);
    in = c.input(1);
    in.var_text = nullptr;
    CHECK(dv_gvcf_rows(&in, &t) == DV_ERR_INVALID_ARGUMENT && t == nullptr);
    dv_gvcf_rows_stats stats;
    CHECK(dv_gvcf_rows_last_stats(&stats) == DV_OK && dv_gvcf_rows_last_stats(nullptr) == DV_ERR_INVALID_ARGUMENT);
  }
  std::printf("gvcf_rows_check ok: %lld layouts\n", static_cast<long long>(layouts));
  return 0;
}
