// The rule of csrc/realign_finish.h -- the general finish step of FastPassAligner::align_reads as the finish kernels
// of csrc/realign_finish.hip run it -- compiled for the host and applied to seeded random windows, against
// FastPassAligner run in phases: prepare_alignments -> the host aligner -> finish_alignments.  No device needed: the
// sweep kernel's words per pair are rebuilt here from the host aligner's results (corners, band, the M/I/D runs of the
// text CIGAR, last run first).
//   realign_finish_check N [threads] [seed]   N windows (default 100000): references of 150-400 bases with tandem
//                                             repeats, N and lower case; 1-40 haplotypes with substitutions,
//                                             insertions, deletions and changed ends; reads of 30-250 bases, some past
//                                             the haplotype ends, some with their own indels or N; normalize_reads and
//                                             force_alignment on and off; four scoring sets
// Before the windows it runs hand-made cases named for the things a restatement gets wrong, and a fuzz of the merge
// alone (random read and haplotype CIGARs against calculate_read_to_ref_alignment).
// Build (from the repository root; host code only, so the sanitizers apply):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//     -Ideepvariant_amd/csrc tools/realign_finish_check.cpp deepvariant_amd/csrc/fast_pass_aligner.cpp \
//     deepvariant_amd/csrc/local_align.cpp -lpthread -o /tmp/realign_finish_check
// Prints one line of counts; exit status 1 and the first differences on stdout when anything differs.
#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "fast_pass_aligner.h"
#include "realign_finish.h"
#include "realign_finish_stage.h"

namespace {

namespace fin = dv::fin;

constexpr int kMaxBand = 31, kMaxRuns = 64, kOutWords = 8 + kMaxRuns;

struct Counts {
  long windows = 0, windows_on_host = 0, reads = 0, differences = 0, status[3] = {0, 0, 0}, cancelled_reads = 0;
  long hand_cases = 0, merges = 0;
  void add(const Counts& o) {
    windows += o.windows;
    windows_on_host += o.windows_on_host;
    reads += o.reads;
    differences += o.differences;
    for (int i = 0; i < 3; ++i) status[i] += o.status[i];
    cancelled_reads += o.cancelled_reads;
    hand_cases += o.hand_cases;
    merges += o.merges;
  }
};

std::mutex g_print;

struct Rng {
  std::mt19937_64 g;
  explicit Rng(uint64_t seed) : g(seed) {}
  int rnd(int lo, int hi) { return lo + static_cast<int>(g() % static_cast<uint64_t>(hi - lo + 1)); }
  bool chance(double p) { return (g() >> 11) * (1.0 / 9007199254740992.0) < p; }
  std::string bases(int n) {
    std::string s(static_cast<size_t>(n), 'A');
    for (char& c : s) c = "ACGT"[g() % 4];
    return s;
  }
};

// ---------------------------------------------------------------- the sweep's words, rebuilt on the host
// The M/I/D runs of a text CIGAR between its soft clips: '=' and 'X' runs side by side are one M run.
std::vector<uint32_t> runs_of(const std::string& text) {
  std::vector<std::pair<int, int>> runs;
  for (const dv::CigarOp& op : dv::parse_cigar(text)) {
    if (op.op == dv::kOpSoftClip) continue;
    const int k = op.op == dv::kOpMatch ? 0 : op.op == dv::kOpInsert ? 1 : 2;
    if (!runs.empty() && runs.back().first == 0 && k == 0) {
      runs.back().second += op.length;
    } else {
      runs.emplace_back(k, op.length);
    }
  }
  std::vector<uint32_t> words;
  for (size_t i = runs.size(); i-- > 0;) words.push_back((static_cast<uint32_t>(runs[i].second) << 2) | static_cast<uint32_t>(runs[i].first));
  return words;
}

struct FakeSweep {
  std::vector<int32_t> out, seq_off;
  std::vector<fin::SweepItemView> items;
  std::vector<uint8_t> codes;
  bool within_limits = true;

  void build(const dv::AlignmentPairs& pairs, const std::vector<dv::LocalAlignment>& results, const std::vector<char>& ok) {
    seq_off.assign(1, 0);
    for (const dv::CodedSequence& s : pairs.sequences) {
      for (int8_t c : s) codes.push_back(static_cast<uint8_t>(c));
      seq_off.push_back(static_cast<int32_t>(codes.size()));
    }
    const size_t n = pairs.pair_ref.size();
    out.assign(n * kOutWords, 0);
    for (size_t k = 0; k < n; ++k) {
      items.push_back(fin::SweepItemView{pairs.pair_ref[k], pairs.pair_query[k], 1, static_cast<int32_t>(k), 0});
      int32_t* o = out.data() + k * kOutWords;
      const dv::LocalAlignment& al = results[k];
      if (!ok[k]) {                 // an empty sequence, or the reverse pass missed the score
        o[0] = 1;
        o[3] = 0;
        continue;
      }
      o[0] = o[3] = al.score;
      if (al.score <= 0) continue;
      o[1] = al.ref_end;
      o[2] = al.query_end;
      o[4] = al.ref_begin;
      o[5] = al.query_begin;
      const std::vector<uint32_t> words = runs_of(al.cigar);
      if (al.band > kMaxBand || words.size() > static_cast<size_t>(kMaxRuns) || al.band < 1) {
        within_limits = false;      // the device hands such a window back
        continue;
      }
      o[6] = 1;
      o[7] = static_cast<int32_t>(words.size()) | (al.band << 16);
      for (size_t x = 0; x < words.size(); ++x) o[8 + x] = static_cast<int32_t>(words[x]);
    }
  }
  fin::Sweep view() const {
    fin::Sweep s;
    s.out = out.data();
    s.out_words = kOutWords;
    s.n_items = static_cast<int32_t>(items.size());
    s.items = items.data();
    s.seq_off = seq_off.data();
    s.codes = codes.data();
    return s;
  }
};

// ---------------------------------------------------------------- one window through both
struct Case {
  std::string name;               // hand-made cases only
  std::string reference;
  std::vector<std::string> haplotypes, reads;
  dv::AlignerOptions options;
  bool normalize_reads = false;
  int prefix = 0, suffix = 0;
  uint64_t ref_start = 1000;
};

std::string words_text(const std::vector<uint32_t>& w) {
  std::string s;
  for (uint32_t x : w) s += std::to_string(x >> 4) + "?MID?S"[x & 15u];
  return s;
}

// -> differences; `expect` (may be null) receives the host's answer
int run_case(const Case& c, Counts* counts, std::vector<dv::RealignedRead>* expect, long* cancelled_out = nullptr) {
  dv::FastPassAligner a;
  std::string why;
  if (!a.set_options(c.options, &why)) return 0;
  a.set_normalize_reads(c.normalize_reads);
  a.set_ref_prefix_len(c.prefix);
  a.set_ref_suffix_len(c.suffix);
  a.set_reference(c.reference);
  a.set_ref_start(c.ref_start);
  a.set_haplotypes(c.haplotypes);
  dv::AlignmentPairs pairs;
  a.prepare_alignments(c.reads, &pairs);
  std::vector<dv::LocalAlignment> results;
  std::vector<char> ok;
  a.align_pairs_on_host(pairs, 0, pairs.pair_ref.size(), &results, &ok);
  FakeSweep sweep;
  sweep.build(pairs, results, ok);
  fin::Staged staged;
  std::vector<int32_t> item_of_pair(pairs.pair_ref.size());
  for (size_t k = 0; k < item_of_pair.size(); ++k) item_of_pair[k] = static_cast<int32_t>(k);
  fin::stage_window(a, pairs, item_of_pair.data(), static_cast<int64_t>(c.ref_start), &staged);
  const std::vector<dv::RealignedRead> host = a.finish_alignments(pairs, results.data(), ok.data());
  if (expect) *expect = host;
  ++counts->windows;
  if (!sweep.within_limits) {
    ++counts->windows_on_host;
    return 0;
  }
  const fin::Batch b = staged.view(sweep.view(), c.options.force_alignment, c.normalize_reads);
  std::vector<fin::HapState> states(static_cast<size_t>(b.n_haps));
  for (int g = 0; g < b.n_haps; ++g) states[static_cast<size_t>(g)] = fin::hap_state(b, g);
  int differences = 0;
  for (int d = 0; d < b.n_reads; ++d) {
    int cancelled = 0, again = 0;
    const fin::ReadOut count = fin::finish_read(b, states.data(), d, nullptr, &cancelled);
    std::vector<uint32_t> words(static_cast<size_t>(count.n_words) + 1, 0xdeadbeefu);
    std::vector<uint32_t> all(static_cast<size_t>(c.reads[static_cast<size_t>(d)].size()) * 2 + 8);
    const fin::ReadOut write = fin::finish_read(b, states.data(), d, all.data(), &again);
    for (int x = 0; x < count.n_words; ++x) words[static_cast<size_t>(x)] = all[static_cast<size_t>(x)];
    words.pop_back();
    const dv::RealignedRead& e = host[static_cast<size_t>(d)];
    std::vector<uint32_t> want;
    if (e.status == 1) {
      for (const dv::CigarOp& op : e.cigar) want.push_back((static_cast<uint32_t>(op.length) << 4) | static_cast<uint32_t>(op.op));
    }
    const bool same = count.status == e.status && write.status == count.status && write.n_words == count.n_words &&
                      write.position == count.position && count.position == (e.status == 1 ? e.position : 0) &&
                      words == want;
    ++counts->reads;
    ++counts->status[e.status >= 0 && e.status <= 2 ? e.status : 0];
    if (cancelled > 0) {
      ++counts->cancelled_reads;
      if (cancelled_out) ++*cancelled_out;
    }
    if (!same) {
      ++differences;
      std::lock_guard<std::mutex> hold(g_print);
      if (counts->differences + differences <= 5) {
        std::printf("DIFFERENCE %s read %d: host status %d position %lld cigar %s | rule status %d position %lld cigar %s\n",
                    c.name.c_str(), d, e.status, static_cast<long long>(e.position), dv::cigar_text(e.cigar).c_str(),
                    count.status, static_cast<long long>(count.position), words_text(words).c_str());
      }
    }
  }
  return differences;
}

// ---------------------------------------------------------------- seeded windows
Case draw(uint64_t seed) {
  Rng r(seed);
  Case c;
  c.name = "seed " + std::to_string(seed);
  std::string ref = r.bases(r.rnd(150, 400));
  if (r.chance(0.6)) {
    const int p = r.rnd(20, static_cast<int>(ref.size()) - 40);
    const std::string unit = r.bases(r.rnd(1, 5));
    std::string repeat;
    for (int i = r.rnd(3, 12); i > 0; --i) repeat += unit;
    ref.replace(static_cast<size_t>(p), std::min(repeat.size(), ref.size() - static_cast<size_t>(p) - 10), repeat);
  }
  if (ref.size() > 400) ref.resize(400);
  const int n = static_cast<int>(ref.size());
  c.prefix = r.rnd(0, 40);
  c.suffix = r.rnd(0, 40);
  // haplotypes: edits of the upper-case reference
  const int n_haps = r.chance(0.15) ? r.rnd(17, 40) : r.rnd(1, 8);
  std::vector<std::string> haps;
  for (int h = 0; h < n_haps; ++h) {
    std::string s = ref;
    if (h > 0 && r.chance(0.25)) s = haps[static_cast<size_t>(r.rnd(0, h - 1))];   // a relative (or a twin) of an earlier one
    for (int e = r.rnd(0, 4); e > 0; --e) {
      const int len = static_cast<int>(s.size());
      if (len < 60) break;
      const int p = r.rnd(5, len - 20);
      switch (r.rnd(0, 5)) {
        case 0: s[static_cast<size_t>(p)] = "ACGT"[r.rnd(0, 3)]; break;
        case 1: s.insert(static_cast<size_t>(p), r.chance(0.5) ? s.substr(static_cast<size_t>(p), static_cast<size_t>(r.rnd(1, 6))) : r.bases(r.rnd(1, 12))); break;
        case 2: s.erase(static_cast<size_t>(p), static_cast<size_t>(r.rnd(1, 12))); break;
        case 3: s.replace(0, static_cast<size_t>(r.rnd(1, 12)), r.bases(r.rnd(1, 12))); break;                  // a changed front: soft clip
        case 4: s.replace(s.size() - static_cast<size_t>(r.rnd(1, 12)), std::string::npos, r.bases(r.rnd(1, 12))); break;   // a changed end
        default: s[static_cast<size_t>(p)] = 'N'; break;
      }
    }
    if (r.chance(0.02)) s.assign(s.size(), 'N');
    haps.push_back(s);
  }
  if (r.chance(0.5)) haps[static_cast<size_t>(r.rnd(0, n_haps - 1))] = ref;
  // N and lower case in the reference as handed over
  for (int e = r.rnd(0, 3); e > 0; --e) ref[static_cast<size_t>(r.rnd(0, n - 1))] = 'N';
  if (r.chance(0.3)) {
    const int p = r.rnd(0, n - 10), len = r.rnd(1, 9);
    for (int i = p; i < p + len; ++i) ref[static_cast<size_t>(i)] = static_cast<char>(std::tolower(static_cast<unsigned char>(ref[static_cast<size_t>(i)])));
  }
  c.reference = ref;
  c.haplotypes = haps;
  // reads: pieces of the haplotypes
  const int n_reads = r.rnd(1, r.chance(0.1) ? 70 : 24);
  const int base_len = r.rnd(30, 250);
  for (int i = 0; i < n_reads; ++i) {
    const std::string& h = haps[static_cast<size_t>(r.rnd(0, n_haps - 1))];
    const int hl = static_cast<int>(h.size());
    int len = r.chance(0.7) ? base_len : r.rnd(30, 250);
    len = std::min(len, hl);
    const int p = r.rnd(0, hl - len);
    std::string s = h.substr(static_cast<size_t>(p), static_cast<size_t>(len));
    if (r.chance(0.35)) {                                   // its own differences
      for (int e = r.rnd(1, 3); e > 0; --e) {
        const int q = r.rnd(1, static_cast<int>(s.size()) - 2);
        switch (r.rnd(0, 3)) {
          case 0: s[static_cast<size_t>(q)] = "ACGT"[r.rnd(0, 3)]; break;
          case 1: s.insert(static_cast<size_t>(q), r.chance(0.5) ? s.substr(static_cast<size_t>(q), 1) : r.bases(r.rnd(1, 8))); break;
          case 2: s.erase(static_cast<size_t>(q), static_cast<size_t>(r.rnd(1, 8))); break;
          default: s[static_cast<size_t>(q)] = 'N'; break;
        }
      }
    }
    if (r.chance(0.15)) s = r.chance(0.5) ? r.bases(r.rnd(1, 20)) + s : s + r.bases(r.rnd(1, 20));   // past the haplotype
    if (r.chance(0.1)) {
      for (char& ch : s) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
    }
    if (s.size() < 30) s += r.bases(30 - static_cast<int>(s.size()));
    if (s.size() > 250) s.resize(250);
    c.reads.push_back(s);
  }
  static const int kScoring[4][4] = {{4, 6, 8, 1}, {1, 4, 6, 1}, {2, 3, 5, 2}, {4, 6, 8, 2}};
  const int* sc = kScoring[r.rnd(0, 3)];
  c.options.match = sc[0];
  c.options.mismatch = sc[1];
  c.options.gap_open = sc[2];
  c.options.gap_extend = sc[3];
  c.options.kmer_size = r.chance(0.5) ? 32 : r.rnd(8, 31);
  c.options.read_size = static_cast<int>(c.reads[0].size());
  c.options.max_num_of_mismatches = r.rnd(1, 3);
  c.options.similarity_threshold = r.chance(0.5) ? 0.85 : 0.5 + 0.1 * r.rnd(0, 4);
  c.options.force_alignment = r.chance(0.3);
  c.normalize_reads = r.chance(0.5);
  c.ref_start = static_cast<uint64_t>(r.rnd(0, 1) ? r.rnd(0, 5) : r.rnd(1000, 2000000000));
  return c;
}

// ---------------------------------------------------------------- the merge alone, against the host's own function
// Text tokens -> an Ops over words in the sweep's layout.
struct OwnedOps {
  std::vector<uint32_t> words;
  std::vector<uint8_t> rc, qc;      // codes that give the text's '=' / 'X' pieces back
  fin::Ops ops;
  explicit OwnedOps(const std::string& text) {
    const dv::Cigar all = dv::parse_cigar(text);
    size_t first = 0, last = all.size();
    if (first < last && all[first].op == dv::kOpSoftClip) ops.lead = all[first++].length;
    if (first < last && all[last - 1].op == dv::kOpSoftClip) ops.tail = all[--last].length;
    std::string middle;
    for (size_t i = first; i < last; ++i) middle += std::to_string(all[i].length) + (all[i].op == dv::kOpMatch ? '=' : all[i].op == dv::kOpInsert ? 'I' : 'D');
    words = runs_of(middle);
    {
      size_t i = 0;
      while (i < text.size()) {                 // the tokens once more, this time telling '=' from 'X'
        size_t j = i;
        int len = 0;
        while (j < text.size() && std::isdigit(static_cast<unsigned char>(text[j]))) len = len * 10 + (text[j++] - '0');
        const char op = text[j];
        if (op == '=' || op == 'X') {
          rc.insert(rc.end(), static_cast<size_t>(len), 0);
          qc.insert(qc.end(), static_cast<size_t>(len), op == '=' ? 0 : 1);
        } else if (op == 'I') {
          qc.insert(qc.end(), static_cast<size_t>(len), 2);
        } else if (op == 'D') {
          rc.insert(rc.end(), static_cast<size_t>(len), 2);
        }
        i = j + 1;
      }
      rc.push_back(3);
      qc.push_back(3);
    }
    ops.rc = rc.data();
    ops.qc = qc.data();
    ops.n_runs = static_cast<int>(words.size());
    ops.runs = words.data();
  }
};

int read_bases(const dv::Cigar& c) {
  int n = 0;
  for (const dv::CigarOp& o : c) n += o.op != dv::kOpDelete ? o.length : 0;
  return n;
}

// -> true when the rule's words equal calculate_read_to_ref_alignment's
bool merge_agrees(const std::string& read_cigar, const std::string& hap_cigar, int position, const char* name, std::string* got_text = nullptr) {
  const dv::Cigar r_ops = dv::parse_cigar(read_cigar);
  const int read_len = read_bases(r_ops);
  dv::FastPassAligner a;
  a.set_reads({std::string(static_cast<size_t>(read_len), 'A')});
  dv::ReadAlignment ra;
  ra.position = static_cast<uint16_t>(position);
  ra.cigar = read_cigar;
  ra.score = 1;
  dv::Cigar want;
  std::string error;
  const bool host_ok = a.calculate_read_to_ref_alignment(0, ra, dv::parse_cigar(hap_cigar), &want, &error);
  if (!host_ok) want.clear();
  const OwnedOps r(read_cigar), h(hap_cigar);
  fin::Queue r2h, h2r;
  r2h.ops = &r.ops;
  r2h.n = r.ops.size();
  h2r.ops = &h.ops;
  h2r.n = h.ops.size();
  std::vector<uint32_t> out(static_cast<size_t>(read_len) * 2 + 8);
  dv::alt::Merger m;
  m.read_len = read_len;
  m.out = out.data();
  const std::vector<uint8_t> read_bytes(static_cast<size_t>(read_len) + 1, 'A');
  m.read = read_bytes.data();
  std::vector<uint32_t> got;
  int cancelled = 0;
  if (fin::left_trim(&h2r, position)) {
    const bool cleared = fin::merge_walk(r2h, h2r, &m, &cancelled);
    m.flush();
    if (!cleared) got.assign(out.begin(), out.begin() + m.n_out);
  }
  std::vector<uint32_t> want_words;
  for (const dv::CigarOp& op : want) want_words.push_back((static_cast<uint32_t>(op.length) << 4) | static_cast<uint32_t>(op.op));
  if (got_text) *got_text = words_text(got);
  if (got == want_words) return true;
  std::lock_guard<std::mutex> hold(g_print);
  std::printf("DIFFERENCE merge %s: read %s at %d on haplotype %s: host %s | rule %s\n", name, read_cigar.c_str(), position,
              hap_cigar.c_str(), dv::cigar_text(want).c_str(), words_text(got).c_str());
  return false;
}

std::string random_cigar(Rng& r, bool read_side, int* consumed) {
  // [S] (=|X|I|D)+ [S]: starts and ends with a match, no two indels of a kind side by side
  std::string s;
  *consumed = 0;
  auto add = [&](int len, char op) {
    s += std::to_string(len) + op;
    if (op != 'D') *consumed += len;
  };
  if (r.chance(0.3)) add(r.rnd(1, 6), 'S');
  add(r.rnd(1, 12), '=');
  char last = '=';
  for (int k = r.rnd(0, read_side ? 5 : 7); k > 0; --k) {
    const int t = r.rnd(0, 3);
    const char op = t == 0 ? 'I' : t == 1 ? 'D' : t == 2 ? 'X' : '=';
    if (op == last) continue;
    add(r.rnd(1, op == '=' ? 12 : 4), op);
    last = op;
  }
  if (last == 'I' || last == 'D') add(r.rnd(1, 9), '=');
  if (r.chance(0.3)) add(r.rnd(1, 6), 'S');
  return s;
}

// ---------------------------------------------------------------- hand-made cases, named for what they hold
bool sort_order_agrees(int n, uint64_t seed) {
  Rng r(seed);
  std::vector<dv::HaplotypeAlignment> real(static_cast<size_t>(n));
  std::vector<int32_t> scores(static_cast<size_t>(n)), perm(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    scores[static_cast<size_t>(i)] = r.chance(0.5) ? 0 : 100 * r.rnd(1, 4);
    real[static_cast<size_t>(i)].haplotype_index = static_cast<size_t>(i);
    real[static_cast<size_t>(i)].haplotype_score = scores[static_cast<size_t>(i)];
    real[static_cast<size_t>(i)].reads.resize(3);
    real[static_cast<size_t>(i)].cigar = "12=";
  }
  std::sort(real.begin(), real.end(), [](const dv::HaplotypeAlignment& a, const dv::HaplotypeAlignment& b) {
    return a.haplotype_score < b.haplotype_score;
  });
  fin::sorted_order(scores.data(), n, perm.data());
  for (int i = 0; i < n; ++i) {
    if (static_cast<size_t>(perm[static_cast<size_t>(i)]) != real[static_cast<size_t>(i)].haplotype_index) return false;
  }
  return true;
}

bool map_agrees(const std::string& cigar, int size) {
  const std::vector<int> want = dv::positions_map(cigar, static_cast<size_t>(size));
  const OwnedOps o(cigar);
  for (int p = 0; p < size; ++p) {
    if (fin::map_value(o.ops, p) != want[static_cast<size_t>(p)]) {
      std::printf("DIFFERENCE positions_map %s at %d: host %d | rule %d\n", cigar.c_str(), p, want[static_cast<size_t>(p)], fin::map_value(o.ops, p));
      return false;
    }
  }
  return true;
}

int hand_cases(Counts* counts) {
  int bad = 0;
  auto expect = [&](bool ok, const char* name) {
    ++counts->hand_cases;
    if (!ok) {
      ++bad;
      std::printf("HAND CASE FAILED: %s\n", name);
    }
  };
  // 1. order of the haplotypes: std::sort over (score, index) moves as it does over the real objects
  for (int n : {1, 2, 16, 17, 40, 96}) {
    for (uint64_t s = 0; s < 20; ++s) expect(sort_order_agrees(n, 77 * static_cast<uint64_t>(n) + s), "order_of_haplotypes");
  }
  // 3. positions_map: S lowers then fills, D raises, I fills and lowers per base
  expect(map_agrees("3S5=2D4=3I6=2S", 30), "positions_map_all_kinds");
  expect(map_agrees("10=", 14), "positions_map_short_cigar_leaves_zeroes");
  expect(map_agrees("", 5), "positions_map_empty");
  // 4. the left trim
  std::string got;
  expect(merge_agrees("4=", "5=3D6=", 5, "left_trim_front_d_dropped", &got) && got == "4M", "left_trim_front_d_dropped");
  expect(merge_agrees("4=", "5=3I6=", 6, "left_trim_inside_insertion", &got) && got == "2I2M", "left_trim_inside_insertion");
  expect(merge_agrees("4=", "5=", 5, "left_trim_nothing_left", &got) && got.empty(), "left_trim_nothing_left");
  expect(merge_agrees("4=", "2S5=2D", 7, "left_trim_only_d_left", &got) && got.empty(), "left_trim_only_d_left");
  // 5. the base-by-base merge
  expect(merge_agrees("2=3I4=", "2=2D9=", 0, "merge_i3_x_d2", &got) && got == "2M1I6M", "merge_i3_x_d2");
  expect(merge_agrees("2=1I4=", "2=3D9=", 0, "merge_i1_x_d3", &got), "merge_i1_x_d3");
  expect(merge_agrees("2=2D4=", "2=3I9=", 0, "merge_d2_x_i3", &got), "merge_d2_x_i3");
  expect(merge_agrees("2=3D4=", "2=1I9=", 0, "merge_d3_x_i1", &got), "merge_d3_x_i1");
  expect(merge_agrees("3S4=", "9=", 2, "merge_leading_soft_clip", &got) && got == "3S4M", "merge_leading_soft_clip");
  expect(merge_agrees("4=3S", "6=", 2, "merge_soft_clipped_tail_past_the_end", &got) && got == "4M3S", "merge_soft_clipped_tail_past_the_end");
  expect(merge_agrees("8=", "6=", 2, "merge_read_past_the_haplotype_is_cleared", &got) && got.empty(), "merge_read_past_the_haplotype_is_cleared");
  expect(merge_agrees("4=2I3=", "5=2S", 0, "merge_s_over_i", &got), "merge_s_over_i");
  {
    Rng r(4242);
    int bad_merges = 0;
    for (int i = 0; i < 200000; ++i) {
      int read_len = 0, hap_len = 0;
      const std::string rc = random_cigar(r, true, &read_len), hc = random_cigar(r, false, &hap_len);
      const int position = r.rnd(0, hap_len + 1);
      if (!merge_agrees(rc, hc, position, "fuzz")) {
        if (++bad_merges > 5) break;
      }
      ++counts->merges;
    }
    expect(bad_merges == 0, "merge_fuzz");
    for (int i = 0; i < 20000; ++i) {
      int len = 0;
      const std::string hc = random_cigar(r, false, &len);
      if (!map_agrees(hc, len + r.rnd(0, 3))) {
        expect(false, "positions_map_fuzz");
        break;
      }
    }
  }
  // whole windows
  const std::string ref = "GATTACAGGCTTAACCGGTTAGCATCGATCGGATATCGCGCTAAGGCTTACGGATCAGTCAGGCTAGCTAAGCTTGGCCAATCGATTGCAGTCAAGCTTGACCGTAGCTAGGATCCAGTCA";
  auto window = [&](const char* name, std::vector<std::string> haps, std::vector<std::string> reads, bool force, bool normalize) {
    Case c;
    c.name = name;
    c.reference = ref;
    c.haplotypes = std::move(haps);
    c.reads = std::move(reads);
    c.options.kmer_size = 12;
    c.options.read_size = static_cast<int>(c.reads[0].size());
    c.options.force_alignment = force;
    c.normalize_reads = normalize;
    Counts own;
    std::vector<dv::RealignedRead> host;
    const int d = run_case(c, &own, &host);
    expect(d == 0 && own.windows_on_host == 0, name);
    return host;
  };
  std::string ins = ref, del = ref, clipped = ref;
  ins.insert(60, "TTTGGG");
  del.erase(60, 5);
  clipped.replace(0, 8, "TTTTTTTT");
  {
    // 2. is_reference: a lower-case twin of the reference is not byte-equal but aligns as one '=' run
    std::string lower = ref;
    for (char& ch : lower) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
    const auto host = window("is_reference_by_alignment", {lower, ins}, {ref.substr(10, 60), ins.substr(30, 60)}, true, false);
    expect(host[0].status == 1, "is_reference_by_alignment: the reference read is placed");
  }
  {
    const auto host = window("haplotype_with_insertion_and_deletion", {ref, ins, del}, {ins.substr(30, 60), del.substr(30, 60), ins.substr(62, 40), del.substr(60, 40)}, false, true);
    expect(host[0].status == 1 && host[0].cigar.size() == 3 && host[0].cigar[1].op == dv::kOpInsert, "a read over the haplotype's insertion carries it");
    expect(host[1].status == 1 && host[1].cigar.size() == 3 && host[1].cigar[1].op == dv::kOpDelete, "a read over the haplotype's deletion carries it");
    expect(host[2].status == 1 && host[2].cigar[0].op == dv::kOpInsert, "a read starting inside the insertion starts with I");
    expect(host[3].status == 1 && host[3].cigar[0].op == dv::kOpMatch, "a read right behind the deletion starts with M");
  }
  {
    // 3. a haplotype that cannot be aligned keeps an empty CIGAR: its reads come out with status 0
    const std::string all_n(ref.size(), 'N');
    const auto host = window("haplotype_all_n", {ref, all_n}, {ref.substr(5, 50), std::string(40, 'N')}, false, false);
    expect(host[1].status == 0, "haplotype_all_n: status 0");
  }
  {
    // 6. offset < 0: the haplotype's own alignment starts with a soft clip
    window("haplotype_with_soft_clips_offset_negative", {clipped, ref}, {clipped.substr(0, 50), clipped.substr(2, 60)}, false, false);
    window("haplotype_with_soft_clips_normalize", {clipped, ins}, {clipped.substr(0, 50), ins.substr(40, 50)}, false, true);
  }
  {
    // 7. force_alignment: status 2 without an alignment, and a target that is not the reference is dropped
    const auto host = window("force_alignment_no_alignment", {ref}, {std::string(40, 'N'), ref.substr(3, 40)}, true, false);
    expect(host[0].status == 2 && host[1].status == 1, "force_alignment: status 2 / 1");
    std::string read = ins.substr(40, 50);
    read[25] = read[25] == 'A' ? 'C' : 'A';
    read[3] = read[3] == 'A' ? 'C' : 'A';
    read[40] = read[40] == 'A' ? 'C' : 'A';
    window("force_alignment_haplotype_not_the_reference", {ins, ref}, {read, ref.substr(0, 50)}, true, false);
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  const long n = argc > 1 ? std::atol(argv[1]) : 100000;
  const int threads = argc > 2 ? std::max(1, std::atoi(argv[2])) : 1;
  const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 1;
  Counts total;
  const int bad_cases = hand_cases(&total);
  total.windows = 0;      // the hand-made windows are counted as cases
  total.reads = 0;
  total.status[0] = total.status[1] = total.status[2] = 0;
  total.cancelled_reads = 0;
  std::atomic<long> next{0};
  std::mutex lock;
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t) {
    pool.emplace_back([&] {
      Counts own;
      for (;;) {
        const long i = next.fetch_add(1);
        if (i >= n) break;
        const Case c = draw(seed * 1000003ull + static_cast<uint64_t>(i));
        own.differences += run_case(c, &own, nullptr);
      }
      std::lock_guard<std::mutex> hold(lock);
      total.add(own);
    });
  }
  for (std::thread& t : pool) t.join();
  std::printf("realign_finish_check: seed %llu windows %ld (handed back %ld) reads %ld differences %ld status0 %ld status1 %ld "
              "status2 %ld reads_with_id_cancellation %ld hand_cases %ld failed %d merge_fuzz %ld\n",
              static_cast<unsigned long long>(seed), total.windows, total.windows_on_host, total.reads, total.differences,
              total.status[0], total.status[1], total.status[2], total.cancelled_reads, total.hand_cases, bad_cases,
              total.merges);
  return total.differences == 0 && bad_cases == 0 ? 0 : 1;
}
