// The rule of csrc/debruijn_paths.h -- prune + candidate_haplotypes as a closed form, the pieces the paths kernel of
// csrc/debruijn.hip runs -- compiled for the host and applied to DeBruijnGraph::build_compact's output alone, against
// DeBruijnGraph::build(...)->candidate_haplotypes() on seeded random windows with pruning on.  No device needed.
//   debruijn_paths_check N [threads]     N windows (default 100000): 120-320-base references with tandem repeats, N
//                                        and lower case in reference and reads, up to five alternative haplotypes
//                                        with up to three edits each, 20-140 reads; min_k {10, 12, 15}, max_k
//                                        {31, 51, 101}, step_k {1, 2}, min_edge_weight {1, 2, 3}, max_num_paths
//                                        {2, 4, 8, 256}
// The counts follow the kernel's shape: pending out-edge counters, in-edge lists, a reverse peel from the vertices
// with nothing pending, a vertex's count summed over its out-edges when its last target resolves.
// Build (from the repository root; host code only, so the sanitizers apply):
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//     -Ideepvariant_amd/csrc tools/debruijn_paths_check.cpp deepvariant_amd/csrc/debruijn_graph.cpp -lpthread \
//     -o /tmp/debruijn_paths_check
// (neither file needs HIP; hipcc compiles them as plain C++ too).  Prints one line of counts; exit status 1 and the first
// differing windows on stdout when anything differs.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "debruijn_graph.h"
#include "debruijn_paths.h"

namespace {

struct Window {
  std::string ref;
  std::vector<std::string> bases;
  std::vector<std::vector<uint8_t>> quals;
  std::vector<int> mapq;
  dv::DeBruijnOptions options;
};

Window draw(uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto rnd = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<uint64_t>(hi - lo + 1)); };
  auto chance = [&](double p) { return (rng() >> 11) * (1.0 / 9007199254740992.0) < p; };
  auto random_bases = [&](int n) {
    std::string s(static_cast<size_t>(n), 'A');
    for (char& c : s) c = "ACGT"[rng() % 4];
    return s;
  };
  Window w;
  w.ref = random_bases(rnd(120, 320));
  if (chance(0.4)) {
    const int p = rnd(30, static_cast<int>(w.ref.size()) - 60);
    const std::string unit = random_bases(rnd(1, 4));
    std::string repeat;
    for (int i = rnd(5, 13); i > 0; --i) repeat += unit;
    w.ref.insert(static_cast<size_t>(p), repeat);
  }
  std::vector<std::string> haps{w.ref};
  for (int h = rnd(0, 5); h > 0; --h) {
    std::string s = w.ref;
    for (int e = rnd(1, 3); e > 0; --e) {
      const int p = rnd(25, static_cast<int>(s.size()) - 26);
      const int kind = rnd(0, 9);
      if (kind < 4) {
        s[p] = "ACGT"[rng() % 4];
      } else if (kind < 7) {
        s.insert(static_cast<size_t>(p), random_bases(rnd(1, 9)));
      } else {
        s.erase(static_cast<size_t>(p), static_cast<size_t>(rnd(1, 9)));
      }
    }
    haps.push_back(s);
  }
  // the reference's own oddities, after the haplotypes were cut from the clean one: reads never match them
  if (chance(0.25)) w.ref[rnd(0, static_cast<int>(w.ref.size()) - 1)] = 'N';
  if (chance(0.25)) {
    char& c = w.ref[rnd(0, static_cast<int>(w.ref.size()) - 1)];
    c = static_cast<char>(c - 'A' + 'a');
  }
  for (int i = rnd(20, 140); i > 0; --i) {
    const std::string& hap = haps[rng() % haps.size()];
    const int len = rnd(60, std::min<int>(150, static_cast<int>(hap.size())) - 1);
    const int s0 = rnd(0, static_cast<int>(hap.size()) - len);
    std::string seq = hap.substr(static_cast<size_t>(s0), static_cast<size_t>(len));
    std::vector<uint8_t> q(static_cast<size_t>(len));
    for (uint8_t& x : q) x = static_cast<uint8_t>(rnd(16, 44));
    if (chance(0.08)) q[static_cast<size_t>(rnd(0, len - 1))] = 5;
    if (chance(0.15)) seq[static_cast<size_t>(rnd(0, len - 1))] = "ACGTN"[rng() % 5];
    if (chance(0.1)) {
      for (char& c : seq) c = static_cast<char>(c >= 'A' && c <= 'Z' ? c - 'A' + 'a' : c);
    }
    w.bases.push_back(seq);
    w.quals.push_back(q);
    w.mapq.push_back(rnd(8, 60));
  }
  w.options.min_k = (int[]){10, 12, 15}[rng() % 3];
  w.options.max_k = (int[]){31, 51, 101}[rng() % 3];
  w.options.step_k = (int[]){1, 2}[rng() % 2];
  w.options.min_edge_weight = (int[]){1, 2, 3}[rng() % 3];
  w.options.max_num_paths = (int[]){2, 4, 8, 256}[rng() % 4];
  w.options.disable_graph_pruning = false;
  return w;
}

constexpr uint32_t kNone = 0xffffffffu;

// The rule on a compact graph.  false: the tables are inconsistent (never expected).  *too_many, or the walks' text.
bool rule(const Window& w, const dv::CompactGraph& c, bool* too_many, uint32_t* n_walks, std::vector<std::string>* haps) {
  namespace P = dv::paths;
  const int k = c.k;
  const size_t nv = c.vertex_seq.size(), ne = c.edge_from.size();
  const uint32_t source = 0, sink = static_cast<uint32_t>(w.ref.size()) - static_cast<uint32_t>(k);
  const uint32_t cap = P::count_cap(w.options.max_num_paths);
  auto last_byte = [&](uint32_t v) -> int {
    const int32_t seq = c.vertex_seq[v];
    const size_t at = static_cast<size_t>(c.vertex_pos[v]) + static_cast<size_t>(k) - 1;
    if (seq == 0) return static_cast<unsigned char>(w.ref[at]);
    const char ch = w.bases[static_cast<size_t>(seq) - 1][at];
    return static_cast<unsigned char>(ch >= 'a' && ch <= 'z' ? ch - 'a' + 'A' : ch);
  };
  auto alive = [&](size_t e) {
    return P::edge_alive(static_cast<uint32_t>(c.edge_weight[e]), c.edge_is_ref[e] != 0, w.options.min_edge_weight);
  };
  // (a) out-edge lists, pending counters and in-edge lists
  std::vector<uint32_t> head(nv, kNone), enext(ne, kNone), inhead(nv, kNone), innext(ne, kNone), pending(nv, 0), cnt(nv, 0);
  for (size_t e = 0; e < ne; ++e) {
    const uint32_t from = static_cast<uint32_t>(c.edge_from[e]), to = static_cast<uint32_t>(c.edge_to[e]);
    enext[e] = head[from];
    head[from] = static_cast<uint32_t>(e);
    if (from == sink || !alive(e)) continue;
    ++pending[from];
    innext[e] = inhead[to];
    inhead[to] = static_cast<uint32_t>(e);
  }
  cnt[sink] = 1;
  // (b) the reverse peel
  std::vector<uint32_t> work;
  for (uint32_t v = 0; v < nv; ++v) {
    if (pending[v] == 0) work.push_back(v);
  }
  size_t resolved = 0;
  for (size_t at = 0; at < work.size(); ++at) {
    ++resolved;
    for (uint32_t e = inhead[work[at]]; e != kNone; e = innext[e]) {
      const uint32_t u = static_cast<uint32_t>(c.edge_from[e]);
      if (--pending[u] != 0) continue;
      uint32_t sum = 0;
      for (uint32_t f = head[u]; f != kNone; f = enext[f]) {
        if (alive(f)) sum = P::saturating_add(sum, cnt[static_cast<uint32_t>(c.edge_to[f])], cap);
      }
      cnt[u] = sum;
      work.push_back(u);
    }
  }
  if (resolved != nv) return false;
  // (c)
  const uint32_t T = cnt[source];
  *n_walks = T;
  *too_many = T >= cap;
  haps->clear();
  if (*too_many) return true;
  if (T == 0) return false;
  // (d) unranking
  for (uint32_t number = 0; number < T; ++number) {
    uint32_t r = number, v = source;
    std::string text = w.ref.substr(0, static_cast<size_t>(k));
    for (size_t steps = 0; v != sink; ++steps) {
      if (steps >= nv) return false;
      int after = P::kNoByte, byte = 0;
      uint32_t chosen = kNone;
      for (size_t rounds = 0; rounds <= ne; ++rounds) {
        int best = P::kPastBytes;
        uint32_t best_to = kNone;
        for (uint32_t e = head[v]; e != kNone; e = enext[e]) {
          if (!alive(e)) continue;
          const uint32_t to = static_cast<uint32_t>(c.edge_to[e]);
          const int b = last_byte(to);
          if (P::next_in_order(after, b, best)) {
            best = b;
            best_to = to;
          }
        }
        if (best_to == kNone) break;
        if (P::take_edge(&r, cnt[best_to])) {
          chosen = best_to;
          byte = best;
          break;
        }
        after = best;
      }
      if (chosen == kNone) return false;
      text.push_back(static_cast<char>(byte));
      v = chosen;
    }
    haps->push_back(text);
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const long n = argc > 1 ? std::atol(argv[1]) : 100000;
  const int n_threads = argc > 2 ? std::atoi(argv[2]) : static_cast<int>(std::max(1u, std::thread::hardware_concurrency()));
  std::atomic<long> next{0}, differ{0}, no_graph{0}, over{0}, multi{0};
  std::mutex lock;
  long largest_t = 0, largest_bytes = 0;
  auto work = [&] {
    for (;;) {
      const long i = next.fetch_add(1);
      if (i >= n) return;
      const Window w = draw(0x5eed0000ull + static_cast<uint64_t>(i));
      std::vector<dv::AssemblyRead> reads;
      for (size_t r = 0; r < w.bases.size(); ++r) {
        reads.push_back(dv::AssemblyRead{w.bases[r], w.quals[r].data(), w.mapq[r]});
      }
      dv::CompactGraph c;
      dv::DeBruijnGraph::build_compact(w.ref, reads, w.options, &c);
      const std::unique_ptr<dv::DeBruijnGraph> graph = dv::DeBruijnGraph::build(w.ref, reads, w.options);
      bool same = (c.k == 0) == !graph;
      if (same && graph) {
        const std::vector<std::string> want = graph->candidate_haplotypes();
        bool too_many = false;
        uint32_t walks = 0;
        std::vector<std::string> got;
        same = c.k == graph->kmer_size() && rule(w, c, &too_many, &walks, &got) && too_many == want.empty() && got == want;
        if (same) {
          long bytes = 0;
          for (const std::string& h : got) bytes += static_cast<long>(h.size());
          if (too_many) ++over;
          if (got.size() > 1) ++multi;
          std::lock_guard<std::mutex> hold(lock);
          largest_t = std::max(largest_t, static_cast<long>(got.size()));
          largest_bytes = std::max(largest_bytes, bytes);
        }
      } else if (same) {
        ++no_graph;
      }
      if (!same && differ.fetch_add(1) < 10) {
        std::lock_guard<std::mutex> hold(lock);
        std::printf("window %ld differs (k %d, min_edge_weight %d, max_num_paths %d)\n", i, c.k, w.options.min_edge_weight,
                    w.options.max_num_paths);
      }
    }
  };
  std::vector<std::thread> threads;
  for (int t = 1; t < n_threads; ++t) threads.emplace_back(work);
  work();
  for (std::thread& t : threads) t.join();
  std::printf("windows %ld differences %ld no_graph %ld over_max_num_paths %ld multi_path %ld largest_T %ld "
              "largest_hap_bytes %ld\n",
              n, differ.load(), no_graph.load(), over.load(), multi.load(), largest_t, largest_bytes);
  return differ.load() ? 1 : 0;
}
