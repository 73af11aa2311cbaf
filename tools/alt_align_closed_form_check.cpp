// finish_pair (csrc/alt_align.h, the closed form the finish kernels of alt_align.hip run) compiled for the host and
// compared with FastPassAligner's own code, no device needed.  Two modes:
//   alt_align_closed_form_check N        N seeds of 24 reads against one target (random, low-complexity, with N,
//                                        lower-case or homopolymer blocks): fast pass, local aligner and
//                                        finish_alignments give the expected status, position and CIGAR per read
//   alt_align_closed_form_check N syn    N random run lists -- not an aligner's output: zero lengths, soft clips in
//                                        the middle, lengths that over- or under-run the read, any position --
//                                        against calculate_read_to_ref_alignment + is_alignment_normalized.  This
//                                        is the mode that reaches the read_len cap, the cleared CIGAR and the
//                                        single-call cancel past the haplotype's end, which no alignment of the
//                                        local aligner produces.
// Build (from the repository root, after libdvhip.so):
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Iinclude -Ideepvariant_amd/csrc tools/alt_align_closed_form_check.cpp \
//     -Ldeepvariant_amd -ldvhip -Wl,-rpath,$PWD/deepvariant_amd -o /tmp/alt_align_closed_form_check
// Exit status 1 and the first differing cases on stdout when anything differs.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "alt_align.h"
#include "fast_pass_aligner.h"
#include "fast_pass_device.h"

int synthetic(int n_cases) {
  long long bad = 0, st[2] = {0, 0}, unnorm = 0;
  std::mt19937 rng(7);
  auto rnd = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); };
  for (int it = 0; it < n_cases; ++it) {
    const int n = rnd(1, 40);
    std::string target(n, 'A');
    for (char& c : target) c = "AC"[rng() % 2];
    dv::Cigar runs;
    const int n_runs = rnd(0, 7);
    int read_consumed = 0;
    for (int x = 0; x < n_runs; ++x) {
      const int op = (x == 0 || x == n_runs - 1) && rng() % 3 == 0 ? 5 : (int[]){1, 1, 2, 3, 5}[rng() % (rng() % 8 == 0 ? 5 : 4)];
      const int len = rng() % 10 == 0 ? 0 : rnd(1, 12);
      runs.push_back({op, len});
      if (op != 3) read_consumed += len;
    }
    const int L = rng() % 4 == 0 ? rnd(0, read_consumed + 3) : read_consumed;
    std::string read(L, 'A');
    for (char& c : read) c = "AC"[rng() % 2];
    const int p = rnd(0, n + 1);
    for (int normalize = 0; normalize < 2; ++normalize) {
      dv::FastPassAligner a;
      a.set_reference(target);
      a.set_haplotypes({target});
      a.set_reads({read});
      dv::Cigar want;
      if (p < n) {
        dv::ReadAlignment ra;
        ra.position = static_cast<uint16_t>(p);
        ra.cigar = dv::cigar_text(runs);
        std::string error;
        if (!a.calculate_read_to_ref_alignment(0, ra, dv::Cigar{{1, n}}, &want, &error)) want.clear();
        if (!want.empty() && !a.is_alignment_normalized(want, p, read)) {
          ++unnorm;
          if (!normalize) want.clear();
        }
      }
      std::string bytes = read + target;
      std::vector<uint32_t> words;
      for (const dv::CigarOp& op : runs) words.push_back((static_cast<uint32_t>(op.length) << 4) | op.op);
      dv::alt::PairIn pr{L, n, 0, L, dv::alt::kKindSw, p, 0, static_cast<int>(words.size())};
      std::vector<uint32_t> out(2 * words.size() + 8, 0);
      int32_t nw = 0;
      const int s = dv::alt::finish_pair(pr, reinterpret_cast<const uint8_t*>(bytes.data()), words.data(), normalize, out.data(), &nw);
      bool same = s == (want.empty() ? 0 : 1) && nw == static_cast<int>(want.size());
      for (int x = 0; x < nw && same; ++x) same = out[x] == ((static_cast<uint32_t>(want[x].length) << 4) | want[x].op);
      ++st[want.empty() ? 0 : 1];
      if (!same && ++bad < 10) {
        dv::Cigar got;
        for (int x = 0; x < nw; ++x) got.push_back({static_cast<int>(out[x] & 15), static_cast<int>(out[x] >> 4)});
        std::printf("case %d norm %d: r2h %s p %d n %d L %d: want %s got %d %s\n", it, normalize, dv::cigar_text(runs).c_str(), p, n, L, dv::cigar_text(want).c_str(), s, dv::cigar_text(got).c_str());
      }
    }
  }
  std::printf("synthetic: bad %lld status %lld/%lld not-normalised %lld\n", bad, st[0], st[1], unnorm);
  return bad != 0;
}

int main(int argc, char** argv) {
  const int n_seeds = argc > 1 ? std::atoi(argv[1]) : 200;
  if (argc > 2) return synthetic(n_seeds);
  long long pairs = 0, bad = 0, st[3] = {0, 0, 0}, id_pairs = 0;
  for (int seed = 0; seed < n_seeds; ++seed) {
    std::mt19937 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); };
    const int n = rnd(60, 260);
    const bool low_complexity = seed % 3 == 0;
    std::string target(n, 'A');
    for (char& c : target) c = low_complexity ? "AC"[rng() % 2] : "ACGT"[rng() % 4];
    if (seed % 5 == 0) for (int i = 20; i < 40 && i < n; ++i) target[i] = 'A';
    if (seed % 7 == 1) for (int i = 0; i < n; ++i) if (rng() % 6 == 0) target[i] = 'N';
    if (seed % 7 == 2) for (int i = 0; i + 8 < n; i += 16) for (int j = 0; j < 8; ++j) target[i + j] = "ACGT"[(i / 16) % 4];
    if (seed % 7 == 3) for (int i = 0; i < n; ++i) if (rng() % 4 == 0) target[i] = static_cast<char>(std::tolower(target[i]));
    std::vector<std::string> reads;
    for (int r = 0; r < 24; ++r) {
      int L = rnd(8, 230);
      int s = rnd(-20, n - 1);
      std::string read;
      for (int i = 0; i < L; ++i) {
        const int t = s + i;
        read += t >= 0 && t < n ? target[t] : "ACGT"[rng() % 4];
      }
      const int kind = rnd(0, 7);
      if (kind == 1) for (int m = rnd(1, 4); m > 0; --m) read[rng() % read.size()] = "ACGT"[rng() % 4];
      if (kind == 2 || kind == 6) read.insert(rng() % read.size(), std::string(rnd(1, 6), "ACGT"[rng() % 4]));
      if (kind == 3 || kind == 6) { size_t at = rng() % read.size(); read.erase(at, rnd(1, 6)); }
      if (kind == 4) { size_t at = rng() % read.size(); const int k = rnd(1, 5); read.erase(at, k); if (at < read.size()) read.insert(at, std::string(rnd(1, 5), "ACGT"[rng() % 4])); }
      if (kind == 5) read = std::string(rnd(8, 60), "ACGT"[rng() % 4]);
      if (kind == 7) { size_t at = rng() % read.size(); read.insert(at, read.substr(at, rnd(1, 4))); }
      if (read.empty()) read = "A";
      reads.push_back(read);
    }
    for (int normalize = 0; normalize < 2; ++normalize) {
      dv::FastPassAligner a;
      dv::AlignerOptions o;
      o.match = 4; o.mismatch = 6; o.gap_open = 8; o.gap_extend = seed % 2 ? 2 : 1; o.kmer_size = seed % 4 == 0 ? 8 : 32;
      o.max_num_of_mismatches = 2; o.similarity_threshold = 0.16934; o.force_alignment = true; o.read_size = 200;
      std::string error;
      a.set_options(o, &error);
      a.set_normalize_reads(normalize);
      a.set_reference(target);
      a.set_ref_start(1000);
      a.set_haplotypes({target});
      a.begin_alignments(reads);
      dv::FastPassResults fast;
      dv::fast_pass_on_host({dv::fast_pass_window_of(a)}, dv::fast_pass_scoring_of(a), &fast);
      a.install_fast_pass(fast.haplotype_score.data(), fast.haplotype_discarded.data(), fast.read_position.data(), fast.read_score.data());
      dv::AlignmentPairs ap;
      a.collect_alignments(reads.size(), &ap);
      std::vector<dv::LocalAlignment> results;
      std::vector<char> ok;
      a.align_pairs_on_host(ap, 0, ap.pair_ref.size(), &results, &ok);
      const std::vector<dv::RealignedRead> want = a.finish_alignments(ap, results.data(), ok.data());
      const dv::HaplotypeAlignment& ha = a.haplotype_alignments()[0];
      // the byte table: upper-cased reads, then the target
      std::string bytes;
      std::vector<int> off;
      for (const std::string& r : a.reads()) { off.push_back(bytes.size()); bytes += r; }
      const int t_off = bytes.size();
      bytes += target;
      for (size_t r = 0; r < reads.size(); ++r) {
        const dv::ReadAlignment& ra = ha.reads[r];
        dv::alt::PairIn pr{t_off, n, off[r], static_cast<int>(reads[r].size()), dv::alt::kKindNone, 0, 0, 0};
        std::vector<uint32_t> runs;
        if (ra.score > 0) {
          const bool placed = fast.haplotype_score[0] != 0 && fast.read_position[r] >= 0 && fast.read_score[r] > 0;
          pr.p = ra.position;
          if (placed) {
            pr.kind = dv::alt::kKindFast;
          } else {
            pr.kind = dv::alt::kKindSw;
            for (const dv::CigarOp& op : dv::parse_cigar(ra.cigar)) runs.push_back((static_cast<uint32_t>(op.length) << 4) | op.op);
            pr.n_runs = runs.size();
            for (size_t x = 0; x + 1 < runs.size(); ++x) {
              const int o1 = runs[x] & 15, o2 = runs[x + 1] & 15;
              if ((o1 == 2 && o2 == 3) || (o1 == 3 && o2 == 2)) ++id_pairs;
            }
          }
        }
        std::vector<uint32_t> out(2 * runs.size() + 8, 0);
        int32_t nw = 0, nw2 = 0;
        const int s1 = dv::alt::finish_pair(pr, reinterpret_cast<const uint8_t*>(bytes.data()), runs.data(), normalize, nullptr, &nw);
        const int s2 = dv::alt::finish_pair(pr, reinterpret_cast<const uint8_t*>(bytes.data()), runs.data(), normalize, out.data(), &nw2);
        ++pairs;
        ++st[want[r].status];
        bool same = s1 == want[r].status && s2 == s1 && nw == nw2 && nw == (s1 == 1 ? static_cast<int>(want[r].cigar.size()) : 0);
        if (same && s1 == 1) {
          same = want[r].position == 1000 + pr.p;
          for (int x = 0; x < nw && same; ++x) same = out[x] == ((static_cast<uint32_t>(want[r].cigar[x].length) << 4) | want[r].cigar[x].op);
        }
        if (!same) {
          if (++bad < 10) std::printf("seed %d read %zu norm %d: want %d (%s) got %d nw %d; r2h %s at %d; L %zu n %d\n", seed, r, normalize, want[r].status, dv::cigar_text(want[r].cigar).c_str(), s1, nw, ra.cigar.c_str(), ra.position, reads[r].size(), n);
        }
      }
    }
  }
  std::printf("pairs %lld bad %lld status %lld/%lld/%lld I-beside-D %lld\n", pairs, bad, st[0], st[1], st[2], id_pairs);
  return bad != 0;
}
