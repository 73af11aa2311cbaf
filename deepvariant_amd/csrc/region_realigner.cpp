// dv_realign_regions (include/dvhip.h, "the window realigner over many regions"): the body of
// Realigner.realign_reads (deepvariant/realigner/realigner.py:795-855) for a batch of calling
// regions, with the (region, window) tasks spread over host threads.
//
//   phase 1, one task per candidate window: the reads that overlap the window, in row order,
//            go into a de Bruijn graph with the window's reference (call_debruijn_graph,
//            :703-738); a window survives when its haplotypes are not just the reference;
//   between: per region every read joins the surviving window it shares most bases with,
//            the first one on ties (assign_reads_to_assembled_regions, :596-619);
//   phase 2, one task per surviving window with reads: FastPassAligner::AlignReads against
//            the haplotypes padded with the reference out to the reads' span + margin
//            (call_fast_pass_aligner, :740-793).
//
// dv_realign_regions_device is the same call with the local alignments of phase 2 on the device
// (local_align.hip): phase 2 becomes
//   2a, one task per window: the aligner is set up and runs up to its local alignments
//       (FastPassAligner::prepare_alignments), leaving the pairs it needs; with DV_REALIGN_DEVICE_FASTPASS=1
//       in three steps: i, per window, set-up and reads (begin_alignments); ii, once, the fast pass of every
//       (window, haplotype) of the batch in one kernel launch (fast_pass.hip); iii, per window, its results
//       installed (install_fast_pass) and the pairs collected (collect_alignments);
//   2b, once: the pairs of all windows go through one kernel launch; the CIGARs of the pairs that
//       aligned (LocalAligner::complete) are spread over the worker pool;
//   2c, one task per window: FastPassAligner::finish_alignments.
// With DV_REALIGN_DEVICE_FINISH=1 (honoured only with DV_REALIGN_DEVICE_TRACEBACK=1) 2b's launch leaves its result on the
// device and downloads the corners, traced flag, run count and band of each pair; its worker-pool loop makes text
// (LocalAligner::complete) only for the windows the device hands back -- a pair outside the sweep kernel's limits, or
// an alignment the kernel did not trace back --, and 2c becomes one call of realign_finish.hip's kernels for all
// other windows plus finish_alignments for those.
// With DV_REALIGN_DEVICE_ASSEMBLY=1 the device route's phase 1 becomes 1a, the batch's window list; 1b, once, the
// graph of every window in one kernel launch (debruijn.hip), choice of k and cycle test included; 1c, one task per
// window: DeBruijnGraph::from_compact (which prunes), candidate_haplotypes and the comparison with the reference.
// With DV_REALIGN_DEVICE_PATHS=1 on top of that, 1b also prunes and enumerates on the device (its paths kernel) and 1c
// is the comparison alone; a window the device hands back is built by its task as the host route builds it.
// The read assignment and the result arrays are the same code for both routes.
//
// Tasks are independent (each builds its own graph / aligner; the aligner's scratch buffers are
// thread_local), so a phase is a parallel loop over a task list ordered longest first.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "debruijn_device.h"
#include "debruijn_graph.h"
#include "dv_internal.h"
#include "fast_pass_aligner.h"
#include "fast_pass_device.h"
#include "local_align_device.h"
#include "realign_finish_device.h"

struct dv_realign_result {
  std::vector<int64_t> region_row_off;
  std::vector<int32_t> order, status;
  std::vector<int64_t> position, cigar_off;
  std::vector<uint32_t> cigar;
  std::vector<int32_t> region_assembled_off, assembled_window, assembled_hap_off;
  std::vector<int64_t> hap_text_off;
  std::string hap_text;
};

namespace {

struct Window {            // one candidate window of one region
  int region = 0, index = 0;
  std::vector<std::string> haplotypes;   // empty: dropped
  std::vector<int32_t> rows;             // the reads it claimed, ascending
  std::vector<dv::RealignedRead> aligned;   // parallel to rows; empty: alignments kept
  // device route, between 2a and 2c
  std::unique_ptr<dv::FastPassAligner> aligner;
  dv::AlignmentPairs pairs;
  size_t first_pair = 0;                    // of this window in the batch's pair list
};

struct DeviceRoute {       // dv_realign_regions_device's extra arguments
  void* stream;
  dv_realign_device_stats* stats;
};

// The worker threads live as long as the library: no thread creation per call, and the aligner's
// thread_local scratch tables (MBs for a heavy window) stay allocated from one call to the next.
// One job at a time; the calling thread works too.
class WorkerPool {
 public:
  static WorkerPool& get() {
    static WorkerPool* pool = new WorkerPool();      // never destroyed: workers may outlive main()'s statics
    return *pool;
  }

  void run(const std::vector<int>& tasks, int n_threads, const std::function<void(int)>& fn) {
    const int n = static_cast<int>(tasks.size());
    if (n_threads <= 1 || n <= 1) {
      for (int t : tasks) fn(t);
      return;
    }
    std::lock_guard<std::mutex> one_job(job_lock_);
    const int helpers = std::min(n_threads, n) - 1;
    {
      std::lock_guard<std::mutex> hold(lock_);
      if (pid_ != getpid()) {
        // after fork() the helper threads do not exist in the child: forget them (their std::thread objects are
        // leaked on purpose -- destroying a joinable one terminates) and start over with this process's own
        pid_ = getpid();
        (void)new std::vector<std::thread>(std::move(threads_));
        threads_.clear();
        wanted_ = busy_ = 0;
      }
      error_.clear();
      while (static_cast<int>(threads_.size()) < helpers) threads_.emplace_back([this] { worker(); });
      tasks_ = &tasks;
      fn_ = &fn;
      next_.store(0, std::memory_order_relaxed);
      wanted_ = helpers;
      busy_ = helpers;
      ++generation_;
    }
    wake_.notify_all();
    drain();
    std::unique_lock<std::mutex> hold(lock_);
    done_.wait(hold, [this] { return busy_ == 0; });
    tasks_ = nullptr;
    fn_ = nullptr;
    if (!error_.empty()) throw std::runtime_error(error_);   // on the CALLING thread, after every helper has let go
  }

 private:
  void drain() {
    const int n = static_cast<int>(tasks_->size());
    for (;;) {
      const int i = next_.fetch_add(1, std::memory_order_relaxed);
      if (i >= n) return;
      // an exception (std::bad_alloc, length_error ...) must neither leave a helper thread (std::terminate) nor
      // unwind the caller while helpers still hold tasks_ / fn_: the first one is kept, the rest of the job is
      // skipped, run() rethrows it once everybody is done
      try {
        (*fn_)((*tasks_)[i]);
      } catch (const std::exception& e) {
        fail_job(e.what());
      } catch (...) {
        fail_job("unknown exception in a realigner task");
      }
    }
  }

  void fail_job(const char* what) {
    std::lock_guard<std::mutex> hold(lock_);
    if (error_.empty()) error_ = what;
    next_.store(1 << 30, std::memory_order_relaxed);
  }

  void worker() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> hold(lock_);
        wake_.wait(hold, [&] { return generation_ != seen && wanted_ > 0; });
        seen = generation_;
        --wanted_;
      }
      drain();
      {
        std::lock_guard<std::mutex> hold(lock_);
        if (--busy_ == 0) done_.notify_one();
      }
    }
  }

  std::mutex job_lock_, lock_;
  std::condition_variable wake_, done_;
  std::vector<std::thread> threads_;
  const std::vector<int>* tasks_ = nullptr;
  const std::function<void(int)>* fn_ = nullptr;
  std::atomic<int> next_{0};
  int wanted_ = 0, busy_ = 0;
  uint64_t generation_ = 0;
  std::string error_;
  pid_t pid_ = getpid();
};

void parallel_tasks(const std::vector<int>& tasks, int n_threads, const std::function<void(int)>& fn) {
  WorkerPool::get().run(tasks, n_threads, fn);
}

std::vector<int> longest_first(const std::vector<int64_t>& cost) {
  std::vector<int> order(cost.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
  return order;
}

}  // namespace

extern "C" {

static int realign_regions_impl(const dv_realign_region* regions, int32_t n_regions, const dv_realign_options* o,
                                dv_realign_result** out, dv_realign_output* arrays, const DeviceRoute* device);

// The exception barrier of the entry point: nothing unwinds through extern "C" into ctypes.
int dv_realign_regions(const dv_realign_region* regions, int32_t n_regions, const dv_realign_options* o,
                       dv_realign_result** out, dv_realign_output* arrays) {
  try {
    return realign_regions_impl(regions, n_regions, o, out, arrays, nullptr);
  } catch (const std::bad_alloc&) {
    if (out) *out = nullptr;
    return dv::fail(DV_ERR_OUT_OF_MEMORY, "dv_realign_regions: out of host memory");
  } catch (const std::exception& e) {
    if (out) *out = nullptr;
    return dv::fail(DV_ERR_BAD_INPUT, std::string("dv_realign_regions: ") + e.what());
  }
}

int dv_realign_regions_device(const dv_realign_region* regions, int32_t n_regions, const dv_realign_options* o,
                              void* stream, dv_realign_result** out, dv_realign_output* arrays,
                              dv_realign_device_stats* stats) {
  try {
    if (stats) *stats = dv_realign_device_stats{0, 0, 0, 0};
    dv::last_traceback_stats() = dv::TracebackStats();
    dv::last_fast_pass_stats() = dv::FastPassStats();
    dv::last_assembly_stats() = dv::AssemblyStats();
    dv::last_paths_stats() = dv::PathsStats();
    dv::last_finish_stats() = dv::FinishStats();
    const DeviceRoute device{stream, stats};
    return realign_regions_impl(regions, n_regions, o, out, arrays, &device);
  } catch (const std::bad_alloc&) {
    if (out) *out = nullptr;
    return dv::fail(DV_ERR_OUT_OF_MEMORY, "dv_realign_regions_device: out of host memory");
  } catch (const std::exception& e) {
    if (out) *out = nullptr;
    return dv::fail(DV_ERR_BAD_INPUT, std::string("dv_realign_regions_device: ") + e.what());
  }
}

static int realign_regions_impl(const dv_realign_region* regions, int32_t n_regions, const dv_realign_options* o,
                                dv_realign_result** out, dv_realign_output* arrays, const DeviceRoute* device) {
  if (!out || !arrays || !o || n_regions < 0 || (n_regions > 0 && !regions)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_realign_regions: null argument");
  }
  *out = nullptr;
  if (o->dbg.step_k <= 0 || o->dbg.min_k <= 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_realign_regions: min_k and step_k must be positive");
  }
  if (o->ref_align_margin < 0) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_realign_regions: negative margin");
  std::vector<Window> windows;
  std::vector<int64_t> cost;
  for (int32_t g = 0; g < n_regions; ++g) {
    const dv_realign_region& r = regions[g];
    if (r.n_reads < 0 || r.n_windows < 0 || r.ref_len < 0 || r.ref_start < 0 || r.n_bases < 0 ||
        (r.n_reads > 0 && (!r.bases || !r.quals || !r.read_seq_off || !r.read_mapq || !r.read_start || !r.read_end)) ||
        (r.n_windows > 0 && (!r.window_start || !r.window_end || !r.ref))) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_realign_regions: null or negative field in a region");
    }
    for (int32_t i = 0; i < r.n_reads; ++i) {
      if (r.read_seq_off[i + 1] < r.read_seq_off[i] || r.read_seq_off[i + 1] > r.n_bases) {
        return dv::fail(DV_ERR_BAD_INPUT, "dv_realign_regions: a read's bases lie outside the table");
      }
    }
    for (int32_t w = 0; w < r.n_windows; ++w) {
      const int64_t a = r.window_start[w], b = r.window_end[w];
      if (a < 0 || a > b || a >= r.contig_len || b > r.contig_len) {
        return dv::fail(DV_ERR_BAD_INPUT, "dv_realign_regions: window outside the contig");
      }
      if (a < r.ref_start || b > r.ref_start + r.ref_len) {
        return dv::fail(DV_ERR_BAD_INPUT, "dv_realign_regions: window outside the reference bases handed over");
      }
      Window win;
      win.region = g;
      win.index = w;
      windows.push_back(std::move(win));
      cost.push_back((b - a) * static_cast<int64_t>(r.n_reads + 1));
    }
  }
  if (device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
      return dv::fail(DV_ERR_NO_DEVICE, "dv_realign_regions_device: no HIP device (dv_realign_regions is the host route)");
    }
  }
  int n_threads = o->n_threads;
  if (n_threads <= 0) n_threads = static_cast<int>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())));

  dv::DeBruijnOptions dbg;
  dbg.min_k = o->dbg.min_k;
  dbg.max_k = o->dbg.max_k;
  dbg.step_k = o->dbg.step_k;
  dbg.min_mapq = o->dbg.min_mapq;
  dbg.min_base_quality = o->dbg.min_base_quality;
  dbg.min_edge_weight = o->dbg.min_edge_weight;
  dbg.max_num_paths = o->dbg.max_num_paths;
  dbg.disable_graph_pruning = o->dbg.disable_graph_pruning != 0;

  // ---- phase 1: assembly
  // a window's reference and the reads that overlap it, in row order
  auto assembly_window = [&](const Window& win) {
    const dv_realign_region& r = regions[win.region];
    const int64_t a = r.window_start[win.index], b = r.window_end[win.index];
    dv::AssemblyWindow aw;
    aw.ref = std::string_view(r.ref + (a - r.ref_start), static_cast<size_t>(b - a));
    for (int32_t i = 0; i < r.n_reads; ++i) {
      if (r.read_end[i] > a && b > r.read_start[i]) {
        const uint32_t s0 = r.read_seq_off[i], s1 = r.read_seq_off[i + 1];
        aw.reads.push_back(dv::AssemblyRead{std::string_view(reinterpret_cast<const char*>(r.bases) + s0, s1 - s0),
                                            r.quals + s0, r.read_mapq[i]});
      }
    }
    return aw;
  };
  auto keep_haplotypes = [](Window& win, const dv::DeBruijnGraph* graph, std::string_view ref) {
    if (!graph) return;                                   // haplotypes == [ref]: dropped
    std::vector<std::string> haps = graph->candidate_haplotypes();
    if (haps.empty() || (haps.size() == 1 && haps[0] == ref)) return;
    win.haplotypes = std::move(haps);
  };
  if (!device || !dv::device_assembly_enabled()) {
    parallel_tasks(longest_first(cost), n_threads, [&](int t) {
      const dv::AssemblyWindow aw = assembly_window(windows[t]);
      keep_haplotypes(windows[t], dv::DeBruijnGraph::build(aw.ref, aw.reads, dbg).get(), aw.ref);
    });
  } else if (dv::device_paths_enabled()) {
    // 1a: the batch's window list
    const std::vector<int> by_cost = longest_first(cost);
    std::vector<dv::AssemblyWindow> assembly(windows.size());
    parallel_tasks(by_cost, n_threads, [&](int t) { assembly[t] = assembly_window(windows[t]); });
    // 1b: graphs, pruning and haplotypes of all windows of all regions in one device call
    std::vector<dv::WindowPaths> paths;
    if (int rc = dv::paths_on_device(assembly, dbg, device->stream, /*compute_on_host=*/false, &paths,
                                     &dv::last_paths_stats(), &dv::last_assembly_stats())) {
      return rc;
    }
    // 1c: the comparison with the reference; a window the device handed back is built here, as the host route does
    parallel_tasks(by_cost, n_threads, [&](int t) {
      const dv::AssemblyWindow& aw = assembly[t];
      if (paths[t].on_host) {
        keep_haplotypes(windows[t], dv::DeBruijnGraph::build(aw.ref, aw.reads, dbg).get(), aw.ref);
        return;
      }
      std::vector<std::string>& haps = paths[t].haplotypes;
      if (haps.empty() || (haps.size() == 1 && haps[0] == aw.ref)) return;
      windows[t].haplotypes = std::move(haps);
    });
  } else {
    // 1a: the batch's window list
    const std::vector<int> by_cost = longest_first(cost);
    std::vector<dv::AssemblyWindow> assembly(windows.size());
    parallel_tasks(by_cost, n_threads, [&](int t) { assembly[t] = assembly_window(windows[t]); });
    // 1b: the graphs of all windows of all regions in one device call
    std::vector<dv::CompactGraph> graphs;
    if (int rc = dv::compact_on_device(assembly, dbg, device->stream, &graphs, &dv::last_assembly_stats())) return rc;
    // 1c: pruning and the haplotypes from the compact graphs
    std::atomic<int64_t> rejected{0};
    parallel_tasks(by_cost, n_threads, [&](int t) {
      const dv::AssemblyWindow& aw = assembly[t];
      std::unique_ptr<dv::DeBruijnGraph> graph;
      std::string why;
      if (!dv::DeBruijnGraph::from_compact(aw.ref, aw.reads, dbg, graphs[t], &graph, &why)) {
        rejected.fetch_add(1, std::memory_order_relaxed);      // never expected: the host's own graph instead
        graph = dv::DeBruijnGraph::build(aw.ref, aw.reads, dbg);
      }
      keep_haplotypes(windows[t], graph.get(), aw.ref);
    });
    dv::last_assembly_stats().windows_rejected += rejected.load();
  }

  // ---- reads -> assembled windows (per region; windows of a region are consecutive in `windows`)
  auto res = std::make_unique<dv_realign_result>();
  res->region_row_off.assign(1, 0);
  for (int32_t g = 0; g < n_regions; ++g) res->region_row_off.push_back(res->region_row_off.back() + regions[g].n_reads);
  const int64_t total_rows = res->region_row_off.back();
  std::vector<int32_t> row_window(static_cast<size_t>(total_rows), -1);   // index into `windows`
  {
    size_t w0 = 0;
    for (int32_t g = 0; g < n_regions; ++g) {
      const dv_realign_region& r = regions[g];
      const size_t w1 = w0 + static_cast<size_t>(r.n_windows);
      std::vector<size_t> alive;
      for (size_t w = w0; w < w1; ++w) {
        if (!windows[w].haplotypes.empty()) alive.push_back(w);
      }
      if (!alive.empty()) {
        const int64_t base = res->region_row_off[g];
        for (int32_t i = 0; i < r.n_reads; ++i) {
          int64_t best = 0;
          size_t best_w = 0;
          for (size_t w : alive) {
            const int64_t shared = std::min(r.read_end[i], r.window_end[windows[w].index]) -
                                   std::max(r.read_start[i], r.window_start[windows[w].index]);
            if (shared > best) {       // strictly more: the first window wins ties
              best = shared;
              best_w = w;
            }
          }
          if (best > 0) {
            row_window[base + i] = static_cast<int32_t>(best_w);
            windows[best_w].rows.push_back(i);
          }
        }
      }
      w0 = w1;
    }
  }

  // ---- phase 2: alignment
  std::vector<int> align_tasks;
  std::vector<int64_t> align_cost;
  for (size_t w = 0; w < windows.size(); ++w) {
    if (windows[w].rows.empty()) continue;
    align_tasks.push_back(static_cast<int>(w));
    int64_t hap_bases = 0;
    for (const std::string& h : windows[w].haplotypes) hap_bases += static_cast<int64_t>(h.size()) + 300;
    align_cost.push_back(hap_bases * static_cast<int64_t>(windows[w].haplotypes.size() + windows[w].rows.size()));
  }
  {
    std::vector<int> by_cost = longest_first(align_cost);
    for (int& t : by_cost) t = align_tasks[t];
    align_tasks = std::move(by_cost);
  }
  std::mutex error_lock;
  std::string error;
  // a window's aligner, set up, and its reads' bases; false: the original alignments stay (or `error` is set)
  auto set_up = [&](int t, dv::FastPassAligner& aligner, std::vector<std::string>& sequences) -> bool {
    Window& win = windows[t];
    const dv_realign_region& r = regions[win.region];
    const int64_t a = r.window_start[win.index], b = r.window_end[win.index];
    int64_t lo = r.read_start[win.rows[0]], hi = r.read_end[win.rows[0]];
    for (int32_t i : win.rows) {
      lo = std::min(lo, r.read_start[i]);
      hi = std::max(hi, r.read_end[i]);
    }
    const int64_t ref_start = std::max<int64_t>(0, std::min(lo, a) - o->ref_align_margin);
    const int64_t ref_end = std::min(r.contig_len, std::max(hi, b) + o->ref_align_margin);
    if (ref_end <= b) return false;      // no room for a suffix: the original alignments stay
    if (ref_start < r.ref_start || ref_end > r.ref_start + r.ref_len) {
      std::lock_guard<std::mutex> hold(error_lock);
      error = "dv_realign_regions: reads of a window reach outside the reference bases handed over";
      return false;
    }
    const std::string prefix(r.ref + (ref_start - r.ref_start), static_cast<size_t>(a - ref_start));
    const std::string window_ref(r.ref + (a - r.ref_start), static_cast<size_t>(b - a));
    const std::string suffix(r.ref + (b - r.ref_start), static_cast<size_t>(ref_end - b));
    std::vector<std::string> haplotypes;
    haplotypes.reserve(win.haplotypes.size());
    for (const std::string& h : win.haplotypes) {
      haplotypes.push_back(prefix + h + suffix);
      if (haplotypes.back().size() >= 0xffff) {
        std::lock_guard<std::mutex> hold(error_lock);
        error = "haplotypes are limited to 65534 bases (16-bit read offsets)";
        return false;
      }
    }
    sequences.clear();
    sequences.reserve(win.rows.size());
    for (int32_t i : win.rows) {
      sequences.emplace_back(reinterpret_cast<const char*>(r.bases) + r.read_seq_off[i],
                             r.read_seq_off[i + 1] - r.read_seq_off[i]);
    }
    dv::AlignerOptions ao;
    ao.match = o->aln.match;
    ao.mismatch = o->aln.mismatch;
    ao.gap_open = o->aln.gap_open;
    ao.gap_extend = o->aln.gap_extend;
    ao.kmer_size = o->aln.kmer_size;
    ao.read_size = static_cast<int>(sequences[0].size());
    ao.max_num_of_mismatches = o->aln.max_num_of_mismatches;
    ao.similarity_threshold = o->aln.realignment_similarity_threshold;
    ao.force_alignment = false;
    std::string why;
    if (!aligner.set_options(ao, &why)) {
      std::lock_guard<std::mutex> hold(error_lock);
      error = why;
      return false;
    }
    aligner.set_normalize_reads(o->aln.normalize_reads != 0);
    aligner.set_ref_prefix_len(static_cast<int>(prefix.size()));
    aligner.set_ref_suffix_len(static_cast<int>(suffix.size()));
    aligner.set_reference(prefix + window_ref + suffix);
    aligner.set_ref_start(static_cast<uint64_t>(ref_start));
    aligner.set_haplotypes(haplotypes);
    return true;
  };
  if (!device) {
    parallel_tasks(align_tasks, n_threads, [&](int t) {
      dv::FastPassAligner aligner;
      std::vector<std::string> sequences;
      if (set_up(t, aligner, sequences)) windows[t].aligned = aligner.align_reads(sequences);
    });
  } else {
    // ---- 2a: everything up to the local alignments
    if (!dv::device_fast_pass_enabled()) {
      parallel_tasks(align_tasks, n_threads, [&](int t) {
        auto aligner = std::make_unique<dv::FastPassAligner>();
        std::vector<std::string> sequences;
        if (!set_up(t, *aligner, sequences)) return;
        aligner->prepare_alignments(sequences, &windows[t].pairs);
        windows[t].aligner = std::move(aligner);
      });
      if (!error.empty()) return dv::fail(DV_ERR_BAD_INPUT, error);
    } else {
      // 2a-i: set-up and reads
      parallel_tasks(align_tasks, n_threads, [&](int t) {
        auto aligner = std::make_unique<dv::FastPassAligner>();
        std::vector<std::string> sequences;
        if (!set_up(t, *aligner, sequences)) return;
        aligner->begin_alignments(sequences);
        windows[t].aligner = std::move(aligner);
      });
      if (!error.empty()) return dv::fail(DV_ERR_BAD_INPUT, error);
      // 2a-ii: the fast pass of every (window, haplotype) in one device call
      std::vector<dv::FastPassWindow> fast_windows;
      std::vector<size_t> first_haplotype(windows.size(), 0);
      size_t n_haplotypes = 0;
      const dv::FastPassAligner* any = nullptr;      // the options are the same for every window: they come from `o`
      for (int t : align_tasks) {
        if (!windows[t].aligner) continue;
        any = windows[t].aligner.get();
        fast_windows.push_back(dv::fast_pass_window_of(*any));
        first_haplotype[t] = n_haplotypes;
        n_haplotypes += any->haplotypes().size();
      }
      dv::FastPassResults fast;
      if (any) {
        if (int rc = dv::fast_pass_on_device(fast_windows, dv::fast_pass_scoring_of(*any), device->stream, &fast,
                                             &dv::last_fast_pass_stats())) {
          return rc;
        }
      }
      // 2a-iii: its results installed, then the pairs collected
      parallel_tasks(align_tasks, n_threads, [&](int t) {
        Window& win = windows[t];
        if (!win.aligner) return;
        const size_t h = first_haplotype[t];
        const size_t row = static_cast<size_t>(fast.first_row[h]);
        win.aligner->install_fast_pass(fast.haplotype_score.data() + h, fast.haplotype_discarded.data() + h,
                                       fast.read_position.data() + row, fast.read_score.data() + row);
        win.aligner->collect_alignments(win.aligner->reads().size(), &win.pairs);
      });
    }
    // ---- 2b: the pairs of all windows in one device call
    std::vector<const dv::CodedSequence*> sequences;
    std::vector<int32_t> pair_ref, pair_query;
    const dv::LocalAligner* scoring = nullptr;     // the same for every window: it comes from `o`
    for (int t : align_tasks) {
      Window& win = windows[t];
      if (!win.aligner) continue;
      scoring = &win.aligner->local_aligner();
      const int32_t base = static_cast<int32_t>(sequences.size());
      for (const dv::CodedSequence& s : win.pairs.sequences) sequences.push_back(&s);
      win.first_pair = pair_ref.size();
      for (size_t k = 0; k < win.pairs.pair_ref.size(); ++k) {
        pair_ref.push_back(base + win.pairs.pair_ref[k]);
        pair_query.push_back(base + win.pairs.pair_query[k]);
      }
    }
    std::vector<dv::LocalAlignment> results(pair_ref.size());
    std::vector<char> ok(pair_ref.size(), 0);
    const bool finish_on_device = dv::device_finish_enabled() && dv::device_traceback_enabled();
    dv::ResidentSweep resident;
    std::vector<char> window_on_device(windows.size(), 0);   // finish_on_device: finished by the kernels
    if (!pair_ref.empty() || finish_on_device) {
      std::vector<dv::SweepCorners> corners;
      std::vector<uint8_t> route;
      dv::DeviceAlignStats stats;
      dv::DeviceRuns traced;
      if (!pair_ref.empty()) {
        if (int rc = dv::sweep_pairs_on_device(sequences, pair_ref, pair_query, scoring->match(), scoring->mismatch(),
                                               scoring->gap_open(), scoring->gap_extend(), device->stream, &corners,
                                               &route, &stats, &traced, finish_on_device ? &resident : nullptr)) {
          return rc;
        }
      }
      if (finish_on_device) {
        dv::FinishStats& fs = dv::last_finish_stats();
        fs.bytes_down += resident.bytes_down;
        for (int t : align_tasks) {
          const Window& win = windows[t];
          if (!win.aligner) continue;
          ++fs.windows;
          window_on_device[t] = dv::window_finishes_on_device(win.first_pair, win.pairs.pair_ref.size(), route, corners,
                                                              resident);
          if (!window_on_device[t]) ++fs.windows_on_host;
        }
      }
      if (device->stats) {
        device->stats->pairs = stats.pairs;
        device->stats->pairs_on_host = stats.pairs_on_host;
        device->stats->cells = stats.cells;
        device->stats->launches = stats.launches;
      }
      // the CIGARs' text form, the banded trace-back of the pairs the kernel did not trace, and the whole
      // alignment of a pair outside the kernel's limits, on the worker pool
      constexpr size_t kPairsPerTask = 16;
      std::vector<int> chunks((pair_ref.size() + kPairsPerTask - 1) / kPairsPerTask);
      for (size_t c = 0; c < chunks.size(); ++c) chunks[c] = static_cast<int>(c);
      // finish_on_device: only the pairs of the windows handed back need it
      std::vector<char> pair_skipped;
      if (finish_on_device) {
        pair_skipped.assign(pair_ref.size(), 0);
        for (int t : align_tasks) {
          if (!window_on_device[t]) continue;
          const Window& win = windows[t];
          std::fill(pair_skipped.begin() + static_cast<std::ptrdiff_t>(win.first_pair),
                    pair_skipped.begin() + static_cast<std::ptrdiff_t>(win.first_pair + win.pairs.pair_ref.size()), 1);
        }
      }
      parallel_tasks(chunks, n_threads, [&](int c) {
        const size_t end = std::min(pair_ref.size(), (static_cast<size_t>(c) + 1) * kPairsPerTask);
        for (size_t k = static_cast<size_t>(c) * kPairsPerTask; k < end; ++k) {
          if (finish_on_device && pair_skipped[k]) continue;
          const dv::CodedSequence& ref = *sequences[pair_ref[k]];
          const dv::CodedSequence& q = *sequences[pair_query[k]];
          if (route[k] == dv::kRouteDevice) {
            ok[k] = dv::complete_on_device_route(*scoring, ref, q, corners[k], &traced, k, &results[k]);
          } else if (route[k] == dv::kRouteHost) {
            std::vector<dv::LocalAlignment> one;
            std::vector<char> one_ok;
            scoring->align_pairs({&ref}, {&q}, &one, &one_ok);
            results[k] = std::move(one[0]);
            ok[k] = one_ok[0];
          }
        }
      });
    }
    // ---- 2c: the rest of align_reads, on the device for the windows inside its limits, per window for the others
    if (finish_on_device) {
      std::vector<dv::FinishWindow> on_device;
      const dv::FastPassAligner* any = nullptr;
      for (int t : align_tasks) {
        Window& win = windows[t];
        if (!win.aligner || !window_on_device[t]) continue;
        any = win.aligner.get();
        on_device.push_back(dv::FinishWindow{any, &win.pairs, win.first_pair, &win.aligned});
      }
      if (any) {
        if (!resident.stream) resident.stream = device->stream;
        if (int rc = dv::finish_windows_on_device(on_device, resident, any->force_alignment(), any->normalize_reads(),
                                                  &dv::last_finish_stats())) {
          return rc;
        }
      }
    }
    parallel_tasks(align_tasks, n_threads, [&](int t) {
      Window& win = windows[t];
      if (!win.aligner) return;
      if (window_on_device[t]) {
        win.aligner.reset();
        win.pairs = dv::AlignmentPairs();
        return;
      }
      win.aligned = win.aligner->finish_alignments(win.pairs, results.data() + win.first_pair, ok.data() + win.first_pair);
      win.aligner.reset();
      win.pairs = dv::AlignmentPairs();
    });
  }
  if (!error.empty()) return dv::fail(DV_ERR_BAD_INPUT, error);

  // ---- results
  res->order.resize(static_cast<size_t>(total_rows));
  res->status.assign(static_cast<size_t>(total_rows), 0);
  res->position.assign(static_cast<size_t>(total_rows), 0);
  res->cigar_off.assign(static_cast<size_t>(total_rows) + 1, 0);
  res->region_assembled_off.assign(1, 0);
  res->assembled_hap_off.assign(1, 0);
  res->hap_text_off.assign(1, 0);
  std::vector<const dv::Cigar*> row_cigar(static_cast<size_t>(total_rows), nullptr);
  size_t w0 = 0;
  for (int32_t g = 0; g < n_regions; ++g) {
    const dv_realign_region& r = regions[g];
    const size_t w1 = w0 + static_cast<size_t>(r.n_windows);
    const int64_t base = res->region_row_off[g];
    int64_t at = base;
    for (int32_t i = 0; i < r.n_reads; ++i) {
      if (row_window[base + i] < 0) res->order[at++] = i;
    }
    for (size_t w = w0; w < w1; ++w) {
      const Window& win = windows[w];
      if (win.haplotypes.empty()) continue;
      res->assembled_window.push_back(win.index);
      for (const std::string& h : win.haplotypes) {
        res->hap_text += h;
        res->hap_text_off.push_back(static_cast<int64_t>(res->hap_text.size()));
      }
      res->assembled_hap_off.push_back(static_cast<int32_t>(res->hap_text_off.size() - 1));
      for (size_t k = 0; k < win.rows.size(); ++k) {
        const int32_t i = win.rows[k];
        res->order[at++] = i;
        if (!win.aligned.empty() && win.aligned[k].status == 1) {
          res->status[base + i] = 1;
          res->position[base + i] = win.aligned[k].position;
          row_cigar[base + i] = &win.aligned[k].cigar;
        }
      }
    }
    res->region_assembled_off.push_back(static_cast<int32_t>(res->assembled_window.size()));
    w0 = w1;
  }
  for (int64_t i = 0; i < total_rows; ++i) {
    if (row_cigar[i]) {
      for (const dv::CigarOp& op : *row_cigar[i]) {
        res->cigar.push_back((static_cast<uint32_t>(op.length) << 4) | static_cast<uint32_t>(op.op));
      }
    }
    res->cigar_off[i + 1] = static_cast<int64_t>(res->cigar.size());
  }
  arrays->region_row_off = res->region_row_off.data();
  arrays->order = res->order.data();
  arrays->status = res->status.data();
  arrays->position = res->position.data();
  arrays->cigar_off = res->cigar_off.data();
  arrays->cigar = res->cigar.data();
  arrays->region_assembled_off = res->region_assembled_off.data();
  arrays->assembled_window = res->assembled_window.data();
  arrays->assembled_hap_off = res->assembled_hap_off.data();
  arrays->hap_text_off = res->hap_text_off.data();
  arrays->hap_text = res->hap_text.data();
  *out = res.release();
  return DV_OK;
}

void dv_realign_result_free(dv_realign_result* r) { delete r; }

}  // extern "C"
