// DeBruijnGraph::build up to, but not including, pruning (debruijn_graph.h) for every window of a batch in one
// kernel launch: the choice of k, the cycle test and the graph of the winning k as a CompactGraph.  Contract, kernel
// and runtime: debruijn.hip; the C entry points are there too.
#ifndef DV_DEBRUIJN_DEVICE_H_
#define DV_DEBRUIJN_DEVICE_H_

#include <cstdint>
#include <string_view>
#include <vector>

#include "debruijn_graph.h"
#include "dvhip.h"

namespace dv {

constexpr int kDebruijnMaxVertices = DV_DEBRUIJN_DEVICE_MAX_VERTICES;
constexpr int kDebruijnMaxEdges = DV_DEBRUIJN_DEVICE_MAX_EDGES;
constexpr int kDebruijnMaxBases = DV_DEBRUIJN_DEVICE_MAX_BASES;

struct AssemblyWindow {
  std::string_view ref;
  std::vector<AssemblyRead> reads;            // views into the caller's tables
};

struct AssemblyStats {                        // dv_debruijn_device_stats
  int64_t windows = 0, windows_on_host = 0, kmers = 0, k_tries = 0, launches = 0, windows_rejected = 0;
};
// of the calling thread's last device assembly; the C entry points reset it before they check anything
AssemblyStats& last_assembly_stats();

// DV_REALIGN_DEVICE_ASSEMBLY, read now; unset: off
bool device_assembly_enabled();

// DeBruijnGraph::build_compact, window by window.
void compact_on_host(const std::vector<AssemblyWindow>& windows, const DeBruijnOptions& options,
                     std::vector<CompactGraph>* out);
// One upload, one launch, one download on `stream` (null: a non-blocking stream the library owns), then waits.  A
// window over the kernel's limits, or whose tables overflow at run time, goes through build_compact inside the call.
// Buffers are the calling thread's and are reused.  Returns a dv_status; DV_ERR_NO_DEVICE without a GPU (only when
// there is device work).
int compact_on_device(const std::vector<AssemblyWindow>& windows, const DeBruijnOptions& options, void* stream,
                      std::vector<CompactGraph>* out, AssemblyStats* stats);

// ---- pruning and path enumeration too (debruijn_paths.h has the rule)
constexpr int kDebruijnMaxPaths = DV_DEBRUIJN_DEVICE_MAX_PATHS;
constexpr int kDebruijnMaxHapBytes = DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES;

struct WindowPaths {                          // one window of dv_debruijn_paths
  int k = 0;
  int status = DV_DEBRUIJN_PATHS_NO_GRAPH;
  bool on_host = false;                       // paths_on_device left it to the caller (compute_on_host false)
  std::vector<std::string> haplotypes;        // candidate_haplotypes(), status 0
};

struct PathsStats {                           // dv_debruijn_paths_stats
  int64_t windows = 0, windows_on_host = 0, paths = 0, hap_bytes = 0, launches = 0, bytes_down = 0;
};
// of the calling thread's last device paths call; the C entry points reset it before they check anything
PathsStats& last_paths_stats();

// DV_REALIGN_DEVICE_PATHS, read now; unset: off
bool device_paths_enabled();

// DeBruijnGraph::build and candidate_haplotypes for one window.
void paths_of_window(const AssemblyWindow& window, const DeBruijnOptions& options, WindowPaths* out);
// One upload, the graph launch and the paths launch behind it, one download of headers and haplotype slices on
// `stream`, then waits.  A window the graph kernel hands back, one whose haplotype text passes kDebruijnMaxHapBytes
// and every window of a call the kernel does not cover (disable_graph_pruning, max_num_paths > kDebruijnMaxPaths) go
// through paths_of_window inside the call -- or, with compute_on_host false, come back marked on_host for the
// caller's threads.  `assembly` (may be null) receives the graph kernel's counts.  Returns a dv_status;
// DV_ERR_NO_DEVICE without a GPU (only when there is device work).
int paths_on_device(const std::vector<AssemblyWindow>& windows, const DeBruijnOptions& options, void* stream,
                    bool compute_on_host, std::vector<WindowPaths>* out, PathsStats* stats, AssemblyStats* assembly);

}  // namespace dv

#endif  // DV_DEBRUIJN_DEVICE_H_
