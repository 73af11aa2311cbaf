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

}  // namespace dv

#endif  // DV_DEBRUIJN_DEVICE_H_
