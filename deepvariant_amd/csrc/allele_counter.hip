// allele_counter.hip -- AlleleCounter::Add for a whole region's reads in one launch
// (the per-read, per-base integer work in front of the hot path).
//
// Replaces the read loop around AlleleCounter::Add (deepvariant/allelecounter.cc:873-979,
// called per read from make_examples_core.py's region processor) together with
// MakeIndelReadAllele (:402-469), GetPrevBase (:386-400), CanBasesBeUsed (:206-229) and
// AddReadAlleles (:471-543).  Input is the packed read table the encoder already uses
// (dv_batch's read fields); output is what AlleleCount holds per position:
//   * ref_supporting_read_count[interval length]          (atomic adds)
//   * one EVENT per non-reference read allele that landed in the interval
//     (position, read, type, low-quality flag, where its bases are) -- the host turns
//     events into read_alleles maps / allele sums; no string ever exists on the device.
// One wave per read: CIGAR operations are walked in order (wave-uniform), the bases of an
// alignment-match run are handled 64 at a time, indel quality / canonical-base checks are
// wave reductions.  The reference's "an indel supersedes the base it is anchored on" rule
// (AddReadAlleles: of two consecutive read alleles at the same position the first is
// dropped) is a one-entry pending slot per wave.
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <vector>

#include "allele_counter_plan.h"

// Large results live in pinned host memory (the count array of a 7.7 Mb interval is 31 MB: 1.3 ms
// over PCIe from pinned memory, 5 ms into pageable); small ones -- a 1 kb calling region's 4 KB of
// counts and a few hundred events, once or twice per region -- in ordinary memory: pinning and
// unpinning a buffer costs more than the whole call.
template <typename T>
struct PinnedArray {
  T* ptr = nullptr;
  size_t n = 0;
  bool pinned = false;
  int reserve(size_t count) {
    release();
    if (count == 0) return DV_OK;
    if (count * sizeof(T) < (1u << 20)) {
      ptr = static_cast<T*>(std::malloc(count * sizeof(T)));
      if (!ptr) return dv::fail(DV_ERR_OUT_OF_MEMORY, "malloc");
      pinned = false;
    } else {
      hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&ptr), count * sizeof(T), hipHostMallocDefault);
      if (e != hipSuccess) {
        ptr = nullptr;
        return dv::fail(DV_ERR_OUT_OF_MEMORY, std::string("hipHostMalloc: ") + hipGetErrorString(e));
      }
      pinned = true;
    }
    n = count;
    return DV_OK;
  }
  void release() {
    if (ptr) {
      if (pinned) {
        (void)hipHostFree(ptr);
      } else {
        std::free(ptr);
      }
    }
    ptr = nullptr;
    n = 0;
  }
  ~PinnedArray() { release(); }
};

struct dv_allele_counts {
  PinnedArray<int32_t> ref_count;
  PinnedArray<dv_allele_event> raw;      // as the kernel left them
  std::vector<dv_allele_event> events;   // sorted by (position, read, read_offset)
  std::vector<int32_t> empty_counts;
  int64_t length = 0;
  int32_t n_reads_counted = 0;
};

namespace {

enum : int { kRef = 1, kSub = 2, kIns = 3, kDel = 4, kSoft = 5 };   // AlleleType
enum : int { opM = 1, opI = 2, opD = 3, opN = 4, opS = 5, opH = 6, opP = 7, opEQ = 8, opX = 9 };

using dv::CountArgs;

__device__ __forceinline__ bool canonical(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }

struct Entry {
  bool have;
  int64_t abs_pos;           // absolute reference position of the allele
  int type, low;
  uint32_t read_offset, length;
};

// Reference matches are by far the most frequent outcome (one per aligned base) and pile up
// ~coverage-deep on neighbouring positions: a workgroup counts them in an LDS window that
// starts at its first read and flushes the non-zero counters once, so the device-scope
// atomics shrink by about the pile-up depth of the group's reads; positions outside the
// window (unsorted or very long reads) go straight to memory.
constexpr int kWindow = 4096;        // positions per workgroup window (16 KB of LDS)
constexpr int kReadsPerWave = 16;    // a workgroup of 4 waves takes 64 consecutive reads

constexpr int kBlockEvents = 1024;   // events staged per workgroup before they take global slots

struct BlockState {
  int window[kWindow];
  dv_allele_event events[kBlockEvents];
  int n_events, n_reads;
  uint32_t event_base;
};

__device__ __forceinline__ void emit(const CountArgs& a, uint32_t read, const Entry& e, BlockState* bs,
                                     int64_t window_start) {
  int* window = bs->window;
  const int64_t p = e.abs_pos - a.interval_start;
  if (p < 0 || p >= a.interval_len) return;            // IsValidIntervalOffset
  if (e.type == kRef) {
    if (!e.low) {
      const int64_t w = e.abs_pos - window_start;
      if (w >= 0 && w < kWindow) {
        atomicAdd(&window[w], 1);
      } else {
        atomicAdd(&a.ref_count[p], 1);
      }
    }
    // a REFERENCE read allele exists only where a candidate will be called (allelecounter.cc:504-512)
    if (!a.candidate_mask || !((a.candidate_mask[p >> 5] >> (p & 31)) & 1u)) return;
  }
  dv_allele_event ev;
  ev.position = static_cast<int32_t>(p);
  ev.read = read;
  ev.read_offset = e.read_offset;
  ev.length_type = (static_cast<uint32_t>(e.length) & 0x0fffffffu) | (static_cast<uint32_t>(e.type) << 28) |
                   (e.low ? 0x80000000u : 0u);
  // One counter for the whole launch serialises at ~20 ns per atomic (a quarter of a million
  // events = the whole kernel time): stage in LDS, take the global slots once per workgroup.
  const int local = atomicAdd(&bs->n_events, 1);
  if (local < kBlockEvents) {
    bs->events[local] = ev;
  } else {
    const uint32_t slot = atomicAdd(&a.counters[0], 1u);
    if (slot < a.event_cap) a.events[slot] = ev;
  }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// One base of an alignment-match run -> its read allele (or none).
__device__ __forceinline__ Entry base_entry(const CountArgs& a, uint32_t s0, int64_t abs_pos, uint32_t b) {
  Entry e{};
  if (abs_pos < a.reads_start || abs_pos >= a.reads_end) return e;        // IsValidRefOffset
  const uint8_t base = a.bases[s0 + b], q = a.quals[s0 + b];
  if (!canonical(base) || (a.legacy && q < a.min_bq)) return e;            // CanBasesBeUsed(len 1)
  e.have = true;
  e.abs_pos = abs_pos;
  e.type = a.ref[abs_pos - a.ref_start] == base ? kRef : kSub;
  e.low = (!a.legacy && q < a.min_bq) ? 1 : 0;
  e.read_offset = b;
  e.length = 1;
  return e;
}

__device__ __forceinline__ void count_read(const CountArgs& a, uint32_t r, int lane, BlockState* window,
                                           int64_t window_start) {
  if (a.mapq[r] < a.min_mapq) return;
  if (lane == 0) atomicAdd(&window->n_reads, 1);
  const uint32_t s0 = a.seq_off[r];
  uint32_t read_offset = 0;
  int64_t abs_pos = a.read_pos[r];
  Entry pending{};
  for (uint32_t c = a.cigar_off[r]; c < a.cigar_off[r + 1]; ++c) {
    const uint32_t word = a.cigar[c];
    const int op = word & 15;
    const uint32_t n = word >> 4;
    if (op == opM || op == opEQ || op == opX) {
      // nothing later can share the pending entry's position any more
      if (pending.have && lane == 0) emit(a, r, pending, window, window_start);
      pending.have = false;
      for (uint32_t i = lane; i + 1 < n; i += 64) {
        const Entry e = base_entry(a, s0, abs_pos + i, read_offset + i);
        if (e.have) emit(a, r, e, window, window_start);
      }
      if (n > 0) pending = base_entry(a, s0, abs_pos + n - 1, read_offset + n - 1);   // may be superseded
      read_offset += n;
      abs_pos += n;
    } else if (op == opI || op == opS || op == opD) {
      // MakeIndelReadAllele: anchored on the base before it.  An allele outside the interval is
      // dropped by AddReadAlleles whatever it is (and so is anything it could supersede), so
      // its validity -- which may need reference bases far from the interval -- is not computed.
      Entry e{};
      int prev = -1;
      const int64_t rel = abs_pos - 1 - a.interval_start;
      const bool wanted = rel >= 0 && rel < a.interval_len;
      if (!wanted) {
        // fall through with prev = -1: no entry
      } else if (read_offset == 0) {
        const int64_t pp = abs_pos - 1;                                  // RefBases(ref_offset - 1, 1)
        if (pp >= 0 && pp < a.contig_len) {
          if (pp >= a.ref_start && pp < a.ref_start + a.n_ref) {
            prev = a.ref[pp - a.ref_start];
          } else if (lane == 0) {
            atomicAdd(&a.counters[2], 1u);
          }
        }
      } else {
        prev = a.bases[s0 + read_offset - 1];
      }
      bool ok = prev >= 0 && canonical(static_cast<uint8_t>(prev));
      int low = 0;
      if (ok && op != opD) {                                             // CanBasesBeUsed over the run
        int qsum = 0, bad = 0;
        for (uint32_t i = lane; i < n; i += 64) {
          const uint8_t b = a.bases[s0 + read_offset + i], q = a.quals[s0 + read_offset + i];
          qsum += q;
          bad += (!canonical(b) || (a.legacy && q < a.min_bq)) ? 1 : 0;
        }
        qsum = wave_sum(qsum);
        bad = wave_sum(bad);
        ok = bad == 0;
        low = (!a.legacy && static_cast<int64_t>(qsum) < static_cast<int64_t>(a.min_bq) * n) ? 1 : 0;
      }
      if (ok && op == opD) {                                             // the deleted reference bases
        if (n == 0 || abs_pos < 0 || abs_pos + n > a.contig_len) {
          ok = false;
        } else if (abs_pos < a.ref_start || abs_pos + n > a.ref_start + a.n_ref) {
          ok = false;
          if (lane == 0) atomicAdd(&a.counters[2], 1u);
        } else {
          int bad = 0;
          for (uint32_t i = lane; i < n; i += 64) bad += canonical(a.ref[abs_pos - a.ref_start + i]) ? 0 : 1;
          ok = wave_sum(bad) == 0;
        }
      }
      if (ok) {
        e.have = true;
        e.abs_pos = abs_pos - 1;
        e.type = op == opD ? kDel : op == opI ? kIns : kSoft;
        e.low = low;
        e.read_offset = read_offset;
        e.length = n;
      }
      // AddReadAlleles: of two consecutive alleles at one position the first is dropped.  A
      // skipped allele (position -1 in the reference) never equals a real position.
      if (pending.have && !(e.have && e.abs_pos == pending.abs_pos) && lane == 0) emit(a, r, pending, window, window_start);
      pending = e;
      if (op == opD) {
        abs_pos += n;
      } else {
        read_offset += n;
      }
    } else if (op == opN || op == opP) {
      abs_pos += n;
    }
  }
  if (pending.have && lane == 0) emit(a, r, pending, window, window_start);
}

static_assert(4 * kReadsPerWave == dv::kCountReadsPerBlock, "the plan counts workgroups of 64 reads");

// What one workgroup does for the 64 reads of region `a` that start at read `first` (first < a.n_reads): both
// kernels' whole body.  `a` is the workgroup's own copy of the descriptor.
__device__ __forceinline__ void count_block(const CountArgs& a, uint32_t first, BlockState& bs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kWindow; i += 256) bs.window[i] = 0;
  if (threadIdx.x == 0) bs.n_events = bs.n_reads = 0;
  const int64_t window_start = a.read_pos[first];      // reads arrive position-sorted (BAM order)
  __syncthreads();
  for (int k = 0; k < kReadsPerWave; ++k) {
    const uint32_t r = first + k * 4 + wave;           // neighbouring reads side by side on the four waves
    if (r < static_cast<uint32_t>(a.n_reads)) count_read(a, r, lane, &bs, window_start);
  }
  __syncthreads();
  const int n_ev = bs.n_events < kBlockEvents ? bs.n_events : kBlockEvents;
  if (threadIdx.x == 0) {
    bs.event_base = n_ev ? atomicAdd(&a.counters[0], static_cast<uint32_t>(n_ev)) : 0u;
    if (bs.n_reads) atomicAdd(&a.counters[1], static_cast<uint32_t>(bs.n_reads));
  }
  for (int i = threadIdx.x; i < kWindow; i += 256) {
    const int v = bs.window[i];
    const int64_t p = window_start + i - a.interval_start;
    if (v != 0 && p >= 0 && p < a.interval_len) atomicAdd(&a.ref_count[p], v);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_ev; i += 256) {
    const uint32_t slot = bs.event_base + i;
    if (slot < a.event_cap) a.events[slot] = bs.events[i];
  }
}

// One region per launch: dv_count_alleles, the regions of a batch that go alone, and a batch without the switch.
__global__ __launch_bounds__(256) void count_alleles_kernel(CountArgs a) {
  __shared__ BlockState bs;
  count_block(a, blockIdx.x * (4 * kReadsPerWave), bs);
}

// Every batched region of a call in one grid (DV_COUNT_ONE_LAUNCH).  block_first[s] is the first workgroup of slot
// s, ascending, block_first[n_slots] the grid; a slot has ceil(n_reads / 64) >= 1 workgroups.  The workgroup finds
// its slot by upper-bound bisection -- the same loads and branches on every lane, so the search and the descriptor
// it leads to stay in scalar registers -- and copies the descriptor once: nothing below reads the table again.
__global__ __launch_bounds__(256) void count_alleles_batch_kernel(const CountArgs* regions, const uint32_t* block_first,
                                                                  int32_t n_slots) {
  __shared__ BlockState bs;
  const uint32_t block = blockIdx.x;
  int32_t lo = 0, hi = n_slots;                        // block_first[lo] <= block < block_first[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (block_first[mid] <= block) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  const CountArgs a = regions[lo];
  count_block(a, (block - block_first[lo]) * (4 * kReadsPerWave), bs);
}

template <typename T>
int to_device(dv::DeviceBuffer& buf, const T* src, size_t count, int memory, const T** out, hipStream_t stream) {
  if (memory != DV_MEM_HOST) {
    *out = src;
    return DV_OK;
  }
  if (int rc = buf.reserve_on_current_device(std::max<size_t>(count, 1) * sizeof(T))) return rc;
  DV_HIP_CHECK(hipMemcpyAsync(buf.ptr, src, count * sizeof(T), hipMemcpyHostToDevice, stream));
  *out = static_cast<const T*>(buf.ptr);
  return DV_OK;
}

// Order: (position, read, read_offset).  One read can leave two alleles at one position when
// a skipped allele sits between them (1I 4S 2D with an unusable soft clip: the insertion is
// not superseded, the deletion is added after it); read offsets order them as the CIGAR
// does, so the consumer's "later entry overwrites" matches read_alleles[key] = allele.
// Large lists: LSD radix sort on (position << 32 | read), 16 bits a pass, then the rare ties by offset.
void order_events(dv_allele_counts* res, size_t n_ev) {
  if (n_ev < (1u << 15)) {
    // a calling region's few hundred events: a comparison sort on (position, read, read_offset);
    // the radix passes below cost 65536-entry histograms each, more than the whole launch
    res->events.assign(res->raw.ptr, res->raw.ptr + n_ev);
    std::stable_sort(res->events.begin(), res->events.end(), [](const dv_allele_event& x, const dv_allele_event& y) {
      if (x.position != y.position) return static_cast<uint32_t>(x.position) < static_cast<uint32_t>(y.position);
      if (x.read != y.read) return x.read < y.read;
      return x.read_offset < y.read_offset;
    });
    res->raw.release();
  } else {
    std::vector<uint64_t> key(n_ev), key2(n_ev);
    std::vector<uint32_t> idx(n_ev), idx2(n_ev);
    uint64_t all = 0;
    for (size_t i = 0; i < n_ev; ++i) {
      key[i] = (static_cast<uint64_t>(static_cast<uint32_t>(res->raw.ptr[i].position)) << 32) | res->raw.ptr[i].read;
      idx[i] = static_cast<uint32_t>(i);
      all |= key[i];
    }
    std::vector<size_t> count(65537);
    for (int shift = 0; shift < 64; shift += 16) {
      if (((all >> shift) & 0xffffu) == 0) continue;      // these 16 bits are zero everywhere
      std::fill(count.begin(), count.end(), size_t{0});
      for (size_t i = 0; i < n_ev; ++i) ++count[((key[i] >> shift) & 0xffffu) + 1];
      for (int c = 0; c < 65536; ++c) count[c + 1] += count[c];
      for (size_t i = 0; i < n_ev; ++i) {
        const size_t d = count[(key[i] >> shift) & 0xffffu]++;
        key2[d] = key[i];
        idx2[d] = idx[i];
      }
      key.swap(key2);
      idx.swap(idx2);
    }
    res->events.resize(n_ev);
    for (size_t i = 0; i < n_ev; ++i) res->events[i] = res->raw.ptr[idx[i]];
    for (size_t i = 0; i + 1 < n_ev;) {
      size_t j = i + 1;
      while (j < n_ev && key[j] == key[i]) ++j;
      if (j - i > 1) {
        std::stable_sort(res->events.begin() + i, res->events.begin() + j,
                         [](const dv_allele_event& x, const dv_allele_event& y) { return x.read_offset < y.read_offset; });
      }
      i = j;
    }
    res->raw.release();
  }
}

// The same order with one word per raw event carried along (the candidate pass' event words, which the
// device writes in the kernel's event order).
void order_events_with_words(dv_allele_counts* res, size_t n_ev, const int32_t* raw_words, std::vector<int32_t>* words) {
  std::vector<uint32_t> idx(n_ev);
  for (size_t i = 0; i < n_ev; ++i) idx[i] = static_cast<uint32_t>(i);
  const dv_allele_event* raw = res->raw.ptr;
  std::stable_sort(idx.begin(), idx.end(), [raw](uint32_t i, uint32_t j) {
    const dv_allele_event &x = raw[i], &y = raw[j];
    if (x.position != y.position) return static_cast<uint32_t>(x.position) < static_cast<uint32_t>(y.position);
    if (x.read != y.read) return x.read < y.read;
    return x.read_offset < y.read_offset;
  });
  res->events.resize(n_ev);
  words->resize(n_ev);
  for (size_t i = 0; i < n_ev; ++i) {
    res->events[i] = raw[idx[i]];
    (*words)[i] = raw_words[idx[i]];
  }
  res->raw.release();
}

// Argument and read-table checks shared by the one-region and the batch entry point.
int check_request(const dv_batch* b, const dv_allele_counter_options* o, dv_allele_counts** out, const char* who) {
  const std::string name(who);
  if (!b || !o || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null");
  if (b->n_reads < 0 || o->interval_end < o->interval_start || !o->ref_bases || o->n_ref_bases <= 0 ||
      o->min_base_quality < 0 || o->min_mapping_quality < 0) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": bad argument");
  }
  if (b->n_reads && (!b->read_pos || !b->read_seq_off || !b->read_cigar_off || !b->read_mapq || !b->bases ||
                     !b->quals || !b->cigar)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": read table field missing");
  }
  if (b->memory == DV_MEM_HOST) {
    // the same read-table checks dv_validate_batch applies (a device-resident table is the
    // caller's to validate before the upload, as for dv_encode_batch)
    for (int32_t r = 0; r < b->n_reads; ++r) {
      if (b->read_cigar_off[r + 1] < b->read_cigar_off[r] || b->read_cigar_off[r + 1] > b->n_cigar ||
          b->read_seq_off[r + 1] < b->read_seq_off[r] || b->read_seq_off[r + 1] > b->n_bases) {
        return dv::fail(DV_ERR_INVALID_ARGUMENT, "read offsets are not prefix sums within the arrays");
      }
      uint64_t qlen = 0;
      for (uint32_t c = b->read_cigar_off[r]; c < b->read_cigar_off[r + 1]; ++c) {
        const uint32_t op = b->cigar[c] & 0xF;
        if (op < 1 || op > 9) return dv::fail(DV_ERR_BAD_INPUT, "Unrecognized CIGAR op");
        if (op == 1 || op == 2 || op == 5 || op == 8 || op == 9) qlen += b->cigar[c] >> 4;
      }
      if (qlen > b->read_seq_off[r + 1] - b->read_seq_off[r]) {
        return dv::fail(DV_ERR_BAD_INPUT, "CIGAR consumes more bases than aligned_sequence has");
      }
    }
  }
  if (o->ref_start > dv::reads_start(o) || o->ref_start + o->n_ref_bases < dv::reads_end(o)) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": the reference window must cover the reads interval");
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    return dv::fail(DV_ERR_NO_DEVICE, name + ": no HIP device (there is no CPU fallback)");
  }
  return DV_OK;
}

// ---- one of each piece the one-region entry, the batch entry and the passes behind them share

// Everything of CountArgs but the seven table pointers, `ref`, `candidate_mask` and the outputs.
CountArgs fill_count_args(const dv_batch* b, const dv_allele_counter_options* o, int64_t len) {
  CountArgs a{};
  a.n_reads = b->n_reads;
  a.ref_start = o->ref_start;
  a.n_ref = o->n_ref_bases;
  a.reads_start = dv::reads_start(o);
  a.reads_end = dv::reads_end(o);
  a.interval_start = o->interval_start;
  a.interval_len = len;
  a.contig_len = o->contig_n_bases > 0 ? o->contig_n_bases : o->ref_start + o->n_ref_bases;
  a.min_mapq = o->min_mapping_quality;
  a.min_bq = o->min_base_quality;
  a.legacy = o->keep_legacy_behavior ? 1 : 0;
  return a;
}

// track_ref_reads: one bit per position of the interval, set at the candidate positions; dv::mask_words(len) words.
void build_candidate_mask(const dv_allele_counter_options* o, int64_t len, uint32_t* words) {
  std::memset(words, 0, dv::mask_words(len) * sizeof(uint32_t));
  for (int32_t k = 0; k < o->n_candidate_positions; ++k) {
    const int64_t p = o->candidate_positions[k] - o->interval_start;
    if (p >= 0 && p < len) words[static_cast<size_t>(p >> 5)] |= 1u << (p & 31);
  }
}

void launch_count(const CountArgs& a, int32_t n_reads, hipStream_t stream) {
  dv::ProfileScope prof(dv::kProfOther, stream);
  hipLaunchKernelGGL(count_alleles_kernel, dim3((n_reads + 4 * kReadsPerWave - 1) / (4 * kReadsPerWave)), dim3(256), 0,
                     stream, a);
}

int window_too_small() {           // counters[2] of a launch is not zero
  return dv::fail(DV_ERR_BAD_INPUT, "dv_count_alleles: an indel reaches outside the reference window (pass more margin)");
}

// A region's counts where a pass behind the counter finds them on the device: what GvcfRegion and CandRegion share.
struct CountsOnDevice {
  const int32_t* ref_count;
  const dv_allele_event* events;
  const uint32_t* n_events;
  uint32_t event_cap;
  const int32_t* read_key;         // null: every read is its own key
  const uint8_t* ref;              // of the interval
  int64_t interval_start, len;
};

dv::GvcfRegion gvcf_region(const CountsOnDevice& c, const dv_gvcf_options* gv, int32_t* scratch, dv_gvcf_block* blocks,
                           int32_t* n_blocks) {
  return dv::GvcfRegion{c.ref_count, c.events, c.n_events, c.event_cap, c.read_key, c.ref, c.interval_start,
                        static_cast<int32_t>(c.len), gv->left_padding, static_cast<int32_t>(c.len - gv->right_padding),
                        scratch, blocks, n_blocks};      // in the order of gvcf.h
}

// bases, seq_off: the read table's, which the events point into
dv::CandRegion cand_region(const CountsOnDevice& c, const uint8_t* bases, const uint32_t* seq_off, int32_t* scratch,
                           dv_candidate_site* sites, dv_candidate_allele* alleles, int32_t* words, int32_t* n_out) {
  return dv::CandRegion{c.ref_count, c.events, c.n_events, c.event_cap, c.read_key, c.ref, bases, seq_off,
                        static_cast<int32_t>(c.len), scratch, sites, alleles, words, n_out};   // in the order of candidates.h
}

template <class T>
T* at(void* base, size_t bytes) { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + bytes); }

// ---- a pass over counts that are already on the host (a region that took the one-region path: a device-resident
// read table, no reads, or events beyond the batch's first guess): the counts and sorted events go back up and
// through the same kernels.  The rare path.  One device image per pass:
//   descriptor | n_events and the pass' record counts | ref_count | events | ref | keys   -- the same for both passes
//   | what else the pass uploads | scratch | the pass' records
struct CountsImage {
  dv::Layout lay;
  size_t desc = 0, words = 0, counts = 0, events = 0, ref = 0, keys = 0;
  int64_t len = 0;
  uint32_t n_ev = 0;
  size_t n_keys = 0;
};

CountsImage lay_counts_image(size_t descriptor_bytes, const dv_allele_counts* c, const dv_batch* b, const int32_t* keys) {
  CountsImage im;
  im.len = c->length;
  im.n_ev = static_cast<uint32_t>(c->events.size());
  im.n_keys = keys ? static_cast<size_t>(b->n_reads) : 0;
  im.desc = im.lay.add(descriptor_bytes);
  im.words = im.lay.add(16);
  im.counts = im.lay.add(static_cast<size_t>(im.len) * sizeof(int32_t));
  im.events = im.lay.add(static_cast<size_t>(im.n_ev) * sizeof(dv_allele_event));
  im.ref = im.lay.add(static_cast<size_t>(im.len));
  im.keys = im.lay.add(im.n_keys * sizeof(int32_t));
  return im;
}

// One thread's buffers for one such pass: the upload is staged in pinned memory, so the asynchronous copy reads
// nothing of the caller's; the stage is free again when the pass returns, because it ends on a synchronisation.
struct CountsBuffers {
  dv::PinnedStage stage;
  dv::DeviceBuffer d_img;
};

// Fills the shared sections of the staged image -> where the pass finds them on the device.
CountsOnDevice stage_counts(const CountsImage& im, const dv_allele_counts* c, const dv_allele_counter_options* o,
                            const int32_t* keys, uint8_t* host, uint8_t* dev) {
  std::memset(host + im.words, 0, 16);
  std::memcpy(host + im.words, &im.n_ev, 4);
  const int32_t* cnt = c->ref_count.ptr ? c->ref_count.ptr : c->empty_counts.data();
  if (im.len) std::memcpy(host + im.counts, cnt, static_cast<size_t>(im.len) * sizeof(int32_t));
  if (im.n_ev) std::memcpy(host + im.events, c->events.data(), static_cast<size_t>(im.n_ev) * sizeof(dv_allele_event));
  std::memcpy(host + im.ref, o->ref_bases + (o->interval_start - o->ref_start), static_cast<size_t>(im.len));
  if (im.n_keys) std::memcpy(host + im.keys, keys, im.n_keys * sizeof(int32_t));
  return CountsOnDevice{at<const int32_t>(dev, im.counts), at<const dv_allele_event>(dev, im.events),
                        at<const uint32_t>(dev, im.words), im.n_ev, keys ? at<const int32_t>(dev, im.keys) : nullptr,
                        dev + im.ref, o->interval_start, im.len};
}

// The image's first up_bytes go up and its scratch section is zeroed; no synchronisation.
int upload_counts_image(const CountsBuffers& buf, size_t up_bytes, size_t scratch_at, size_t scratch_bytes,
                        hipStream_t stream) {
  DV_HIP_CHECK(hipMemcpyAsync(buf.d_img.ptr, buf.stage.ptr, up_bytes, hipMemcpyHostToDevice, stream));
  DV_HIP_CHECK(hipMemsetAsync(at<uint8_t>(buf.d_img.ptr, scratch_at), 0, scratch_bytes, stream));
  return DV_OK;
}

// The first step of the download: the pass' record counts, which lie behind n_events.  Waits for the stream.
int download_record_counts(const CountsBuffers& buf, const CountsImage& im, int32_t* n_records, int count,
                           hipStream_t stream) {
  DV_HIP_CHECK(hipMemcpyAsync(n_records, at<uint8_t>(buf.d_img.ptr, im.words + 4), count * sizeof(int32_t),
                              hipMemcpyDeviceToHost, stream));
  DV_HIP_CHECK(hipStreamSynchronize(stream));
  return DV_OK;
}

// The gVCF pass over a region's host counts.  The records land in the result's pageable vector: the copy is
// followed by a synchronisation before the function returns.
int gvcf_from_counts(const dv_allele_counts* c, const dv_allele_counter_options* o, const dv_batch* b,
                     const int32_t* keys, const dv_gvcf_options* gv, const dv_gvcf_site* d_table, hipStream_t stream,
                     dv_gvcf_blocks** out) {
  static thread_local CountsBuffers buf;
  CountsImage im = lay_counts_image(sizeof(dv::GvcfRegion), c, b, keys);
  const size_t up_bytes = im.lay.bytes();
  const size_t o_scr = im.lay.add(dv::gvcf_scratch_ints(im.len, im.n_ev) * sizeof(int32_t));
  const size_t o_blk = im.lay.add_last(static_cast<size_t>(im.len - gv->left_padding - gv->right_padding) * sizeof(dv_gvcf_block));
  if (int rc = buf.stage.reserve(up_bytes)) return rc;
  if (int rc = buf.d_img.reserve_on_current_device(im.lay.bytes())) return rc;
  uint8_t* dev = static_cast<uint8_t*>(buf.d_img.ptr);
  const CountsOnDevice counts = stage_counts(im, c, o, keys, buf.stage.ptr, dev);
  const dv::GvcfRegion g = gvcf_region(counts, gv, at<int32_t>(dev, o_scr), at<dv_gvcf_block>(dev, o_blk),
                                       at<int32_t>(dev, im.words + 4));
  std::memcpy(buf.stage.ptr + im.desc, &g, sizeof(g));
  if (int rc = upload_counts_image(buf, up_bytes, o_scr, o_blk - o_scr, stream)) return rc;
  if (int rc = dv::gvcf_launch(at<const dv::GvcfRegion>(dev, im.desc), 1, im.len, im.n_ev, gv, d_table, nullptr, stream)) {
    return rc;
  }
  int32_t n_blocks = 0;
  if (int rc = download_record_counts(buf, im, &n_blocks, 1, stream)) return rc;
  auto res = std::make_unique<dv_gvcf_blocks>();
  res->blocks.resize(static_cast<size_t>(n_blocks));
  if (n_blocks) {
    DV_HIP_CHECK(hipMemcpyAsync(res->blocks.data(), dev + o_blk, static_cast<size_t>(n_blocks) * sizeof(dv_gvcf_block),
                                hipMemcpyDeviceToHost, stream));
    DV_HIP_CHECK(hipStreamSynchronize(stream));
  }
  *out = res.release();
  return DV_OK;
}

// The candidate pass over a region's host counts, so that the event words come back in the order of
// dv_allele_counts_arrays.  A host-resident read table's offsets and bases go up with the image; a device-resident
// one is read where it lies.  The records land in the result's pageable vectors: the synchronisation at the end
// follows the copies.
int candidates_from_counts(const dv_allele_counts* c, const dv_allele_counter_options* o, const dv_batch* b,
                           const int32_t* keys, const dv_candidate_options* co, hipStream_t stream,
                           dv_candidates** out) {
  static thread_local CountsBuffers buf;
  auto res = std::make_unique<dv_candidates>();
  if (c->length == 0) {
    *out = res.release();
    return DV_OK;
  }
  if (c->length > 0x7fffffff - 2) return dv::fail(DV_ERR_INVALID_ARGUMENT, "interval too long for the candidate pass");
  CountsImage im = lay_counts_image(sizeof(dv::CandRegion), c, b, keys);
  const size_t n_reads = static_cast<size_t>(b->n_reads);
  const bool table_on_host = b->memory == DV_MEM_HOST && n_reads > 0;
  const size_t o_seq = table_on_host ? im.lay.add((n_reads + 1) * sizeof(uint32_t)) : 0;
  const size_t o_bases = table_on_host ? im.lay.add(b->n_bases) : 0;
  const size_t up_bytes = im.lay.bytes();
  const size_t o_scr = im.lay.add(dv::cand_scratch_ints(im.len, im.n_ev) * sizeof(int32_t));
  const size_t o_site = im.lay.add(static_cast<size_t>(im.len) * sizeof(dv_candidate_site));
  const size_t o_all = im.lay.add(static_cast<size_t>(im.n_ev) * sizeof(dv_candidate_allele));
  const size_t o_evw = im.lay.add(static_cast<size_t>(im.n_ev) * sizeof(int32_t));
  if (int rc = buf.stage.reserve(up_bytes)) return rc;
  if (int rc = buf.d_img.reserve_on_current_device(im.lay.bytes())) return rc;
  uint8_t* dev = static_cast<uint8_t*>(buf.d_img.ptr);
  const CountsOnDevice counts = stage_counts(im, c, o, keys, buf.stage.ptr, dev);
  if (table_on_host) {
    std::memcpy(buf.stage.ptr + o_seq, b->read_seq_off, (n_reads + 1) * sizeof(uint32_t));
    std::memcpy(buf.stage.ptr + o_bases, b->bases, b->n_bases);
  }
  const dv::CandRegion g = cand_region(counts, table_on_host ? dev + o_bases : b->bases,
                                       table_on_host ? at<const uint32_t>(dev, o_seq) : b->read_seq_off,
                                       at<int32_t>(dev, o_scr), at<dv_candidate_site>(dev, o_site),
                                       at<dv_candidate_allele>(dev, o_all), at<int32_t>(dev, o_evw),
                                       at<int32_t>(dev, im.words + 4));
  std::memcpy(buf.stage.ptr + im.desc, &g, sizeof(g));
  if (int rc = upload_counts_image(buf, up_bytes, o_scr, o_site - o_scr, stream)) return rc;
  if (int rc = dv::cand_launch(at<const dv::CandRegion>(dev, im.desc), 1, im.n_ev, co, nullptr, nullptr, stream)) return rc;
  int32_t n_out[2] = {0, 0};
  if (int rc = download_record_counts(buf, im, n_out, 2, stream)) return rc;
  res->sites.resize(static_cast<size_t>(n_out[0]));
  if (n_out[0]) {
    DV_HIP_CHECK(hipMemcpyAsync(res->sites.data(), dev + o_site, res->sites.size() * sizeof(dv_candidate_site),
                                hipMemcpyDeviceToHost, stream));
  }
  if (!co->positions_only) {
    res->alleles.resize(static_cast<size_t>(n_out[1]));
    res->words.resize(im.n_ev);
    if (n_out[1]) {
      DV_HIP_CHECK(hipMemcpyAsync(res->alleles.data(), dev + o_all, res->alleles.size() * sizeof(dv_candidate_allele),
                                  hipMemcpyDeviceToHost, stream));
    }
    if (im.n_ev) {
      DV_HIP_CHECK(hipMemcpyAsync(res->words.data(), dev + o_evw, static_cast<size_t>(im.n_ev) * sizeof(int32_t),
                                  hipMemcpyDeviceToHost, stream));
    }
  }
  DV_HIP_CHECK(hipStreamSynchronize(stream));
  *out = res.release();
  return DV_OK;
}

// The window pass over a region's host counts: the candidate pass' image, with the window kernels' descriptor,
// scratch and records behind it.
int windows_from_counts(const dv_allele_counts* c, const dv_allele_counter_options* o, const dv_batch* b,
                        const int32_t* keys, const dv_window_options* wo, hipStream_t stream, dv_windows** out) {
  static thread_local CountsBuffers buf;
  auto res = std::make_unique<dv_windows>();
  if (c->length == 0) {
    *out = res.release();
    return DV_OK;
  }
  if (c->length > 0x7fffffff - 2) return dv::fail(DV_ERR_INVALID_ARGUMENT, "interval too long for the window pass");
  CountsImage im = lay_counts_image(sizeof(dv::CandRegion), c, b, keys);
  const size_t n_reads = static_cast<size_t>(b->n_reads);
  const bool table_on_host = b->memory == DV_MEM_HOST && n_reads > 0;
  const size_t o_wdesc = im.lay.add(sizeof(dv::WindowRegion));
  const size_t o_seq = table_on_host ? im.lay.add((n_reads + 1) * sizeof(uint32_t)) : 0;
  const size_t o_bases = table_on_host ? im.lay.add(b->n_bases) : 0;
  const size_t up_bytes = im.lay.bytes();
  const size_t n_win_cap = dv::win_cap(im.len, wo->min_windows_distance), n_mask = dv::mask_words(im.len);
  const size_t o_scr = im.lay.add(dv::cand_scratch_ints(im.len, im.n_ev) * sizeof(int32_t));
  const size_t o_wscr = im.lay.add(dv::win_scratch_ints(im.len, im.n_ev) * sizeof(int32_t));
  const size_t o_win = im.lay.add(n_win_cap * 2 * sizeof(int64_t));
  const size_t o_score = im.lay.add(static_cast<size_t>(im.len) * sizeof(uint32_t));
  const size_t o_mask = im.lay.add(n_mask * sizeof(uint32_t));
  if (int rc = buf.stage.reserve(up_bytes)) return rc;
  if (int rc = buf.d_img.reserve_on_current_device(im.lay.bytes())) return rc;
  uint8_t* dev = static_cast<uint8_t*>(buf.d_img.ptr);
  const CountsOnDevice counts = stage_counts(im, c, o, keys, buf.stage.ptr, dev);
  if (table_on_host) {
    std::memcpy(buf.stage.ptr + o_seq, b->read_seq_off, (n_reads + 1) * sizeof(uint32_t));
    std::memcpy(buf.stage.ptr + o_bases, b->bases, b->n_bases);
  }
  const dv::CandRegion g = cand_region(counts, table_on_host ? dev + o_bases : b->bases,
                                       table_on_host ? at<const uint32_t>(dev, o_seq) : b->read_seq_off,
                                       at<int32_t>(dev, o_scr), nullptr, nullptr, nullptr, nullptr);
  const bool debug = wo->want_debug != 0;
  const dv::WindowRegion w{o->interval_start, at<int32_t>(dev, o_wscr), at<int64_t>(dev, o_win),
                           at<int32_t>(dev, im.words + 4), debug ? at<uint32_t>(dev, o_mask) : nullptr,
                           debug ? at<uint32_t>(dev, o_score) : nullptr};
  std::memcpy(buf.stage.ptr + im.desc, &g, sizeof(g));
  std::memcpy(buf.stage.ptr + o_wdesc, &w, sizeof(w));
  if (int rc = upload_counts_image(buf, up_bytes, o_scr, o_win - o_scr, stream)) return rc;
  if (int rc = dv::window_launch(at<const dv::CandRegion>(dev, im.desc), at<const dv::WindowRegion>(dev, o_wdesc), 1,
                                 im.n_ev, wo, nullptr, stream)) {
    return rc;
  }
  int32_t n_windows = 0;
  if (int rc = download_record_counts(buf, im, &n_windows, 1, stream)) return rc;
  std::vector<int64_t> pairs(static_cast<size_t>(n_windows) * 2);
  if (n_windows) {
    DV_HIP_CHECK(hipMemcpyAsync(pairs.data(), dev + o_win, pairs.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  }
  if (debug) {
    res->scores.resize(static_cast<size_t>(im.len));
    res->mask.resize(n_mask);
    DV_HIP_CHECK(hipMemcpyAsync(res->scores.data(), dev + o_score, res->scores.size() * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, stream));
    DV_HIP_CHECK(hipMemcpyAsync(res->mask.data(), dev + o_mask, n_mask * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  }
  DV_HIP_CHECK(hipStreamSynchronize(stream));
  res->starts.resize(static_cast<size_t>(n_windows));
  res->ends.resize(static_cast<size_t>(n_windows));
  for (size_t i = 0; i < res->starts.size(); ++i) {
    res->starts[i] = pairs[2 * i];
    res->ends[i] = pairs[2 * i + 1];
  }
  *out = res.release();
  return DV_OK;
}

// ---- the batch entry point's steps, in the order count_batch takes them

// What one call asked for.
struct BatchRequest {
  int32_t n;
  const dv_batch* const* reads;
  const dv_allele_counter_options* const* options;
  const int32_t* const* read_keys;
  const dv_gvcf_options* gv;           // null: no gVCF pass
  const dv_candidate_options* co;      // null: no candidate pass
  const dv_window_options* wo;         // null: no window pass
  bool pos_only;                       // positions or windows only: neither counts nor events come back
  hipStream_t stream;
  const char* who;
  const int32_t* keys_of(int32_t k) const { return read_keys ? read_keys[k] : nullptr; }
};

// The caller's result arrays.  Until release() every result in them is this guard's: on an error exit -- the
// DV_HIP_CHECK returns included -- none is left allocated and every entry is null.  With positions_only (or a
// window pass without counts_out) the counts of a region that went alone live in own_out and never reach the caller.
struct BatchResults {
  int32_t n = 0;
  dv_allele_counts** out = nullptr;
  dv_gvcf_blocks** gout = nullptr;     // null without the pass
  dv_candidates** cout = nullptr;
  dv_windows** wout = nullptr;
  std::vector<dv_allele_counts*> own_out;
  bool released = false;

  void take(int32_t count, dv_allele_counts** counts, dv_gvcf_blocks** blocks, dv_candidates** candidates,
            dv_windows** windows) {
    n = count, out = counts, gout = blocks, cout = candidates, wout = windows;
    for (int32_t k = 0; k < n; ++k) {
      out[k] = nullptr;
      if (gout) gout[k] = nullptr;
      if (cout) cout[k] = nullptr;
      if (wout) wout[k] = nullptr;
    }
  }
  void release() { released = true; }
  template <class T> static void drop(T*& p) {
    delete p;
    p = nullptr;
  }
  ~BatchResults() {
    for (int32_t k = 0; k < n; ++k) {
      if (!released || !own_out.empty()) drop(out[k]);
      if (!released && gout) drop(gout[k]);
      if (!released && cout) drop(cout[k]);
      if (!released && wout) drop(wout[k]);
    }
  }
};

// Everything that can be refused before any device work; hands the result arrays to `results`.
int check_batch(const BatchRequest& rq, dv_allele_counts** out, dv_gvcf_blocks** gout, dv_candidates** cout,
                dv_windows** wout, BatchResults* results) {
  const std::string name(rq.who);
  const int32_t n = rq.n;
  if (rq.pos_only && n > 0) {
    results->own_out.assign(static_cast<size_t>(n), nullptr);
    out = results->own_out.data();
  }
  if (n < 0 || (n > 0 && (!rq.reads || !rq.options || !out || (rq.gv && !gout) || (rq.co && !cout) || (rq.wo && !wout)))) {
    return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": null");
  }
  results->take(n, out, rq.gv ? gout : nullptr, rq.co ? cout : nullptr, rq.wo ? wout : nullptr);
  if (rq.wo) {
    if (int rc = dv::window_check_options(rq.wo, rq.who)) return rc;
  }
  if (rq.gv) {
    if (int rc = dv::gvcf_check_options(rq.gv, rq.who)) return rc;
  }
  if (rq.co) {
    if (int rc = dv::cand_check_options(rq.co, rq.who)) return rc;
    if (rq.pos_only && rq.gv) return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": positions_only excludes the gVCF pass");
  }
  for (int32_t k = 0; k < n; ++k) {
    const dv_allele_counter_options* o = rq.options[k];
    if (rq.gv) {   // before check_request: bad input is reported as such with or without a device
      if (int rc = dv::gvcf_check_region(o, rq.gv, rq.who)) return rc;
    }
    if (int rc = check_request(rq.reads[k], o, &out[k], rq.who)) return rc;
    if (o->track_ref_reads && o->n_candidate_positions > 0 && !o->candidate_positions) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": candidate_positions is null");
    }
    if (rq.co && o->interval_end - o->interval_start > 0x7fffffff - 2) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": interval too long for the candidate pass");
    }
    if (rq.wo && o->interval_end - o->interval_start > 0x7fffffff - 2) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, name + ": interval too long for the window pass");
    }
  }
  return DV_OK;
}

// One host thread's grow-only buffers: pinned staging both ways and the device images.
struct BatchBuffers {
  dv::PinnedStage h_up, h_down, h_second;
  dv::DeviceBuffer d_up, d_res, d_ev;
  dv::DeviceBuffer d_gscr, d_gblk, d_gpack;                              // gVCF: scratch, records, packed records
  dv::DeviceBuffer d_cscr, d_csite, d_call, d_cword, d_cpsite, d_cpall;  // candidates: scratch, sites, alleles, words, packed
  dv::DeviceBuffer d_wscr, d_wwin, d_wpack, d_wscore, d_wmask;           // windows: scratch, windows, packed, scores, masks

  // everything but h_second, whose size the first download tells
  int reserve(const dv::BatchPlan& p) {
    const size_t sites = std::max<size_t>(p.cnt_ints, 1), evs = std::max<size_t>(p.ev_total, 1);
    if (int rc = h_up.reserve(p.up_bytes)) return rc;
    if (int rc = h_down.reserve(p.res_bytes)) return rc;
    if (int rc = d_up.reserve_on_current_device(p.up_bytes)) return rc;
    if (int rc = d_res.reserve_on_current_device(p.res_bytes)) return rc;
    if (int rc = d_ev.reserve_on_current_device(evs * sizeof(dv_allele_event))) return rc;
    if (p.gv.n) {
      const size_t blocks = std::max<size_t>(p.gv.blocks, 1);
      if (int rc = d_gscr.reserve_on_current_device(p.gv.scratch_ints * sizeof(int32_t))) return rc;
      if (int rc = d_gblk.reserve_on_current_device(blocks * sizeof(dv_gvcf_block))) return rc;
      if (int rc = d_gpack.reserve_on_current_device(blocks * sizeof(dv_gvcf_block))) return rc;
    }
    if (p.cd.n) {
      if (int rc = d_cscr.reserve_on_current_device(std::max<size_t>(p.cd.scratch_ints, 1) * sizeof(int32_t))) return rc;
      if (int rc = d_csite.reserve_on_current_device(sites * sizeof(dv_candidate_site))) return rc;
      if (int rc = d_cpsite.reserve_on_current_device(sites * sizeof(dv_candidate_site))) return rc;
      if (int rc = d_call.reserve_on_current_device(evs * sizeof(dv_candidate_allele))) return rc;
      if (int rc = d_cpall.reserve_on_current_device(evs * sizeof(dv_candidate_allele))) return rc;
      if (int rc = d_cword.reserve_on_current_device(evs * sizeof(int32_t))) return rc;
    }
    if (p.win.n) {
      const size_t windows = std::max<size_t>(p.win.windows, 1) * 2 * sizeof(int64_t);
      if (int rc = d_wscr.reserve_on_current_device(p.win.scratch_ints * sizeof(int32_t))) return rc;
      if (int rc = d_wwin.reserve_on_current_device(windows)) return rc;
      if (int rc = d_wpack.reserve_on_current_device(windows)) return rc;
      if (int rc = d_wscore.reserve_on_current_device(sites * sizeof(uint32_t))) return rc;
      if (int rc = d_wmask.reserve_on_current_device(std::max<size_t>(p.win.mask_words, 1) * sizeof(uint32_t))) return rc;
    }
    return DV_OK;
  }
};

// The counting kernel's arguments for region k of the batch.
CountArgs batch_count_args(const BatchRequest& rq, const dv::BatchPlan& plan, int32_t k, const BatchBuffers& buf) {
  const dv::RegionPlan& p = plan.regions[k];
  void* dup = buf.d_up.ptr;
  CountArgs a = fill_count_args(rq.reads[k], rq.options[k], p.len);
  a.read_pos = at<const int32_t>(dup, p.up.read_pos);
  a.seq_off = at<const uint32_t>(dup, p.up.seq_off);
  a.cigar_off = at<const uint32_t>(dup, p.up.cigar_off);
  a.mapq = at<const uint8_t>(dup, p.up.mapq);
  a.bases = at<const uint8_t>(dup, p.up.bases);
  a.quals = at<const uint8_t>(dup, p.up.quals);
  a.cigar = at<const uint32_t>(dup, p.up.cigar);
  a.ref = at<const uint8_t>(dup, p.up.ref);
  a.candidate_mask = p.mask_words ? at<const uint32_t>(dup, p.up.mask) : nullptr;
  a.counters = at<uint32_t>(buf.d_res.ptr, plan.counters_at) + static_cast<size_t>(k) * 4;
  a.ref_count = at<int32_t>(buf.d_res.ptr, plan.counts_at) + p.cnt_off;
  a.events = static_cast<dv_allele_event*>(buf.d_ev.ptr) + p.ev_off;
  a.event_cap = p.cap;
  return a;
}

// Region k's arrays into the staging image, its entry of the one-launch kernel's table where the plan has one, and
// its descriptors for the passes it is in: they point into the device images, at the counts, events and reference
// the counter uses.  Results are indexed by region k, descriptor tables by the region's slot among the batched ones.
void stage_region(const BatchRequest& rq, const dv::BatchPlan& plan, int32_t k, const BatchBuffers& buf) {
  const dv::RegionPlan& p = plan.regions[k];
  const dv_batch* b = rq.reads[k];
  const dv_allele_counter_options* o = rq.options[k];
  const size_t nr = static_cast<size_t>(b->n_reads);
  uint8_t* host = buf.h_up.ptr;
  std::memcpy(host + p.up.read_pos, b->read_pos, nr * 4);
  std::memcpy(host + p.up.seq_off, b->read_seq_off, (nr + 1) * 4);
  std::memcpy(host + p.up.cigar_off, b->read_cigar_off, (nr + 1) * 4);
  std::memcpy(host + p.up.mapq, b->read_mapq, nr);
  std::memcpy(host + p.up.bases, b->bases, b->n_bases);
  std::memcpy(host + p.up.quals, b->quals, b->n_bases);
  std::memcpy(host + p.up.cigar, b->cigar, static_cast<size_t>(b->n_cigar) * 4);
  std::memcpy(host + p.up.ref, o->ref_bases, static_cast<size_t>(o->n_ref_bases));
  if (p.mask_words) build_candidate_mask(o, p.len, at<uint32_t>(host, p.up.mask));
  if (p.has_keys) std::memcpy(host + p.up.keys, rq.keys_of(k), nr * 4);
  if (plan.cnt.one_launch) {
    const CountArgs a = batch_count_args(rq, plan, k, buf);
    std::memcpy(host + plan.cnt.args_up + static_cast<size_t>(p.count_slot) * sizeof(a), &a, sizeof(a));
  }
  if (p.gv.slot < 0 && p.cd.slot < 0 && p.win.slot < 0) return;
  void* dup = buf.d_up.ptr;
  const CountsOnDevice c{at<const int32_t>(buf.d_res.ptr, plan.counts_at) + p.cnt_off,
                         static_cast<const dv_allele_event*>(buf.d_ev.ptr) + p.ev_off,
                         at<const uint32_t>(buf.d_res.ptr, plan.counters_at) + static_cast<size_t>(k) * 4, p.cap,
                         p.has_keys ? at<const int32_t>(dup, p.up.keys) : nullptr,
                         at<const uint8_t>(dup, p.up.ref) + (o->interval_start - o->ref_start), o->interval_start, p.len};
  if (p.cd.slot >= 0) {
    const dv::CandRegion g = cand_region(
        c, at<const uint8_t>(dup, p.up.bases), at<const uint32_t>(dup, p.up.seq_off),
        static_cast<int32_t*>(buf.d_cscr.ptr) + p.cd.scratch_off, static_cast<dv_candidate_site*>(buf.d_csite.ptr) + p.cnt_off,
        static_cast<dv_candidate_allele*>(buf.d_call.ptr) + p.ev_off, static_cast<int32_t*>(buf.d_cword.ptr) + p.ev_off,
        at<int32_t>(buf.d_res.ptr, plan.n_cand_at) + static_cast<size_t>(k) * 2);
    std::memcpy(host + plan.cd.desc_up + static_cast<size_t>(p.cd.slot) * sizeof(g), &g, sizeof(g));
  }
  if (p.win.slot >= 0) {
    // the grouping kernels of the candidate pass work in the first part of the region's scratch and emit nothing
    int32_t* scratch = static_cast<int32_t*>(buf.d_wscr.ptr) + p.win.scratch_off;
    const dv::CandRegion g = cand_region(c, at<const uint8_t>(dup, p.up.bases), at<const uint32_t>(dup, p.up.seq_off),
                                         scratch, nullptr, nullptr, nullptr, nullptr);
    const bool debug = rq.wo->want_debug != 0;
    const dv::WindowRegion w{o->interval_start, scratch + dv::cand_scratch_ints(p.len, p.cap),
                             static_cast<int64_t*>(buf.d_wwin.ptr) + 2 * p.win.window_off,
                             at<int32_t>(buf.d_res.ptr, plan.n_win_at) + k,
                             debug ? static_cast<uint32_t*>(buf.d_wmask.ptr) + p.win.mask_off : nullptr,
                             debug ? static_cast<uint32_t*>(buf.d_wscore.ptr) + p.cnt_off : nullptr};
    std::memcpy(host + plan.win.cand_desc_up + static_cast<size_t>(p.win.slot) * sizeof(g), &g, sizeof(g));
    std::memcpy(host + plan.win.desc_up + static_cast<size_t>(p.win.slot) * sizeof(w), &w, sizeof(w));
  }
  if (p.gv.slot >= 0) {
    const dv::GvcfRegion g = gvcf_region(c, rq.gv, static_cast<int32_t*>(buf.d_gscr.ptr) + p.gv.scratch_off,
                                         static_cast<dv_gvcf_block*>(buf.d_gblk.ptr) + p.gv.block_off,
                                         at<int32_t>(buf.d_res.ptr, plan.n_blocks_at) + k);
    std::memcpy(host + plan.gv.desc_up + static_cast<size_t>(p.gv.slot) * sizeof(g), &g, sizeof(g));
  }
}

// One upload, the counting kernels back to back -- or, where the plan holds their table, the one kernel that
// covers every batched region -- and the passes behind them; no synchronisation.
int stage_and_launch(const BatchRequest& rq, const dv::BatchPlan& plan, const BatchBuffers& buf,
                     const dv_gvcf_site** d_table, dv_count_batch_stats* stats) {
  hipStream_t stream = rq.stream;
  uint32_t* block_first = plan.cnt.one_launch ? at<uint32_t>(buf.h_up.ptr, plan.cnt.first_up) : nullptr;
  uint32_t n_blocks = 0;
  for (int32_t k = 0; k < rq.n; ++k) {
    if (!plan.regions[k].batched) continue;
    stage_region(rq, plan, k, buf);
    if (block_first) {
      block_first[plan.regions[k].count_slot] = n_blocks;
      n_blocks += static_cast<uint32_t>(dv::count_blocks(rq.reads[k]->n_reads));
    }
  }
  if (block_first) block_first[plan.n_batched] = n_blocks;
  DV_HIP_CHECK(hipMemcpyAsync(buf.d_up.ptr, buf.h_up.ptr, plan.up_bytes, hipMemcpyHostToDevice, stream));
  DV_HIP_CHECK(hipMemsetAsync(buf.d_res.ptr, 0, plan.res_bytes, stream));
  if (plan.gv.n) {
    DV_HIP_CHECK(hipMemsetAsync(buf.d_gscr.ptr, 0, plan.gv.scratch_ints * sizeof(int32_t), stream));
    if (int rc = dv::gvcf_table_on_device(rq.gv, d_table, stream)) return rc;
  }
  if (plan.cd.n) DV_HIP_CHECK(hipMemsetAsync(buf.d_cscr.ptr, 0, plan.cd.scratch_ints * sizeof(int32_t), stream));
  if (plan.win.n) DV_HIP_CHECK(hipMemsetAsync(buf.d_wscr.ptr, 0, plan.win.scratch_ints * sizeof(int32_t), stream));
  if (plan.cnt.one_launch) {
    dv::ProfileScope prof(dv::kProfOther, stream);
    hipLaunchKernelGGL(count_alleles_batch_kernel, dim3(n_blocks), dim3(256), 0, stream,
                       at<const CountArgs>(buf.d_up.ptr, plan.cnt.args_up), at<const uint32_t>(buf.d_up.ptr, plan.cnt.first_up),
                       plan.n_batched);
  } else {
    for (int32_t k = 0; k < rq.n; ++k) {
      if (plan.regions[k].batched) launch_count(batch_count_args(rq, plan, k, buf), rq.reads[k]->n_reads, stream);
    }
  }
  DV_HIP_CHECK(hipGetLastError());
  stats->count_launches = plan.cnt.one_launch ? 1 : plan.n_batched;
  stats->count_workgroups = plan.cnt.workgroups;
  if (plan.gv.n) {
    // the reference-confidence pass reads the counts where the kernels above leave them
    if (int rc = dv::gvcf_launch(at<const dv::GvcfRegion>(buf.d_up.ptr, plan.gv.desc_up), plan.gv.n, plan.gv.max_len,
                                 plan.max_cap, rq.gv, *d_table, static_cast<dv_gvcf_block*>(buf.d_gpack.ptr), stream)) {
      return rc;
    }
  }
  if (plan.cd.n) {
    // the candidate caller reads the same counts and events, and the read bases the events point into
    if (int rc = dv::cand_launch(at<const dv::CandRegion>(buf.d_up.ptr, plan.cd.desc_up), plan.cd.n, plan.max_cap, rq.co,
                                 static_cast<dv_candidate_site*>(buf.d_cpsite.ptr),
                                 static_cast<dv_candidate_allele*>(buf.d_cpall.ptr), stream)) {
      return rc;
    }
  }
  if (plan.win.n) {
    // window selection reads the same counts and events
    if (int rc = dv::window_launch(at<const dv::CandRegion>(buf.d_up.ptr, plan.win.cand_desc_up),
                                   at<const dv::WindowRegion>(buf.d_up.ptr, plan.win.desc_up), plan.win.n, plan.max_cap,
                                   rq.wo, static_cast<int64_t*>(buf.d_wpack.ptr), stream)) {
      return rc;
    }
  }
  return DV_OK;
}

// The result image comes home -- with positions_only its counters and record counts only -- and the stream is waited
// for: the events follow once their numbers are known.
int download_first(const BatchRequest& rq, const dv::BatchPlan& plan, const BatchBuffers& buf) {
  if (rq.pos_only) {
    DV_HIP_CHECK(hipMemcpyAsync(buf.h_down.ptr, buf.d_res.ptr, plan.counts_at, hipMemcpyDeviceToHost, rq.stream));
    const size_t records_at = rq.co ? plan.n_cand_at : plan.n_win_at;      // the record counts behind the counts
    DV_HIP_CHECK(hipMemcpyAsync(buf.h_down.ptr + records_at, at<uint8_t>(buf.d_res.ptr, records_at),
                                plan.res_bytes - records_at, hipMemcpyDeviceToHost, rq.stream));
  } else {
    DV_HIP_CHECK(hipMemcpyAsync(buf.h_down.ptr, buf.d_res.ptr, plan.res_bytes, hipMemcpyDeviceToHost, rq.stream));
  }
  DV_HIP_CHECK(hipStreamSynchronize(rq.stream));
  return DV_OK;
}

// The results of the regions the batch answers, sized from the first download.
int allocate_results(const BatchRequest& rq, const dv::BatchPlan& plan, const dv::SecondImage& second,
                     const BatchBuffers& buf, BatchResults* results) {
  const uint32_t* counters = at<const uint32_t>(buf.h_down.ptr, plan.counters_at);
  const int32_t* counts = at<const int32_t>(buf.h_down.ptr, plan.counts_at);
  for (int32_t k = 0; k < rq.n; ++k) {
    const dv::RegionPlan& p = plan.regions[k];
    const dv::SecondImage::Region& r = second.regions[k];
    if (p.batched && counters[4 * k + 2] != 0) return window_too_small();
    if (!r.kept) continue;           // the first guess was too small: this region goes alone (two passes there)
    if (rq.co) {
      results->cout[k] = new dv_candidates();
      results->cout[k]->sites.resize(r.n_sites);
      if (!rq.pos_only) results->cout[k]->alleles.resize(r.n_alleles);
    }
    if (rq.wo) {
      results->wout[k] = new dv_windows();
      results->wout[k]->starts.resize(r.n_windows);
      results->wout[k]->ends.resize(r.n_windows);
    }
    if (rq.pos_only) continue;
    auto res = std::make_unique<dv_allele_counts>();
    res->length = p.len;
    res->n_reads_counted = static_cast<int32_t>(counters[4 * k + 1]);
    if (int rc = res->ref_count.reserve(static_cast<size_t>(p.len))) return rc;
    std::memcpy(res->ref_count.ptr, counts + p.cnt_off, static_cast<size_t>(p.len) * sizeof(int32_t));
    if (int rc = res->raw.reserve(r.n_events)) return rc;
    results->out[k] = res.release();
    if (rq.gv) {
      results->gout[k] = new dv_gvcf_blocks();
      results->gout[k]->blocks.resize(r.n_blocks);
    }
  }
  return DV_OK;
}

// The events and event words of every kept region and the packed records of every region into one pinned image,
// one synchronisation.
int download_second(const BatchRequest& rq, const dv::BatchPlan& plan, const dv::SecondImage& second, BatchBuffers* buf) {
  if (int rc = buf->h_second.reserve(second.bytes)) return rc;
  uint8_t* host = buf->h_second.ptr;
  hipStream_t stream = rq.stream;
  for (int32_t k = 0; k < rq.n; ++k) {
    const dv::SecondImage::Region& r = second.regions[k];
    if (!r.kept || r.n_events == 0) continue;
    const size_t ev_off = plan.regions[k].ev_off;
    DV_HIP_CHECK(hipMemcpyAsync(host + r.events_at, static_cast<const dv_allele_event*>(buf->d_ev.ptr) + ev_off,
                                r.n_events * sizeof(dv_allele_event), hipMemcpyDeviceToHost, stream));
    if (rq.co) {
      DV_HIP_CHECK(hipMemcpyAsync(host + r.words_at, static_cast<const int32_t*>(buf->d_cword.ptr) + ev_off,
                                  r.n_events * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    }
  }
  if (second.packed_sites) {
    DV_HIP_CHECK(hipMemcpyAsync(host + second.sites_at, buf->d_cpsite.ptr, second.packed_sites * sizeof(dv_candidate_site),
                                hipMemcpyDeviceToHost, stream));
  }
  if (second.packed_alleles && !rq.pos_only) {
    DV_HIP_CHECK(hipMemcpyAsync(host + second.alleles_at, buf->d_cpall.ptr,
                                second.packed_alleles * sizeof(dv_candidate_allele), hipMemcpyDeviceToHost, stream));
  }
  if (second.packed_blocks) {
    DV_HIP_CHECK(hipMemcpyAsync(host + second.blocks_at, buf->d_gpack.ptr, second.packed_blocks * sizeof(dv_gvcf_block),
                                hipMemcpyDeviceToHost, stream));
  }
  if (second.packed_windows) {
    DV_HIP_CHECK(hipMemcpyAsync(host + second.windows_at, buf->d_wpack.ptr, second.packed_windows * 2 * sizeof(int64_t),
                                hipMemcpyDeviceToHost, stream));
  }
  if (rq.wo && rq.wo->want_debug && plan.win.n) {
    DV_HIP_CHECK(hipMemcpyAsync(host + second.scores_at, buf->d_wscore.ptr, plan.cnt_ints * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, stream));
    DV_HIP_CHECK(hipMemcpyAsync(host + second.masks_at, buf->d_wmask.ptr, plan.win.mask_words * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, stream));
  }
  DV_HIP_CHECK(hipStreamSynchronize(stream));
  return DV_OK;
}

// Out of the second image into the kept regions' results; the events are put in order.
void unpack(const BatchRequest& rq, const dv::BatchPlan& plan, const dv::SecondImage& second, const BatchBuffers& buf,
            BatchResults* results) {
  const uint8_t* host = buf.h_second.ptr;
  for (int32_t k = 0; k < rq.n; ++k) {
    const dv::SecondImage::Region& r = second.regions[k];
    if (!r.kept) continue;
    if (rq.co) {
      dv_candidates* cand = results->cout[k];
      if (r.n_sites) std::memcpy(cand->sites.data(), host + r.sites_at, r.n_sites * sizeof(dv_candidate_site));
      if (r.n_alleles && !rq.pos_only) {
        std::memcpy(cand->alleles.data(), host + r.alleles_at, r.n_alleles * sizeof(dv_candidate_allele));
      }
    }
    if (rq.wo) {
      dv_windows* win = results->wout[k];
      const dv::RegionPlan& p = plan.regions[k];
      for (size_t i = 0; i < r.n_windows; ++i) {
        std::memcpy(&win->starts[i], host + r.windows_at + 2 * i * sizeof(int64_t), sizeof(int64_t));
        std::memcpy(&win->ends[i], host + r.windows_at + (2 * i + 1) * sizeof(int64_t), sizeof(int64_t));
      }
      if (rq.wo->want_debug) {
        win->scores.resize(static_cast<size_t>(p.len));
        win->mask.resize(dv::mask_words(p.len));
        std::memcpy(win->scores.data(), host + second.scores_at + p.cnt_off * sizeof(uint32_t),
                    win->scores.size() * sizeof(uint32_t));
        std::memcpy(win->mask.data(), host + second.masks_at + p.win.mask_off * sizeof(uint32_t),
                    win->mask.size() * sizeof(uint32_t));
      }
    }
    if (rq.pos_only) continue;
    dv_allele_counts* counts = results->out[k];
    if (r.n_events) std::memcpy(counts->raw.ptr, host + r.events_at, r.n_events * sizeof(dv_allele_event));
    if (rq.co) {
      order_events_with_words(counts, r.n_events, reinterpret_cast<const int32_t*>(host + r.words_at),
                              &results->cout[k]->words);
    } else {
      order_events(counts, r.n_events);
    }
    if (rq.gv && r.n_blocks) {
      std::memcpy(results->gout[k]->blocks.data(), host + r.blocks_at, r.n_blocks * sizeof(dv_gvcf_block));
    }
  }
}

// The regions the batch did not answer, one by one: the one-region entry, then each pass from its counts.
int run_alone(const BatchRequest& rq, const dv::SecondImage& second, const dv_gvcf_site* d_table, BatchResults* results,
              dv_count_batch_stats* stats) {
  for (int32_t k = 0; k < rq.n; ++k) {
    if (second.regions[k].kept) continue;
    if (rq.reads[k]->n_reads != 0 && rq.options[k]->interval_end != rq.options[k]->interval_start) ++stats->regions_alone;
    if (int rc = dv_count_alleles(rq.reads[k], rq.options[k], &results->out[k], rq.stream)) return rc;
    if (rq.co) {
      if (int rc = candidates_from_counts(results->out[k], rq.options[k], rq.reads[k], rq.keys_of(k), rq.co, rq.stream,
                                          &results->cout[k])) {
        return rc;
      }
    }
    if (rq.wo) {
      if (int rc = windows_from_counts(results->out[k], rq.options[k], rq.reads[k], rq.keys_of(k), rq.wo, rq.stream,
                                       &results->wout[k])) {
        return rc;
      }
    }
    if (rq.gv) {
      if (!d_table) {
        if (int rc = dv::gvcf_table_on_device(rq.gv, &d_table, rq.stream)) return rc;
      }
      if (int rc = gvcf_from_counts(results->out[k], rq.options[k], rq.reads[k], rq.keys_of(k), rq.gv, d_table, rq.stream,
                                    &results->gout[k])) {
        return rc;
      }
    }
  }
  return DV_OK;
}

// What the calling thread's last batch call did: dv_count_batch_last_stats.
dv_count_batch_stats& last_batch_stats() {
  static thread_local dv_count_batch_stats stats{};
  return stats;
}

// DV_COUNT_ONE_LAUNCH=1: the batched regions of a call are counted by one launch of count_alleles_batch_kernel.
// Read at every call; off by default.
bool count_one_launch_enabled() { return dv::env_switch("DV_COUNT_ONE_LAUNCH", false); }

}  // namespace

extern "C" {

int dv_count_alleles(const dv_batch* b, const dv_allele_counter_options* o, dv_allele_counts** out, void* stream_v) {
  if (int rc = check_request(b, o, out, "dv_count_alleles")) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const int64_t len = o->interval_end - o->interval_start;
  auto res = std::make_unique<dv_allele_counts>();
  res->length = len;
  if (b->n_reads == 0 || len == 0) {
    res->empty_counts.assign(static_cast<size_t>(len), 0);
    *out = res.release();
    return DV_OK;
  }
  // result / reference scratch is kept per host thread (grow-only): a region driver calls this
  // once per region and hipMalloc + hipFree of ~100 MB cost more than the kernel
  static thread_local dv::DeviceBuffer d_ref, d_cnt, d_ev, d_ctr, d_mask;
  // ... and so are the upload buffers of a host-resident table: seven hipMalloc + hipFree per call
  // were most of the millisecond a 300-read region took (the kernel itself is a few microseconds)
  static thread_local dv::DeviceBuffer up[7];
  CountArgs a = fill_count_args(b, o, len);
  const size_t n = static_cast<size_t>(b->n_reads);
  if (int rc = to_device(up[0], b->read_pos, n, b->memory, &a.read_pos, stream)) return rc;
  if (int rc = to_device(up[1], b->read_seq_off, n + 1, b->memory, &a.seq_off, stream)) return rc;
  if (int rc = to_device(up[2], b->read_cigar_off, n + 1, b->memory, &a.cigar_off, stream)) return rc;
  if (int rc = to_device(up[3], b->read_mapq, n, b->memory, &a.mapq, stream)) return rc;
  if (int rc = to_device(up[4], b->bases, b->n_bases, b->memory, &a.bases, stream)) return rc;
  if (int rc = to_device(up[5], b->quals, b->n_bases, b->memory, &a.quals, stream)) return rc;
  if (int rc = to_device(up[6], b->cigar, b->n_cigar, b->memory, &a.cigar, stream)) return rc;
  if (int rc = d_ref.reserve_on_current_device(static_cast<size_t>(o->n_ref_bases))) return rc;
  DV_HIP_CHECK(hipMemcpyAsync(d_ref.ptr, o->ref_bases, static_cast<size_t>(o->n_ref_bases), hipMemcpyHostToDevice,
                              stream));
  a.ref = static_cast<const uint8_t*>(d_ref.ptr);
  const size_t n_candidate_refs = dv::n_candidate_refs(o);
  if (n_candidate_refs) {
    if (!o->candidate_positions) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_count_alleles: candidate_positions is null");
    std::vector<uint32_t> mask(dv::mask_words(len));
    build_candidate_mask(o, len, mask.data());
    if (int rc = d_mask.reserve_on_current_device(mask.size() * sizeof(uint32_t))) return rc;
    DV_HIP_CHECK(hipMemcpyAsync(d_mask.ptr, mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    DV_HIP_CHECK(hipStreamSynchronize(stream));      // `mask` is a local: the copy must have read it before it goes
    a.candidate_mask = static_cast<const uint32_t*>(d_mask.ptr);
  }
  if (int rc = d_cnt.reserve_on_current_device(static_cast<size_t>(len) * sizeof(int32_t))) return rc;
  if (int rc = d_ctr.reserve_on_current_device(4 * sizeof(uint32_t))) return rc;
  a.ref_count = static_cast<int32_t*>(d_cnt.ptr);
  a.counters = static_cast<uint32_t*>(d_ctr.ptr);
  // the counter keeps counting past the capacity, so a second pass sizes it exactly
  uint32_t cap = dv::first_event_cap(b, n_candidate_refs);
  uint32_t ctr[4] = {0, 0, 0, 0};
  for (int pass = 0; pass < 2; ++pass) {
    if (int rc = d_ev.reserve_on_current_device(static_cast<size_t>(cap) * sizeof(dv_allele_event))) return rc;
    a.events = static_cast<dv_allele_event*>(d_ev.ptr);
    a.event_cap = cap;
    DV_HIP_CHECK(hipMemsetAsync(d_cnt.ptr, 0, static_cast<size_t>(len) * sizeof(int32_t), stream));
    DV_HIP_CHECK(hipMemsetAsync(d_ctr.ptr, 0, 4 * sizeof(uint32_t), stream));
    launch_count(a, b->n_reads, stream);
    DV_HIP_CHECK(hipGetLastError());
    DV_HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.ptr, sizeof(ctr), hipMemcpyDeviceToHost, stream));
    DV_HIP_CHECK(hipStreamSynchronize(stream));
    if (ctr[0] <= cap) break;
    cap = ctr[0];
  }
  if (ctr[2] != 0) return window_too_small();
  res->n_reads_counted = static_cast<int32_t>(ctr[1]);
  if (int rc = res->ref_count.reserve(static_cast<size_t>(len))) return rc;
  if (int rc = res->raw.reserve(ctr[0])) return rc;
  DV_HIP_CHECK(hipMemcpyAsync(res->ref_count.ptr, d_cnt.ptr, static_cast<size_t>(len) * sizeof(int32_t),
                              hipMemcpyDeviceToHost, stream));
  if (ctr[0]) {
    DV_HIP_CHECK(hipMemcpyAsync(res->raw.ptr, d_ev.ptr, static_cast<size_t>(ctr[0]) * sizeof(dv_allele_event),
                                hipMemcpyDeviceToHost, stream));
  }
  DV_HIP_CHECK(hipStreamSynchronize(stream));
  order_events(res.get(), ctr[0]);
  *out = res.release();
  return DV_OK;
}

// Several regions in one go (a region driver's batch of 1 kb calling regions: window selection of
// all of them, then their candidate counts).  What a one-region call spends is not the kernel (a few
// microseconds) but ~10 small pageable uploads, two stream synchronisations and two small
// downloads; here every region's arrays travel in ONE pinned staging image, the kernels are queued
// back to back, and the stream is synchronised twice for the whole batch.  Results per region are
// those of dv_count_alleles (the same kernel on the same arguments).  Regions whose tables are
// device-resident, and the rare region whose events overflow the first guess, take the one-region path.
// With DV_COUNT_ONE_LAUNCH=1 the batched regions' kernels are one launch (count_alleles_batch_kernel: the same
// workgroups in one grid); nothing that comes back differs, and dv_count_batch_last_stats tells which way a call went.
// dv_count_alleles_batch, and with `gv` set dv_count_alleles_gvcf_batch: the gVCF pass (gvcf.hip) is queued
// behind the counting kernels and its records come back with the events.  Without `gv` nothing differs.
// With `co` set dv_call_candidates_batch: the candidate pass (candidates.hip) is queued behind the counting
// kernels in the same way; with positions_only neither counts nor events come back (`out` is not used).
// With `wo` set dv_select_windows_batch: the window pass (window_select.hip) likewise; without `out` only the
// windows come back.
static int count_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                       const int32_t* const* read_keys, const dv_gvcf_options* gv, const dv_candidate_options* co,
                       const dv_window_options* wo, dv_allele_counts** out, dv_gvcf_blocks** gout, dv_candidates** cout,
                       dv_windows** wout, void* stream_v, const char* who) {
  const BatchRequest rq{n, reads, options, read_keys, gv, co, wo, (co && co->positions_only) || (wo && !out),
                        static_cast<hipStream_t>(stream_v), who};
  BatchResults results;              // frees whatever it holds on every return but the last
  dv_count_batch_stats& stats = last_batch_stats();
  stats = dv_count_batch_stats{};
  if (int rc = check_batch(rq, out, gout, cout, wout, &results)) return rc;
  const dv::BatchPlan plan = dv::plan_batch(n, reads, options, read_keys, gv, co, wo, count_one_launch_enabled());
  stats.regions = n;
  stats.regions_batched = plan.n_batched;
  dv::SecondImage second;            // of no region yet: which regions the batch has answered
  second.regions.resize(plan.regions.size());
  const dv_gvcf_site* d_table = nullptr;
  if (plan.n_batched > 0) {
    static thread_local BatchBuffers buf;
    if (int rc = buf.reserve(plan)) return rc;
    if (int rc = stage_and_launch(rq, plan, buf, &d_table, &stats)) return rc;
    if (int rc = download_first(rq, plan, buf)) return rc;
    second = dv::second_image(plan, at<const uint32_t>(buf.h_down.ptr, plan.counters_at),
                              at<const int32_t>(buf.h_down.ptr, plan.n_blocks_at),
                              at<const int32_t>(buf.h_down.ptr, plan.n_cand_at), rq.pos_only,
                              at<const int32_t>(buf.h_down.ptr, plan.n_win_at), wo && wo->want_debug);
    if (int rc = allocate_results(rq, plan, second, buf, &results)) return rc;
    if (int rc = download_second(rq, plan, second, &buf)) return rc;
    unpack(rq, plan, second, buf, &results);
  }
  if (int rc = run_alone(rq, second, d_table, &results, &stats)) return rc;
  results.release();
  return DV_OK;
}

int dv_count_alleles_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                           dv_allele_counts** out, void* stream_v) {
  return count_batch(n, reads, options, nullptr, nullptr, nullptr, nullptr, out, nullptr, nullptr, nullptr, stream_v,
                     "dv_count_alleles_batch");
}

int dv_count_alleles_gvcf_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                                const int32_t* const* read_keys, const dv_gvcf_options* gvcf,
                                dv_allele_counts** counts_out, dv_gvcf_blocks** blocks_out, void* stream) {
  if (!gvcf) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_count_alleles_gvcf_batch: gvcf options are null");
  return count_batch(n, reads, options, read_keys, gvcf, nullptr, nullptr, counts_out, blocks_out, nullptr, nullptr, stream,
                     "dv_count_alleles_gvcf_batch");
}

int dv_call_candidates_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                             const int32_t* const* read_keys, const dv_candidate_options* candidate_options,
                             const dv_gvcf_options* gvcf, dv_allele_counts** counts_out, dv_gvcf_blocks** blocks_out,
                             dv_candidates** candidates_out, void* stream) {
  if (!candidate_options) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_call_candidates_batch: candidate options are null");
  return count_batch(n, reads, options, read_keys, gvcf, candidate_options, nullptr, counts_out, blocks_out, candidates_out,
                     nullptr, stream, "dv_call_candidates_batch");
}

int dv_select_windows_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                            const int32_t* const* read_keys, const dv_window_options* window_options,
                            dv_allele_counts** counts_out, dv_windows** windows_out, void* stream) {
  if (!window_options) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_select_windows_batch: window options are null");
  return count_batch(n, reads, options, read_keys, nullptr, nullptr, window_options, counts_out, nullptr, nullptr,
                     windows_out, stream, "dv_select_windows_batch");
}

int dv_count_batch_last_stats(dv_count_batch_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_count_batch_last_stats: null");
  *out = last_batch_stats();
  return DV_OK;
}

int64_t dv_windows_arrays(const dv_windows* w, const int64_t** starts, const int64_t** ends,
                          const uint32_t** candidate_mask, const uint32_t** scores) {
  if (!w) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_windows_arrays: null");
  if (starts) *starts = w->starts.data();
  if (ends) *ends = w->ends.data();
  if (candidate_mask) *candidate_mask = w->mask.empty() ? nullptr : w->mask.data();
  if (scores) *scores = w->scores.empty() ? nullptr : w->scores.data();
  return static_cast<int64_t>(w->starts.size());
}

void dv_windows_free(dv_windows* w) { delete w; }

int64_t dv_candidates_arrays(const dv_candidates* c, const dv_candidate_site** sites,
                             const dv_candidate_allele** alleles, int32_t* n_alleles, const int32_t** event_words,
                             uint32_t* n_events) {
  if (!c) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_candidates_arrays: null");
  if (sites) *sites = c->sites.data();
  if (alleles) *alleles = c->alleles.data();
  if (n_alleles) *n_alleles = static_cast<int32_t>(c->alleles.size());
  if (event_words) *event_words = c->words.data();
  if (n_events) *n_events = static_cast<uint32_t>(c->words.size());
  return static_cast<int64_t>(c->sites.size());
}

void dv_candidates_free(dv_candidates* c) { delete c; }

int64_t dv_gvcf_blocks_arrays(const dv_gvcf_blocks* b, const dv_gvcf_block** blocks) {
  if (!b) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_gvcf_blocks_arrays: null");
  if (blocks) *blocks = b->blocks.data();
  return static_cast<int64_t>(b->blocks.size());
}

void dv_gvcf_blocks_free(dv_gvcf_blocks* b) { delete b; }

int dv_allele_counts_arrays(const dv_allele_counts* c, const int32_t** ref_supporting_read_count,
                            const dv_allele_event** events, uint32_t* n_events, int32_t* n_reads_counted) {
  if (!c) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_allele_counts_arrays: null");
  if (ref_supporting_read_count) *ref_supporting_read_count = c->ref_count.ptr ? c->ref_count.ptr : c->empty_counts.data();
  if (events) *events = c->events.data();
  if (n_events) *n_events = static_cast<uint32_t>(c->events.size());
  if (n_reads_counted) *n_reads_counted = c->n_reads_counted;
  return static_cast<int>(c->length);
}

void dv_allele_counts_free(dv_allele_counts* c) { delete c; }

}  // extern "C"
