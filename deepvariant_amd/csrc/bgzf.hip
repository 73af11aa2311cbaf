// bgzf.hip -- a text as BGZF, deflated where it lies: dv_bgzf_compress (host code),
// dv_bgzf_compress_device and their result handle (include/dvhip.h).
//
// The rule is bgzf_deflate.h, compiled for both sides.  Device: one staged upload of the CRC tables (and the text when it
// is a host array), five launches queued on one stream, a wait for the 16-byte header, a download of exactly the file.
//   1     per block, one workgroup: the block into the LDS; wave 0 walks the tiles for the candidates while waves 1-3
//         take the CRC-32 in slices; then a lane per segment counts its bits, the workgroup sums them, and the lanes
//         write the member into the block's slot
//   2-4   block_coff = the exclusive sum of the members' sizes (gvcf_merge_device.h); the total goes into the header
//   5     per member, one wave: copy it to its offset; one more wave writes the end-of-file member
// No workgroup reads what another workgroup writes in the same launch, and nothing waits on another lane but at barriers.
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <atomic>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "bgzf_deflate.h"
#include "bgzf_internal.h"
#include "device_round_trip.h"
#include "gvcf_merge_device.h"

static_assert(sizeof(dv_bgzf_parameters) == 16, "dv_bgzf_parameters layout");
static_assert(sizeof(dv_bgzf_view) == 40, "dv_bgzf_view layout");
static_assert(sizeof(dv_bgzf_stats) == 56, "dv_bgzf_stats layout");

namespace {

namespace bz = dv::bz;

static_assert(bz::kBlock <= bz::kSeg * kThreads, "a lane per segment");
static_assert(bz::kTile == 64, "a tile is one wave");

constexpr int kWave = 64;
constexpr int kWavesPerGroup = kThreads / kWave;
constexpr int kCrcLanes = kThreads - kWave;                             // waves 1-3
constexpr int kSlice = (bz::kBlock + kCrcLanes - 1) / kCrcLanes;        // bytes of a block per CRC lane

struct CrcTables {              // host-built, uploaded with every call
  uint32_t byte_table[256];     // the byte-wise CRC
  uint32_t pow_slices[kCrcLanes];       // x^(8 j kSlice) mod P
  uint32_t pow_bytes[kSlice + 1];       // x^(8 r) mod P
};

const CrcTables& crc_tables() {
  static const CrcTables tables = [] {
    CrcTables t;
    for (uint32_t v = 0; v < 256; ++v) {
      uint32_t c = v;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ bz::kCrcPoly : c >> 1;
      t.byte_table[v] = c;
    }
    t.pow_bytes[0] = 0x80000000u;                       // x^0
    for (int r = 1; r <= kSlice; ++r) t.pow_bytes[r] = bz::crc_multiply(t.pow_bytes[r - 1], 0x00800000u);   // * x^8
    t.pow_slices[0] = 0x80000000u;
    for (int j = 1; j < kCrcLanes; ++j) t.pow_slices[j] = bz::crc_multiply(t.pow_slices[j - 1], t.pow_bytes[kSlice]);
    return t;
  }();
  return tables;
}

struct DeflateArgs {
  const uint8_t* text;
  int64_t n;
  const CrcTables* tables;
  uint8_t* slots;               // [n_blocks][kSlot]
  int32_t* size;                // [n_blocks], every member's length
};

// An LSB-first bit stream ORed into zeroed dwords: two segments can share a dword at their edge.
struct DeviceBits {
  uint32_t* words;
  int32_t at;                   // the dword the next bits go to
  int32_t held;                 // bits of `acc` in use, below 32 between calls
  uint64_t acc;
  __device__ DeviceBits(uint32_t* w, int64_t bit) : words(w), at(static_cast<int32_t>(bit >> 5)),
                                                    held(static_cast<int32_t>(bit & 31)), acc(0) {}
  __device__ void put(uint32_t value, int32_t bits) {
    acc |= static_cast<uint64_t>(value) << held;
    held += bits;
    if (held >= 32) {
      atomicOr(words + at, static_cast<uint32_t>(acc));
      ++at;
      acc >>= 32;
      held -= 32;
    }
  }
  __device__ void flush() {
    if (static_cast<uint32_t>(acc) != 0) atomicOr(words + at, static_cast<uint32_t>(acc));
  }
};

__device__ void or_byte(uint32_t* words, int32_t at, uint8_t v) {
  if (v != 0) atomicOr(words + (at >> 2), static_cast<uint32_t>(v) << (8 * (at & 3)));
}

__global__ __launch_bounds__(kThreads) void deflate_blocks_kernel(DeflateArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t data[bz::kBlock];
  __shared__ uint16_t cand[bz::kBlock];
  __shared__ int32_t head[bz::kHeads];
  __shared__ uint32_t byte_table[256];
  __shared__ int64_t rows[2][kThreads];
  __shared__ uint32_t crc_all;
  const int t = static_cast<int>(threadIdx.x);
  const int64_t from = static_cast<int64_t>(blockIdx.x) * bz::kBlock;
  const int32_t n = static_cast<int32_t>(a.n - from < bz::kBlock ? a.n - from : bz::kBlock);
  const uint8_t* src = a.text + from;

  // ---- the block into the LDS, by dwords where the text allows it
  if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
    const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* data4 = reinterpret_cast<uint32_t*>(data);
    for (int32_t i = t; i < n / 4; i += kThreads) data4[i] = src4[i];
    for (int32_t i = (n / 4) * 4 + t; i < n; i += kThreads) data[i] = src[i];
  } else {
    for (int32_t i = t; i < n; i += kThreads) data[i] = src[i];
  }
  for (int32_t i = t; i < bz::kHeads; i += kThreads) head[i] = -1;
  byte_table[t] = a.tables->byte_table[t];
  if (t == 0) crc_all = 0;
  __syncthreads();

  if (t < kWave) {
    // ---- wave 0: the tiles in order.  Every lane reads head before any lane of the tile writes it; the maximum makes
    // the largest position of the tile win whatever order the lanes' writes take.
    for (int32_t base = 0; base < n; base += bz::kTile) {
      const int32_t i = base + t;
      const bool hashed = i + 4 <= n;
      uint32_t h = 0;
      int32_t c = -1;
      if (hashed) {
        h = bz::hash4(data + i);
        c = head[h];
      }
      if (i < n) cand[i] = static_cast<uint16_t>(c < 0 ? bz::kNoCand : c);
      __builtin_amdgcn_wave_barrier();
      if (hashed) atomicMax(&head[h], i);
      __builtin_amdgcn_wave_barrier();
    }
  } else {
    // ---- waves 1-3: slice k's CRC, carried over the bytes behind it.  With n = m kSlice + r the full slice k < m has
    // (m - 1 - k) kSlice + r bytes behind it, and the short slice m has none.
    const int32_t k = t - kWave, lo = k * kSlice;
    if (lo < n) {
      const int32_t m = n / kSlice, r = n % kSlice;
      uint32_t crc = bz::crc_bytes(byte_table, data, lo, lo + kSlice < n ? lo + kSlice : n);
      if (k < m) crc = bz::crc_multiply(bz::crc_multiply(crc, a.tables->pow_slices[m - 1 - k]), a.tables->pow_bytes[r]);
      atomicXor(&crc_all, crc);
    }
  }
  __syncthreads();

  // ---- a lane per segment: its bits, their exclusive sum, stored or fixed
  const int32_t begin = t * bz::kSeg, end = begin + bz::kSeg < n ? begin + bz::kSeg : n;
  bz::CountSink counted;
  if (begin < n) bz::walk_segment(data, cand, begin, end, counted);
  const int64_t* scanned = workgroup_scan<Sum>(static_cast<int64_t>(counted.bits), rows);
  const int64_t token_bits = scanned[kThreads - 1], before = scanned[t] - counted.bits;
  const bool stored = bz::keeps_bytes(token_bits, n);
  const int32_t payload = stored ? n + bz::kStoredBytes : bz::fixed_payload_bytes(token_bits);
  const int32_t member = bz::kHeadBytes + payload + bz::kTailBytes;
  uint8_t* slot = a.slots + static_cast<int64_t>(blockIdx.x) * bz::kSlot;
  const uint32_t crc = crc_all, isize = static_cast<uint32_t>(n);
  if (t == 0) a.size[blockIdx.x] = member;

  if (stored) {
    // plain byte stores only: nothing here shares a byte with another lane
    if (t < bz::kHeadBytes) slot[t] = bz::head_byte(t, member);
    if (t == kWave) {
      uint8_t* p = slot + bz::kHeadBytes;
      p[0] = 1;                                         // BFINAL = 1, BTYPE = 00
      p[1] = static_cast<uint8_t>(n & 0xff);
      p[2] = static_cast<uint8_t>(n >> 8);
      p[3] = static_cast<uint8_t>(~n & 0xff);
      p[4] = static_cast<uint8_t>((~n >> 8) & 0xff);
    }
    if (t == 2 * kWave) {
      uint8_t* p = slot + bz::kHeadBytes + payload;
      for (int k = 0; k < 4; ++k) {
        p[k] = static_cast<uint8_t>(crc >> (8 * k));
        p[4 + k] = static_cast<uint8_t>(isize >> (8 * k));
      }
    }
    uint8_t* dst = slot + bz::kHeadBytes + bz::kStoredBytes;
    for (int32_t i = t; i < n; i += kThreads) dst[i] = data[i];
    return;
  }

  // fixed Huffman: zero the member's dwords, then everything is ORed in
  uint32_t* words = reinterpret_cast<uint32_t*>(slot);
  for (int32_t i = t; i < (member + 3) / 4; i += kThreads) words[i] = 0;
  __syncthreads();
  if (begin < n) {
    DeviceBits out(words, 8 * bz::kHeadBytes + bz::kBlockBits + before);
    bz::BitSink<DeviceBits> sink{&out};
    bz::walk_segment(data, cand, begin, end, sink);
    out.flush();
  }
  // symbol 256 is seven zero bits: they are there already
  if (t == kThreads - 1) {
    for (int k = 0; k < bz::kHeadBytes; ++k) or_byte(words, k, bz::head_byte(k, member));
    or_byte(words, bz::kHeadBytes, 3);                  // BFINAL = 1, BTYPE = 01
    for (int k = 0; k < 4; ++k) {
      or_byte(words, bz::kHeadBytes + payload + k, static_cast<uint8_t>(crc >> (8 * k)));
      or_byte(words, bz::kHeadBytes + payload + 4 + k, static_cast<uint8_t>(isize >> (8 * k)));
    }
  }
}

struct SizeSource {             // element b = member b's length; the exclusive sum is its offset in the file
  const int32_t* size;
  int64_t* coff;
  __device__ int64_t load(int64_t i) const { return size[i]; }
  __device__ void store(int64_t i, int64_t before, int64_t /*with*/) const { coff[i] = before; }
};

// A wave per member; wave n_blocks writes the end-of-file member and its offset.  cap: the bytes behind `out`.
__global__ __launch_bounds__(kThreads) void copy_members_kernel(const uint8_t* slots, const int32_t* size, int64_t* coff,
                                                                const int64_t* total, int64_t n_blocks, uint8_t* out,
                                                                int64_t cap) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kWavesPerGroup + static_cast<int64_t>(threadIdx.x / kWave);
  const int lane = static_cast<int>(threadIdx.x % kWave);
  if (j < n_blocks) {
    const int64_t at = coff[j];
    const int32_t n = size[j];
    if (at < 0 || n < 0 || n > bz::kSlot || at + n > cap) return;       // the host refuses the total
    // The slot is dword-aligned, the member's place in the file is not: bytes up to the first aligned address there,
    // then whole dwords put together from two aligned loads, then the bytes that are left.
    const uint8_t* src = slots + j * bz::kSlot;
    uint8_t* dst = out + at;
    const int32_t to_aligned = static_cast<int32_t>((4 - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
    const int32_t lead = to_aligned < n ? to_aligned : n;
    const int32_t words = (n - lead) / 4;
    for (int32_t k = lane; k < lead; k += kWave) dst[k] = src[k];
    const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dst4 = reinterpret_cast<uint32_t*>(dst + lead);
    const int32_t shift = 8 * (lead & 3);
    for (int32_t w = lane; w < words; w += kWave) {
      const int32_t q = (lead >> 2) + w;                // bytes lead + 4 w .. + 3 lie in dwords q and, shifted, q + 1
      uint32_t v = src4[q];
      if (shift != 0) v = (v >> shift) | (src4[q + 1] << (32 - shift));       // q + 1 is still inside the slot
      dst4[w] = v;
    }
    for (int32_t k = lead + 4 * words + lane; k < n; k += kWave) dst[k] = src[k];
  } else if (j == n_blocks) {
    const int64_t at = *total;
    if (at < 0 || at + bz::kEofBytes > cap) return;
    if (lane < bz::kEofBytes) out[at + lane] = bz::eof_byte(lane);
    if (lane == 0) coff[n_blocks] = at;
  }
}

dv_bgzf_stats& last_stats() {
  static thread_local dv_bgzf_stats stats;
  return stats;
}

// An LSB-first bit stream into bytes, whole bytes at a time.
struct HostBits {
  uint8_t* bytes;
  int64_t at = 0;               // the byte the next bits go to
  int32_t held = 0;             // bits of `acc` in use, below 8 between calls
  uint64_t acc = 0;
  void put(uint32_t value, int32_t bits) {
    acc |= static_cast<uint64_t>(value) << held;
    held += bits;
    while (held >= 8) {
      bytes[at++] = static_cast<uint8_t>(acc);
      acc >>= 8;
      held -= 8;
    }
  }
  void flush() {
    if (held > 0) bytes[at] = static_cast<uint8_t>(acc);
  }
};

struct HostScratch {
  std::vector<uint16_t> cand = std::vector<uint16_t>(bz::kBlock);
  std::vector<int32_t> head = std::vector<int32_t>(bz::kHeads);
};

// One block -> its member at `slot` (kSlot bytes) -> the member's length.
int32_t member_on_host(const uint8_t* data, int32_t n, HostScratch* s, uint8_t* slot) {
  uint16_t* cand = s->cand.data();
  int32_t* head = s->head.data();
  std::fill(s->head.begin(), s->head.end(), -1);
  uint32_t hashes[bz::kTile];
  for (int32_t base = 0; base < n; base += bz::kTile) {
    const int32_t stop = base + bz::kTile < n ? base + bz::kTile : n;
    for (int32_t i = base; i < stop; ++i) {
      cand[i] = bz::kNoCand;
      if (i + 4 > n) continue;
      hashes[i - base] = bz::hash4(data + i);
      const int32_t c = head[hashes[i - base]];
      if (c >= 0) cand[i] = static_cast<uint16_t>(c);
    }
    for (int32_t i = base; i < stop && i + 4 <= n; ++i) head[hashes[i - base]] = i;    // ascending: the largest stays
  }
  int64_t token_bits = 0;
  for (int32_t begin = 0; begin < n; begin += bz::kSeg) {
    bz::CountSink counted;
    bz::walk_segment(data, cand, begin, begin + bz::kSeg < n ? begin + bz::kSeg : n, counted);
    token_bits += counted.bits;
  }
  const bool stored = bz::keeps_bytes(token_bits, n);
  const int32_t payload = stored ? n + bz::kStoredBytes : bz::fixed_payload_bytes(token_bits);
  const int32_t member = bz::kHeadBytes + payload + bz::kTailBytes;
  std::memset(slot, 0, static_cast<size_t>(member));
  for (int k = 0; k < bz::kHeadBytes; ++k) slot[k] = bz::head_byte(k, member);
  uint8_t* p = slot + bz::kHeadBytes;
  if (stored) {
    p[0] = 1;
    p[1] = static_cast<uint8_t>(n & 0xff);
    p[2] = static_cast<uint8_t>(n >> 8);
    p[3] = static_cast<uint8_t>(~n & 0xff);
    p[4] = static_cast<uint8_t>((~n >> 8) & 0xff);
    std::memcpy(p + bz::kStoredBytes, data, static_cast<size_t>(n));
  } else {
    HostBits out{p};
    out.put(3, bz::kBlockBits);
    bz::BitSink<HostBits> sink{&out};
    for (int32_t begin = 0; begin < n; begin += bz::kSeg) {
      bz::walk_segment(data, cand, begin, begin + bz::kSeg < n ? begin + bz::kSeg : n, sink);
    }
    out.put(0, bz::kEndBits);
    out.flush();
  }
  const uint32_t crc = static_cast<uint32_t>(crc32(0L, data, static_cast<uInt>(n))), isize = static_cast<uint32_t>(n);
  for (int k = 0; k < 4; ++k) {
    p[payload + k] = static_cast<uint8_t>(crc >> (8 * k));
    p[payload + 4 + k] = static_cast<uint8_t>(isize >> (8 * k));
  }
  return member;
}

void append_eof(std::vector<uint8_t>* data) {
  for (int k = 0; k < bz::kEofBytes; ++k) data->push_back(bz::eof_byte(k));
}

int64_t stored_members(const dv_bgzf_file& f) {
  int64_t n = 0;
  for (int64_t b = 0; b < f.n_blocks; ++b) n += (f.data[static_cast<size_t>(f.block_coff[b]) + bz::kHeadBytes] & 6) == 0;
  return n;
}

}  // namespace

namespace dv {

void bgzf_compress_on_host(const uint8_t* text, int64_t n, dv_bgzf_file* out) {
  const int64_t n_blocks = (n + bz::kBlock - 1) / bz::kBlock;
  out->n_blocks = n_blocks;
  out->block_coff.assign(static_cast<size_t>(n_blocks) + 1, 0);
  std::vector<uint8_t> slots(static_cast<size_t>(n_blocks) * bz::kSlot);
  std::vector<int32_t> size(static_cast<size_t>(n_blocks));
  std::atomic<int64_t> next{0};
  auto work = [&]() {
    HostScratch scratch;
    for (;;) {
      const int64_t b = next.fetch_add(1);
      if (b >= n_blocks) return;
      const int64_t from = b * bz::kBlock;
      size[b] = member_on_host(text + from, static_cast<int32_t>(n - from < bz::kBlock ? n - from : bz::kBlock), &scratch,
                               slots.data() + b * bz::kSlot);
    }
  };
  const int64_t cores = static_cast<int64_t>(std::thread::hardware_concurrency());
  const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(cores, 8), n_blocks / 4)));
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  int64_t total = 0;
  for (int64_t b = 0; b < n_blocks; ++b) {
    out->block_coff[b] = total;
    total += size[b];
  }
  out->block_coff[n_blocks] = total;
  out->data.clear();
  out->data.reserve(static_cast<size_t>(total) + bz::kEofBytes);
  for (int64_t b = 0; b < n_blocks; ++b) {
    out->data.insert(out->data.end(), slots.begin() + b * bz::kSlot, slots.begin() + b * bz::kSlot + size[b]);
  }
  append_eof(&out->data);
}

int bgzf_compress_on_device(const char* who, const uint8_t* text, bool text_on_device, int64_t n, void* stream,
                            dv_bgzf_file* out) {
  dv_bgzf_stats& stats = last_stats();
  stats = dv_bgzf_stats();
  stats.text_bytes = n;
  if (n == 0) {
    bgzf_compress_on_host(text, 0, out);
    stats.file_bytes = static_cast<int64_t>(out->data.size());
    return DV_OK;
  }
  const size_t n_blocks = static_cast<size_t>((n + bz::kBlock - 1) / bz::kBlock);
  const size_t chunks = (n_blocks + kChunk - 1) / kChunk;
  const size_t out_cap = n_blocks * bz::kSlot + bz::kEofBytes;
  dv::Layout up;
  const size_t u_tables = up.add(sizeof(CrcTables));
  dv::Layout down;
  const size_t d_header = down.add(2 * sizeof(int64_t));     // the members' bytes, unused
  dv::Layout scratch;
  const size_t s_text = scratch.add(text_on_device ? 0 : static_cast<size_t>(n));
  const size_t s_slots = scratch.add(n_blocks * bz::kSlot);
  const size_t s_size = scratch.add(n_blocks * sizeof(int32_t));
  const size_t s_coff = scratch.add((n_blocks + 1) * sizeof(int64_t));
  const size_t s_totals = scratch.add(chunks * sizeof(int64_t));
  const size_t s_out = scratch.add(out_cap);

  static thread_local dv::RoundTrip rt;
  if (int rc = rt.begin(std::string(who) + ": no HIP device (dv_bgzf_compress is the host code)", stream, up.bytes(),
                        down.bytes(), scratch.bytes())) {
    return rc;
  }
  std::memcpy(rt.host_up<CrcTables>(u_tables), &crc_tables(), sizeof(CrcTables));
  if (int rc = rt.upload(up.bytes())) return rc;
  stats.bytes_up = static_cast<int64_t>(up.bytes());
  uint8_t* const base = static_cast<uint8_t*>(rt.d_scratch.ptr);
  const uint8_t* d_text = text;
  if (!text_on_device) {
    DV_HIP_CHECK(hipMemcpyAsync(base + s_text, text, static_cast<size_t>(n), hipMemcpyHostToDevice, rt.stream()));
    d_text = base + s_text;
    stats.bytes_up += n;
  }
  int64_t* const header = rt.dev_down<int64_t>(d_header);
  int32_t* const size = reinterpret_cast<int32_t*>(base + s_size);
  int64_t* const coff = reinterpret_cast<int64_t*>(base + s_coff);
  DV_HIP_CHECK(hipMemsetAsync(header, 0, 2 * sizeof(int64_t), rt.stream()));
  {
    dv::ProfileScope prof(dv::kProfOther, rt.stream());
    const dim3 threads(kThreads);
    const DeflateArgs args{d_text, n, rt.dev_up<const CrcTables>(u_tables), base + s_slots, size};
    hipLaunchKernelGGL(deflate_blocks_kernel, dim3(static_cast<unsigned>(n_blocks)), threads, 0, rt.stream(), args);
    DV_HIP_CHECK(hipGetLastError());
    ++stats.launches;
    const SizeSource src{size, coff};
    if (int rc = scan_on_device<Sum>(src, static_cast<int64_t>(n_blocks), reinterpret_cast<int64_t*>(base + s_totals), header,
                                     rt.stream(), &stats.launches)) {
      return rc;
    }
    const unsigned copy_groups = static_cast<unsigned>((n_blocks + 1 + kWavesPerGroup - 1) / kWavesPerGroup);
    hipLaunchKernelGGL(copy_members_kernel, dim3(copy_groups), threads, 0, rt.stream(), base + s_slots, size, coff, header,
                       static_cast<int64_t>(n_blocks), base + s_out, static_cast<int64_t>(out_cap));
    DV_HIP_CHECK(hipGetLastError());
    ++stats.launches;
  }
  // the one extra wait: the header says how much there is to fetch
  if (int rc = rt.finish(down.bytes())) return rc;
  const int64_t members = rt.host_down<int64_t>(d_header)[0];
  const int64_t least = static_cast<int64_t>(n_blocks) * (bz::kHeadBytes + bz::kTailBytes + 1);
  if (members < least || static_cast<size_t>(members) + bz::kEofBytes > out_cap) {
    return dv::fail(DV_ERR_HIP, std::string(who) + ": the device counted " + std::to_string(members) + " bytes for " +
                                    std::to_string(n_blocks) + " blocks");
  }
  out->n_blocks = static_cast<int64_t>(n_blocks);
  out->data.resize(static_cast<size_t>(members) + bz::kEofBytes);
  out->block_coff.resize(n_blocks + 1);
  DV_HIP_CHECK(hipMemcpyAsync(out->data.data(), base + s_out, out->data.size(), hipMemcpyDeviceToHost, rt.stream()));
  DV_HIP_CHECK(hipMemcpyAsync(out->block_coff.data(), coff, (n_blocks + 1) * sizeof(int64_t), hipMemcpyDeviceToHost,
                              rt.stream()));
  DV_HIP_CHECK(hipStreamSynchronize(rt.stream()));
  stats.bytes_down = static_cast<int64_t>(down.bytes() + out->data.size() + (n_blocks + 1) * sizeof(int64_t));
  stats.file_bytes = static_cast<int64_t>(out->data.size());
  stats.blocks = out->n_blocks;
  stats.stored_blocks = stored_members(*out);
  return DV_OK;
}

}  // namespace dv

extern "C" {

int dv_bgzf_params(dv_bgzf_parameters* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_bgzf_params: null");
  out->block = bz::kBlock;
  out->tile = bz::kTile;
  out->seg = bz::kSeg;
  out->hash_bits = bz::kHashBits;
  return DV_OK;
}

int dv_bgzf_compress(const void* text, int64_t n, dv_bgzf_file** out) {
  return dv::guarded("dv_bgzf_compress", [&]() -> int {
    if (out) *out = nullptr;
    if (!out || n < 0 || (!text && n > 0)) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_bgzf_compress: null pointer or negative count");
    }
    auto res = std::make_unique<dv_bgzf_file>();
    dv::bgzf_compress_on_host(static_cast<const uint8_t*>(text), n, res.get());
    *out = res.release();
    return DV_OK;
  });
}

int dv_bgzf_compress_device(const void* text, int32_t memory, int64_t n, dv_bgzf_file** out, void* stream) {
  return dv::guarded("dv_bgzf_compress_device", [&]() -> int {
    last_stats() = dv_bgzf_stats();
    if (out) *out = nullptr;
    if (!out || n < 0 || (!text && n > 0) || (memory != DV_MEM_HOST && memory != DV_MEM_DEVICE)) {
      return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_bgzf_compress_device: null pointer, negative count or unknown memory");
    }
    auto res = std::make_unique<dv_bgzf_file>();
    if (int rc = dv::bgzf_compress_on_device("dv_bgzf_compress_device", static_cast<const uint8_t*>(text),
                                             memory == DV_MEM_DEVICE, n, stream, res.get())) {
      return rc;
    }
    *out = res.release();
    return DV_OK;
  });
}

int dv_bgzf_arrays(const dv_bgzf_file* f, dv_bgzf_view* out) {
  if (!f || !out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_bgzf_arrays: null");
  out->data = f->data.data();
  out->n_bytes = static_cast<int64_t>(f->data.size());
  out->n_blocks = f->n_blocks;
  out->block_coff = f->block_coff.data();
  out->stored_blocks = stored_members(*f);
  return DV_OK;
}

void dv_bgzf_free(dv_bgzf_file* f) { delete f; }

int dv_bgzf_last_stats(dv_bgzf_stats* out) {
  if (!out) return dv::fail(DV_ERR_INVALID_ARGUMENT, "dv_bgzf_last_stats: null");
  *out = last_stats();
  return DV_OK;
}

}  // extern "C"
