// A stand-alone run of the BGZF host code (csrc/bgzf_deflate.h through dv_bgzf_compress) for AddressSanitizer and
// UBSan, on the CPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Ideepvariant_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/bgzf_check.cpp deepvariant_amd/csrc/bgzf.hip deepvariant_amd/csrc/common.hip -lz -o bgzf_check
//   ./bgzf_check
//
// 20,000 seeded texts (rows repeated, noise, runs of one letter; up to a little over two blocks), each walked member by
// member: the BGZF header, BSIZE, block_coff, the payload inflated alone by zlib and compared with its slice of the text,
// CRC-32 and ISIZE, the end-of-file member.  Then the length edges and the arguments the entry points refuse.  First
// every length 3..258 and every distance 1..32768 through length_code and distance_code against RFC 1951's tables
// (segments of 128 bytes never reach the long lengths, so no text would show a wrong symbol there).
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bgzf_deflate.h"
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
      std::fprintf(stderr, "bgzf_check: line %d: %s (%s)\n", __LINE__, #cond, dv_last_error()); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

const uint8_t kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

dv_bgzf_parameters params;

uint32_t le(const uint8_t* p, int n) {
  uint32_t v = 0;
  for (int k = 0; k < n; ++k) v |= static_cast<uint32_t>(p[k]) << (8 * k);
  return v;
}

// -> the stored members
int64_t check_text(const std::vector<uint8_t>& text) {
  dv_bgzf_file* file = nullptr;
  const int64_t n = static_cast<int64_t>(text.size());
  CHECK(dv_bgzf_compress(n > 0 ? text.data() : nullptr, n, &file) == DV_OK && file != nullptr);
  dv_bgzf_view v;
  CHECK(dv_bgzf_arrays(file, &v) == DV_OK);
  CHECK(v.n_blocks == (n + params.block - 1) / params.block);
  std::vector<uint8_t> plain(static_cast<size_t>(params.block) + 1);
  int64_t at = 0, stored = 0;
  for (int64_t b = 0; b < v.n_blocks; ++b) {
    CHECK(v.block_coff[b] == at && at + 26 <= v.n_bytes);
    const uint8_t* m = v.data + at;
    CHECK(m[0] == 0x1f && m[1] == 0x8b && m[2] == 8 && m[3] == 4 && le(m + 4, 4) == 0 && m[8] == 0 && m[9] == 0xff);
    CHECK(le(m + 10, 2) == 6 && m[12] == 'B' && m[13] == 'C' && le(m + 14, 2) == 2);
    const int64_t size = static_cast<int64_t>(le(m + 16, 2)) + 1;
    CHECK(size <= 65536 && at + size <= v.n_bytes);
    const int64_t from = b * params.block, want = n - from < params.block ? n - from : params.block;
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    CHECK(inflateInit2(&zs, -15) == Z_OK);
    zs.next_in = const_cast<Bytef*>(m + 18);
    zs.avail_in = static_cast<uInt>(size - 26);
    zs.next_out = plain.data();
    zs.avail_out = static_cast<uInt>(plain.size());
    const int rc = inflate(&zs, Z_FINISH);
    const int64_t got = static_cast<int64_t>(zs.total_out);
    const bool all_read = zs.avail_in == 0;
    inflateEnd(&zs);
    CHECK(rc == Z_STREAM_END && all_read && got == want);
    CHECK(std::memcmp(plain.data(), text.data() + from, static_cast<size_t>(want)) == 0);
    CHECK(le(m + size - 8, 4) == static_cast<uint32_t>(crc32(0L, text.data() + from, static_cast<uInt>(want))));
    CHECK(le(m + size - 4, 4) == static_cast<uint32_t>(want));
    stored += (m[18] & 6) == 0;
    at += size;
  }
  CHECK(v.block_coff[v.n_blocks] == at && v.n_bytes == at + 28 && std::memcmp(v.data + at, kEof, 28) == 0);
  CHECK(v.stored_blocks == stored);
  dv_bgzf_free(file);
  return stored;
}

std::vector<uint8_t> seeded_text(int64_t n) {
  static const char row[] = "chr20\t10000001\t.\tA\t<*>\t0\t.\tEND=10000042\tGT:GQ:MIN_DP:PL\t0/0:50:31:0,90,899\n";
  std::vector<uint8_t> text;
  text.reserve(static_cast<size_t>(n) + 512);
  while (static_cast<int64_t>(text.size()) < n) {
    const int64_t kind = below(4), count = 1 + below(kind == 1 ? 40 : 300);
    if (kind == 0) {
      for (int64_t k = 0; k < count; ++k) text.push_back(static_cast<uint8_t>(below(256)));
    } else if (kind == 1) {
      const int64_t skip = below(30);
      for (int64_t k = 0; k < count; ++k) text.insert(text.end(), row + skip, row + sizeof row - 1);
    } else if (kind == 2) {
      text.insert(text.end(), static_cast<size_t>(count), static_cast<uint8_t>('A' + below(4)));
    } else {                                            // an earlier stretch again, at any distance
      if (text.empty()) continue;
      const int64_t from = below(static_cast<int64_t>(text.size()));
      for (int64_t k = 0; k < count && from + k < static_cast<int64_t>(text.size()); ++k) text.push_back(text[from + k]);
    }
  }
  text.resize(static_cast<size_t>(n));
  return text;
}

}  // namespace

int main() {
  CHECK(dv_bgzf_params(&params) == DV_OK);
  CHECK(params.block > 0 && params.block + 31 <= 65536 && params.seg > 0 && params.tile > 0);
  for (int32_t len = 3; len <= 258; ++len) CHECK(dv::bz::rfc::length_is(len));
  for (int32_t dist = 1; dist <= 32768; ++dist) CHECK(dv::bz::rfc::distance_is(dist));
  int64_t stored = 0, bytes = 0;
  for (int t = 0; t < 20000; ++t) {
    // most texts are short; one in 50 passes a block's end, one in 200 two
    const int64_t most = t % 200 == 0 ? 2 * params.block + 700 : t % 50 == 0 ? params.block + 700 : 3000;
    const std::vector<uint8_t> text = seeded_text(below(most + 1));
    stored += check_text(text);
    bytes += static_cast<int64_t>(text.size());
  }
  const int64_t b = params.block, s = params.seg;
  for (int64_t n : {int64_t{0}, int64_t{1}, int64_t{3}, int64_t{4}, int64_t{5}, s - 1, s, s + 1, b - 1, b, b + 1, 2 * b + 1}) {
    check_text(seeded_text(n));
    check_text(std::vector<uint8_t>(static_cast<size_t>(n), 'A'));
    std::vector<uint8_t> noise(static_cast<size_t>(n));
    for (auto& c : noise) c = static_cast<uint8_t>(below(256));
    CHECK(check_text(noise) >= n / b);                          // a full block of noise is stored
  }
  dv_bgzf_file* file = reinterpret_cast<dv_bgzf_file*>(1);
  CHECK(dv_bgzf_compress("abc", -1, &file) == DV_ERR_INVALID_ARGUMENT && file == nullptr);
  CHECK(dv_bgzf_compress(nullptr, 3, &file) == DV_ERR_INVALID_ARGUMENT);
  CHECK(dv_bgzf_compress("abc", 3, nullptr) == DV_ERR_INVALID_ARGUMENT);
  CHECK(dv_bgzf_compress_device("abc", DV_MEM_HOST, -1, &file, nullptr) == DV_ERR_INVALID_ARGUMENT);
  CHECK(dv_bgzf_compress_device("abc", 5, 3, &file, nullptr) == DV_ERR_INVALID_ARGUMENT);
  CHECK(dv_bgzf_compress_device("abc", DV_MEM_HOST, 3, nullptr, nullptr) == DV_ERR_INVALID_ARGUMENT);
  CHECK(dv_bgzf_compress_device(nullptr, DV_MEM_HOST, 0, &file, nullptr) == DV_OK && file != nullptr);   // no device needed
  dv_bgzf_free(file);
  CHECK(dv_bgzf_arrays(nullptr, nullptr) == DV_ERR_INVALID_ARGUMENT);
  CHECK(dv_bgzf_params(nullptr) == DV_ERR_INVALID_ARGUMENT && dv_bgzf_last_stats(nullptr) == DV_ERR_INVALID_ARGUMENT);
  dv_bgzf_free(nullptr);
  std::printf("bgzf_check: 20000 texts (%lld bytes, %lld stored members), the length edges and the refused arguments: ok\n",
              static_cast<long long>(bytes), static_cast<long long>(stored));
  return 0;
}
