// What bgzf.hip offers the other translation units of libdvhip.so: the file handle of include/dvhip.h and the two
// compressors behind dv_bgzf_compress[_device], for gvcf_rows.hip, whose text lies on the device already.
#ifndef DV_BGZF_INTERNAL_H_
#define DV_BGZF_INTERNAL_H_

#include <cstdint>
#include <vector>

#include "dv_internal.h"

struct dv_bgzf_file {
  std::vector<uint8_t> data;            // the members and the end-of-file member
  std::vector<int64_t> block_coff;      // [n_blocks + 1]: every member's offset, the end-of-file member's last
  int64_t n_blocks = 0;
  std::vector<int64_t> row_off;         // dv_gvcf_rows_bgzf[_device] with want_row_off: the view of its meta
};

namespace dv {

// text[0 .. n) -> *out, on the host.  n >= 0.
void bgzf_compress_on_host(const uint8_t* text, int64_t n, dv_bgzf_file* out);

// The same on the device; `text` is read where it lies (device memory must stay valid on `stream`).  Resets and fills
// the calling thread's dv_bgzf_last_stats.  n == 0 needs no device.
int bgzf_compress_on_device(const char* who, const uint8_t* text, bool text_on_device, int64_t n, void* stream,
                            dv_bgzf_file* out);

}  // namespace dv

#endif  // DV_BGZF_INTERNAL_H_
