// The host side of "stage an image, upload it, launch, download the result, wait" as the realigner's device calls do
// it (local_align.hip, fast_pass.hip, debruijn.hip, trim_reads.hip): the layout of a staged image and a thread's
// buffers and stream.  The kernels, their launches and the ProfileScope around them stay with their files.
#ifndef DV_DEVICE_ROUND_TRIP_H_
#define DV_DEVICE_ROUND_TRIP_H_

#include "dv_internal.h"

namespace dv {

inline size_t align16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

// Bump allocator for the sections of a staged image: every section starts on a 16-byte boundary.
struct Layout {
  size_t add(size_t bytes) {            // -> the section's offset
    const size_t at = total_;
    total_ += align16(bytes);
    return at;
  }
  size_t add_last(size_t bytes) {       // the same for a last section whose end is the image's, unpadded
    const size_t at = total_;
    total_ += bytes;
    return at;
  }
  size_t bytes() const { return total_; }

 private:
  size_t total_ = 0;
};

// One calling thread's staging for one kernel family: pinned images, their device copies, device-only scratch, and a
// non-blocking stream of the thread's own for callers that pass none.  Everything grows and is reused, so there is no
// allocation in steady state.  Meant to be `static thread_local`, one instance per family: the buffers of two
// families are live at once.  There is no destructor on purpose: a thread's instance is leaked when the thread ends,
// because a HIP call from a thread-local destructor after the runtime has shut down is a crash.
struct RoundTrip {
  PinnedStage up, down;
  DeviceBuffer d_up, d_down, d_scratch;

  // Checks for a device (`no_device_message` goes with DV_ERR_NO_DEVICE), makes the current device the calling
  // thread's (the thread may not have used it yet), picks `caller_stream` or the thread's own, created on first use
  // and again after a device change, and reserves the buffers; no scratch is reserved for scratch_bytes == 0.
  int begin(const std::string& no_device_message, void* caller_stream, size_t up_bytes, size_t down_bytes,
            size_t scratch_bytes);
  hipStream_t stream() const { return stream_; }    // of the call that `begin` opened
  int upload(size_t up_bytes);                      // up -> d_up, asynchronous on stream()
  int finish(size_t down_bytes);                    // d_down -> down, then waits for the stream

  template <class T> T* host_up(size_t off) const { return reinterpret_cast<T*>(up.ptr + off); }
  template <class T> T* dev_up(size_t off) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(d_up.ptr) + off); }
  template <class T> T* dev_down(size_t off) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(d_down.ptr) + off); }
  template <class T> const T* host_down(size_t off) const { return reinterpret_cast<const T*>(down.ptr + off); }

 private:
  hipStream_t stream_ = nullptr;
  hipStream_t own_stream_ = nullptr;
  int own_stream_device_ = -1;
};

}  // namespace dv

#endif  // DV_DEVICE_ROUND_TRIP_H_
