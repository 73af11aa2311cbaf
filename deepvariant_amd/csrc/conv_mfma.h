// conv_mfma.hip's interface: the streaming / resident / pooling MFMA convolution kernels, each behind a host
// function that picks the template instance, the grid and the dynamic LDS size from the launch arguments.
#ifndef DV_CONV_MFMA_H_
#define DV_CONV_MFMA_H_

#include "conv_common.h"

namespace dv {
namespace convk {

constexpr int kSlabChunks = 8;   // K chunks (of 16 channels) per weight slab

// LDS bytes of a whole 96-cout tile's packed weights (conv_resident_kernel, conv_pool_resident_kernel)
inline size_t resident_lds_bytes(const ConvArgs& a) {
  return static_cast<size_t>(a.n_slabs) * kSlabChunks * 3 * 32 * kChunk * 2;
}

void launch_conv(const ConvArgs& a, int nb, hipStream_t stream);                   // conv_mfma_kernel, nb = 1..4, 6
void launch_conv_resident(const ConvArgs& a, int n_cus, hipStream_t stream);       // conv_resident_kernel<3, 2>
void launch_conv_pool_resident(const ConvArgs& a, int n_cus, hipStream_t stream);  // conv_pool_resident_kernel<3>
void launch_conv_pool1x1(const ConvArgs& a, int nb, hipStream_t stream);           // conv_pool1x1_kernel, nb = 1..4, 7

}  // namespace convk
}  // namespace dv

#endif  // DV_CONV_MFMA_H_
