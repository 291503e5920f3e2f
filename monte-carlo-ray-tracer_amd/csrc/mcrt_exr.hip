// OpenEXR output (include/mcrt.h mcrt_exr_save*): the kernel and its launch function. This translation unit is the whole of
// libmcrt_exr.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links, the way libmcrt_accumulate.so is built -
// the device code of libmcrt_hip.so stays the render path's. The host side is csrc/mcrt_exr_host.hip, the file csrc/mcrt_exr_file.hpp.
//   exrPackKernel   a lane per 4-byte word of the packed buffer, 16 words per lane a workgroup's 256 lanes apart (dword stores, a wave's
//                   256 bytes contiguous); the channel table (at most 1024 x 32 bytes) in LDS, where every byte's binary search reads it
// Text: mcrt_exr.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_exr.hpp"
#include "mcrt_exr_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kExrPackBlock) exrPackKernel(ExrPack pk) {
    extern __shared__ uint64_t exr_table_words[];
    const uint64_t* src = (const uint64_t*)pk.table;
    const uint32_t words = pk.count * (uint32_t)(sizeof(ExrChannelRec) / 8);
    for (uint32_t i = threadIdx.x; i < words; i += kExrPackBlock) exr_table_words[i] = src[i];
    __syncthreads();
    exrPackLane(pk, (const ExrChannelRec*)exr_table_words, blockIdx.x, threadIdx.x);
}

}  // namespace

namespace mcrt {
int launchExrPack(void* stream, const ExrPack& pk) {
    static_assert(sizeof(ExrChannelRec) == 32, "the table is copied to LDS as 8-byte words");
    const uint64_t blocks = exrPackBlocks(pk);
    if (blocks == 0 || pk.count == 0 || pk.count > MCRT_EXR_MAX_CHANNELS) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(exrPackKernel, dim3((uint32_t)blocks), dim3(kExrPackBlock), exrPackLds(pk), (hipStream_t)stream, pk);
    return (int)hipGetLastError();
}
}  // namespace mcrt
