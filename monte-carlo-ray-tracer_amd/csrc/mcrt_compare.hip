// Frame comparison (include/mcrt.h mcrt_frame_compare*): the three kernels and their launch functions. This translation unit is the
// whole of libmcrt_compare.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links, the way the other image
// passes are built - the device code of libmcrt_hip.so stays the render path's. The host side is csrc/mcrt_compare_host.hip.
//   comparePixelsKernel  level 0 of the tree sums: a workgroup per 256 pixels, the one read of the frames and the mask; counts, maximum, maps
//   compareLevelKernel   one upper level of the tree sums, up to four at once, and of the maximum's pairs
//   compareSsimKernel    a workgroup per tile of 32 x 16 window centres, tile and halo staged in LDS; the per-centre ssim and its map
// Text: mcrt_compare.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_compare.hpp"
#include "mcrt_compare_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kCompareBlock) comparePixelsKernel(ComparePixels cp) {
    __shared__ __align__(16) double stage[kCompareStageWords];
    comparePixelsBlock(cp, blockIdx.x, threadIdx.x, stage);
}

__global__ void __launch_bounds__(kCompareBlock) compareLevelKernel(CompareLevel lv) {
    __shared__ double t[kCompareLevelWords];
    compareLevelBlock(lv, blockIdx.x, threadIdx.x, t);
}

__global__ void __launch_bounds__(kSsimBlock) compareSsimKernel(CompareSsim cs) {
    __shared__ double lds[ssimLdsWords(kSsimTileW, kSsimTileH)];
    compareSsimBlock<kSsimTileW, kSsimTileH>(cs, blockIdx.x, threadIdx.x, lds);
}

}  // namespace

namespace mcrt {
int launchComparePixels(void* stream, const ComparePixels& cp) {
    const uint64_t blocks = compareBlocks(cp.pixels);
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(comparePixelsKernel, dim3((uint32_t)blocks), dim3(kCompareBlock), 0, (hipStream_t)stream, cp);
    return (int)hipGetLastError();
}
int launchCompareLevel(void* stream, const CompareLevel& lv) {
    const uint64_t blocks = compareLevelBlocks(lv);
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(compareLevelKernel, dim3((uint32_t)blocks), dim3(kCompareBlock), 0, (hipStream_t)stream, lv);
    return (int)hipGetLastError();
}
int launchCompareSsim(void* stream, const CompareSsim& cs) {
    const uint64_t blocks = ssimTiles(cs.width, cs.height, kSsimTileW, kSsimTileH);
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(compareSsimKernel, dim3((uint32_t)blocks), dim3(kSsimBlock), 0, (hipStream_t)stream, cs);
    return (int)hipGetLastError();
}
}  // namespace mcrt
