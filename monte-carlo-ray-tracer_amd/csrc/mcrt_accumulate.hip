// Accumulated rendering (include/mcrt.h mcrt_frame_merge*): the kernel and its launch function. This translation unit is the whole of
// libmcrt_accumulate.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links, the way libmcrt_robust.so is built -
// the device code of libmcrt_hip.so stays the render path's. The host side, the stopping loop of mcrt_render_converged* included, is
// csrc/mcrt_accumulate_host.hip.
//   frameMergeKernel   a lane per pixel: the summaries of two sample sets in, the summary of their concatenation out
// Text: mcrt_accumulate.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_accumulate.hpp"
#include "mcrt_accumulate_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kFrameMergeBlock) frameMergeKernel(FrameMerge fm) {
    frameMergeLane(fm, (uint64_t)blockIdx.x * kFrameMergeBlock + threadIdx.x);
}

}  // namespace

namespace mcrt {
int launchFrameMerge(void* stream, const FrameMerge& fm) {
    const uint64_t blocks = (fm.pixels + kFrameMergeBlock - 1) / kFrameMergeBlock;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(frameMergeKernel, dim3((uint32_t)blocks), dim3(kFrameMergeBlock), 0, (hipStream_t)stream, fm);
    return (int)hipGetLastError();
}
}  // namespace mcrt
