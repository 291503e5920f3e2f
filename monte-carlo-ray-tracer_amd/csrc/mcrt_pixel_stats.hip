// Per-pixel sample statistics and the frame summary (include/mcrt.h mcrt_render_pixel_stats*, mcrt_frame_noise*): the two kernels and
// their launch functions. This translation unit is the whole of libmcrt_pixel_stats.so, which libmcrt_hip.so (and its tolerance twin:
// the same exact object) links, the way libmcrt_aov.so and libmcrt_denoise.so are built - the device code of libmcrt_hip.so stays the
// render path's. The host side is csrc/mcrt_pixel_stats_host.hip; the launch of a pass sits in the pass loops of csrc/mcrt_hip.hip.
//   pixelStatsKernel   a lane per two channel words of a pass's per-sample store: variance and the two half-buffers
//   frameNoiseKernel   one level of the summary's tree sum, a workgroup per block of 256 values
// Text: mcrt_pixel_stats.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_pixel_stats.hpp"
#include "mcrt_pixel_stats_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kPixelStatsBlock) pixelStatsKernel(PixelStatsPass ps) {
    pixelStatsLane(ps, (uint64_t)blockIdx.x * kPixelStatsBlock + threadIdx.x);
}

__global__ void __launch_bounds__(kFrameNoiseBlock) frameNoiseKernel(FrameNoiseLevel lv) {
    __shared__ double te[kFrameNoiseBlock], tg[kFrameNoiseBlock];
    frameNoiseBlock(lv, blockIdx.x, threadIdx.x, te, tg);
}

}  // namespace

namespace mcrt {
int launchPixelStats(void* stream, const PixelStatsPass& ps) {
    const uint64_t blocks = (pixelStatsLanes(ps.words) + kPixelStatsBlock - 1) / kPixelStatsBlock;
    if (blocks == 0) return (int)hipSuccess;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(pixelStatsKernel, dim3((uint32_t)blocks), dim3(kPixelStatsBlock), 0, (hipStream_t)stream, ps);
    return (int)hipGetLastError();
}
int launchFrameNoiseLevel(void* stream, const FrameNoiseLevel& lv) {
    const uint64_t blocks = frameNoiseBlocks(lv.n);
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(frameNoiseKernel, dim3((uint32_t)blocks), dim3(kFrameNoiseBlock), 0, (hipStream_t)stream, lv);
    return (int)hipGetLastError();
}
}  // namespace mcrt
