// Denoised output (include/mcrt.h mcrt_denoise*): the kernels of the edge-avoiding a-trous filter and their launch functions. This
// translation unit is the whole of libmcrt_denoise.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links, the
// way libmcrt_aov.so is built - the device code of libmcrt_hip.so stays the render path's. The host side is csrc/mcrt_denoise_host.hip.
//   denoisePrepKernel   one lane per pixel: guides packed into 80-byte records, beauty / albedo factor into the first irradiance frame
//   denoisePlainKernel  an iteration, one lane per pixel, the 25 taps from memory
//   denoiseTileKernel   an iteration, a workgroup per 16 x 16 tile of one residue class of the step, the taps from LDS (41.6 KB)
// The last iteration of either form multiplies the albedo factor back in and writes the caller's frame. Text: mcrt_denoise.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_denoise.hpp"
#include "mcrt_atrous_launch.hpp"
#include "mcrt_denoise_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kDenoiseBlock) denoisePrepKernel(DenoiseFrame f) {
    const uint64_t p = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (p < (uint64_t)f.width * f.height) denoisePrepPixel(f, p);
}

__global__ void __launch_bounds__(kDenoiseBlock) denoisePlainKernel(DenoiseStep st) {
    const uint64_t p = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (p < (uint64_t)st.width * st.height) denoisePlainPixel(st, p);
}

__global__ void __launch_bounds__(kDenoiseBlock) denoiseTileKernel(DenoiseStep st) {
    __shared__ double tile[kDenoiseTileWords];
    denoiseTileBlock(st, blockIdx.x, threadIdx.x, tile);
}

}  // namespace

namespace mcrt {
int launchDenoisePrep(void* stream, const DenoiseFrame& f) {
    hipLaunchKernelGGL(denoisePrepKernel, dim3(denoisePixelBlocks(f.width, f.height)), dim3(kDenoiseBlock), 0, (hipStream_t)stream, f);
    return (int)hipGetLastError();
}
int launchDenoiseStep(void* stream, const DenoiseStep& st, bool tile) {
    return launchAtrousStep<DenoiseStep, denoiseTileKernel, denoisePlainKernel>(stream, st, tile);
}
}  // namespace mcrt
