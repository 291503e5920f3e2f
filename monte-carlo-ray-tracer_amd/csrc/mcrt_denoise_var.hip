// Variance-guided denoised output (include/mcrt.h mcrt_denoise_variance*): the kernels of the filter and their launch functions. This
// translation unit is the whole of libmcrt_denoise_var.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links,
// the way libmcrt_denoise.so is built - the device code of libmcrt_hip.so stays the render path's. The host side is
// csrc/mcrt_denoise_var_host.hip.
//   denoiseVarPrepKernel   one lane per pixel: guides packed into 80-byte records; beauty / albedo factor and the 3 x 3 prefiltered
//                          variance of the mean into the first {I, V} frame
//   denoiseVarPlainKernel  an iteration, one lane per pixel, the 25 taps from memory
//   denoiseVarTileKernel   an iteration, a workgroup per 16 x 16 tile of one residue class of the step, the taps from LDS (51 200 B)
// The last iteration of either form multiplies the albedo factor back in and writes the caller's frames. Text: mcrt_denoise_var.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_denoise_var.hpp"
#include "mcrt_atrous_launch.hpp"
#include "mcrt_denoise_var_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kDenoiseBlock) denoiseVarPrepKernel(DenoiseVarFrame f) {
    const uint64_t p = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (p < (uint64_t)f.width * f.height) denoiseVarPrepPixel(f, p);
}

__global__ void __launch_bounds__(kDenoiseBlock) denoiseVarPlainKernel(DenoiseVarStep st) {
    const uint64_t p = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (p < (uint64_t)st.width * st.height) denoiseVarPlainPixel(st, p);
}

__global__ void __launch_bounds__(kDenoiseBlock) denoiseVarTileKernel(DenoiseVarStep st) {
    __shared__ double tile[kDenoiseVarTileWords];
    denoiseVarTileBlock(st, blockIdx.x, threadIdx.x, tile);
}

}  // namespace

namespace mcrt {
int launchDenoiseVarPrep(void* stream, const DenoiseVarFrame& f) {
    hipLaunchKernelGGL(denoiseVarPrepKernel, dim3(denoisePixelBlocks(f.width, f.height)), dim3(kDenoiseBlock), 0, (hipStream_t)stream, f);
    return (int)hipGetLastError();
}
int launchDenoiseVarStep(void* stream, const DenoiseVarStep& st, bool tile) {
    return launchAtrousStep<DenoiseVarStep, denoiseVarTileKernel, denoiseVarPlainKernel>(stream, st, tile);
}
}  // namespace mcrt
