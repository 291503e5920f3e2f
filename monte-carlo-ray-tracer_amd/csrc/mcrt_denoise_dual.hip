// Dual-buffer denoised output (include/mcrt.h mcrt_denoise_dual*): the kernels of the filter and their launch functions. This
// translation unit is the whole of libmcrt_denoise_dual.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links,
// the way libmcrt_denoise_var.so is built - the device code of libmcrt_hip.so stays the render path's. The host side is
// csrc/mcrt_denoise_dual_host.hip.
//   denoiseDualPrepKernel   one lane per pixel: the 3 x 3 prefiltered variance, then {A, B, V0} packed into one 72-byte record
//   denoiseDualPlainKernel  the filter, one lane per pixel, the definition as written, records from memory
//   denoiseDualTileKernel   the filter, a workgroup per 16 x 16 tile: records, per-offset patch terms and row sums in dynamic LDS,
//                           denoiseDualTileLdsBytes(R, F) of it (above 64 KiB from R + F = 5 on: the launch raises the kernel's limit)
// Text: mcrt_denoise_dual.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_denoise_dual.hpp"
#include "mcrt_denoise_dual_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kDenoiseBlock) denoiseDualPrepKernel(DenoiseDualFrame f) {
    const uint64_t p = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (p < (uint64_t)f.width * f.height) denoiseDualPrepPixel(f, p);
}

__global__ void __launch_bounds__(kDenoiseBlock) denoiseDualPlainKernel(DenoiseDualStep st) {
    const uint64_t p = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (p < (uint64_t)st.width * st.height) denoiseDualPlainPixel(st, p);
}

__global__ void __launch_bounds__(kDenoiseDualTileMaxLanes) denoiseDualTileKernel(DenoiseDualStep st) {
    MCRT_DYNAMIC_LDS(lds, 16);
    denoiseDualTileBlock(st, blockIdx.x, threadIdx.x, blockDim.x, reinterpret_cast<double*>(lds));
}

uint32_t pixelBlocks(uint32_t width, uint32_t height) { return (uint32_t)(((uint64_t)width * height + kDenoiseBlock - 1) / kDenoiseBlock); }

}  // namespace

namespace mcrt {
int launchDenoiseDualPrep(void* stream, const DenoiseDualFrame& f) {
    hipLaunchKernelGGL(denoiseDualPrepKernel, dim3(pixelBlocks(f.width, f.height)), dim3(kDenoiseBlock), 0, (hipStream_t)stream, f);
    return (int)hipGetLastError();
}
int launchDenoiseDualFilter(void* stream, const DenoiseDualStep& st, uint32_t tile_lanes) {
    if (!tile_lanes) {
        hipLaunchKernelGGL(denoiseDualPlainKernel, dim3(pixelBlocks(st.width, st.height)), dim3(kDenoiseBlock), 0, (hipStream_t)stream, st);
        return (int)hipGetLastError();
    }
    // the limit is state of the kernel FUNCTION, shared by every context of the process: always the same value, so no launch can find
    // it lower than it needs
    if (hipError_t e = hipFuncSetAttribute((const void*)denoiseDualTileKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDenoiseDualTileLdsMaxBytes)) return (int)e;
    const uint32_t lds = denoiseDualTileLdsBytes(st.window_radius, st.patch_radius);
    hipLaunchKernelGGL(denoiseDualTileKernel, dim3((uint32_t)denoiseDualTileBlocks(st.width, st.height)), dim3(tile_lanes), lds, (hipStream_t)stream, st);
    return (int)hipGetLastError();
}
}  // namespace mcrt
