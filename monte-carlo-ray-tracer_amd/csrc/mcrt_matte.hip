// ID mattes (include/mcrt.h mcrt_render_matte*, mcrt_matte_rank_device): the ranking kernels and their launch function. This translation
// unit is the whole of libmcrt_matte.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links, the way the other
// image passes are built - the device code of libmcrt_hip.so stays the render path's. The host side is csrc/mcrt_matte_host.hip.
//   matteRankKernel        a workgroup per tile of up to 16 pixels: their keys staged in LDS with lanes along pixels (mapped from
//                          surfaces on the way), then one wavefront per pixel
//   matteRankMemoryKernel  one wavefront per pixel, its keys gathered into the pass's scratch: any number of samples per pixel
// Text: mcrt_matte.hpp. The two forms give the same bits.
#include <hip/hip_runtime.h>

#include "mcrt_matte.hpp"
#include "mcrt_matte_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kMatteBlock) matteRankKernel(MatteRank mr) {
    MCRT_DYNAMIC_LDS(lds, 16);
    matteRankTileBlock(mr, blockIdx.x, threadIdx.x, (MCRT_LDS_AS uint32_t*)lds);
}

__global__ void __launch_bounds__(kMatteBlock) matteRankMemoryKernel(MatteRank mr) {
    const uint64_t p = (uint64_t)blockIdx.x * kMatteWaves + threadIdx.x / 64u;
    if (p < mr.pixels) matteRankMemoryWave(mr, (uint32_t)p, threadIdx.x % 64u);
}

}  // namespace

namespace mcrt {
int launchMatteRank(void* stream, const MatteRank& mr, int form) {
    if (form == kMatteFormTile) {
        if (mr.tile == 0 || mr.tile != matteTilePixels(mr.spp)) return (int)hipErrorInvalidValue;
        const uint32_t lds = matteTileLdsWords(mr.spp, mr.tile) * 4u;
        hipLaunchKernelGGL(matteRankKernel, dim3((mr.pixels + mr.tile - 1) / mr.tile), dim3(kMatteBlock), lds, (hipStream_t)stream, mr);
    } else {
        if (!mr.work) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(matteRankMemoryKernel, dim3((mr.pixels + kMatteWaves - 1) / kMatteWaves), dim3(kMatteBlock), 0, (hipStream_t)stream, mr);
    }
    return (int)hipGetLastError();
}
}  // namespace mcrt
