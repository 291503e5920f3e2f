// The launch geometry of the a-trous filters' kernels (mcrt_denoise.hip, mcrt_denoise_var.hip): one lane per pixel, or the tile form's
// workgroups. Each of the two translation units instantiates launchAtrousStep with its own two iteration kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "mcrt_atrous.hpp"

namespace mcrt {

inline uint32_t denoisePixelBlocks(uint32_t width, uint32_t height) { return (uint32_t)(((uint64_t)width * height + kDenoiseBlock - 1) / kDenoiseBlock); }

// One iteration on `stream`: the tile form if asked for, unless its grid is more than the runtime takes (frames of a few rows and
// billions of columns go the plain way). Returns the launch's hipError_t as an int.
template <class Step, void (*TileKernel)(Step), void (*PlainKernel)(Step)>
int launchAtrousStep(void* stream, const Step& st, bool tile) {
    const uint64_t tiles = denoiseTileBlocks(denoiseTiling(st.width, st.height, st.step));
    if (tile && tiles <= 0x7FFFFFFFull)
        hipLaunchKernelGGL(TileKernel, dim3((uint32_t)tiles), dim3(kDenoiseBlock), 0, (hipStream_t)stream, st);
    else
        hipLaunchKernelGGL(PlainKernel, dim3(denoisePixelBlocks(st.width, st.height)), dim3(kDenoiseBlock), 0, (hipStream_t)stream, st);
    return (int)hipGetLastError();
}

}  // namespace mcrt
