// The launches of the a-trous filter: defined in csrc/mcrt_denoise.hip (libmcrt_denoise.so, the filter's own code object), called by
// csrc/mcrt_denoise_host.hip (libmcrt_hip.so). Each queues one kernel on `stream` (a hipStream_t) and returns the launch's hipError_t as
// an int.
#pragma once

#include "mcrt_denoise.hpp"

namespace mcrt {

int launchDenoisePrep(void* stream, const DenoiseFrame& f);
int launchDenoiseStep(void* stream, const DenoiseStep& st, bool tile);  // tile: the LDS-staged form, else one lane per pixel

}  // namespace mcrt
