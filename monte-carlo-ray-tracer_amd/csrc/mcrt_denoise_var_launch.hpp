// The launches of the variance-guided a-trous filter: defined in csrc/mcrt_denoise_var.hip (libmcrt_denoise_var.so, the filter's own code
// object), called by csrc/mcrt_denoise_var_host.hip (libmcrt_hip.so). Each queues one kernel on `stream` (a hipStream_t) and returns the
// launch's hipError_t as an int.
#pragma once

#include "mcrt_denoise_var.hpp"

namespace mcrt {

int launchDenoiseVarPrep(void* stream, const DenoiseVarFrame& f);
int launchDenoiseVarStep(void* stream, const DenoiseVarStep& st, bool tile);  // tile: the LDS-staged form, else one lane per pixel

}  // namespace mcrt
