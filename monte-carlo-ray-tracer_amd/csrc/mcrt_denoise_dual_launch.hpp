// The launches of the dual-buffer filter: defined in csrc/mcrt_denoise_dual.hip (libmcrt_denoise_dual.so, the filter's own code object),
// called by csrc/mcrt_denoise_dual_host.hip (libmcrt_hip.so). Each queues one kernel on `stream` (a hipStream_t) and returns the
// launch's hipError_t as an int.
#pragma once

#include "mcrt_denoise_dual.hpp"

namespace mcrt {

int launchDenoiseDualPrep(void* stream, const DenoiseDualFrame& f);
// tile_lanes: the lanes of the LDS-staged form's workgroup (256, 512 or 1024); 0: the plain form, one lane per pixel
int launchDenoiseDualFilter(void* stream, const DenoiseDualStep& st, uint32_t tile_lanes);

}  // namespace mcrt
