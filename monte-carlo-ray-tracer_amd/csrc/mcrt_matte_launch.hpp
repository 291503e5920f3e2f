// The launch of the ID mattes' ranking: defined in csrc/mcrt_matte.hip (libmcrt_matte.so, the pass's own code object), called by
// csrc/mcrt_matte_host.hip (libmcrt_hip.so). It queues one kernel on `stream` (a hipStream_t) and returns the launch's hipError_t as an int.
#pragma once

#include "mcrt_matte.hpp"

namespace mcrt {

// form: kMatteFormTile (mr.tile = matteTilePixels(mr.spp), not 0) or kMatteFormMemory (mr.work set).
int launchMatteRank(void* stream, const MatteRank& mr, int form);

}  // namespace mcrt
