// The launches of the firefly suppression: defined in csrc/mcrt_robust.hip (libmcrt_robust.so, a code object of its own), called by
// csrc/mcrt_hip.hip (the pass loops) and csrc/mcrt_robust_host.hip (libmcrt_hip.so). Each queues one kernel on `stream` (a hipStream_t)
// and returns the launch's hipError_t as an int.
#pragma once

#include "mcrt_robust.hpp"

namespace mcrt {

int launchHighlights(void* stream, const HighlightsPass& hp);
int launchRobustResolve(void* stream, const RobustResolve& rr);

}  // namespace mcrt
