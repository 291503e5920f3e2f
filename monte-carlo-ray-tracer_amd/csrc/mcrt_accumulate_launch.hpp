// The launch of the frame merge: defined in csrc/mcrt_accumulate.hip (libmcrt_accumulate.so, a code object of its own), called by
// csrc/mcrt_accumulate_host.hip (libmcrt_hip.so). It queues one kernel on `stream` (a hipStream_t) and returns the launch's hipError_t as
// an int.
#pragma once

#include "mcrt_accumulate.hpp"

namespace mcrt {

int launchFrameMerge(void* stream, const FrameMerge& fm);

}  // namespace mcrt
