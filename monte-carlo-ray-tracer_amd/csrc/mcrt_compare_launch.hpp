// The launches of the frame comparison: defined in csrc/mcrt_compare.hip (libmcrt_compare.so, the pass's own code object), called by
// csrc/mcrt_compare_host.hip (libmcrt_hip.so). Each queues one kernel on `stream` (a hipStream_t) and returns the launch's hipError_t as an int.
#pragma once

#include "mcrt_compare.hpp"

namespace mcrt {

int launchComparePixels(void* stream, const ComparePixels& cp);
int launchCompareLevel(void* stream, const CompareLevel& lv);
int launchCompareSsim(void* stream, const CompareSsim& cs);  // a frame with centres only

}  // namespace mcrt
