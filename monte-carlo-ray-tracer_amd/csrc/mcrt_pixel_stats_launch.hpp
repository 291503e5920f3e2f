// The launches of the per-pixel sample statistics and the frame summary: defined in csrc/mcrt_pixel_stats.hip (libmcrt_pixel_stats.so,
// a code object of its own), called by csrc/mcrt_hip.hip (the pass loops) and csrc/mcrt_pixel_stats_host.hip (libmcrt_hip.so). Each
// queues one kernel on `stream` (a hipStream_t) and returns the launch's hipError_t as an int.
#pragma once

#include "mcrt_pixel_stats.hpp"

namespace mcrt {

int launchPixelStats(void* stream, const PixelStatsPass& ps);
int launchFrameNoiseLevel(void* stream, const FrameNoiseLevel& lv);

}  // namespace mcrt
