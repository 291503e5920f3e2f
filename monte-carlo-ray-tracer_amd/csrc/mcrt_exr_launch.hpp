// The launch of the OpenEXR pack: defined in csrc/mcrt_exr.hip (libmcrt_exr.so, a code object of its own), called by
// csrc/mcrt_exr_host.hip (libmcrt_hip.so). It queues one kernel on `stream` (a hipStream_t) and returns the launch's hipError_t as an
// int. exrPackGeometry is what both the launch and the emulation (tests/emu/exr_emu.cpp) cut the work by.
#pragma once

#include "mcrt_exr.hpp"

namespace mcrt {

// Workgroups of kExrPackBlock lanes, kExrPackWordsPerLane words each; 0 when the buffer is empty or past what one grid holds
inline uint64_t exrPackBlocks(const ExrPack& pk) {
    const uint64_t per_block = (uint64_t)kExrPackBlock * kExrPackWordsPerLane;
    const uint64_t blocks = (exrPackedWords(pk) + per_block - 1) / per_block;
    return blocks > 0x7FFFFFFFull ? 0 : blocks;
}
// The bytes of the channel table a workgroup keeps in LDS
inline uint32_t exrPackLds(const ExrPack& pk) { return pk.count * (uint32_t)sizeof(ExrChannelRec); }

int launchExrPack(void* stream, const ExrPack& pk);

}  // namespace mcrt
