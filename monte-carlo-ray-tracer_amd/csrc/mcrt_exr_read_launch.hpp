// The launches of the OpenEXR input: defined in csrc/mcrt_exr_read.hip (libmcrt_exr_read.so, a code object of its own), called by
// csrc/mcrt_exr_read_host.hip (libmcrt_hip.so). Each queues one kernel on `stream` (a hipStream_t) and returns the launch's hipError_t
// as an int. The geometry functions are what both the launches and the emulation (tests/emu/exr_read_emu.cpp) cut the work by.
#pragma once

#include "mcrt_exr_read.hpp"

namespace mcrt {

// Scan tiles of a chunk (of a full one: the last chunk's tiles past its bytes sum to nothing and store nothing)
inline uint64_t exrReadTilesPerChunk(uint64_t chunk_bytes) { return (chunk_bytes + kExrReadTileBytes - 1) / kExrReadTileBytes; }
// Workgroups of the tile sums and of the undo: one per (chunk, tile); 0 past what one grid holds
inline uint64_t exrReadTileBlocks(const ExrRead& rd) {
    const uint64_t blocks = (uint64_t)rd.chunks * rd.tiles_per_chunk;
    return blocks > 0x7FFFFFFFull ? 0 : blocks;
}
// Workgroups of the gather per requested channel, and in all; 0 past what one grid holds
inline uint64_t exrReadBlocksPerTarget(uint64_t pixels) { return (pixels + kExrReadBlock - 1) / kExrReadBlock; }
inline uint64_t exrReadGatherBlocks(const ExrRead& rd) {
    const uint64_t blocks = (uint64_t)rd.count * rd.blocks_per_target;
    return blocks > 0x7FFFFFFFull ? 0 : blocks;
}
// The bytes of LDS: the scan's words of a workgroup; the table of requested channels
inline uint32_t exrReadScanLds() { return kExrReadBlock / 64 * (uint32_t)sizeof(uint32_t); }
inline uint32_t exrReadGatherLds(const ExrRead& rd) { return rd.count * (uint32_t)sizeof(ExrReadTarget); }

int launchExrReadSum(void* stream, const ExrRead& rd);     // exrReadSumKernel: tile_sums[chunk][tile] = the tile's byte sum
int launchExrReadScan(void* stream, const ExrRead& rd);    // exrReadScanKernel: ... = the sum of the chunk's tiles before it
int launchExrReadUndo(void* stream, const ExrRead& rd);    // exrReadUndoKernel: plane = t of the transformed chunks
int launchExrReadGather(void* stream, const ExrRead& rd);  // exrReadGatherKernel: the destinations

}  // namespace mcrt
