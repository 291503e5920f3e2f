// OpenEXR input (include/mcrt.h mcrt_exr_load*): the kernels and their launch functions. This translation unit is the whole of
// libmcrt_exr_read.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links, the way libmcrt_exr.so is built -
// the device code of libmcrt_hip.so stays the render path's, that of libmcrt_exr.so the pack's. The host side is
// csrc/mcrt_exr_read_host.hip, the file csrc/mcrt_exr_read_file.hpp.
//   exrReadSumKernel     a workgroup per (chunk, 4 KiB tile) of a transformed chunk: a lane's 16 payload bytes in one load, their sum
//                        in the lane (SWAR), across the wave (DPP) and across the waves (LDS)
//   exrReadScanKernel    a workgroup per chunk: the tile sums become the sums before each tile, 256 tiles a trip
//   exrReadUndoKernel    a workgroup per (chunk, tile): the running byte sum within the lane's four words, the lanes' totals scanned
//                        like the tile sums, one 16-byte store of t to the plane buffer per lane
//   exrReadGatherKernel  a lane per (requested channel, pixel), x fastest: the value's two or four bytes from the plane (transformed
//                        chunk) or the payload (raw chunk), widened on the bits, one 8-byte or 4-byte store; the table of requested
//                        channels (at most 1024 x 32 bytes) in LDS
// Text: mcrt_exr_read.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_exr_read.hpp"
#include "mcrt_exr_read_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kExrReadBlock) exrReadSumKernel(ExrRead rd) {
    __shared__ uint32_t lds[kExrReadBlock / 64];
    exrReadSumBlock(rd, blockIdx.x, threadIdx.x, lds);
}

__global__ void __launch_bounds__(kExrReadBlock) exrReadScanKernel(ExrRead rd) {
    __shared__ uint32_t lds[kExrReadBlock / 64];
    exrReadScanBlock(rd, blockIdx.x, threadIdx.x, lds);
}

__global__ void __launch_bounds__(kExrReadBlock) exrReadUndoKernel(ExrRead rd) {
    __shared__ uint32_t lds[kExrReadBlock / 64];
    exrReadUndoBlock(rd, blockIdx.x, threadIdx.x, lds);
}

__global__ void __launch_bounds__(kExrReadBlock) exrReadGatherKernel(ExrRead rd) {
    extern __shared__ uint64_t exr_read_table_words[];
    const uint64_t* src = (const uint64_t*)rd.table;
    const uint32_t words = rd.count * (uint32_t)(sizeof(ExrReadTarget) / 8);
    for (uint32_t i = threadIdx.x; i < words; i += kExrReadBlock) exr_read_table_words[i] = src[i];
    __syncthreads();
    exrReadGatherLane(rd, (const ExrReadTarget*)exr_read_table_words, blockIdx.x, threadIdx.x);
}

bool scanShape(const ExrRead& rd) {
    return rd.chunks != 0 && rd.tiles_per_chunk != 0 && rd.tiles_per_chunk == exrReadTilesPerChunk(rd.chunk_bytes) &&
           rd.plane_pitch == (uint64_t)rd.tiles_per_chunk * kExrReadTileBytes && exrReadTileBlocks(rd) != 0;
}

}  // namespace

namespace mcrt {

int launchExrReadSum(void* stream, const ExrRead& rd) {
    if (!scanShape(rd)) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(exrReadSumKernel, dim3((uint32_t)exrReadTileBlocks(rd)), dim3(kExrReadBlock), 0, (hipStream_t)stream, rd);
    return (int)hipGetLastError();
}

int launchExrReadScan(void* stream, const ExrRead& rd) {
    if (!scanShape(rd)) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(exrReadScanKernel, dim3(rd.chunks), dim3(kExrReadBlock), 0, (hipStream_t)stream, rd);
    return (int)hipGetLastError();
}

int launchExrReadUndo(void* stream, const ExrRead& rd) {
    if (!scanShape(rd)) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(exrReadUndoKernel, dim3((uint32_t)exrReadTileBlocks(rd)), dim3(kExrReadBlock), 0, (hipStream_t)stream, rd);
    return (int)hipGetLastError();
}

int launchExrReadGather(void* stream, const ExrRead& rd) {
    static_assert(sizeof(ExrReadTarget) == 32, "the table is copied to LDS as 8-byte words");
    const uint64_t blocks = exrReadGatherBlocks(rd);
    if (blocks == 0 || rd.count == 0 || rd.count > MCRT_EXR_MAX_CHANNELS || rd.blocks_per_target != exrReadBlocksPerTarget(rd.pixels))
        return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(exrReadGatherKernel, dim3((uint32_t)blocks), dim3(kExrReadBlock), exrReadGatherLds(rd), (hipStream_t)stream, rd);
    return (int)hipGetLastError();
}

}  // namespace mcrt
