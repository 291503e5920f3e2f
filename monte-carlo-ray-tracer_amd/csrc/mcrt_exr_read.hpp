// OpenEXR input (include/mcrt.h "OpenEXR input"): the text that the kernels of csrc/mcrt_exr_read.hip run and that
// tests/emu/exr_read_emu.cpp drives on the host - the two widenings, on the bits; the inverse of ZIP's predictor, a prefix sum of bytes
// modulo 256 cut into tiles; and the map from a (requested channel, pixel) to the bytes of its value in a transformed or a raw chunk.
// Integer arithmetic only: no floating-point instruction, so no rounding or denormal mode of the device takes part.
// What comes in is the payload buffer of csrc/mcrt_exr_read_file.hpp: chunk k's payload at k * chunk_bytes (every chunk but the last
// holds lines_per_chunk scan lines), total_bytes in all, a transformed chunk still in ZIP's order u; and a flag per chunk, 1 = transformed.
// The predictor of the transformed chunks is undone into a plane buffer of its own, chunk k's t at k * plane_pitch: a chunk of a ZIPS
// file starts at any even byte of the payload buffer, and the plane's 16-byte stores want their alignment whatever the file's widths.
#pragma once

#include <cstdint>

#include "../../include/mcrt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MCRT_EXR_READ_HD __host__ __device__ inline
#else
#define MCRT_EXR_READ_HD inline
#endif

namespace mcrt {

// A requested channel. line_at: where its W values start within a scan line's bytes; bytes: 2 (HALF) or 4. HALF and FLOAT go to
// 8-byte elements of data, UINT to 4-byte ones.
struct ExrReadTarget {
    void* data;
    uint64_t line_at;
    uint32_t stride, offset, pixel_type, bytes;
};

struct ExrRead {
    const ExrReadTarget* table;    // [count], in the caller's order
    const unsigned char* payload;  // [total_bytes, and 32 readable bytes behind], 16-byte aligned
    const uint32_t* flags;         // [chunks]: 1 = the payload is ZIP's transformed order u, 0 = raw bytes
    unsigned char* plane;          // [chunks * plane_pitch]: t of the transformed chunks, 16-byte aligned
    uint32_t* tile_sums;           // [chunks * tiles_per_chunk]: a tile's byte sum, then the sum of the tiles before it, modulo 256
    uint64_t line_bytes;           // W * the sum of ALL the file's channels' bytes
    uint64_t chunk_bytes;          // lines_per_chunk * line_bytes
    uint64_t total_bytes;          // H * line_bytes
    uint64_t plane_pitch;          // tiles_per_chunk * kExrReadTileBytes
    uint64_t pixels;               // W * H
    uint32_t width, height, count, lines_per_chunk, chunks, tiles_per_chunk;
    uint32_t blocks_per_target;    // workgroups of the gather per requested channel
    uint32_t reserved;
};

constexpr uint32_t kExrReadBlock = 256;                            // lanes of a workgroup
constexpr uint32_t kExrReadLaneBytes = 16;                         // payload bytes of a lane: one 16-byte load and store
constexpr uint32_t kExrReadTileBytes = kExrReadBlock * kExrReadLaneBytes;  // a scan tile: what one workgroup undoes

// binary16 -> binary64, exact
MCRT_EXR_READ_HD uint64_t exrHalfWiden(uint32_t h) {
    const uint64_t sign = (uint64_t)(h & 0x8000u) << 48;
    const uint32_t e = (h >> 10) & 31u, f = h & 1023u;
    if (e == 0) {
        if (f == 0) return sign;
        const uint32_t k = 31u - (uint32_t)__builtin_clz(f);
        return sign | ((uint64_t)(999u + k) << 52) | ((uint64_t)(f ^ (1u << k)) << (52u - k));
    }
    if (e == 31) return f == 0 ? sign | 0x7FF0000000000000ull : sign | 0x7FF8000000000000ull | ((uint64_t)f << 42);
    return sign | ((uint64_t)(e + 1008u) << 52) | ((uint64_t)f << 42);
}

// binary32 -> binary64, exact
MCRT_EXR_READ_HD uint64_t exrFloatWiden(uint32_t b) {
    const uint64_t sign = (uint64_t)(b & 0x80000000u) << 32;
    const uint32_t e = (b >> 23) & 255u, f = b & 0x7FFFFFu;
    if (e == 0) {
        if (f == 0) return sign;
        const uint32_t k = 31u - (uint32_t)__builtin_clz(f);
        return sign | ((uint64_t)(874u + k) << 52) | ((uint64_t)(f ^ (1u << k)) << (52u - k));
    }
    if (e == 255) return f == 0 ? sign | 0x7FF0000000000000ull : sign | 0x7FF8000000000000ull | ((uint64_t)f << 29);
    return sign | ((uint64_t)(e + 896u) << 52) | ((uint64_t)f << 29);
}

// The raw bytes of chunk k: all of them but in the last chunk
MCRT_EXR_READ_HD uint64_t exrReadChunkBytes(const ExrRead& rd, uint64_t k) {
    const uint64_t left = rd.total_bytes - k * rd.chunk_bytes;
    return left < rd.chunk_bytes ? left : rd.chunk_bytes;
}

// The file's bits of the value whose first raw byte is byte r (even) of chunk k
MCRT_EXR_READ_HD uint32_t exrReadValueBits(const ExrRead& rd, uint64_t k, uint64_t r, uint32_t bytes) {
    if (rd.flags[k]) {  // raw[2i] = t[i], raw[2i + 1] = t[h + i]
        const unsigned char* t = rd.plane + k * rd.plane_pitch;
        const uint64_t h = exrReadChunkBytes(rd, k) >> 1, i = r >> 1;
        uint32_t v = (uint32_t)t[i] | (uint32_t)t[h + i] << 8;
        if (bytes == 4) v |= (uint32_t)t[i + 1] << 16 | (uint32_t)t[h + i + 1] << 24;
        return v;
    }
    const uint16_t* q = (const uint16_t*)(rd.payload + k * rd.chunk_bytes + r);  // (every offset here is even)
    uint32_t v = q[0];
    if (bytes == 4) v |= (uint32_t)q[1] << 16;
    return v;
}

// Lane `lane` of workgroup `block` of the gather: requested channel block / blocks_per_target, pixel (block % blocks_per_target) * 256
// + lane - x fastest across lanes - located, widened and stored as one 8-byte or 4-byte element.
MCRT_EXR_READ_HD void exrReadGatherLane(const ExrRead& rd, const ExrReadTarget* table, uint64_t block, uint32_t lane) {
    const uint32_t c = (uint32_t)(block / rd.blocks_per_target);
    const uint64_t p = (block - (uint64_t)c * rd.blocks_per_target) * kExrReadBlock + lane;
    if (c >= rd.count || p >= rd.pixels) return;
    const ExrReadTarget& tg = table[c];
    const uint32_t y = (uint32_t)p / rd.width, x = (uint32_t)p - y * rd.width;  // (pixels < 2^32)
    const uint32_t k = y / rd.lines_per_chunk, line = y - k * rd.lines_per_chunk;
    const uint64_t r = (uint64_t)line * rd.line_bytes + tg.line_at + (uint64_t)x * tg.bytes;
    const uint32_t bits = exrReadValueBits(rd, k, r, tg.bytes);
    const uint64_t at = p * tg.stride + tg.offset;
    if (tg.pixel_type == MCRT_EXR_UINT) ((uint32_t*)tg.data)[at] = bits;
    else ((uint64_t*)tg.data)[at] = tg.pixel_type == MCRT_EXR_HALF ? exrHalfWiden(bits) : exrFloatWiden(bits);
}

// Four bytes added to four bytes, each modulo 256
MCRT_EXR_READ_HD uint32_t exrReadAddBytes(uint32_t a, uint32_t b) { return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u); }

typedef uint32_t ExrReadVec4 __attribute__((vector_size(16)));  // (one 16-byte load or store)

// The 16 payload bytes of chunk k from byte `at` of it (a multiple of 16) on, as four little-endian words; bytes at and past the
// chunk's n read as 0. The chunk starts at an even byte of the payload buffer: a start that is no multiple of 16 takes five aligned
// words and shifts.
MCRT_EXR_READ_HD void exrReadLaneWords(const ExrRead& rd, uint64_t k, uint64_t n, uint64_t at, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (at >= n) return;
    const uint64_t a = k * rd.chunk_bytes + at;
    const uint32_t* words = (const uint32_t*)rd.payload + (a >> 2);
    if ((a & 15u) == 0) {
        const ExrReadVec4 q = *(const ExrReadVec4*)words;
        w[0] = q[0], w[1] = q[1], w[2] = q[2], w[3] = q[3];
    } else {
        const uint32_t sh = ((uint32_t)a & 3u) * 8u;  // 0 or 16
        uint32_t in[5];
        for (uint32_t j = 0; j < 5; j++) in[j] = words[j];
        for (uint32_t j = 0; j < 4; j++) w[j] = sh ? (in[j] >> sh) | (in[j + 1] << (32u - sh)) : in[j];
    }
    const uint64_t left = n - at;  // even, >= 2
    for (uint32_t j = 0; j < 4; j++) {
        const uint64_t have = left > 4u * j ? left - 4u * j : 0;
        if (have < 4) w[j] &= have == 0 ? 0u : 0xFFFFu;
    }
}

#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

// Inclusive sum over the 64 lanes of a wave: four steps within the rows of 16, then the rows' last lanes into the rows behind them
__device__ __forceinline__ uint32_t exrReadWaveScan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1, 0 where the row has no such lane
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast31 -> rows 2, 3
    return v;
}

// Inclusive sum over the kExrReadBlock lanes of a workgroup and, in *total, the sum of all of them. lds: kExrReadBlock / 64 words.
// Every lane of the workgroup calls it.
__device__ __forceinline__ uint32_t exrReadBlockScan(uint32_t v, uint32_t tid, uint32_t* lds, uint32_t* total) {
    const uint32_t inclusive = exrReadWaveScan(v);
    __syncthreads();  // (the words of a call before this one are read)
    if ((tid & 63u) == 63u) lds[tid >> 6] = inclusive;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kExrReadBlock / 64; w++) {
        const uint32_t s = lds[w];
        if (w < (tid >> 6)) before += s;
        all += s;
    }
    *total = all;
    return inclusive + before;
}

// The sum, modulo 256, of the bytes of tile `block % tiles_per_chunk` of chunk `block / tiles_per_chunk`
__device__ __forceinline__ void exrReadSumBlock(const ExrRead& rd, uint64_t block, uint32_t tid, uint32_t* lds) {
    const uint64_t k = block / rd.tiles_per_chunk, tile = block - k * rd.tiles_per_chunk;
    if (!rd.flags[k]) return;  // (the whole workgroup)
    uint32_t w[4];
    exrReadLaneWords(rd, k, exrReadChunkBytes(rd, k), tile * kExrReadTileBytes + (uint64_t)tid * kExrReadLaneBytes, w);
    uint32_t pairs = 0;  // two 16-bit sums of at most eight bytes each
    for (uint32_t j = 0; j < 4; j++) pairs += (w[j] & 0x00FF00FFu) + ((w[j] >> 8) & 0x00FF00FFu);
    uint32_t total;
    (void)exrReadBlockScan((pairs & 0xFFFFu) + (pairs >> 16), tid, lds, &total);
    if (tid == 0) rd.tile_sums[block] = total & 0xFFu;
}

// The tile sums of chunk k become the sums of the tiles before each, modulo 256
__device__ __forceinline__ void exrReadScanBlock(const ExrRead& rd, uint64_t k, uint32_t tid, uint32_t* lds) {
    if (!rd.flags[k]) return;
    uint32_t* sums = rd.tile_sums + k * rd.tiles_per_chunk;
    uint32_t carry = 0;
    for (uint32_t first = 0; first < rd.tiles_per_chunk; first += kExrReadBlock) {  // (the same trips for every lane)
        const uint32_t i = first + tid;
        const uint32_t v = i < rd.tiles_per_chunk ? sums[i] : 0u;
        uint32_t total;
        const uint32_t inclusive = exrReadBlockScan(v, tid, lds, &total);
        if (i < rd.tiles_per_chunk) sums[i] = (carry + inclusive - v) & 0xFFu;
        carry += total;
    }
}

// t of a tile: within a word and from word to word in the lane's registers, from lane to lane by the workgroup's scan, from tile
// to tile by tile_sums; t[i] = (u[0] + .. + u[i] - 128 i) mod 256, and - 128 i is + 128 at the odd bytes of a word.
__device__ __forceinline__ void exrReadUndoBlock(const ExrRead& rd, uint64_t block, uint32_t tid, uint32_t* lds) {
    const uint64_t k = block / rd.tiles_per_chunk, tile = block - k * rd.tiles_per_chunk;
    if (!rd.flags[k]) return;
    const uint64_t n = exrReadChunkBytes(rd, k), at = tile * kExrReadTileBytes + (uint64_t)tid * kExrReadLaneBytes;
    uint32_t w[4];
    exrReadLaneWords(rd, k, n, at, w);
    uint32_t run = 0;
    for (uint32_t j = 0; j < 4; j++) {
        uint32_t p = exrReadAddBytes(w[j], w[j] << 8);
        p = exrReadAddBytes(p, p << 16);
        w[j] = exrReadAddBytes(p, run * 0x01010101u);
        run = w[j] >> 24;
    }
    uint32_t total;
    const uint32_t inclusive = exrReadBlockScan(run, tid, lds, &total);
    const uint32_t base = ((rd.tile_sums[block] + inclusive - run) & 0xFFu) * 0x01010101u;
    if (at >= n) return;
    ExrReadVec4 q;
    for (uint32_t j = 0; j < 4; j++) q[j] = exrReadAddBytes(w[j], base) ^ 0x80008000u;
    *(ExrReadVec4*)(rd.plane + k * rd.plane_pitch + at) = q;
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

}  // namespace mcrt
