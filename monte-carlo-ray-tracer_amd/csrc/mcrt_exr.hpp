// OpenEXR output (include/mcrt.h "OpenEXR output"): the text that the pack kernel of csrc/mcrt_exr.hip runs and that tests/emu/exr_emu.cpp
// drives on the host as a loop over its lanes - the two conversions, on the bits, and the map from a byte of the packed buffer to the
// value it comes from, in file order (NONE) and in ZIP's pre-deflate order. Integer arithmetic only: no floating-point instruction, so no
// rounding or denormal mode of the device takes part.
// The packed buffer is the sequence of the chunks' payloads, chunk k at k * chunk_bytes (every chunk but the last holds lines_per_chunk
// scan lines), total_bytes in all: written as it is (NONE) or deflated chunk by chunk (ZIP) by csrc/mcrt_exr_file.hpp.
#pragma once

#include <cstdint>

#include "../../include/mcrt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MCRT_EXR_HD __host__ __device__ inline
#else
#define MCRT_EXR_HD inline
#endif

namespace mcrt {

// A channel of the sorted list. line_at: where its W values start within a scan line's bytes; bytes: 2 (HALF) or 4.
struct ExrChannelRec {
    const void* data;
    uint64_t line_at;
    uint32_t stride, offset, pixel_type, bytes;
};

struct ExrPack {
    const ExrChannelRec* table;   // [count], sorted by name, line_at ascending
    unsigned char* out;           // [total_bytes rounded up to 4]
    uint64_t line_bytes;          // W * the sum of the channels' bytes
    uint64_t chunk_bytes;         // lines_per_chunk * line_bytes
    uint64_t total_bytes;         // H * line_bytes
    uint32_t width, height, count, lines_per_chunk;
    uint32_t zip;                 // 0: file order, 1: ZIP's transformed order
    uint32_t flags;               // MCRT_EXR_HALF_INF
};

constexpr uint32_t kExrPackBlock = 256;       // lanes of a workgroup
constexpr uint32_t kExrPackWordsPerLane = 16; // 4-byte words of the packed buffer per lane: a workgroup fills 16 KiB, lane-adjacent words adjacent

// binary64 -> binary16, one rounding to nearest even. The 53-bit significand m (value m * 2^(e - 1075)) keeps 11 bits at a normal result
// (shift 42) and fewer at a subnormal one; the carry of the rounding walks into the exponent field by itself.
MCRT_EXR_HD uint32_t exrHalfBits(uint64_t b, bool keep_inf) {
    const uint32_t sign = (uint32_t)(b >> 48) & 0x8000u;
    const uint64_t a = b & 0x7FFFFFFFFFFFFFFFull;
    if (a > 0x7FF0000000000000ull) return sign | 0x7e00u;
    if (a == 0x7FF0000000000000ull) return sign | 0x7c00u;
    const int e = (int)(a >> 52);
    if (e == 0) return sign;  // zero or a binary64 subnormal: far below half of the smallest half subnormal
    const int eh = e - 1008;  // the half's exponent field, were the result normal
    const uint32_t over = keep_inf ? 0x7c00u : 0x7bffu;
    if (eh >= 31) return sign | over;
    const int shift = eh >= 1 ? 42 : 43 - eh;
    if (shift > 54) return sign;
    const uint64_t m = (a & 0x000FFFFFFFFFFFFFull) | 0x0010000000000000ull;
    uint32_t r = (uint32_t)(m >> shift);
    const uint64_t rem = m & ((1ull << shift) - 1ull), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) r++;
    const uint32_t v = (eh >= 1 ? (uint32_t)(eh - 1) << 10 : 0u) + r;
    return sign | (v >= 0x7c00u ? over : v);
}

// binary64 -> binary32, one rounding to nearest even, subnormal results kept, overflow to Inf, NaN quiet with its sign and the top of its payload
MCRT_EXR_HD uint32_t exrFloatBits(uint64_t b) {
    const uint32_t sign = (uint32_t)(b >> 32) & 0x80000000u;
    const uint64_t a = b & 0x7FFFFFFFFFFFFFFFull;
    if (a > 0x7FF0000000000000ull) return sign | 0x7fc00000u | (uint32_t)((a & 0x000FFFFFFFFFFFFFull) >> 29);
    if (a == 0x7FF0000000000000ull) return sign | 0x7f800000u;
    const int e = (int)(a >> 52);
    if (e == 0) return sign;
    const int ef = e - 896;
    if (ef >= 255) return sign | 0x7f800000u;
    const int shift = ef >= 1 ? 29 : 30 - ef;
    if (shift > 54) return sign;
    const uint64_t m = (a & 0x000FFFFFFFFFFFFFull) | 0x0010000000000000ull;
    uint32_t r = (uint32_t)(m >> shift);
    const uint64_t rem = m & ((1ull << shift) - 1ull), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) r++;
    return sign | ((ef >= 1 ? (uint32_t)(ef - 1) << 23 : 0u) + r);  // (a carry out of the top exponent gives 0x7f800000)
}

// The file's bits of channel c at pixel p
MCRT_EXR_HD uint32_t exrValueBits(const ExrChannelRec& c, uint64_t p, uint32_t flags) {
    const uint64_t at = p * c.stride + c.offset;
    if (c.pixel_type == MCRT_EXR_UINT) return ((const uint32_t*)c.data)[at];
    const uint64_t b = ((const uint64_t*)c.data)[at];
    return c.pixel_type == MCRT_EXR_HALF ? exrHalfBits(b, (flags & MCRT_EXR_HALF_INF) != 0) : exrFloatBits(b);
}

// Where a raw byte comes from: byte r of chunk k's raw bytes (scan line ascending, channel in sorted order, W values) is byte `byte`
// of channel `channel` at pixel (x, y).
struct ExrByteSource {
    uint32_t y, x, channel, byte;
};

MCRT_EXR_HD ExrByteSource exrRawSource(const ExrPack& pk, const ExrChannelRec* table, uint64_t k, uint64_t r) {
    uint64_t line, in_line;
    if ((r | pk.line_bytes) >> 32) {
        line = r / pk.line_bytes;
        in_line = r - line * pk.line_bytes;
    } else {  // (the usual case: one 32-bit division)
        line = (uint32_t)r / (uint32_t)pk.line_bytes;
        in_line = (uint32_t)r - (uint32_t)line * (uint32_t)pk.line_bytes;
    }
    uint32_t lo = 0, hi = pk.count;  // the last channel whose line_at <= in_line
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (table[mid].line_at <= in_line) lo = mid; else hi = mid;
    }
    const uint64_t rel = in_line - table[lo].line_at;
    ExrByteSource s;
    s.y = (uint32_t)(k * pk.lines_per_chunk + line);
    s.channel = lo;
    if (table[lo].bytes == 2) {
        s.x = (uint32_t)(rel >> 1);
        s.byte = (uint32_t)rel & 1u;
    } else {
        s.x = (uint32_t)(rel >> 2);
        s.byte = (uint32_t)rel & 3u;
    }
    return s;
}

MCRT_EXR_HD uint32_t exrRawByte(const ExrPack& pk, const ExrChannelRec* table, uint64_t k, uint64_t r) {
    const ExrByteSource s = exrRawSource(pk, table, k, r);
    const uint32_t v = exrValueBits(table[s.channel], (uint64_t)s.y * pk.width + s.x, pk.flags);
    return (v >> (8u * s.byte)) & 0xFFu;
}

// The raw bytes of chunk k: all of them but in the last chunk
MCRT_EXR_HD uint64_t exrChunkBytes(const ExrPack& pk, uint64_t k) {
    const uint64_t left = pk.total_bytes - k * pk.chunk_bytes;
    return left < pk.chunk_bytes ? left : pk.chunk_bytes;
}

// ZIP's byte planes: t[i] is raw[2i] in the first half and raw[2(i - h) + 1] in the second
MCRT_EXR_HD uint64_t exrZipSource(uint64_t i, uint64_t h) { return i < h ? 2 * i : 2 * (i - h) + 1; }

// Byte i of chunk k's payload. ZIP: the delta against the untransformed neighbour t[i-1], which at i = h is the last byte of the first plane.
MCRT_EXR_HD uint32_t exrPayloadByte(const ExrPack& pk, const ExrChannelRec* table, uint64_t k, uint64_t i) {
    if (!pk.zip) return exrRawByte(pk, table, k, i);
    const uint64_t h = exrChunkBytes(pk, k) >> 1;
    const uint32_t t = exrRawByte(pk, table, k, exrZipSource(i, h));
    if (i == 0) return t;
    return (t - exrRawByte(pk, table, k, exrZipSource(i - 1, h)) + 128u) & 0xFFu;
}

// The value a lane converted last: the raw bytes next to one another in a word of file order, and two apart in ZIP order, are often bytes
// of one FLOAT or HALF value, which is then located, loaded and converted once.
struct ExrLastValue {
    uint64_t k = ~0ull, first = 0;  // chunk, and the raw index of the value's byte 0
    uint32_t bytes = 0, bits = 0;
};

MCRT_EXR_HD uint32_t exrRawByteCached(const ExrPack& pk, const ExrChannelRec* table, uint64_t k, uint64_t r, ExrLastValue& last) {
    if (last.k != k || r < last.first || r - last.first >= last.bytes) {
        const ExrByteSource s = exrRawSource(pk, table, k, r);
        last.k = k;
        last.first = r - s.byte;
        last.bytes = table[s.channel].bytes;
        last.bits = exrValueBits(table[s.channel], (uint64_t)s.y * pk.width + s.x, pk.flags);
    }
    return (last.bits >> (8u * (uint32_t)(r - last.first))) & 0xFFu;
}

// Word w of the packed buffer (bytes 4w .. 4w + 3, little-endian; bytes past total_bytes are 0): exrPayloadByte of its four bytes. Within a
// chunk the t of one byte is the neighbour of the next, so a word of ZIP order takes five raw bytes, not eight.
MCRT_EXR_HD uint32_t exrPackedWord(const ExrPack& pk, const ExrChannelRec* table, uint64_t w) {
    uint64_t g = 4 * w;
    uint64_t k = g / pk.chunk_bytes, i = g - k * pk.chunk_bytes;
    uint64_t n = exrChunkBytes(pk, k), h = n >> 1;
    uint32_t word = 0, prev = 0;
    bool have_prev = false;
    ExrLastValue last;
    for (uint32_t j = 0; j < 4 && g < pk.total_bytes; j++, g++, i++) {
        if (i == n) {  // the word crosses into the next chunk
            k++;
            i = 0;
            n = exrChunkBytes(pk, k);
            h = n >> 1;
            have_prev = false;
        }
        uint32_t byte;
        if (!pk.zip) {
            byte = exrRawByteCached(pk, table, k, i, last);
        } else {
            if (i > 0 && !have_prev) prev = exrRawByteCached(pk, table, k, exrZipSource(i - 1, h), last);
            const uint32_t t = exrRawByteCached(pk, table, k, exrZipSource(i, h), last);
            byte = i == 0 ? t : (t - prev + 128u) & 0xFFu;
            prev = t;
            have_prev = true;
        }
        word |= byte << (8u * j);
    }
    return word;
}

// The words of the packed buffer
MCRT_EXR_HD uint64_t exrPackedWords(const ExrPack& pk) { return (pk.total_bytes + 3) / 4; }

// Lane `lane` of workgroup `block`: words block * 4096 + j * 256 + lane, j = 0 .. 15
MCRT_EXR_HD void exrPackLane(const ExrPack& pk, const ExrChannelRec* table, uint64_t block, uint32_t lane) {
    const uint64_t words = exrPackedWords(pk);
    const uint64_t first = block * (uint64_t)(kExrPackBlock * kExrPackWordsPerLane) + lane;
    for (uint32_t j = 0; j < kExrPackWordsPerLane; j++) {
        const uint64_t w = first + (uint64_t)j * kExrPackBlock;
        if (w >= words) return;
        ((uint32_t*)pk.out)[w] = exrPackedWord(pk, table, w);
    }
}

}  // namespace mcrt
