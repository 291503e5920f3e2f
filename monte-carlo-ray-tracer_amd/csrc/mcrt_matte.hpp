// ID mattes (include/mcrt.h "ID mattes"): the per-pixel ranking of the camera samples' keys, the Cryptomatte code of a name, and the
// checks the entry points share. The per-pixel text is what the two gfx950 kernels of mcrt_matte.hip run and what the host emulation of
// the CPU tests (tests/emu/matte_emu.cpp) runs on emulated wavefronts: both run this text.
//
// One wavefront ranks one pixel. Its n keys lie in an array `keys` (LDS in the tile form, the pass's scratch in the memory form), a
// second array `cnt` of n words beside it. Lane l owns the samples i = l, l + 64, ...:
//   claim    the distinct keys one after the other, in the order of their first appearance: a ballot over the cursor's row of 64
//            samples finds the first sample no key has claimed - a first appearance f, its key k read by all lanes (a broadcast) -,
//            then one sweep over the rows from there on compares every lane's own samples with k: the ballots' population counts add
//            up to c, the matching samples are claimed (cnt = 0), and cnt[f] = c. d distinct keys cost d x n / 64 compares a lane at
//            most: n^2 / 64 only when every sample has a key of its own.
//   rounds   `ranks` times: every lane's best owned (cnt, smallest i), a butterfly maximum of cnt over the wave, a butterfly minimum
//            of i among the lanes that hold it; the owner clears cnt[i], lane 0 writes the rank. (c descending, f ascending) is a
//            total order, so the result does not depend on which lane holds what.
// No lane reads a cnt word another lane wrote; `keys` is complete before the claiming starts (the caller's barrier). The ranking is exact
// for any number of distinct keys: nothing is bounded by a table.
#pragma once

#include "../../include/mcrt.h"
#include "mcrt_math.hpp"

namespace mcrt {

constexpr uint32_t kMatteNoKey = 0xFFFFFFFFu;
constexpr uint32_t kMatteBlock = 256;                  // 4 wavefronts, one pixel each at a time
constexpr uint32_t kMatteWaves = kMatteBlock / 64;
constexpr uint32_t kMatteUnclaimed = 0xFFFFFFFFu;      // a cnt word of a hit sample no key has claimed yet (a count is below kMatteMaxSamples)
constexpr uint32_t kMatteTileMaxPixels = 16;           // lanes along pixels in the staging: 64 contiguous bytes per sample row
constexpr uint32_t kMatteLdsWords = 16384;             // 64 KiB: the static limit, two workgroups per CU
constexpr uint64_t kMatteMaxSamples = 0xFFF00000ull;   // pixels * spp of one ranking (the closest-hit search's limit per launch)
enum { kMatteFormAuto = 0, kMatteFormTile = 1, kMatteFormMemory = 2 };
constexpr uint32_t kMatteTileAutoMaxSpp = 512;          // unset MCRT_MATTE_FORM: the tile form up to here (4 workgroups' LDS per CU), the memory form past it

// The pixels of a tile at spp samples per pixel: their keys and one cnt array per wavefront have to fit kMatteLdsWords. 0: the keys of
// kMatteWaves pixels do not fit (spp > 2048) - the memory form.
MCRT_HD uint32_t matteTilePixels(uint32_t spp) {
    const uint32_t fit = kMatteLdsWords / spp;  // arrays of spp words
    if (fit < 2 * kMatteWaves) return 0;
    const uint32_t t = (fit - kMatteWaves) / kMatteWaves * kMatteWaves;
    return t < kMatteTileMaxPixels ? t : kMatteTileMaxPixels;
}
MCRT_HD uint32_t matteTileLdsWords(uint32_t spp, uint32_t tile) { return (tile + kMatteWaves) * spp; }

// One ranking: `pixels` pixels of spp samples each, written at the packed pixels first_pixel + p of `out`.
struct MatteRank {
    const uint32_t* keys;   // [spp][pixels] sample-major; with `map`, the closest hits' surfaces
    const uint32_t* map;    // [num_surfaces] surface -> key, or null: the words of `keys` are the keys
    const uint32_t* codes;  // [num_keys] or null: layer not written
    uint32_t* work;         // memory form: [2][pixels][spp] - the pixels' keys, then their cnt arrays
    mcrt_matte_buffers out;
    uint64_t first_pixel;
    uint32_t pixels, spp, ranks, tile;  // tile: matteTilePixels(spp) (tile form)
};

// Record r of the ranking as a key: a miss (0xFFFFFFFF) has none.
MCRT_HD uint32_t matteKeyOf(const MatteRank& mr, uint64_t r) {
    const uint32_t s = mr.keys[r];
    return (s == kMatteNoKey || !mr.map) ? s : mr.map[s];
}

MCRT_HD float matteFloatOfBits(uint32_t bits) {
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

// Rank r of packed pixel q: key k with count c of n samples, or the empty rank (k == kMatteNoKey).
MCRT_HD void matteStoreRank(const MatteRank& mr, uint64_t q, uint32_t r, uint32_t k, uint32_t c) {
    const uint64_t at = q * mr.ranks + r;
    const bool some = k != kMatteNoKey;
    const double coverage = some ? (double)c / (double)mr.spp : 0.0;
    if (mr.out.id) mr.out.id[at] = k;
    if (mr.out.coverage) mr.out.coverage[at] = coverage;
    if (mr.out.layer && mr.codes) {
        mr.out.layer[2 * at] = some ? (double)matteFloatOfBits(mr.codes[k]) : 0.0;
        mr.out.layer[2 * at + 1] = coverage;
    }
}

// ------------------------------------------------------------------ codes and names (host)
inline uint32_t matteRotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
inline uint32_t matteMurmur3(const unsigned char* data, size_t len) {  // MurmurHash3_x86_32, seed 0
    uint32_t h = 0;
    const size_t blocks = len / 4;
    for (size_t b = 0; b < blocks; b++) {
        uint32_t k = (uint32_t)data[4 * b] | (uint32_t)data[4 * b + 1] << 8 | (uint32_t)data[4 * b + 2] << 16 | (uint32_t)data[4 * b + 3] << 24;
        k *= 0xcc9e2d51u;
        k = matteRotl(k, 15);
        k *= 0x1b873593u;
        h ^= k;
        h = matteRotl(h, 13);
        h = h * 5u + 0xe6546b64u;
    }
    const unsigned char* tail = data + 4 * blocks;
    uint32_t k = 0;
    switch (len & 3) {
        case 3: k ^= (uint32_t)tail[2] << 16;  // fall through
        case 2: k ^= (uint32_t)tail[1] << 8;   // fall through
        case 1:
            k ^= (uint32_t)tail[0];
            k *= 0xcc9e2d51u;
            k = matteRotl(k, 15);
            k *= 0x1b873593u;
            h ^= k;
    }
    h ^= (uint32_t)len;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
inline uint32_t matteCodeOf(const unsigned char* data, size_t len) {
    uint32_t h = matteMurmur3(data, len);
    const uint32_t e = (h >> 23) & 255u;
    if (e == 0u || e == 255u) h ^= 1u << 23;
    return h;
}
// A key's name: 1 .. 255 bytes of printable ASCII.
inline bool matteNameOk(const char* name) {
    if (!name) return false;
    size_t len = 0;
    for (; name[len]; len++)
        if (len >= 255 || (unsigned char)name[len] < 0x20 || (unsigned char)name[len] > 0x7e) return false;
    return len >= 1;
}
inline const char* matteDefaultNameFormat(uint32_t key) { return key == MCRT_MATTE_SURFACE ? "surface%u" : key == MCRT_MATTE_CUSTOM ? "key%u" : "material%u"; }
// ranks as the entry points take it (0 = the default); nullptr when it is fine
inline const char* matteRanksError(uint32_t ranks) {
    return (ranks < 2 || ranks > MCRT_MATTE_MAX_RANKS || (ranks & 1u)) ? "ranks must be even and 2 .. 16" : nullptr;
}

#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

__device__ __forceinline__ uint32_t matteWaveMax(uint32_t v) {
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t matteWaveMin(uint32_t v) {
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

// One wavefront (all 64 lanes, `lane` of them this one) ranks packed pixel q from its n = mr.spp keys in keys[0 .. n), complete and
// visible to every lane; cnt[0 .. n) is the wavefront's own. KP: a pointer to uint32_t in LDS or in memory.
template <class KP>
__device__ __forceinline__ void matteRankPixel(const MatteRank& mr, uint64_t q, uint32_t lane, KP keys, KP cnt) {
    const uint32_t n = mr.spp, rows = (n + 63u) / 64u;
    for (uint32_t j = 0; j < rows; j++) {
        const uint32_t i = 64u * j + lane;
        if (i < n) cnt[i] = keys[i] != kMatteNoKey ? kMatteUnclaimed : 0u;
    }
    // the distinct keys in the order of their first appearance: every sample before the cursor's first unclaimed one is claimed
    uint32_t distinct = 0;
    for (uint32_t row = 0; row < rows;) {
        const uint32_t i0 = 64u * row + lane;
        const unsigned long long open = waveBallot(i0 < n && cnt[i0] == kMatteUnclaimed);
        if (!open) {
            row++;
            continue;
        }
        const uint32_t f = 64u * row + (uint32_t)__ffsll((long long)open) - 1u;
        const uint32_t k = keys[f];
        uint32_t c = 0;
        for (uint32_t j = row; j < rows; j++) {  // (a sample claimed before has another key, a miss has none)
            const uint32_t i = 64u * j + lane;
            const bool eq = i < n && keys[i] == k;
            c += (uint32_t)__popcll(waveBallot(eq));
            if (eq) cnt[i] = 0u;
        }
        if ((f & 63u) == lane) cnt[f] = c;
        distinct++;
    }
    if (lane == 0 && mr.out.distinct) mr.out.distinct[q] = distinct;
    for (uint32_t r = 0; r < mr.ranks; r++) {
        uint32_t best_c = 0u, best_i = kMatteNoKey;
        if (r < distinct)  // (uniform over the wave)
            for (uint32_t i = lane; i < n; i += 64u) {
                const uint32_t v = cnt[i];
                if (v > best_c) {
                    best_c = v;
                    best_i = i;
                }
            }
        const uint32_t top = matteWaveMax(best_c);
        const uint32_t win = matteWaveMin(best_c == top && top != 0u ? best_i : kMatteNoKey);
        if (win != kMatteNoKey && (win & 63u) == lane) cnt[win] = 0u;
        if (lane == 0) matteStoreRank(mr, q, r, win != kMatteNoKey ? keys[win] : kMatteNoKey, top);
    }
}

// Tile form: workgroup `block` of kMatteBlock lanes (`tid` this one) ranks the pixels [block * tile, block * tile + tile) of the ranking.
// lds: matteTileLdsWords(spp, tile) words - the tile's keys [pixel][sample], then one cnt array per wavefront. The staging reads with
// lanes along the tile's pixels - a sample row of the tile is contiguous in memory - and maps surfaces to keys on the way.
__device__ __forceinline__ void matteRankTileBlock(const MatteRank& mr, uint32_t block, uint32_t tid, MCRT_LDS_AS uint32_t* lds) {
    const uint32_t p0 = block * mr.tile;
    const uint32_t tile = mr.pixels - p0 < mr.tile ? mr.pixels - p0 : mr.tile;
    for (uint32_t e = tid; e < mr.spp * tile; e += kMatteBlock) {
        const uint32_t i = e / tile, px = e % tile;
        lds[px * mr.spp + i] = matteKeyOf(mr, (uint64_t)i * mr.pixels + p0 + px);
    }
    __syncthreads();
    const uint32_t wave = tid / 64u, lane = tid % 64u;
    MCRT_LDS_AS uint32_t* cnt = lds + (mr.tile + wave) * mr.spp;
    for (uint32_t px = wave; px < tile; px += kMatteWaves) matteRankPixel(mr, mr.first_pixel + p0 + px, lane, lds + px * mr.spp, cnt);
}

// Memory form: one wavefront ranks pixel p of the ranking from mr.work, which it first fills with the pixel's keys.
__device__ __forceinline__ void matteRankMemoryWave(const MatteRank& mr, uint32_t p, uint32_t lane) {
    uint32_t* keys = mr.work + (uint64_t)p * mr.spp;
    uint32_t* cnt = mr.work + ((uint64_t)mr.pixels + p) * mr.spp;
    for (uint32_t i = lane; i < mr.spp; i += 64u) keys[i] = matteKeyOf(mr, (uint64_t)i * mr.pixels + p);
    __threadfence_block();  // the wavefront's own stores, before any of its lanes reads them
    __builtin_amdgcn_wave_barrier();
    matteRankPixel(mr, mr.first_pixel + p, lane, keys, cnt);
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

}  // namespace mcrt
