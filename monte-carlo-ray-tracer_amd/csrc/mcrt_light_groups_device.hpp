// What the kernels of the passes that walk live paths share (mcrt_light_groups.hip and mcrt_path_classes.hip, each a code object of its
// own; device code only): the launch shape, the tables and the refraction history in LDS, and the wave-aggregated append to a live list.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcrt_light_groups.hpp"

namespace mcrt {

constexpr uint32_t kLgBlock = 256;
constexpr uint32_t kLgGridMost = 4096;  // (the shading kernels stage 28 KB per block: a block takes several rounds of lanes)

__device__ __forceinline__ void lgStageTables(uint32_t* ltab, const uint32_t* sobol_tab) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)kSobolTableWords; i += blockDim.x) ltab[i] = sobol_tab[i];
    glibc235::stageSinCosTab();
    __syncthreads();
}

__device__ __forceinline__ RefractionHistory lgLaneHistory(double* liors) {
    RefractionHistory rh;
    rh.iors = (MCRT_LDS_AS double*)liors + threadIdx.x;
    rh.stride = kLgBlock;
    rh.size = 0;
    return rh;
}

// All lanes of the wave call this together. The survivors' samples go behind one another at the end of `list`.
__device__ __forceinline__ void lgAppendLive(uint32_t* list, uint32_t* count, bool alive, uint32_t sample) {
    const unsigned long long m = waveBallot(alive);
    if (m == 0ull) return;  // (the same for every lane)
    const uint32_t behind = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0u;
    if ((int)__lane_id() == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    if (alive) list[base + behind] = sample;
}

inline uint32_t lgGridFor(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + kLgBlock - 1) / kLgBlock, kLgGridMost); }

}  // namespace mcrt
