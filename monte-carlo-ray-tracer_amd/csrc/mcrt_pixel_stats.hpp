// Per-pixel sample statistics and the frame summary (include/mcrt.h mcrt_render_pixel_stats*, mcrt_frame_noise*): the text of the two
// gfx950 kernels of mcrt_pixel_stats.hip, shared with the host emulation of the CPU tests (tests/emu/pixel_stats_emu.cpp): both run this
// file. Only FP64 + - * /, compare and select, in the order include/mcrt.h states, built uncontracted like the rest of the exact build.
//
// pixelStatsKernel reads a pass's per-sample store, [spp][pass_pixels][3] FP64 - as far as it is concerned [spp][words] with words =
// pass_pixels * 3, every word a sum of its own - a second time after sampleResolveKernel and before the next pass overwrites it. A lane
// owns two consecutive words, so a wave reads 1 KB of a sample plane at a time, as 16-byte loads where the planes are 16-byte aligned
// (the store's base is, a plane's offset s * words * 8 only when words is even) and as pairs of 8-byte loads otherwise; kPixelStatsUnroll
// planes are loaded before the first of them is added, so that many loads are in flight per lane. Two passes over the samples: the
// sums, then the squared distances from the mean.
//
// frameNoiseKernel is one level of the header's treesum: a workgroup per block of 256 consecutive values, the pairing k with k + stride
// through LDS. Level 0 computes the two per-pixel values from the frame and its variance, the levels above reduce the block values.
#pragma once

#include "../../include/mcrt.h"
#include "mcrt_math.hpp"

namespace mcrt {

constexpr uint32_t kPixelStatsBlock = 256;   // lanes of a workgroup; each owns two words
constexpr uint32_t kPixelStatsUnroll = 8;    // sample planes loaded before the first is added (even: a batch starts at an even sample)
constexpr uint32_t kFrameNoiseBlock = 256;   // the treesum's block: values and lanes
static_assert(kPixelStatsUnroll % 2 == 0, "a batch starts at an even sample");

// One pass of a frame: `words` channel words of `spp` sample planes; outputs (nullptr = not wanted) already offset to the pass's first row.
struct PixelStatsPass {
    const double* samples;  // [spp][words]
    uint64_t words;         // pass_pixels * 3
    uint32_t spp;
    uint32_t vec;           // every plane is 16-byte aligned (pixelStatsVec): 16-byte loads
    double *variance, *half_a, *half_b;
};
inline uint32_t pixelStatsVec(const double* samples, uint64_t words) { return ((uintptr_t)samples & 15u) == 0 && (words & 1u) == 0 ? 1u : 0u; }
inline uint64_t pixelStatsLanes(uint64_t words) { return (words + 1) / 2; }

struct PixelStatsPair {
    double x, y;
};
typedef double PixelStatsVec2 __attribute__((vector_size(16)));  // (one 16-byte load)

// The two words [2 * lane, 2 * lane + 1] of sample plane `plane`; `two`: the second exists. kVec: the plane is 16-byte aligned there.
template <bool kVec>
MCRT_HD PixelStatsPair pixelStatsLoad(const double* plane, bool two) {
    PixelStatsPair v;
    if (kVec) {
        const PixelStatsVec2 q = *reinterpret_cast<const PixelStatsVec2*>(plane);
        v.x = q[0];
        v.y = q[1];
    } else {
        v.x = plane[0];
        v.y = two ? plane[1] : 0.0;
    }
    return v;
}

template <bool kVec>
MCRT_HD void pixelStatsLaneT(const PixelStatsPass& ps, uint64_t lane) {
    const uint64_t w = lane * 2;
    if (w >= ps.words) return;
    const bool two = w + 1 < ps.words;
    const uint32_t n = ps.spp;
    const double* base = ps.samples + w;
    PixelStatsPair sum{0.0, 0.0}, even{0.0, 0.0}, odd{0.0, 0.0};
    uint32_t s = 0;
    for (; s + kPixelStatsUnroll <= n; s += kPixelStatsUnroll) {
        PixelStatsPair v[kPixelStatsUnroll];
#pragma unroll
        for (uint32_t k = 0; k < kPixelStatsUnroll; k++) v[k] = pixelStatsLoad<kVec>(base + (uint64_t)(s + k) * ps.words, two);
#pragma unroll
        for (uint32_t k = 0; k < kPixelStatsUnroll; k++) {
            sum.x = sum.x + v[k].x;
            sum.y = sum.y + v[k].y;
            PixelStatsPair& half = (k & 1u) ? odd : even;
            half.x = half.x + v[k].x;
            half.y = half.y + v[k].y;
        }
    }
    for (; s < n; s++) {
        const PixelStatsPair v = pixelStatsLoad<kVec>(base + (uint64_t)s * ps.words, two);
        sum.x = sum.x + v.x;
        sum.y = sum.y + v.y;
        PixelStatsPair& half = (s & 1u) ? odd : even;
        half.x = half.x + v.x;
        half.y = half.y + v.y;
    }
    if (ps.half_a) {
        const double d = (double)((n + 1) / 2);
        ps.half_a[w] = even.x / d;
        if (two) ps.half_a[w + 1] = even.y / d;
    }
    if (ps.half_b) {
        const double d = (double)(n / 2);
        ps.half_b[w] = n > 1 ? odd.x / d : 0.0;
        if (two) ps.half_b[w + 1] = n > 1 ? odd.y / d : 0.0;
    }
    if (!ps.variance) return;
    PixelStatsPair q{0.0, 0.0};
    if (n > 1) {
        const double mx = sum.x / (double)n, my = sum.y / (double)n;
        s = 0;
        for (; s + kPixelStatsUnroll <= n; s += kPixelStatsUnroll) {
            PixelStatsPair v[kPixelStatsUnroll];
#pragma unroll
            for (uint32_t k = 0; k < kPixelStatsUnroll; k++) v[k] = pixelStatsLoad<kVec>(base + (uint64_t)(s + k) * ps.words, two);
#pragma unroll
            for (uint32_t k = 0; k < kPixelStatsUnroll; k++) {
                const double dx = v[k].x - mx, dy = v[k].y - my;
                q.x = q.x + dx * dx;
                q.y = q.y + dy * dy;
            }
        }
        for (; s < n; s++) {
            const PixelStatsPair v = pixelStatsLoad<kVec>(base + (uint64_t)s * ps.words, two);
            const double dx = v.x - mx, dy = v.y - my;
            q.x = q.x + dx * dx;
            q.y = q.y + dy * dy;
        }
        q.x = q.x / (double)(n - 1);
        q.y = q.y / (double)(n - 1);
    }
    ps.variance[w] = q.x;
    if (two) ps.variance[w + 1] = q.y;
}

MCRT_HD void pixelStatsLane(const PixelStatsPass& ps, uint64_t lane) {
    if (ps.vec) pixelStatsLaneT<true>(ps, lane);
    else pixelStatsLaneT<false>(ps, lane);
}

// One level of treesum, for the two sums at once. Level 0 (rgb != nullptr): the values are e_p and g_p of pixel p, computed from the frame
// and its variance; above it they are the block values of the level below (in_e, in_g). Block b writes out_e[b], out_g[b].
struct FrameNoiseLevel {
    const double *rgb, *variance;  // level 0: [n][3] each
    const double *in_e, *in_g;     // the levels above: [n] each
    double *out_e, *out_g;         // [frameNoiseBlocks(n)] each
    uint64_t n;
    double spp;                    // (double)spp
};
inline uint64_t frameNoiseBlocks(uint64_t n) { return (n + kFrameNoiseBlock - 1) / kFrameNoiseBlock; }
constexpr uint64_t kFrameNoiseMaxPixels = 1ull << 38;  // (2^30 workgroups at level 0: a grid the runtime takes)

#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

// One workgroup (kFrameNoiseBlock lanes, `tid` of them this one); te, tg: kFrameNoiseBlock doubles of LDS each. Every lane reaches every barrier.
__device__ __forceinline__ void frameNoiseBlock(const FrameNoiseLevel& lv, uint64_t block, uint32_t tid, double* te, double* tg) {
    const uint64_t first = block * kFrameNoiseBlock;
    const uint64_t left = lv.n - first;
    const uint32_t len = left < kFrameNoiseBlock ? (uint32_t)left : kFrameNoiseBlock;
    if (tid < len) {
        const uint64_t p = first + tid;
        if (lv.rgb) {
            const double* v = lv.variance + p * 3;
            const double* c = lv.rgb + p * 3;
            te[tid] = ((v[0] + v[1]) + v[2]) / lv.spp;
            tg[tid] = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
        } else {
            te[tid] = lv.in_e[p];
            tg[tid] = lv.in_g[p];
        }
    }
    __syncthreads();
    for (uint32_t stride = kFrameNoiseBlock / 2; stride > 0; stride >>= 1) {
        if (tid < stride && tid + stride < len) {
            te[tid] = te[tid] + te[tid + stride];
            tg[tid] = tg[tid] + tg[tid + stride];
        }
        __syncthreads();
    }
    if (tid == 0) {
        lv.out_e[block] = te[0];
        lv.out_g[block] = tg[0];
    }
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

}  // namespace mcrt
