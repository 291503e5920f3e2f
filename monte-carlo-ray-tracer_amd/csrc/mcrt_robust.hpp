// Firefly suppression (include/mcrt.h mcrt_render_highlights*, mcrt_robust_resolve*): the text of the two gfx950 kernels of
// mcrt_robust.hip, shared with the host emulation of the CPU tests (tests/emu/robust_emu.cpp): both run this file. Only FP64 + - * /,
// compare and select, in the order include/mcrt.h states, built uncontracted like the rest of the exact build.
//
// robustHighlightsKernel reads a pass's per-sample store, [spp][pass_pixels][3] FP64, after sampleResolveKernel and before the next pass
// overwrites it: a lane per pixel, twice over the samples. The first reading selects - the K-list of the header as K (luminance, sample
// index) pairs in named registers, every sample one fully unrolled compare-select insertion, no array that a run-time index could send
// to scratch -, the second adds up the samples that are not in the list; the list's rgb is then read from the store by index, four
// loads more. A lane's 24 B of a plane are 8-byte aligned only (odd pixels start at 8 mod 16), so a plane is three 8-byte loads per
// lane; a wave reads 1 536 consecutive bytes of a plane either way, and kHighlightsUnroll planes are loaded before the first of them is
// used, so that many loads are in flight per lane. K = 0 (fewer than 4 samples) reads once.
//
// robustResolveKernel is a lane per pixel of the gathered frame: the window's largest level, then the clamp of the pixel's own tops.
#pragma once

#include "../../include/mcrt.h"
#include "mcrt_math.hpp"

namespace mcrt {

constexpr uint32_t kHighlightsBlock = 256;   // lanes of a workgroup; each owns a pixel
constexpr uint32_t kHighlightsUnroll = 8;    // sample planes loaded before the first is used
constexpr uint32_t kRobustResolveBlock = 256;
constexpr uint32_t kRobustMaxRadius = 8;
constexpr uint32_t kHighlightsNone = 0xFFFFFFFFu;  // an empty place of the list
static_assert(MCRT_ROBUST_TOPS == 4, "the list is four named places");

MCRT_HD uint32_t robustTops(uint32_t n) { return n / 4 < MCRT_ROBUST_TOPS ? n / 4 : MCRT_ROBUST_TOPS; }
MCRT_HD double robustLuminance(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }

// One pass of a frame: `pixels` pixels of `spp` sample planes; outputs (nullptr = not wanted) already offset to the pass's first row.
struct HighlightsPass {
    const double* samples;  // [spp][pixels][3]
    uint64_t pixels;
    uint32_t spp;
    uint32_t reserved;
    double* tops;           // [pixels][MCRT_ROBUST_TOPS][3]
    double* level;          // [pixels]
};

struct HighlightsRgb {
    double r, g, b;
};
MCRT_HD HighlightsRgb highlightsLoad(const double* p) { return HighlightsRgb{p[0], p[1], p[2]}; }

// The K-list: luminance and sample index of its places, kHighlightsNone = empty (the empty places are the last ones).
struct HighlightsList {
    double l0, l1, l2, l3;
    uint32_t i0, i1, i2, i3;
};

// Sample i of luminance l goes before the first entry it exceeds, or into the first empty place; what is pushed past place K - 1 is
// dropped; a NaN never enters. b_j: "place j exists and the sample goes at or before it" - true from the insertion place on, because the
// list is sorted and its empty places are its last.
MCRT_HD void highlightsInsert(HighlightsList& t, uint32_t K, double l, uint32_t i) {
    const bool ok = l == l;
    const bool b0 = ok && K > 0 && (t.i0 == kHighlightsNone || l > t.l0);
    const bool b1 = ok && K > 1 && (t.i1 == kHighlightsNone || l > t.l1);
    const bool b2 = ok && K > 2 && (t.i2 == kHighlightsNone || l > t.l2);
    const bool b3 = ok && K > 3 && (t.i3 == kHighlightsNone || l > t.l3);
    const bool s3 = b2 && K > 3, s2 = b1 && K > 2, s1 = b0 && K > 1;  // place j takes place j - 1's entry (a place past K - 1 stays empty)
    t.l3 = s3 ? t.l2 : b3 ? l : t.l3;
    t.i3 = s3 ? t.i2 : b3 ? i : t.i3;
    t.l2 = s2 ? t.l1 : b2 ? l : t.l2;
    t.i2 = s2 ? t.i1 : b2 ? i : t.i2;
    t.l1 = s1 ? t.l0 : b1 ? l : t.l1;
    t.i1 = s1 ? t.i0 : b1 ? i : t.i1;
    t.l0 = b0 ? l : t.l0;
    t.i0 = b0 ? i : t.i0;
}

MCRT_HD void highlightsLane(const HighlightsPass& hp, uint64_t pixel) {
    if (pixel >= hp.pixels) return;
    const uint32_t n = hp.spp, K = robustTops(n);
    const uint64_t stride = hp.pixels * 3;  // words of a plane
    const double* base = hp.samples + pixel * 3;
    HighlightsList t{0.0, 0.0, 0.0, 0.0, kHighlightsNone, kHighlightsNone, kHighlightsNone, kHighlightsNone};
    uint32_t s = 0;
    if (K > 0) {
        for (; s + kHighlightsUnroll <= n; s += kHighlightsUnroll) {
            HighlightsRgb v[kHighlightsUnroll];
#pragma unroll
            for (uint32_t k = 0; k < kHighlightsUnroll; k++) v[k] = highlightsLoad(base + (uint64_t)(s + k) * stride);
#pragma unroll
            for (uint32_t k = 0; k < kHighlightsUnroll; k++) highlightsInsert(t, K, robustLuminance(v[k].r, v[k].g, v[k].b), s + k);
        }
        for (; s < n; s++) {
            const HighlightsRgb v = highlightsLoad(base + (uint64_t)s * stride);
            highlightsInsert(t, K, robustLuminance(v.r, v.g, v.b), s);
        }
    }
    if (hp.tops) {
        const HighlightsRgb zero{0.0, 0.0, 0.0};
        const HighlightsRgb e0 = t.i0 != kHighlightsNone ? highlightsLoad(base + (uint64_t)t.i0 * stride) : zero;
        const HighlightsRgb e1 = t.i1 != kHighlightsNone ? highlightsLoad(base + (uint64_t)t.i1 * stride) : zero;
        const HighlightsRgb e2 = t.i2 != kHighlightsNone ? highlightsLoad(base + (uint64_t)t.i2 * stride) : zero;
        const HighlightsRgb e3 = t.i3 != kHighlightsNone ? highlightsLoad(base + (uint64_t)t.i3 * stride) : zero;
        double* o = hp.tops + pixel * (MCRT_ROBUST_TOPS * 3);
        o[0] = e0.r, o[1] = e0.g, o[2] = e0.b;
        o[3] = e1.r, o[4] = e1.g, o[5] = e1.b;
        o[6] = e2.r, o[7] = e2.g, o[8] = e2.b;
        o[9] = e3.r, o[10] = e3.g, o[11] = e3.b;
    }
    if (!hp.level) return;
    HighlightsRgb rest{0.0, 0.0, 0.0};
    s = 0;
    for (; s + kHighlightsUnroll <= n; s += kHighlightsUnroll) {
        HighlightsRgb v[kHighlightsUnroll];
#pragma unroll
        for (uint32_t k = 0; k < kHighlightsUnroll; k++) v[k] = highlightsLoad(base + (uint64_t)(s + k) * stride);
#pragma unroll
        for (uint32_t k = 0; k < kHighlightsUnroll; k++) {
            const uint32_t i = s + k;
            const bool listed = i == t.i0 || i == t.i1 || i == t.i2 || i == t.i3;
            rest.r = listed ? rest.r : rest.r + v[k].r;
            rest.g = listed ? rest.g : rest.g + v[k].g;
            rest.b = listed ? rest.b : rest.b + v[k].b;
        }
    }
    for (; s < n; s++) {
        const HighlightsRgb v = highlightsLoad(base + (uint64_t)s * stride);
        const bool listed = s == t.i0 || s == t.i1 || s == t.i2 || s == t.i3;
        rest.r = listed ? rest.r : rest.r + v.r;
        rest.g = listed ? rest.g : rest.g + v.g;
        rest.b = listed ? rest.b : rest.b + v.b;
    }
    const double d = (double)(n - K);
    hp.level[pixel] = robustLuminance(rest.r / d, rest.g / d, rest.b / d);
}

// The resolve of a gathered frame. out may be rgb: a lane reads and writes its own pixel of them only.
struct RobustResolve {
    const double *rgb, *tops, *level;  // [height][width][3], [height][width][MCRT_ROBUST_TOPS][3], [height][width]
    double* out;                       // [height][width][3]
    double* removed;                   // [height][width][3] or nullptr
    uint32_t* clamped;                 // [height][width] or nullptr
    uint32_t width, height, spp, radius;
    double kappa, floor;
};

MCRT_HD void robustResolveLane(const RobustResolve& rr, uint64_t pixel) {
    if (pixel >= (uint64_t)rr.width * rr.height) return;
    const int32_t x = (int32_t)(pixel % rr.width), y = (int32_t)(pixel / rr.width), R = (int32_t)rr.radius;
    double M = -__builtin_huge_val();
    for (int32_t dy = -R; dy <= R; dy++) {
        const int32_t qy = y + dy;
        if (qy < 0 || qy >= (int32_t)rr.height) continue;
        for (int32_t dx = -R; dx <= R; dx++) {
            const int32_t qx = x + dx;
            if (qx < 0 || qx >= (int32_t)rr.width) continue;
            const double lq = rr.level[(uint64_t)qy * rr.width + (uint32_t)qx];
            M = M < lq ? lq : M;
        }
    }
    const double t = rr.kappa * M;
    const double T = t > rr.floor ? t : rr.floor;
    const uint32_t K = robustTops(rr.spp);
    const double* top = rr.tops + pixel * (MCRT_ROBUST_TOPS * 3);
    double rem_r = 0.0, rem_g = 0.0, rem_b = 0.0;
    uint32_t count = 0;
#pragma unroll
    for (uint32_t k = 0; k < MCRT_ROBUST_TOPS; k++) {
        if (k >= K) break;
        const double r = top[k * 3], g = top[k * 3 + 1], b = top[k * 3 + 2];
        const double l = robustLuminance(r, g, b);
        if (l > T) {
            const double f = T / l;
            rem_r = rem_r + (r - r * f);
            rem_g = rem_g + (g - g * f);
            rem_b = rem_b + (b - b * f);
            count = count + 1;
        }
    }
    const double n = (double)rr.spp;
    const double* c = rr.rgb + pixel * 3;
    const double c_r = c[0], c_g = c[1], c_b = c[2];
    const double q_r = rem_r / n, q_g = rem_g / n, q_b = rem_b / n;
    double o_r = c_r - q_r, o_g = c_g - q_g, o_b = c_b - q_b;
    o_r = o_r < 0.0 ? 0.0 : o_r;
    o_g = o_g < 0.0 ? 0.0 : o_g;
    o_b = o_b < 0.0 ? 0.0 : o_b;
    double* o = rr.out + pixel * 3;
    o[0] = count ? o_r : c_r;  // (nothing clamped: the frame's bits, a -0.0 or a negative value of a frame that is not a render's included)
    o[1] = count ? o_g : c_g;
    o[2] = count ? o_b : c_b;
    if (rr.removed) {
        double* q = rr.removed + pixel * 3;
        q[0] = q_r, q[1] = q_g, q[2] = q_b;
    }
    if (rr.clamped) rr.clamped[pixel] = count;
}

}  // namespace mcrt
