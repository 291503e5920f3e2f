// Adaptive sampling (include/mcrt.h "Adaptive sampling"): a per-pixel stopping rule over lists of noisy pixels. The text of the gfx950
// kernels of mcrt_adaptive.hip, shared with the host emulation of the CPU tests (tests/emu/adaptive_emu.cpp): both run this file. What
// decides anything here - the batch summary, the merge, the criterion - is only FP64 + - * /, compare and select, in the order
// include/mcrt.h states, built uncontracted like the rest of the exact build.
//
// Three parts. The RULE: a lane per pixel evaluates the criterion over its window on the accumulators and writes a flag. The LIST: the
// flags compacted into the ascending list of pixels - per workgroup a ballot and a population count per wave and four words of LDS
// across the waves; across workgroups a count launch, ONE workgroup that scans the block counts, and a scatter launch: no workgroup
// waits for another. The WALK: the light groups' path walk (mcrt_light_groups.hpp) over chunks of that list - a chunk names its pixels
// through the list (AdaptiveChunk, chunkPixel) -, with one plane, and a resolve that turns a pixel's samples into the batch summary
// mcrt_render_pixel_stats would deliver and merges it into the pixel's accumulators by mcrt_frame_merge's formulas, so that no batch
// frame exists.
#pragma once

#include <cmath>

#include "mcrt_accumulate.hpp"  // mergeWeighted
#include "mcrt_light_groups.hpp"

namespace mcrt {

constexpr uint32_t kAdaptiveBlock = 256;    // lanes of a workgroup; in the rule, the list and the resolve each owns a pixel
constexpr uint32_t kAdaptiveWindowMax = 4;  // the largest Chebyshev radius of the dilation
constexpr uint32_t kAdaptiveWaves = kAdaptiveBlock / 64;
constexpr double kAdaptiveFloorFraction = 0.01;  // the default floor as a fraction of the root mean square radiance after batch 0

// A chunk of a pixel list: entries [first_pixel, first_pixel + pixels) of `list` (first_pixel counts list entries here), every listed
// pixel with all its spp samples, sample-major like a chunk of the frame. A pixel's samples are those of ITS next batch: the seed is
// global_seed + count / spp, with the count the pixel has before the chunk's resolve adds to it (a pixel is in one chunk of a batch).
struct AdaptiveChunk : AovChunk {
    const uint32_t* list;
    const uint32_t* count;  // [frame pixels]
};
MCRT_HD uint64_t chunkPixel(const AdaptiveChunk& c, uint32_t p) { return c.list[c.first_pixel + p]; }
MCRT_HD uint32_t chunkSeed(const AdaptiveChunk& c, uint32_t p) { return c.global_seed + c.count[chunkPixel(c, p)] / c.spp; }

// One listed pixel with its packed index and its seed looked up: what a lane of the camera-ray kernel holds while it goes through the
// pixel's samples, so that the list and the counts are read once per pixel, not once per sample.
struct AdaptivePixel {
    const mcrt_camera_desc& cam;
    uint64_t pixel;
    uint32_t global_seed;
};
MCRT_HD uint64_t chunkPixel(const AdaptivePixel& c, uint32_t) { return c.pixel; }
MCRT_HD uint32_t chunkSeed(const AdaptivePixel& c, uint32_t) { return c.global_seed; }

// Camera-ray kernel, pixel p of the chunk: the AOV pass's camera ray of every sample i into record i * pixels + p (sample-major).
template <bool kLdsTab>
MCRT_HD void adaptiveCameraRays(const AdaptiveChunk& c, double scene_ior, uint32_t p, SobolTab tab, double* start, double* direction) {
    const AdaptivePixel one{c.cam, chunkPixel(c, p), chunkSeed(c, p)};
    for (uint32_t i = 0; i < c.spp; i++) {
        const Ray ray = aovCameraRay<kLdsTab>(one, scene_ior, 0u, i, tab);
        const uint64_t r = (uint64_t)i * c.pixels + p;
        aovStore3(start, r, ray.start);
        aovStore3(direction, r, ray.direction);
    }
}

// The accumulators: one summary and one sample count per pixel of the frame.
struct AdaptiveFrame {
    double *rgb, *variance, *half_a, *half_b;  // [pixels][3] each
    uint32_t* count;                           // [pixels]
};

// What does not change between two batches. force: every pixel that has room for a batch is listed (fewer than min_batches so far, or no target).
struct AdaptiveRule {
    double t2, f2;  // target * target, floor * floor
    uint32_t width, height, n, max_spp, window, force;
};

// ---------------------------------------------------------------------------------------------- the settings (host and emulation)
struct AdaptiveSettings {
    double target, floor;  // floor < 0: the default, derived from the frame after batch 0
    uint32_t max_spp, min_batches, window;
};

// What the calls refuse about the parameters, and the defaults: MCRT_OK, or the status with *why set.
inline int adaptiveSettings(const mcrt_adaptive_params* p, uint32_t sqrtspp, AdaptiveSettings& s, const char** why) {
    const uint64_t n = (uint64_t)sqrtspp * sqrtspp;
    if (n == 0 || n > 0xFFFFFFFFull) return *why = "sqrtspp must be 1 .. 65535", MCRT_ERR_INVALID;
    s.target = 0.0;
    s.floor = -1.0;
    s.max_spp = n > 1024u ? (uint32_t)n : 1024u;
    s.min_batches = 1u;
    s.window = 1u;
    if (p) {
        // (the comparisons are written so that a NaN fails them)
        if (!(p->target_relative_error >= 0.0 && p->target_relative_error <= 1.7976931348623157e308))
            return *why = "target_relative_error must be finite and not negative", MCRT_ERR_INVALID;
        if (!(p->floor >= 0.0 && p->floor <= 1.7976931348623157e308)) return *why = "floor must be finite and not negative", MCRT_ERR_INVALID;
        if (p->window > kAdaptiveWindowMax && p->window != MCRT_ADAPTIVE_WINDOW_NONE) return *why = "window is more than 4", MCRT_ERR_INVALID;
        s.target = p->target_relative_error;
        if (p->floor != 0.0) s.floor = p->floor;
        if (p->max_spp != 0) s.max_spp = p->max_spp;
        if (p->min_batches != 0) s.min_batches = p->min_batches;
        if (p->window != 0) s.window = p->window == MCRT_ADAPTIVE_WINDOW_NONE ? 0u : p->window;
    }
    if (s.max_spp < n) return *why = "max_spp is less than one batch", MCRT_ERR_INVALID;
    if (sqrtspp == 1 && s.min_batches < 2) s.min_batches = 2;  // a 1-sample batch has variance 0
    return MCRT_OK;
}

// The default floor from mcrt_frame_noise's `signal` of the frame after batch 0 (treesum of r r + g g + b b): a hundredth of the root
// mean square radiance; 0 when that is not a finite number.
inline double adaptiveDefaultFloor(double signal, uint64_t pixels) {
    const double f = kAdaptiveFloorFraction * std::sqrt(signal / (double)pixels);
    return f >= 0.0 && f <= 1.7976931348623157e308 ? f : 0.0;
}

// ---------------------------------------------------------------------------------------------- the batch summary and the merge
struct AdaptiveSummary {
    d3 rgb, variance, half_a, half_b;
};

// What mcrt_render_pixel_stats delivers for a pixel whose n samples are x(0) .. x(n - 1) (each a d3), in ascending order.
template <class Sample>
MCRT_HD AdaptiveSummary adaptiveSummarize(uint32_t n, Sample x) {
    d3 sum = splat(0.0), even = splat(0.0), odd = splat(0.0);
    for (uint32_t i = 0; i < n; i++) {
        const d3 v = x(i);
        sum = sum + v;
        if (i & 1u) odd = odd + v;
        else even = even + v;
    }
    const double dn = (double)n;
    const d3 m = sum / dn;
    AdaptiveSummary s;
    s.rgb = d3{gmax(m.x, 0.0), gmax(m.y, 0.0), gmax(m.z, 0.0)};  // the render's frame: Splat::get's max(mean, 0)
    s.half_a = even / (double)((n + 1) / 2);
    s.half_b = n > 1 ? odd / (double)(n / 2) : splat(0.0);
    d3 q = splat(0.0);
    if (n > 1) {
        for (uint32_t i = 0; i < n; i++) {
            const d3 d = x(i) - m;
            q = q + d * d;
        }
        q = q / (double)(n - 1);
    }
    s.variance = q;
    return s;
}

MCRT_HD double adaptiveMergeVariance(double a, double b, double t, double m_a, double m_b, double v_a, double v_b) {
    const double d = m_b - m_a;
    const double w = (a * b) / t;
    return (((a - 1.0) * v_a + (b - 1.0) * v_b) + (d * d) * w) / (t - 1.0);
}

// The batch summary `s` of n samples into the accumulators of packed pixel q: frameMergeLane's operations (mcrt_accumulate.hpp) with
// n_a = count[q], n_b = n, in place; a pixel without samples takes the summary as it is. Then count[q] += n.
MCRT_HD void adaptiveMergePixel(const AdaptiveFrame& f, uint64_t q, const AdaptiveSummary& s, uint32_t n) {
    const uint32_t n_a = f.count[q], n_b = n;
    double* rgb = f.rgb + 3 * q;
    double* var = f.variance + 3 * q;
    double* ha = f.half_a + 3 * q;
    double* hb = f.half_b + 3 * q;
    f.count[q] = n_a + n_b;
    if (n_a == 0u) {
        rgb[0] = s.rgb.x, rgb[1] = s.rgb.y, rgb[2] = s.rgb.z;
        var[0] = s.variance.x, var[1] = s.variance.y, var[2] = s.variance.z;
        ha[0] = s.half_a.x, ha[1] = s.half_a.y, ha[2] = s.half_a.z;
        hb[0] = s.half_b.x, hb[1] = s.half_b.y, hb[2] = s.half_b.z;
        return;
    }
    const double a = (double)n_a, b = (double)n_b, t = a + b;
    const double m_r = rgb[0], m_g = rgb[1], m_b = rgb[2];
    var[0] = adaptiveMergeVariance(a, b, t, m_r, s.rgb.x, var[0], s.variance.x);
    var[1] = adaptiveMergeVariance(a, b, t, m_g, s.rgb.y, var[1], s.variance.y);
    var[2] = adaptiveMergeVariance(a, b, t, m_b, s.rgb.z, var[2], s.variance.z);
    rgb[0] = (a * m_r + b * s.rgb.x) / t;
    rgb[1] = (a * m_g + b * s.rgb.y) / t;
    rgb[2] = (a * m_b + b * s.rgb.z) / t;
    const uint32_t e_a = (n_a + 1) / 2, o_a = n_a / 2, e_b = (n_b + 1) / 2, o_b = n_b / 2;
    const bool swap = (n_a & 1u) != 0;  // the batch's even samples become odd ones
    const d3 pe = swap ? s.half_b : s.half_a, po = swap ? s.half_a : s.half_b;
    const uint32_t c_e = swap ? o_b : e_b, c_o = swap ? e_b : o_b;
    const double ha_r = ha[0], ha_g = ha[1], ha_b = ha[2], hb_r = hb[0], hb_g = hb[1], hb_b = hb[2];
    ha[0] = mergeWeighted(e_a, ha_r, c_e, pe.x);
    ha[1] = mergeWeighted(e_a, ha_g, c_e, pe.y);
    ha[2] = mergeWeighted(e_a, ha_b, c_e, pe.z);
    hb[0] = mergeWeighted(o_a, hb_r, c_o, po.x);
    hb[1] = mergeWeighted(o_a, hb_g, c_o, po.y);
    hb[2] = mergeWeighted(o_a, hb_b, c_o, po.z);
}

// Resolve kernel of the walk, pixel p of the chunk: the samples' radiances of plane 0, summarised and merged into list[first + p].
MCRT_HD void adaptiveResolvePixel(const AdaptiveChunk& c, const LgState& st, uint32_t p, const AdaptiveFrame& f) {
    const double* r = st.radiance + p;
    const uint64_t n = st.n, pixels = c.pixels;
    const AdaptiveSummary s = adaptiveSummarize(c.spp, [&](uint32_t i) {
        const uint64_t at = (uint64_t)i * pixels;
        return d3{r[at], r[n + at], r[2 * n + at]};
    });
    adaptiveMergePixel(f, chunkPixel(c, p), s, c.spp);
}

// Merge kernel of a full batch that was rendered (mcrt_render_pixel_stats_device into the frames of `batch`): pixel q of the frame.
MCRT_HD void adaptiveMergeFramePixel(const AdaptiveFrame& f, const AdaptiveFrame& batch, uint64_t q, uint32_t n) {
    AdaptiveSummary s;
    s.rgb = ld3(batch.rgb + 3 * q);
    s.variance = ld3(batch.variance + 3 * q);
    s.half_a = ld3(batch.half_a + 3 * q);
    s.half_b = ld3(batch.half_b + 3 * q);
    adaptiveMergePixel(f, q, s, n);
}

// ---------------------------------------------------------------------------------------------- the rule
MCRT_HD bool adaptiveNoisy(const AdaptiveFrame& f, const AdaptiveRule& r, uint64_t q) {
    const double* v = f.variance + 3 * q;
    const double* c = f.rgb + 3 * q;
    const double e = ((v[0] + v[1]) + v[2]) / (double)f.count[q];
    const double g = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    return g == g && e > r.t2 * (g > r.f2 ? g : r.f2);  // (a NaN e or bound fails the comparison by itself; a NaN g would select the floor)
}

// Is packed pixel q listed for the next batch?
MCRT_HD bool adaptiveListed(const AdaptiveFrame& f, const AdaptiveRule& r, uint64_t q) {
    if ((uint64_t)f.count[q] + r.n > r.max_spp) return false;
    if (r.force) return true;
    const uint32_t x = (uint32_t)(q % r.width), y = (uint32_t)(q / r.width);
    const uint32_t x0 = x > r.window ? x - r.window : 0u, y0 = y > r.window ? y - r.window : 0u;
    const uint32_t x1 = r.width - 1u - x > r.window ? x + r.window : r.width - 1u, y1 = r.height - 1u - y > r.window ? y + r.window : r.height - 1u;
    bool any = false;
    for (uint32_t yy = y0; yy <= y1; yy++)
        for (uint32_t xx = x0; xx <= x1; xx++) any = any || adaptiveNoisy(f, r, (uint64_t)yy * r.width + xx);
    return any;
}

inline uint32_t adaptiveBlocks(uint64_t pixels) { return (uint32_t)((pixels + kAdaptiveBlock - 1) / kAdaptiveBlock); }

#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

// ---------------------------------------------------------------------------------------------- the list
// One workgroup of kAdaptiveBlock lanes, `tid` of them this one, every lane of it calls this once: the place of the lane among the
// workgroup's set flags (for a lane whose flag is set) and their number. wave_sums: kAdaptiveWaves words of LDS.
__device__ __forceinline__ uint32_t adaptiveBlockRank(bool flag, uint32_t tid, uint32_t* wave_sums, uint32_t& total) {
    const unsigned long long m = waveBallot(flag);
    const uint32_t behind = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const uint32_t wave = tid >> 6;
    if ((tid & 63u) == 0u) wave_sums[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = 0u;
    total = 0u;
    for (uint32_t w = 0; w < kAdaptiveWaves; w++) {
        const uint32_t s = wave_sums[w];
        base += w < wave ? s : 0u;
        total += s;
    }
    return base + behind;
}

// Count launch, workgroup `block`: the set flags among its kAdaptiveBlock pixels.
__device__ __forceinline__ void adaptiveCountBlock(const uint8_t* flags, uint64_t pixels, uint32_t block, uint32_t tid, uint32_t* wave_sums, uint32_t* block_counts) {
    const uint64_t q = (uint64_t)block * kAdaptiveBlock + tid;
    uint32_t total;
    (void)adaptiveBlockRank(q < pixels && flags[q] != 0, tid, wave_sums, total);
    if (tid == 0u) block_counts[block] = total;
}

// Scan launch, ONE workgroup: offsets[b] = the set flags of the blocks before b, *length = all of them. A lane adds up a run of
// consecutive blocks; the lanes' sums are scanned through LDS (sums: 2 * kAdaptiveBlock words, ping-ponged).
__device__ __forceinline__ void adaptiveScanBlocks(const uint32_t* block_counts, uint32_t blocks, uint32_t tid, uint32_t* sums, uint32_t* offsets, uint32_t* length) {
    const uint32_t per = (blocks + kAdaptiveBlock - 1) / kAdaptiveBlock;
    const uint64_t first = (uint64_t)tid * per;
    const uint64_t end = first + per < blocks ? first + per : blocks;
    uint32_t own = 0u;
    for (uint64_t b = first; b < end; b++) own += block_counts[b];
    uint32_t src = 0u;
    sums[tid] = own;
    __syncthreads();
    for (uint32_t step = 1u; step < kAdaptiveBlock; step <<= 1) {
        const uint32_t v = sums[src * kAdaptiveBlock + tid] + (tid >= step ? sums[src * kAdaptiveBlock + tid - step] : 0u);
        src ^= 1u;
        sums[src * kAdaptiveBlock + tid] = v;
        __syncthreads();
    }
    const uint32_t inclusive = sums[src * kAdaptiveBlock + tid];
    uint32_t run = inclusive - own;
    for (uint64_t b = first; b < end; b++) {
        offsets[b] = run;
        run += block_counts[b];
    }
    if (tid == kAdaptiveBlock - 1u) *length = inclusive;
}

// Scatter launch, workgroup `block`: its flagged pixels behind one another from list[offsets[block]] on, ascending.
__device__ __forceinline__ void adaptiveScatterBlock(const uint8_t* flags, uint64_t pixels, uint32_t block, uint32_t tid, uint32_t* wave_sums, const uint32_t* offsets,
                                                      uint32_t* list) {
    const uint64_t q = (uint64_t)block * kAdaptiveBlock + tid;
    const bool flag = q < pixels && flags[q] != 0;
    uint32_t total;
    const uint32_t rank = adaptiveBlockRank(flag, tid, wave_sums, total);
    if (flag) list[offsets[block] + rank] = (uint32_t)q;
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

}  // namespace mcrt
