// Denoised output (include/mcrt.h mcrt_denoise*): the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010, guided by the first-hit
// AOV frame. The per-pixel text, shared by the three gfx950 kernels of mcrt_denoise.hip and the host emulation of the CPU tests
// (tests/emu/denoise_emu.cpp): both run this file. Only FP64 + - * /, compare and select, in the order include/mcrt.h states, built
// uncontracted like the rest of the exact build - the filtered frame is a function of its inputs bit for bit.
//
// Memory (device scratch, per pixel): one GUIDE record of 10 doubles {Ns.xyz, N.xyz, P.xyz, coverage} (80 B, packed once by the prep
// pass: nothing in it changes between iterations) and one IRRADIANCE record of 3 doubles (24 B) in each of two frames that the
// iterations ping-pong. A tap of step s is s records away: a strided read fetches the cache lines the record touches (one or two of
// 128 B for a guide record, which 16-byte alignment never splits inside a double), and the other residue classes of the step read
// their neighbours in the same lines.
//
// Two forms of an iteration, the same denoisePixel behind two tap sources:
//   plain  one lane per pixel, taps from memory
//   tile   taps of step s only connect pixels of one residue class (x mod s, y mod s): a workgroup of 256 lanes takes a 16 x 16 tile of
//          ONE class, stages its 20 x 20 records (2 of halo each side, field-major: lanes of a row read consecutive doubles) in LDS -
//          13 x 400 doubles = 41.6 KB - and runs the 25 taps from there after one barrier
#pragma once

#include "../../include/mcrt.h"
#include "mcrt_math.hpp"

namespace mcrt {

constexpr uint32_t kDenoiseGuideWords = 10;  // Ns.xyz, N.xyz, P.xyz, coverage
constexpr uint32_t kDenoiseRecWords = 13;    // ... and the irradiance, in LDS
constexpr uint32_t kDenoiseBlock = 256;
constexpr uint32_t kDenoiseTile = 16;                                       // a workgroup's pixels of one residue class: 16 x 16
constexpr uint32_t kDenoiseSide = kDenoiseTile + 4;                         // ... with 2 records of halo on every side
constexpr uint32_t kDenoiseTileRecs = kDenoiseSide * kDenoiseSide;          // 400
constexpr uint32_t kDenoiseTileWords = kDenoiseRecWords * kDenoiseTileRecs;  // 5200 doubles of LDS
constexpr uint32_t kDenoiseMaxIterations = 16, kDenoiseMaxNormalPowerLog2 = 32;
static_assert(kDenoiseTile * kDenoiseTile == kDenoiseBlock, "one lane per pixel of the tile");

// mcrt_denoise_params with its defaults filled in (NULL or a zero field = the default).
struct DenoiseSettings {
    uint32_t iterations, normal_power_log2, flags;
    double sigma_color, sigma_plane, albedo_floor;
};
inline DenoiseSettings denoiseSettings(const mcrt_denoise_params* p) {
    DenoiseSettings s{5u, 7u, 0u, 2.0, 0.1, 1e-3};
    if (!p) return s;
    if (p->iterations) s.iterations = p->iterations;
    if (p->normal_power_log2) s.normal_power_log2 = p->normal_power_log2;
    if (p->sigma_color != 0.0) s.sigma_color = p->sigma_color;
    if (p->sigma_plane != 0.0) s.sigma_plane = p->sigma_plane;
    if (p->albedo_floor != 0.0) s.albedo_floor = p->albedo_floor;
    s.flags = p->flags;
    return s;
}

// The prep pass: full frames in, packed guides and the demodulated frame I_0 out.
struct DenoiseFrame {
    uint32_t width, height;
    const double *rgb, *shading_normal, *normal, *position, *coverage;
    const double* albedo;  // nullptr: MCRT_DENOISE_NO_ALBEDO (a = 1)
    double albedo_floor;
    double* guide;  // [pixels][kDenoiseGuideWords]
    double* irr;    // [pixels][3]
};

// One iteration: irradiance `in` -> `out`; the last one multiplies the albedo factor back in and writes the caller's frame.
struct DenoiseStep {
    uint32_t width, height, step, normal_power_log2;
    double inv_c, sz2, albedo_floor;
    const double* guide;
    const double* in;
    double* out;
    const double* albedo;  // the LAST iteration (out = the caller's frame) with albedo: remodulate; nullptr otherwise
};
// The constants of iteration i, computed once on the host: s = 2^i, inv_c = 1 / (sigma_color 2^-i)^2, sz2 = sigma_plane^2.
inline void denoiseStepConstants(const DenoiseSettings& s, uint32_t i, DenoiseStep& st) {
    double sc = s.sigma_color;
    for (uint32_t k = 0; k < i; k++) sc = sc * 0.5;
    st.step = 1u << i;
    st.inv_c = 1.0 / (sc * sc);
    st.sz2 = s.sigma_plane * s.sigma_plane;
    st.normal_power_log2 = s.normal_power_log2;
    st.albedo_floor = s.albedo_floor;
}

struct DenoiseRec {
    d3 ns, n, p, irr;
};

MCRT_HD d3 denoiseLd3(const double* a) { return d3{a[0], a[1], a[2]}; }
MCRT_HD double denoiseMax0(double x) { return x < 0.0 ? 0.0 : x; }  // (a NaN stays a NaN)
MCRT_HD double denoiseAlbedoFactor(double albedo, double floor) { return albedo > floor ? albedo : 1.0; }

MCRT_HD void denoisePrepPixel(const DenoiseFrame& f, uint64_t p) {
    // every load before the first store: the frames may alias as far as the compiler knows, and a store in between would order them
    const d3 ns = denoiseLd3(f.shading_normal + 3 * p), n = denoiseLd3(f.normal + 3 * p), pos = denoiseLd3(f.position + 3 * p);
    const d3 c = denoiseLd3(f.rgb + 3 * p), alb = f.albedo ? denoiseLd3(f.albedo + 3 * p) : splat(1.0);
    const double cov = f.coverage[p];
    const d3 a = f.albedo ? d3{denoiseAlbedoFactor(alb.x, f.albedo_floor), denoiseAlbedoFactor(alb.y, f.albedo_floor), denoiseAlbedoFactor(alb.z, f.albedo_floor)}
                          : splat(1.0);
    const d3 irr = c / a;
    double* g = f.guide + p * kDenoiseGuideWords;
    g[0] = ns.x, g[1] = ns.y, g[2] = ns.z;
    g[3] = n.x, g[4] = n.y, g[5] = n.z;
    g[6] = pos.x, g[7] = pos.y, g[8] = pos.z;
    g[9] = cov;
    f.irr[3 * p] = irr.x, f.irr[3 * p + 1] = irr.y, f.irr[3 * p + 2] = irr.z;
}

// The geometric part of a tap's weight, (h w_n) w_z, from the centre's Ns, N, P and the tap's Ns, P: shared with the variance-guided
// filter (mcrt_denoise_var.hpp), whose colour weight alone differs.
MCRT_HD double denoiseGeometricWeight(uint32_t normal_power_log2, double sz2, const d3& c_ns, const d3& c_n, const d3& c_p, const d3& q_ns,
                                      const d3& q_p, double h) {
    double wn = denoiseMax0(dot(c_ns, q_ns));
    for (uint32_t k = 0; k < normal_power_log2; k++) wn = wn * wn;
    const d3 delta = q_p - c_p;
    const double dd = dot(delta, delta), d = dot(c_n, delta);
    const double xz = dd == 0.0 ? 0.0 : (d * d) / (sz2 * dd);
    double wz = denoiseMax0(1.0 - xz);
    wz = wz * wz;
    return (h * wn) * wz;
}

// Weight of tap q of centre c, h = h[dy] * h[dx]: (((h w_n) w_z) w_c).
MCRT_HD double denoiseWeight(const DenoiseStep& st, const DenoiseRec& c, const DenoiseRec& q, double h) {
    const double wg = denoiseGeometricWeight(st.normal_power_log2, st.sz2, c.ns, c.n, c.p, q.ns, q.p, h);
    const d3 di = c.irr - q.irr;
    const double e = dot(di, di), den = dot(c.irr, c.irr) + dot(q.irr, q.irr);
    const double xc = den == 0.0 ? 0.0 : (e / den) * st.inv_c;
    double wc = denoiseMax0(1.0 - xc);
    wc = wc * wc;
    return wg * wc;
}

// I_{i+1} of a covered pixel whose own record is c. src.tap(dx, dy, q): the record of tap (dx, dy) into q, false when the tap is outside
// the frame or has coverage 0.
template <class Src>
MCRT_HD d3 denoisePixel(const DenoiseStep& st, const Src& src, const DenoiseRec& c) {
    const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    d3 sum = splat(0.0);
    double wsum = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            double w;
            DenoiseRec q;
            if (dx == 0 && dy == 0) {
                w = 9.0 / 64.0;
                q.irr = c.irr;
            } else {
                if (!src.tap(dx, dy, q)) continue;
                w = denoiseWeight(st, c, q, h[dy + 2] * h[dx + 2]);
            }
            sum = sum + w * q.irr;
            wsum += w;
        }
    }
    return sum * (1.0 / wsum);
}

// The pixel's new value into st.out: the last iteration multiplies the albedo factor back in.
MCRT_HD void denoiseStore(const DenoiseStep& st, uint64_t p, d3 v) {
    if (st.albedo) {
        v.x = v.x * denoiseAlbedoFactor(st.albedo[3 * p], st.albedo_floor);
        v.y = v.y * denoiseAlbedoFactor(st.albedo[3 * p + 1], st.albedo_floor);
        v.z = v.z * denoiseAlbedoFactor(st.albedo[3 * p + 2], st.albedo_floor);
    }
    st.out[3 * p] = v.x;
    st.out[3 * p + 1] = v.y;
    st.out[3 * p + 2] = v.z;
}

// ---- plain form ------------------------------------------------------------------------------------------------------------------
struct DenoiseGlobalTaps {
    const DenoiseStep& st;
    uint32_t x, y;
    MCRT_HD bool tap(int dx, int dy, DenoiseRec& q) const {
        const int64_t qx = (int64_t)x + (int64_t)st.step * dx, qy = (int64_t)y + (int64_t)st.step * dy;
        if (qx < 0 || qy < 0 || qx >= (int64_t)st.width || qy >= (int64_t)st.height) return false;
        const uint64_t r = (uint64_t)qy * st.width + (uint64_t)qx;
        const double* g = st.guide + r * kDenoiseGuideWords;
        if (g[9] == 0.0) return false;
        q.ns = denoiseLd3(g);
        q.p = denoiseLd3(g + 6);
        q.irr = denoiseLd3(st.in + 3 * r);
        return true;
    }
};

MCRT_HD void denoisePlainPixel(const DenoiseStep& st, uint64_t p) {
    const uint32_t x = (uint32_t)(p % st.width), y = (uint32_t)(p / st.width);
    const double* g = st.guide + p * kDenoiseGuideWords;
    DenoiseRec c;
    c.irr = denoiseLd3(st.in + 3 * p);
    if (g[9] == 0.0) return denoiseStore(st, p, c.irr);
    c.ns = denoiseLd3(g);
    c.n = denoiseLd3(g + 3);
    c.p = denoiseLd3(g + 6);
    denoiseStore(st, p, denoisePixel(st, DenoiseGlobalTaps{st, x, y}, c));
}

// ---- tile form -------------------------------------------------------------------------------------------------------------------
// Workgroups of an iteration: for every residue class (rx, ry) that has pixels, tiles_x x tiles_y tiles of 16 x 16 class members (sized
// for class 0, the largest: a narrower class leaves its last tiles empty). Block b: bx = b % (ncx tiles_x), by = b / (ncx tiles_x);
// rx = bx % ncx, tile column bx / ncx - neighbouring blocks are neighbouring classes of one tile, which share cache lines.
struct DenoiseTiling {
    uint32_t ncx, ncy, tiles_x, tiles_y;
};
MCRT_HD DenoiseTiling denoiseTiling(uint32_t width, uint32_t height, uint32_t step) {
    DenoiseTiling t;
    t.ncx = step < width ? step : width;
    t.ncy = step < height ? step : height;
    const uint32_t cw = (uint32_t)(((uint64_t)width + step - 1) / step), chh = (uint32_t)(((uint64_t)height + step - 1) / step);
    t.tiles_x = (cw + kDenoiseTile - 1) / kDenoiseTile;
    t.tiles_y = (chh + kDenoiseTile - 1) / kDenoiseTile;
    return t;
}
MCRT_HD uint64_t denoiseTileBlocks(const DenoiseTiling& t) { return (uint64_t)t.ncx * t.tiles_x * t.ncy * t.tiles_y; }

#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

struct DenoiseLdsTaps {
    const double* lds;  // [kDenoiseRecWords][kDenoiseTileRecs]
    uint32_t r;         // the centre's record
    MCRT_HD bool tap(int dx, int dy, DenoiseRec& q) const {
        const uint32_t t = (uint32_t)((int)r + dy * (int)kDenoiseSide + dx);
        if (lds[9 * kDenoiseTileRecs + t] == 0.0) return false;
        q.ns = d3{lds[t], lds[kDenoiseTileRecs + t], lds[2 * kDenoiseTileRecs + t]};
        q.p = d3{lds[6 * kDenoiseTileRecs + t], lds[7 * kDenoiseTileRecs + t], lds[8 * kDenoiseTileRecs + t]};
        q.irr = d3{lds[10 * kDenoiseTileRecs + t], lds[11 * kDenoiseTileRecs + t], lds[12 * kDenoiseTileRecs + t]};
        return true;
    }
};

// One workgroup (kDenoiseBlock lanes, `tid` of them this one) of the tile form; lds: kDenoiseTileWords doubles.
__device__ __forceinline__ void denoiseTileBlock(const DenoiseStep& st, uint32_t block, uint32_t tid, double* lds) {
    const DenoiseTiling tl = denoiseTiling(st.width, st.height, st.step);
    const uint32_t per_row = tl.ncx * tl.tiles_x;
    const uint32_t bx = block % per_row, by = block / per_row;
    const uint32_t rx = bx % tl.ncx, ry = by % tl.ncy;
    const int64_t cx0 = (int64_t)(bx / tl.ncx) * kDenoiseTile, cy0 = (int64_t)(by / tl.ncy) * kDenoiseTile;  // the tile's first class member
    for (uint32_t r = tid; r < kDenoiseTileRecs; r += kDenoiseBlock) {
        const int64_t x = (int64_t)rx + (int64_t)st.step * (cx0 - 2 + (int64_t)(r % kDenoiseSide));
        const int64_t y = (int64_t)ry + (int64_t)st.step * (cy0 - 2 + (int64_t)(r / kDenoiseSide));
        if (x >= 0 && y >= 0 && x < (int64_t)st.width && y < (int64_t)st.height) {
            const uint64_t p = (uint64_t)y * st.width + (uint64_t)x;
            const double* g = st.guide + p * kDenoiseGuideWords;
#pragma unroll
            for (uint32_t k = 0; k < kDenoiseGuideWords; k++) lds[k * kDenoiseTileRecs + r] = g[k];
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) lds[(10 + k) * kDenoiseTileRecs + r] = st.in[3 * p + k];
        } else {
            lds[9 * kDenoiseTileRecs + r] = 0.0;  // outside the frame: skipped like a tap without coverage (its other words are not read)
        }
    }
    __syncthreads();
    const uint32_t lx = tid % kDenoiseTile, ly = tid / kDenoiseTile;
    const int64_t x = (int64_t)rx + (int64_t)st.step * (cx0 + lx), y = (int64_t)ry + (int64_t)st.step * (cy0 + ly);
    if (x >= (int64_t)st.width || y >= (int64_t)st.height) return;
    const uint64_t p = (uint64_t)y * st.width + (uint64_t)x;
    const uint32_t r = (ly + 2) * kDenoiseSide + lx + 2;
    DenoiseRec c;
    c.irr = d3{lds[10 * kDenoiseTileRecs + r], lds[11 * kDenoiseTileRecs + r], lds[12 * kDenoiseTileRecs + r]};
    if (lds[9 * kDenoiseTileRecs + r] == 0.0) return denoiseStore(st, p, c.irr);
    c.ns = d3{lds[r], lds[kDenoiseTileRecs + r], lds[2 * kDenoiseTileRecs + r]};
    c.n = d3{lds[3 * kDenoiseTileRecs + r], lds[4 * kDenoiseTileRecs + r], lds[5 * kDenoiseTileRecs + r]};
    c.p = d3{lds[6 * kDenoiseTileRecs + r], lds[7 * kDenoiseTileRecs + r], lds[8 * kDenoiseTileRecs + r]};
    denoiseStore(st, p, denoisePixel(st, DenoiseLdsTaps{lds, r}, c));
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

}  // namespace mcrt
