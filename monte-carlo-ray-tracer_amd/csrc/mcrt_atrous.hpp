// The edge-avoiding a-trous wavelet filter of Dammertz et al. 2010, guided by the first-hit AOV frame: the skeleton of the filters built
// on it (mcrt_denoise.hpp, mcrt_denoise_var.hpp) - guide record, geometric weight, 25-tap loop, its two tap sources, the tiling of a step.
// A filter states what is its own as a description F:
//   F::Step, F::Rec         an iteration's constants {width, height, step, guide, in, ...}; a pixel's record {ns, n, p, value fields}
//   F::kValueWords          the doubles per pixel that the iterations ping-pong (st.in: [pixels][kValueWords])
//   F::loadValue(q, ld)     fills q's value fields; ld(k) is the d3 at words k .. k + 2 of the pixel's value, in memory or in LDS
//   F::weight(st, c, q, h)  the weight of tap q of centre c, h = h[dy] * h[dx]
//   F::Acc                  the sums over the taps: add(w, q), result() -> a Rec whose value fields are the pixel's new value
//   F::store(st, p, rec)    rec's value fields into the iteration's output
// Memory (device scratch, per pixel): one GUIDE record of 10 doubles {Ns.xyz, N.xyz, P.xyz, coverage} (80 B, packed once by the filter's
// prep pass) and one VALUE record in each of two frames that the iterations ping-pong. A tap of step s is s records away: a strided
// read fetches the cache lines the record touches (one or two of 128 B for a guide record), and the other residue classes of the step
// read their neighbours in the same lines.
// Two forms of an iteration, the same atrousPixel behind two tap sources:
//   plain  one lane per pixel, taps from memory
//   tile   taps of step s only connect pixels of one residue class (x mod s, y mod s): a workgroup of 256 lanes takes a 16 x 16 tile of
//          ONE class, stages its 20 x 20 records (2 of halo each side, field-major: lanes of a row read consecutive doubles) in LDS -
//          (10 + F::kValueWords) x 400 doubles - and runs the 25 taps from there after one barrier
#pragma once

#include "../../include/mcrt.h"
#include "mcrt_math.hpp"

namespace mcrt {

constexpr uint32_t kDenoiseGuideWords = 10;  // Ns.xyz, N.xyz, P.xyz, coverage
constexpr uint32_t kDenoiseBlock = 256;
constexpr uint32_t kDenoiseTile = 16;                               // a workgroup's pixels of one residue class: 16 x 16
constexpr uint32_t kDenoiseSide = kDenoiseTile + 4;                 // ... with 2 records of halo on every side
constexpr uint32_t kDenoiseTileRecs = kDenoiseSide * kDenoiseSide;  // 400
constexpr uint32_t kDenoiseMaxIterations = 16, kDenoiseMaxNormalPowerLog2 = 32;
static_assert(kDenoiseTile * kDenoiseTile == kDenoiseBlock, "one lane per pixel of the tile");

MCRT_HD d3 denoiseLd3(const double* a) { return d3{a[0], a[1], a[2]}; }
MCRT_HD double denoiseMax0(double x) { return x < 0.0 ? 0.0 : x; }  // (a NaN stays a NaN)
MCRT_HD double denoiseAlbedoFactor(double albedo, double floor) { return albedo > floor ? albedo : 1.0; }

// The geometric part of a tap's weight, (h w_n) w_z, from the centre's Ns, N, P and the tap's Ns, P: the filters' colour weights differ.
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

// The new value of a covered pixel whose own record is c. src.tap(dx, dy, q): the record of tap (dx, dy) into q, false when the tap is
// outside the frame or has coverage 0.
template <class F, class Src>
MCRT_HD typename F::Rec atrousPixel(const typename F::Step& st, const Src& src, const typename F::Rec& c) {
    const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    typename F::Acc acc;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            if (dx == 0 && dy == 0) {
                acc.add(9.0 / 64.0, c);
                continue;
            }
            typename F::Rec q;
            if (!src.tap(dx, dy, q)) continue;
            acc.add(F::weight(st, c, q, h[dy + 2] * h[dx + 2]), q);
        }
    }
    return acc.result();
}

// ---- plain form ------------------------------------------------------------------------------------------------------------------
template <class F>
struct AtrousGlobalTaps {
    const typename F::Step& st;
    uint32_t x, y;
    MCRT_HD bool tap(int dx, int dy, typename F::Rec& q) const {
        const int64_t qx = (int64_t)x + (int64_t)st.step * dx, qy = (int64_t)y + (int64_t)st.step * dy;
        if (qx < 0 || qy < 0 || qx >= (int64_t)st.width || qy >= (int64_t)st.height) return false;
        const uint64_t r = (uint64_t)qy * st.width + (uint64_t)qx;
        const double* g = st.guide + r * kDenoiseGuideWords;
        if (g[9] == 0.0) return false;
        q.ns = denoiseLd3(g);
        q.p = denoiseLd3(g + 6);
        const double* v = st.in + r * F::kValueWords;
        F::loadValue(q, [v](uint32_t k) { return denoiseLd3(v + k); });
        return true;
    }
};

template <class F>
MCRT_HD void atrousPlainPixel(const typename F::Step& st, uint64_t p) {
    const uint32_t x = (uint32_t)(p % st.width), y = (uint32_t)(p / st.width);
    const double *g = st.guide + p * kDenoiseGuideWords, *v = st.in + p * F::kValueWords;
    typename F::Rec c;
    F::loadValue(c, [v](uint32_t k) { return denoiseLd3(v + k); });
    if (g[9] == 0.0) return F::store(st, p, c);
    c.ns = denoiseLd3(g);
    c.n = denoiseLd3(g + 3);
    c.p = denoiseLd3(g + 6);
    F::store(st, p, atrousPixel<F>(st, AtrousGlobalTaps<F>{st, x, y}, c));
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

// The doubles of LDS a workgroup of the tile form stages: [kDenoiseGuideWords + F::kValueWords][kDenoiseTileRecs], field-major.
template <class F>
constexpr uint32_t kAtrousTileWords = (kDenoiseGuideWords + F::kValueWords) * kDenoiseTileRecs;

#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

// Fields `field` .. `field` + 2 of record t.
MCRT_HD d3 atrousLds3(const double* lds, uint32_t field, uint32_t t) {
    return d3{lds[field * kDenoiseTileRecs + t], lds[(field + 1) * kDenoiseTileRecs + t], lds[(field + 2) * kDenoiseTileRecs + t]};
}

template <class F>
struct AtrousLdsTaps {
    const double* lds;  // [kDenoiseGuideWords + F::kValueWords][kDenoiseTileRecs]
    uint32_t r;         // the centre's record
    MCRT_HD bool tap(int dx, int dy, typename F::Rec& q) const {
        const uint32_t t = (uint32_t)((int)r + dy * (int)kDenoiseSide + dx);
        if (lds[9 * kDenoiseTileRecs + t] == 0.0) return false;
        q.ns = atrousLds3(lds, 0, t);
        q.p = atrousLds3(lds, 6, t);
        F::loadValue(q, [this, t](uint32_t k) { return atrousLds3(lds, kDenoiseGuideWords + k, t); });
        return true;
    }
};

// One workgroup (kDenoiseBlock lanes, `tid` of them this one) of the tile form; lds: kAtrousTileWords<F> doubles.
template <class F>
__device__ __forceinline__ void atrousTileBlock(const typename F::Step& st, uint32_t block, uint32_t tid, double* lds) {
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
            const double *g = st.guide + p * kDenoiseGuideWords, *v = st.in + p * F::kValueWords;
#pragma unroll
            for (uint32_t k = 0; k < kDenoiseGuideWords; k++) lds[k * kDenoiseTileRecs + r] = g[k];
#pragma unroll
            for (uint32_t k = 0; k < F::kValueWords; k++) lds[(kDenoiseGuideWords + k) * kDenoiseTileRecs + r] = v[k];
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
    typename F::Rec c;
    F::loadValue(c, [lds, r](uint32_t k) { return atrousLds3(lds, kDenoiseGuideWords + k, r); });
    if (lds[9 * kDenoiseTileRecs + r] == 0.0) return F::store(st, p, c);
    c.ns = atrousLds3(lds, 0, r);
    c.n = atrousLds3(lds, 3, r);
    c.p = atrousLds3(lds, 6, r);
    F::store(st, p, atrousPixel<F>(st, AtrousLdsTaps<F>{lds, r}, c));
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

}  // namespace mcrt
