// Variance-guided denoised output (include/mcrt.h mcrt_denoise_variance*): the a-trous filter of mcrt_denoise.hpp with a colour weight in
// units of the pixels' estimated variance, and that variance carried through the iterations. The per-pixel text, shared by the three
// gfx950 kernels of mcrt_denoise_var.hip and the host emulation of the CPU tests (tests/emu/denoise_var_emu.cpp): both run this file.
// Only FP64 + - * /, compare and select, in the order include/mcrt.h states, built uncontracted - both outputs are functions of the
// inputs bit for bit. dot, max0, the albedo factor, the geometric weights and the tiling of a step are mcrt_denoise.hpp's own.
//
// Memory (device scratch, per pixel): the GUIDE record of mcrt_denoise.hpp (10 doubles, packed once by the prep pass) and one record of
// 6 doubles {I.xyz, V.xyz} (48 B) in each of two frames that the iterations ping-pong: a tap reads irradiance and variance together.
//
// Two forms of an iteration, the same denoiseVarPixel behind two tap sources, as in mcrt_denoise.hpp:
//   plain  one lane per pixel, taps from memory
//   tile   a workgroup of 256 lanes takes a 16 x 16 tile of ONE residue class of the step and stages its 20 x 20 records (field-major)
//          in LDS - 16 x 400 doubles = 51 200 B, three workgroups in a CU's 160 KB - and runs the 25 taps from there after one barrier
#pragma once

#include "mcrt_denoise.hpp"

namespace mcrt {

constexpr uint32_t kDenoiseVarIvWords = 6;                                            // I.xyz, V.xyz
constexpr uint32_t kDenoiseVarRecWords = kDenoiseGuideWords + kDenoiseVarIvWords;      // 16 doubles per record in LDS
constexpr uint32_t kDenoiseVarTileWords = kDenoiseVarRecWords * kDenoiseTileRecs;      // 6400 doubles
constexpr uint32_t kDenoiseVarTileLdsBytes = kDenoiseVarTileWords * 8;                 // 51 200 B (tests/test_denoise_var_library.py)
static_assert(3 * kDenoiseVarTileLdsBytes <= 160 * 1024, "three workgroups per CU by LDS");

// mcrt_denoise_variance_params with its defaults filled in (NULL or a zero field = the default).
struct DenoiseVarSettings {
    uint32_t iterations, normal_power_log2, flags;
    double sigma_variance, sigma_floor, sigma_plane, albedo_floor;
};
inline DenoiseVarSettings denoiseVarSettings(const mcrt_denoise_variance_params* p) {
    DenoiseVarSettings s{5u, 7u, 0u, 6.0, 0.02, 0.1, 1e-3};
    if (!p) return s;
    if (p->iterations) s.iterations = p->iterations;
    if (p->normal_power_log2) s.normal_power_log2 = p->normal_power_log2;
    if (p->sigma_variance != 0.0) s.sigma_variance = p->sigma_variance;
    if (p->sigma_floor != 0.0) s.sigma_floor = p->sigma_floor;
    if (p->sigma_plane != 0.0) s.sigma_plane = p->sigma_plane;
    if (p->albedo_floor != 0.0) s.albedo_floor = p->albedo_floor;
    s.flags = p->flags;
    return s;
}
// A sigma the calls refuse: negative or not finite (x - x is 0.0 for every finite x and NaN otherwise).
inline bool denoiseVarBadSigma(double x) { return !(x >= 0.0) || !(x - x == 0.0); }
// What the calls refuse about the settings, or nullptr.
inline const char* denoiseVarSettingsError(const DenoiseVarSettings& s) {
    if (s.iterations > kDenoiseMaxIterations) return "more than 16 iterations";
    if (s.normal_power_log2 > kDenoiseMaxNormalPowerLog2) return "normal_power_log2 above 32";
    if (denoiseVarBadSigma(s.sigma_variance)) return "sigma_variance is negative or not finite";
    if (denoiseVarBadSigma(s.sigma_floor)) return "sigma_floor is negative or not finite";
    if (denoiseVarBadSigma(s.sigma_plane)) return "sigma_plane is negative or not finite";
    return nullptr;
}

// The prep pass: full frames in; packed guides, the demodulated frame I_0 and the prefiltered variance V_0 out.
struct DenoiseVarFrame {
    uint32_t width, height;
    double spp;  // (double)n
    const double *rgb, *variance, *shading_normal, *normal, *position, *coverage;
    const double* albedo;  // nullptr: MCRT_DENOISE_NO_ALBEDO (a = 1)
    double albedo_floor;
    double* guide;  // [pixels][kDenoiseGuideWords]
    double* iv;     // [pixels][kDenoiseVarIvWords]
};

// One iteration: records `in` -> `out`; the last one multiplies the albedo factor back in and writes the caller's frames instead.
struct DenoiseVarStep {
    uint32_t width, height, step, normal_power_log2;
    double sv2, sf2, sz2, albedo_floor, spp;
    const double* guide;
    const double* in;      // [pixels][kDenoiseVarIvWords]
    double* out;           // ... of the next iteration; nullptr in the LAST iteration, which writes:
    double* out_rgb;       //   the caller's frame
    double* out_variance;  //   the caller's variance frame, or nullptr: not wanted
    const double* albedo;  //   with albedo: remodulate; nullptr otherwise
};
// The constants of a call, computed once on the host; iteration i has step 2^i and the same sigmas.
inline void denoiseVarStepConstants(const DenoiseVarSettings& s, uint32_t spp, DenoiseVarStep& st) {
    st.sv2 = s.sigma_variance * s.sigma_variance;
    st.sf2 = s.sigma_floor * s.sigma_floor;
    st.sz2 = s.sigma_plane * s.sigma_plane;
    st.normal_power_log2 = s.normal_power_log2;
    st.albedo_floor = s.albedo_floor;
    st.spp = (double)spp;
}

struct DenoiseVarRec {
    d3 ns, n, p, irr, var;
};

MCRT_HD double denoiseVarG(const d3& v) { return (v.x + v.y) + v.z; }
MCRT_HD d3 denoiseVarAlbedoFactor(const double* albedo, uint64_t p, double floor) {
    if (!albedo) return splat(1.0);
    return d3{denoiseAlbedoFactor(albedo[3 * p], floor), denoiseAlbedoFactor(albedo[3 * p + 1], floor), denoiseAlbedoFactor(albedo[3 * p + 2], floor)};
}
// u of pixel q: the variance of the pixel's mean in the demodulated frame.
MCRT_HD d3 denoiseVarOfMean(const DenoiseVarFrame& f, uint64_t q) {
    const d3 v = denoiseLd3(f.variance + 3 * q), a = denoiseVarAlbedoFactor(f.albedo, q, f.albedo_floor);
    return d3{(v.x / f.spp) / (a.x * a.x), (v.y / f.spp) / (a.y * a.y), (v.z / f.spp) / (a.z * a.z)};
}

MCRT_HD void denoiseVarPrepPixel(const DenoiseVarFrame& f, uint64_t p) {
    // every load before the first store, as in denoisePrepPixel; the 3 x 3 neighbours' v, albedo and coverage come from the input frames
    const d3 ns = denoiseLd3(f.shading_normal + 3 * p), n = denoiseLd3(f.normal + 3 * p), pos = denoiseLd3(f.position + 3 * p);
    const d3 c = denoiseLd3(f.rgb + 3 * p), a = denoiseVarAlbedoFactor(f.albedo, p, f.albedo_floor);
    const double cov = f.coverage[p];
    const d3 irr = c / a;
    d3 var = denoiseVarOfMean(f, p);
    if (!(cov == 0.0)) {
        const uint32_t x = (uint32_t)(p % f.width), y = (uint32_t)(p / f.width);
        const double k[3] = {1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0};
        d3 s = splat(0.0);
        double ks = 0.0;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int64_t qx = (int64_t)x + dx, qy = (int64_t)y + dy;
                if (qx < 0 || qy < 0 || qx >= (int64_t)f.width || qy >= (int64_t)f.height) continue;
                const uint64_t q = (uint64_t)qy * f.width + (uint64_t)qx;
                if (f.coverage[q] == 0.0) continue;
                const double kw = k[dy + 1] * k[dx + 1];
                s = s + kw * denoiseVarOfMean(f, q);
                ks += kw;
            }
        }
        var = s * (1.0 / ks);
    }
    double* g = f.guide + p * kDenoiseGuideWords;
    g[0] = ns.x, g[1] = ns.y, g[2] = ns.z;
    g[3] = n.x, g[4] = n.y, g[5] = n.z;
    g[6] = pos.x, g[7] = pos.y, g[8] = pos.z;
    g[9] = cov;
    double* o = f.iv + p * kDenoiseVarIvWords;
    o[0] = irr.x, o[1] = irr.y, o[2] = irr.z;
    o[3] = var.x, o[4] = var.y, o[5] = var.z;
}

// Weight of tap q of centre c, h = h[dy] * h[dx]: (((h w_n) w_z) w_c), w_c in units of the variance of the difference.
MCRT_HD double denoiseVarWeight(const DenoiseVarStep& st, const DenoiseVarRec& c, const DenoiseVarRec& q, double h) {
    const double wg = denoiseGeometricWeight(st.normal_power_log2, st.sz2, c.ns, c.n, c.p, q.ns, q.p, h);
    const d3 di = c.irr - q.irr;
    const double e = dot(di, di), m = dot(c.irr, c.irr) + dot(q.irr, q.irr);
    const double den = (st.sv2 * (denoiseVarG(c.var) + denoiseVarG(q.var))) + (st.sf2 * m);
    const double xc = e == 0.0 ? 0.0 : e / den;
    double wc = denoiseMax0(1.0 - xc);
    wc = wc * wc;
    return wg * wc;
}

// I_{i+1} and V_{i+1} of a covered pixel whose own record is c. src.tap(dx, dy, q): the record of tap (dx, dy) into q, false when the tap
// is outside the frame or has coverage 0.
template <class Src>
MCRT_HD void denoiseVarPixel(const DenoiseVarStep& st, const Src& src, const DenoiseVarRec& c, d3& irr, d3& var) {
    const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    d3 sum = splat(0.0), vsum = splat(0.0);
    double wsum = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            double w;
            DenoiseVarRec q;
            if (dx == 0 && dy == 0) {
                w = 9.0 / 64.0;
                q.irr = c.irr;
                q.var = c.var;
            } else {
                if (!src.tap(dx, dy, q)) continue;
                w = denoiseVarWeight(st, c, q, h[dy + 2] * h[dx + 2]);
            }
            sum = sum + w * q.irr;
            vsum = vsum + (w * w) * q.var;
            wsum += w;
        }
    }
    const double r = 1.0 / wsum;
    irr = sum * r;
    var = vsum * (r * r);
}

// The pixel's new record into st.out; the last iteration multiplies the albedo factor back in and writes the caller's frames.
MCRT_HD void denoiseVarStore(const DenoiseVarStep& st, uint64_t p, d3 irr, d3 var) {
    if (st.out) {
        double* o = st.out + p * kDenoiseVarIvWords;
        o[0] = irr.x, o[1] = irr.y, o[2] = irr.z;
        o[3] = var.x, o[4] = var.y, o[5] = var.z;
        return;
    }
    const d3 a = denoiseVarAlbedoFactor(st.albedo, p, st.albedo_floor);
    if (st.albedo) irr = d3{irr.x * a.x, irr.y * a.y, irr.z * a.z};
    st.out_rgb[3 * p] = irr.x;
    st.out_rgb[3 * p + 1] = irr.y;
    st.out_rgb[3 * p + 2] = irr.z;
    if (st.out_variance) {
        st.out_variance[3 * p] = (var.x * (a.x * a.x)) * st.spp;
        st.out_variance[3 * p + 1] = (var.y * (a.y * a.y)) * st.spp;
        st.out_variance[3 * p + 2] = (var.z * (a.z * a.z)) * st.spp;
    }
}

// ---- plain form ------------------------------------------------------------------------------------------------------------------
struct DenoiseVarGlobalTaps {
    const DenoiseVarStep& st;
    uint32_t x, y;
    MCRT_HD bool tap(int dx, int dy, DenoiseVarRec& q) const {
        const int64_t qx = (int64_t)x + (int64_t)st.step * dx, qy = (int64_t)y + (int64_t)st.step * dy;
        if (qx < 0 || qy < 0 || qx >= (int64_t)st.width || qy >= (int64_t)st.height) return false;
        const uint64_t r = (uint64_t)qy * st.width + (uint64_t)qx;
        const double* g = st.guide + r * kDenoiseGuideWords;
        if (g[9] == 0.0) return false;
        q.ns = denoiseLd3(g);
        q.p = denoiseLd3(g + 6);
        q.irr = denoiseLd3(st.in + r * kDenoiseVarIvWords);
        q.var = denoiseLd3(st.in + r * kDenoiseVarIvWords + 3);
        return true;
    }
};

MCRT_HD void denoiseVarPlainPixel(const DenoiseVarStep& st, uint64_t p) {
    const uint32_t x = (uint32_t)(p % st.width), y = (uint32_t)(p / st.width);
    const double* g = st.guide + p * kDenoiseGuideWords;
    DenoiseVarRec c;
    c.irr = denoiseLd3(st.in + p * kDenoiseVarIvWords);
    c.var = denoiseLd3(st.in + p * kDenoiseVarIvWords + 3);
    if (g[9] == 0.0) return denoiseVarStore(st, p, c.irr, c.var);
    c.ns = denoiseLd3(g);
    c.n = denoiseLd3(g + 3);
    c.p = denoiseLd3(g + 6);
    d3 irr, var;
    denoiseVarPixel(st, DenoiseVarGlobalTaps{st, x, y}, c, irr, var);
    denoiseVarStore(st, p, irr, var);
}

// ---- tile form -------------------------------------------------------------------------------------------------------------------
// The workgroups of an iteration are denoiseTiling's (mcrt_denoise.hpp): the same tiles of the same residue classes.
#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

MCRT_HD d3 denoiseVarLds3(const double* lds, uint32_t field, uint32_t t) {
    return d3{lds[field * kDenoiseTileRecs + t], lds[(field + 1) * kDenoiseTileRecs + t], lds[(field + 2) * kDenoiseTileRecs + t]};
}

struct DenoiseVarLdsTaps {
    const double* lds;  // [kDenoiseVarRecWords][kDenoiseTileRecs]
    uint32_t r;         // the centre's record
    MCRT_HD bool tap(int dx, int dy, DenoiseVarRec& q) const {
        const uint32_t t = (uint32_t)((int)r + dy * (int)kDenoiseSide + dx);
        if (lds[9 * kDenoiseTileRecs + t] == 0.0) return false;
        q.ns = denoiseVarLds3(lds, 0, t);
        q.p = denoiseVarLds3(lds, 6, t);
        q.irr = denoiseVarLds3(lds, 10, t);
        q.var = denoiseVarLds3(lds, 13, t);
        return true;
    }
};

// One workgroup (kDenoiseBlock lanes, `tid` of them this one) of the tile form; lds: kDenoiseVarTileWords doubles.
__device__ __forceinline__ void denoiseVarTileBlock(const DenoiseVarStep& st, uint32_t block, uint32_t tid, double* lds) {
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
            const double* iv = st.in + p * kDenoiseVarIvWords;
#pragma unroll
            for (uint32_t k = 0; k < kDenoiseGuideWords; k++) lds[k * kDenoiseTileRecs + r] = g[k];
#pragma unroll
            for (uint32_t k = 0; k < kDenoiseVarIvWords; k++) lds[(kDenoiseGuideWords + k) * kDenoiseTileRecs + r] = iv[k];
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
    DenoiseVarRec c;
    c.irr = denoiseVarLds3(lds, 10, r);
    c.var = denoiseVarLds3(lds, 13, r);
    if (lds[9 * kDenoiseTileRecs + r] == 0.0) return denoiseVarStore(st, p, c.irr, c.var);
    c.ns = denoiseVarLds3(lds, 0, r);
    c.n = denoiseVarLds3(lds, 3, r);
    c.p = denoiseVarLds3(lds, 6, r);
    d3 irr, var;
    denoiseVarPixel(st, DenoiseVarLdsTaps{lds, r}, c, irr, var);
    denoiseVarStore(st, p, irr, var);
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

}  // namespace mcrt
