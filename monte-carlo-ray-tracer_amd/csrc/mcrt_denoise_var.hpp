// Variance-guided denoised output (include/mcrt.h mcrt_denoise_variance*): the a-trous filter of mcrt_atrous.hpp with a colour weight in
// units of the pixels' estimated variance, and that variance carried through the iterations. What is this filter's own - settings, the
// prep pixel, the colour weight, the sums and the store; the 25-tap loop, the tap sources and the tile form are mcrt_atrous.hpp's. The
// per-pixel text, shared by the three gfx950 kernels of mcrt_denoise_var.hip and the host emulation of the CPU tests
// (tests/emu/denoise_var_emu.cpp): both run this file. Only FP64 + - * /, compare and select, in the order include/mcrt.h states, built
// uncontracted - both outputs are functions of the inputs bit for bit.
//
// Memory (device scratch, per pixel): the GUIDE record of mcrt_atrous.hpp (10 doubles, packed once by the prep pass) and one record of
// 6 doubles {I.xyz, V.xyz} (48 B) in each of two frames that the iterations ping-pong: a tap reads irradiance and variance together.
// The tile form's LDS is 16 x 400 doubles = 51 200 B, three workgroups in a CU's 160 KB.
#pragma once

#include "mcrt_atrous.hpp"

namespace mcrt {

constexpr uint32_t kDenoiseVarIvWords = 6;  // I.xyz, V.xyz

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
    // every load before the first store, as in denoisePrepPixel (mcrt_denoise.hpp): the frames may alias as far as the compiler knows; the
    // 3 x 3 neighbours' v, albedo and coverage come from the input frames
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

// What mcrt_atrous.hpp's skeleton asks of a filter.
struct DenoiseVarFilter {
    using Step = DenoiseVarStep;
    using Rec = DenoiseVarRec;
    static constexpr uint32_t kValueWords = kDenoiseVarIvWords;
    template <class Ld>
    static MCRT_HD void loadValue(Rec& q, const Ld& ld) {
        q.irr = ld(0);
        q.var = ld(3);
    }
    static MCRT_HD double weight(const Step& st, const Rec& c, const Rec& q, double h) { return denoiseVarWeight(st, c, q, h); }
    struct Acc {
        d3 sum = splat(0.0), vsum = splat(0.0);
        double wsum = 0.0;
        MCRT_HD void add(double w, const Rec& q) {
            sum = sum + w * q.irr;
            vsum = vsum + (w * w) * q.var;
            wsum += w;
        }
        MCRT_HD Rec result() const {
            const double r = 1.0 / wsum;
            Rec o{};
            o.irr = sum * r;
            o.var = vsum * (r * r);
            return o;
        }
    };
    static MCRT_HD void store(const Step& st, uint64_t p, const Rec& rec) { denoiseVarStore(st, p, rec.irr, rec.var); }
};
constexpr uint32_t kDenoiseVarTileWords = kAtrousTileWords<DenoiseVarFilter>;  // 6400 doubles
constexpr uint32_t kDenoiseVarTileLdsBytes = kDenoiseVarTileWords * 8;         // 51 200 B (tests/test_denoise_var_library.py)
static_assert(3 * kDenoiseVarTileLdsBytes <= 160 * 1024, "three workgroups per CU by LDS");

// An iteration's pixel in the plain form, and one workgroup (lane `tid` of kDenoiseBlock) of the tile form; lds: kDenoiseVarTileWords doubles.
MCRT_HD void denoiseVarPlainPixel(const DenoiseVarStep& st, uint64_t p) { atrousPlainPixel<DenoiseVarFilter>(st, p); }
#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)
__device__ __forceinline__ void denoiseVarTileBlock(const DenoiseVarStep& st, uint32_t block, uint32_t tid, double* lds) {
    atrousTileBlock<DenoiseVarFilter>(st, block, tid, lds);
}
#endif

}  // namespace mcrt
