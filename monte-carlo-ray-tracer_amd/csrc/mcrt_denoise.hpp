// Denoised output (include/mcrt.h mcrt_denoise*): the edge-avoiding a-trous filter of mcrt_atrous.hpp with a colour weight relative to the
// two pixels' irradiance. What is this filter's own - settings, the prep pixel, the colour weight, the sums and the store; the 25-tap
// loop, the tap sources and the tile form are mcrt_atrous.hpp's. The per-pixel text, shared by the three gfx950 kernels of
// mcrt_denoise.hip and the host emulation of the CPU tests (tests/emu/denoise_emu.cpp): both run this file. Only FP64 + - * /, compare
// and select, in the order include/mcrt.h states, built uncontracted like the rest of the exact build - the filtered frame is a function
// of its inputs bit for bit.
//
// Memory (device scratch, per pixel): the GUIDE record of mcrt_atrous.hpp (10 doubles, packed once by the prep pass) and one IRRADIANCE
// record of 3 doubles (24 B) in each of two frames that the iterations ping-pong; the tile form's LDS is 13 x 400 doubles = 41.6 KB.
#pragma once

#include "mcrt_atrous.hpp"

namespace mcrt {

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

// What mcrt_atrous.hpp's skeleton asks of a filter.
struct DenoiseFilter {
    using Step = DenoiseStep;
    using Rec = DenoiseRec;
    static constexpr uint32_t kValueWords = 3;  // I.xyz
    template <class Ld>
    static MCRT_HD void loadValue(Rec& q, const Ld& ld) { q.irr = ld(0); }
    static MCRT_HD double weight(const Step& st, const Rec& c, const Rec& q, double h) { return denoiseWeight(st, c, q, h); }
    struct Acc {
        d3 sum = splat(0.0);
        double wsum = 0.0;
        MCRT_HD void add(double w, const Rec& q) {
            sum = sum + w * q.irr;
            wsum += w;
        }
        MCRT_HD Rec result() const {
            Rec r{};
            r.irr = sum * (1.0 / wsum);
            return r;
        }
    };
    static MCRT_HD void store(const Step& st, uint64_t p, const Rec& rec) { denoiseStore(st, p, rec.irr); }
};
constexpr uint32_t kDenoiseTileWords = kAtrousTileWords<DenoiseFilter>;  // 5200 doubles of LDS

// An iteration's pixel in the plain form, and one workgroup (lane `tid` of kDenoiseBlock) of the tile form; lds: kDenoiseTileWords doubles.
MCRT_HD void denoisePlainPixel(const DenoiseStep& st, uint64_t p) { atrousPlainPixel<DenoiseFilter>(st, p); }
#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)
__device__ __forceinline__ void denoiseTileBlock(const DenoiseStep& st, uint32_t block, uint32_t tid, double* lds) {
    atrousTileBlock<DenoiseFilter>(st, block, tid, lds);
}
#endif

}  // namespace mcrt
