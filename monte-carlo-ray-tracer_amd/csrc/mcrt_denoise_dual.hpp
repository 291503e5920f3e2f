// Dual-buffer denoised output (include/mcrt.h mcrt_denoise_dual*): the non-local-means filter of Rousselle, Knaus and Zwicker 2012 on the
// two half-buffers of a render - each half filtered with weights computed from the other, the squared difference of the filtered halves
// the filtered frame's error. The per-pixel text, shared by the three gfx950 kernels of mcrt_denoise_dual.hip and the host emulation of
// the CPU tests (tests/emu/denoise_dual_emu.cpp): both run this file. Only FP64 + - * /, compare and select, in the order include/mcrt.h
// states, built uncontracted - every output is a function of the inputs bit for bit, whatever the form.
//
// Memory (device scratch, per pixel): one packed record {A.rgb, B.rgb, V0.rgb} of 9 doubles (72 B), written by the prep pass - the filter
// reads nothing else, so every output may alias an input.
// Two forms of the filter:
//   plain  one lane per pixel, the definition as written: per window offset the (2F+1)^2 patch elements, records from memory
//   tile   a workgroup of 512 or 1024 lanes (denoiseDualTileLanes) takes a 16 x 16 tile and stages its (16 + 2(R+F))^2 records in LDS, field-major (lanes of a row read
//          consecutive doubles). A patch element's term depends on (element position, offset, half, channel) alone and a patch row's sum
//          on (x, row, offset, half): per window offset the workgroup computes the 6 (16+2F)^2 terms once, a barrier, the 2 x 16 (16+2F) row
//          sums, a barrier, and each of the first 256 lanes adds the 2F+1 row sums of its pixel in the stated order - (2F+1)^2 times fewer divisions than
//          the plain form, the same bits. Records outside the frame are neither staged nor read: validity comes from the coordinates.
//          LDS: denoiseDualTileLdsBytes(R, F) - 89 120 B at the defaults (5, 2), 132 832 B at the limits (8, 3): dynamic, one workgroup per CU.
#pragma once

#include "mcrt_atrous.hpp"

namespace mcrt {

constexpr uint32_t kDenoiseDualRecWords = 9;  // A.rgb, B.rgb, V0.rgb
constexpr uint32_t kDenoiseDualMaxWindow = 8, kDenoiseDualMaxPatch = 3;
constexpr uint32_t kDenoiseDualTileMaxLanes = 1024;  // the tile form's workgroup: 256, 512 or 1024 lanes on one 16 x 16 tile

// mcrt_denoise_dual_params with its defaults filled in (NULL or a zero field = the default).
struct DenoiseDualSettings {
    uint32_t window_radius, patch_radius, flags;
    double k, alpha, epsilon;
};
inline DenoiseDualSettings denoiseDualSettings(const mcrt_denoise_dual_params* p) {
    DenoiseDualSettings s{5u, 2u, 0u, 0.45, 1.0, 1e-10};
    if (!p) return s;
    if (p->window_radius) s.window_radius = p->window_radius;
    if (p->patch_radius) s.patch_radius = p->patch_radius;
    if (p->k != 0.0) s.k = p->k;
    if (p->alpha != 0.0) s.alpha = p->alpha;
    if (p->epsilon != 0.0) s.epsilon = p->epsilon;
    s.flags = p->flags;
    return s;
}
// negative or not finite (x - x is 0.0 for every finite x and NaN otherwise)
inline bool denoiseDualBad(double x) { return !(x >= 0.0) || !(x - x == 0.0); }
// What the calls refuse about the settings, or nullptr.
inline const char* denoiseDualSettingsError(const DenoiseDualSettings& s) {
    if (s.window_radius > kDenoiseDualMaxWindow) return "window_radius above 8";
    if (s.patch_radius > kDenoiseDualMaxPatch) return "patch_radius above 3";
    if (denoiseDualBad(s.k)) return "k is negative or not finite";
    if (denoiseDualBad(s.alpha)) return "alpha is negative or not finite";
    if (denoiseDualBad(s.epsilon) || !(s.epsilon > 0.0)) return "epsilon is negative or not finite";
    return nullptr;
}

// The prep pass: full frames in, one packed record per pixel out.
struct DenoiseDualFrame {
    uint32_t width, height;
    const double *half_a, *half_b, *variance;
    double* rec;  // [pixels][kDenoiseDualRecWords]
};

// The filter: records in, the caller's frames out.
struct DenoiseDualStep {
    uint32_t width, height, window_radius, patch_radius;
    double ia, ib, fa, fb, fafb, k2, alpha, epsilon, spp;
    const double* rec;
    double *out_rgb, *out_variance, *out_half_a, *out_half_b;  // out_rgb required; nullptr: not wanted
};
// The constants of a call, computed once on the host.
inline void denoiseDualStepConstants(const DenoiseDualSettings& s, uint32_t spp, DenoiseDualStep& st) {
    const uint32_t n_a = spp - spp / 2, n_b = spp / 2;  // (n + 1) / 2 without the overflow
    st.window_radius = s.window_radius;
    st.patch_radius = s.patch_radius;
    st.ia = 1.0 / (double)n_a;
    st.ib = 1.0 / (double)n_b;
    st.fa = (double)n_a / (double)spp;
    st.fb = (double)n_b / (double)spp;
    st.fafb = st.fa * st.fb;
    st.k2 = s.k * s.k;
    st.alpha = s.alpha;
    st.epsilon = s.epsilon;
    st.spp = (double)spp;
}

MCRT_HD bool denoiseDualInside(int64_t x, int64_t y, uint32_t width, uint32_t height) {
    return x >= 0 && y >= 0 && x < (int64_t)width && y < (int64_t)height;
}

MCRT_HD void denoiseDualPrepPixel(const DenoiseDualFrame& f, uint64_t p) {
    // every load before the first store (the frames may alias as far as the compiler knows)
    const d3 a = denoiseLd3(f.half_a + 3 * p), b = denoiseLd3(f.half_b + 3 * p);
    const uint32_t x = (uint32_t)(p % f.width), y = (uint32_t)(p / f.width);
    const double k[3] = {1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0};
    d3 s = splat(0.0);
    double ks = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int64_t qx = (int64_t)x + dx, qy = (int64_t)y + dy;
            if (!denoiseDualInside(qx, qy, f.width, f.height)) continue;
            const double kw = k[dy + 1] * k[dx + 1];
            s = s + kw * denoiseLd3(f.variance + 3 * ((uint64_t)qy * f.width + (uint64_t)qx));
            ks += kw;
        }
    }
    const d3 v0 = s * (1.0 / ks);
    double* o = f.rec + p * kDenoiseDualRecWords;
    o[0] = a.x, o[1] = a.y, o[2] = a.z;
    o[3] = b.x, o[4] = b.y, o[5] = b.z;
    o[6] = v0.x, o[7] = v0.y, o[8] = v0.z;
}

// One channel of one patch element: half X's values xp, xq and prefiltered variances v0p, v0q at p' and q', ix = 1 / n_x.
MCRT_HD double denoiseDualTerm(const DenoiseDualStep& st, double xp, double xq, double v0p, double v0q, double ix) {
    const double vp = v0p * ix, vq = v0q * ix;
    const double delta = xp - xq;
    const double vm = vq < vp ? vq : vp;
    const double num = delta * delta - st.alpha * (vp + vm);
    const double den = st.epsilon + st.k2 * (vp + vq);
    return num / den;
}
// The weight of a tap from its patch sum S over cnt elements.
MCRT_HD double denoiseDualWeight(double S, uint32_t cnt) {
    const double D = S / (double)(3u * cnt);
    const double x = denoiseMax0(D);
    const double w = denoiseMax0(1.0 - x);
    return w * w;
}

// A pixel's sums over the window taps. wa: the weight computed from half A (applied to B); wb: from half B (applied to A).
struct DenoiseDualAcc {
    d3 sum_a = splat(0.0), sum_b = splat(0.0);
    double wsum_a = 0.0, wsum_b = 0.0;
    MCRT_HD void add(double wa, double wb, const d3& a_q, const d3& b_q) {
        sum_a = sum_a + wb * a_q;
        wsum_b += wb;
        sum_b = sum_b + wa * b_q;
        wsum_a += wa;
    }
};
MCRT_HD void denoiseDualSt3(double* frame, uint64_t p, const d3& v) {
    frame[3 * p] = v.x, frame[3 * p + 1] = v.y, frame[3 * p + 2] = v.z;
}
MCRT_HD void denoiseDualStore(const DenoiseDualStep& st, uint64_t p, const DenoiseDualAcc& acc) {
    const d3 af = acc.sum_a * (1.0 / acc.wsum_b), bf = acc.sum_b * (1.0 / acc.wsum_a);
    denoiseDualSt3(st.out_rgb, p, (st.fa * af) + (st.fb * bf));
    if (st.out_variance) {
        const d3 dl = af - bf;
        denoiseDualSt3(st.out_variance, p, ((dl * dl) * st.fafb) * st.spp);
    }
    if (st.out_half_a) denoiseDualSt3(st.out_half_a, p, af);
    if (st.out_half_b) denoiseDualSt3(st.out_half_b, p, bf);
}

// ---- plain form ------------------------------------------------------------------------------------------------------------------
MCRT_HD void denoiseDualPlainPixel(const DenoiseDualStep& st, uint64_t p) {
    const int64_t x = (int64_t)(p % st.width), y = (int64_t)(p / st.width);
    const int R = (int)st.window_radius, F = (int)st.patch_radius;
    DenoiseDualAcc acc;
    for (int dy = -R; dy <= R; dy++) {
        for (int dx = -R; dx <= R; dx++) {
            const int64_t qx = x + dx, qy = y + dy;
            if (!denoiseDualInside(qx, qy, st.width, st.height)) continue;
            const double* rq = st.rec + ((uint64_t)qy * st.width + (uint64_t)qx) * kDenoiseDualRecWords;
            double wa = 1.0, wb = 1.0;
            if (dx != 0 || dy != 0) {
                double sa = 0.0, sb = 0.0;
                uint32_t cnt = 0;
                for (int j = -F; j <= F; j++) {
                    double row_a = 0.0, row_b = 0.0;
                    for (int i = -F; i <= F; i++) {
                        if (!denoiseDualInside(x + i, y + j, st.width, st.height) || !denoiseDualInside(qx + i, qy + j, st.width, st.height)) continue;
                        cnt += 1;
                        const double* ep = st.rec + ((uint64_t)(y + j) * st.width + (uint64_t)(x + i)) * kDenoiseDualRecWords;
                        const double* eq = st.rec + ((uint64_t)(qy + j) * st.width + (uint64_t)(qx + i)) * kDenoiseDualRecWords;
#pragma unroll
                        for (int ch = 0; ch < 3; ch++) {
                            row_a = row_a + denoiseDualTerm(st, ep[ch], eq[ch], ep[6 + ch], eq[6 + ch], st.ia);
                            row_b = row_b + denoiseDualTerm(st, ep[3 + ch], eq[3 + ch], ep[6 + ch], eq[6 + ch], st.ib);
                        }
                    }
                    sa = sa + row_a;
                    sb = sb + row_b;
                }
                wa = denoiseDualWeight(sa, cnt);
                wb = denoiseDualWeight(sb, cnt);
            }
            acc.add(wa, wb, denoiseLd3(rq), denoiseLd3(rq + 3));
        }
    }
    denoiseDualStore(st, p, acc);
}

// ---- tile form -------------------------------------------------------------------------------------------------------------------
// The doubles of LDS of a workgroup: the staged records [9][side^2], side = 16 + 2 (R + F); the terms of one offset [6][E^2],
// E = 16 + 2 F; the row sums of one offset [2][E][16].
constexpr uint32_t denoiseDualTileLdsWords(uint32_t R, uint32_t F) {
    return kDenoiseDualRecWords * (kDenoiseTile + 2 * (R + F)) * (kDenoiseTile + 2 * (R + F)) + 6 * (kDenoiseTile + 2 * F) * (kDenoiseTile + 2 * F) +
           2 * (kDenoiseTile + 2 * F) * kDenoiseTile;
}
constexpr uint32_t denoiseDualTileLdsBytes(uint32_t R, uint32_t F) { return 8 * denoiseDualTileLdsWords(R, F); }
constexpr uint32_t kDenoiseDualTileLdsMaxBytes = denoiseDualTileLdsBytes(kDenoiseDualMaxWindow, kDenoiseDualMaxPatch);  // 132 832 B
static_assert(kDenoiseDualTileLdsMaxBytes <= 160 * 1024, "a workgroup's LDS at the limits fits a CU");
// The lanes of the tile form's workgroup when MCRT_DENOISE_DUAL_LANES does not say: the terms and the row sums of an offset are dealt to
// all of them, and only they hide the latency of its divisions. Above half a CU's LDS one workgroup has the CU to itself and takes all 16
// waves it can hold; below, two or three workgroups share it and 8 waves each were faster (measured at 1080p: (5, 2) 14.9 / 10.1 / 8.7 ms
// and (8, 3) 44.2 / 30.3 / 25.2 ms at 256 / 512 / 1024 lanes, (3, 1) 2.87 / 2.34 / 2.98 ms; profiles/NOTES_denoise_dual.md).
constexpr uint32_t denoiseDualTileLanes(uint32_t R, uint32_t F) { return denoiseDualTileLdsBytes(R, F) > 80 * 1024 ? 1024u : 512u; }

MCRT_HD uint64_t denoiseDualTileBlocks(uint32_t width, uint32_t height) {
    return (uint64_t)((width + kDenoiseTile - 1) / kDenoiseTile) * ((height + kDenoiseTile - 1) / kDenoiseTile);
}
// How many of c + i, i = -F .. F, are inside [0, size) together with c + i + d: the patch elements of one axis that count.
MCRT_HD uint32_t denoiseDualCount(int64_t c, int64_t d, int64_t F, int64_t size) {
    int64_t lo = -F, hi = F;
    if (-c > lo) lo = -c;
    if (-c - d > lo) lo = -c - d;
    if (size - 1 - c < hi) hi = size - 1 - c;
    if (size - 1 - c - d < hi) hi = size - 1 - c - d;
    return hi >= lo ? (uint32_t)(hi - lo + 1) : 0u;
}

#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

// One workgroup (`lanes` lanes, a multiple of 64 and at least 256, `tid` of them this one) at patch radius F; lds:
// denoiseDualTileLdsWords(R, F) doubles. Every lane takes part in the staging, the terms and the row sums; the first 256 own a pixel.
template <uint32_t F>
__device__ __forceinline__ void denoiseDualTileBlockF(const DenoiseDualStep& st, uint32_t block, uint32_t tid, uint32_t lanes, double* lds) {
    constexpr uint32_t T = kDenoiseTile, E = T + 2 * F, E2 = E * E;
    const int R = (int)st.window_radius;
    const uint32_t halo = (uint32_t)R + F, side = T + 2 * halo, nrec = side * side;
    double* rec = lds;                                  // [9][nrec]
    double* el = lds + kDenoiseDualRecWords * nrec;     // [6][E2]: half x channel, element position
    double* rs = el + 6 * E2;                           // [2][E][T]: half, element row, pixel column
    const uint32_t tiles_x = (st.width + T - 1) / T;
    const int64_t x0 = (int64_t)(block % tiles_x) * T, y0 = (int64_t)(block / tiles_x) * T;
    for (uint32_t r = tid; r < nrec; r += lanes) {
        const int64_t gx = x0 - (int64_t)halo + (int64_t)(r % side), gy = y0 - (int64_t)halo + (int64_t)(r / side);
        if (!denoiseDualInside(gx, gy, st.width, st.height)) continue;  // never read
        const double* src = st.rec + ((uint64_t)gy * st.width + (uint64_t)gx) * kDenoiseDualRecWords;
#pragma unroll
        for (uint32_t k = 0; k < kDenoiseDualRecWords; k++) rec[k * nrec + r] = src[k];
    }
    __syncthreads();
    const uint32_t lx = tid % T, ly = tid / T;
    const int64_t x = x0 + lx, y = y0 + ly;
    const bool active = tid < T * T && x < (int64_t)st.width && y < (int64_t)st.height;  // every lane takes part in the cooperative steps
    const uint32_t rc = (ly + halo) * side + lx + halo;                   // the lane's own record
    DenoiseDualAcc acc;
    for (int dy = -R; dy <= R; dy++) {
        for (int dx = -R; dx <= R; dx++) {
            if (dx == 0 && dy == 0) {
                if (active) acc.add(1.0, 1.0, d3{rec[rc], rec[nrec + rc], rec[2 * nrec + rc]}, d3{rec[3 * nrec + rc], rec[4 * nrec + rc], rec[5 * nrec + rc]});
                continue;
            }
            // 1. the terms of this offset: element (ex, ey) of the tile's (16 + 2F)^2, half and channel hc = 3 half + ch
            for (uint32_t it = tid; it < 6 * E2; it += lanes) {
                const uint32_t hc = it / E2, pos = it % E2, ey = pos / E, ex = pos % E;
                const int64_t gx = x0 - (int64_t)F + ex, gy = y0 - (int64_t)F + ey;
                if (!denoiseDualInside(gx, gy, st.width, st.height) || !denoiseDualInside(gx + dx, gy + dy, st.width, st.height)) continue;
                const uint32_t rp = (ey + (uint32_t)R) * side + ex + (uint32_t)R;
                const uint32_t rq = (uint32_t)((int)rp + dy * (int)side + dx);
                const uint32_t vf = 6 + (hc < 3 ? hc : hc - 3);
                el[it] = denoiseDualTerm(st, rec[hc * nrec + rp], rec[hc * nrec + rq], rec[vf * nrec + rp], rec[vf * nrec + rq], hc < 3 ? st.ia : st.ib);
            }
            __syncthreads();
            // 2. the row sums: pixel column cx, element row ry, elements i = -F .. F and their channels in the stated order
            for (uint32_t it = tid; it < 2 * E * T; it += lanes) {
                const uint32_t half = it / (E * T), rem = it % (E * T), ry = rem / T, cx = rem % T;
                const int64_t gy = y0 - (int64_t)F + ry;
                double row = 0.0;
                if (gy >= 0 && gy < (int64_t)st.height && gy + dy >= 0 && gy + dy < (int64_t)st.height) {
                    const double* e = el + (3 * half) * E2 + ry * E + cx;
#pragma unroll
                    for (uint32_t i = 0; i <= 2 * F; i++) {
                        const int64_t gx = x0 + cx - (int64_t)F + i;
                        if (gx < 0 || gx >= (int64_t)st.width || gx + dx < 0 || gx + dx >= (int64_t)st.width) continue;
                        row = row + e[i];
                        row = row + e[E2 + i];
                        row = row + e[2 * E2 + i];
                    }
                }
                rs[it] = row;
            }
            __syncthreads();
            // 3. the pixel's 2F+1 row sums, the weights and the sums
            if (active && denoiseDualInside(x + dx, y + dy, st.width, st.height)) {
                double sa = 0.0, sb = 0.0;
#pragma unroll
                for (uint32_t j = 0; j <= 2 * F; j++) {
                    sa = sa + rs[(ly + j) * T + lx];
                    sb = sb + rs[E * T + (ly + j) * T + lx];
                }
                const uint32_t cnt = denoiseDualCount(x, dx, F, st.width) * denoiseDualCount(y, dy, F, st.height);
                const uint32_t rq = (uint32_t)((int)rc + dy * (int)side + dx);
                acc.add(denoiseDualWeight(sa, cnt), denoiseDualWeight(sb, cnt), d3{rec[rq], rec[nrec + rq], rec[2 * nrec + rq]},
                        d3{rec[3 * nrec + rq], rec[4 * nrec + rq], rec[5 * nrec + rq]});
            }
        }
    }
    if (active) denoiseDualStore(st, (uint64_t)y * st.width + (uint64_t)x, acc);
}

// ... at st.patch_radius (1 .. 3, uniform over the launch).
__device__ __forceinline__ void denoiseDualTileBlock(const DenoiseDualStep& st, uint32_t block, uint32_t tid, uint32_t lanes, double* lds) {
    if (st.patch_radius == 1) denoiseDualTileBlockF<1>(st, block, tid, lanes, lds);
    else if (st.patch_radius == 2) denoiseDualTileBlockF<2>(st, block, tid, lanes, lds);
    else denoiseDualTileBlockF<3>(st, block, tid, lanes, lds);
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

}  // namespace mcrt
