// Frame comparison (include/mcrt.h "Frame comparison", mcrt_frame_compare*): the text of the three gfx950 kernels of mcrt_compare.hip,
// shared with the host emulation of the CPU tests (tests/emu/compare_emu.cpp): both run this file. Only FP64 + - * /, compare and
// select, in the order include/mcrt.h states, built uncontracted like the rest of the exact build.
//
// comparePixelsKernel is level 0 of the header's treesum and the one read of the two frames and the mask: a workgroup per block of 256
// consecutive pixels, a lane per pixel. The layout is chosen for the sums, not for the loads: the tree pairs PIXEL k with pixel
// k + stride, so a lane has to end up with the three channels of one pixel - but a pixel is 24 bytes, and no split of 24-byte records
// over lanes gives every lane one aligned 16-byte load (odd pixels start at 8 mod 16). So the block's 256 x 3 words of either frame -
// 6 144 consecutive bytes, which start 16-byte aligned whenever the frame does, 256 * 24 being a multiple of 16 - are first copied to
// LDS word for word with lanes along WORDS (16-byte loads, as pixelStatsLoad does them, where both frames are 16-byte aligned; 8-byte
// loads otherwise; a ragged block's odd last word alone), and then every lane reads its own pixel's three words back from LDS. The
// channels straddle lanes in the copy and nowhere else. The mask and the maps are one word per pixel: plain 8-byte accesses per lane.
// The staging area is reused for the tree (a barrier between). The counts are ballots per wavefront, added up per block and then along
// the levels like the sums (integers: any order gives the same) - not atomics: nearly every pixel of a real pair of frames differs, and
// 32 400 wavefronts of a 1080p frame adding to one address take longer than reading the frames (measured: profiles/NOTES_compare.md).
// The maximum is a (value, index) pair, index = pixel * 3 + channel, the lower index winning ties, which is associative, so it rides
// along the sums' strides too. Only the SSIM's excluded centres - none in a finite frame - are counted with an atomic.
//
// compareLevelKernel is one upper level of the treesum for up to four sums at once (se, ae, rel and - with SSIM - ssim, whose column
// starts from the per-centre values and so has a length of its own) and for the maximum's pairs. A column of one value passes through.
//
// compareSsimKernel: a workgroup owns a tile of kTileW x kTileH centres; it stages the luminances Lx, Lr of the tile plus a 5-pixel halo
// in LDS, writes the five horizontal sums of the (kTileH + 10) x kTileW positions to LDS, and does the vertical pass and the ssim
// formula per centre. Every centre's value is a function of its own window in the header's order - nothing is summed across centres
// here - and goes to the per-centre array in row-major order of the centre grid, from which the treesum takes its blocks: so no result
// depends on the tile shape. LDS at 32 x 16: 2 * 42 * 26 * 8 + 5 * 26 * 32 * 8 = 50 752 bytes, three workgroups (12 waves) per CU of
// 160 KB; the halo makes 2.1 staged pixels per centre (2.6 at 16 x 16), and a lane owns two centres.
#pragma once

#include "../../include/mcrt.h"
#include "mcrt_math.hpp"
#include "mcrt_robust.hpp"

namespace mcrt {

constexpr uint32_t kCompareBlock = 256;    // the treesum's block: values and lanes (include/mcrt.h, mcrt_frame_noise)
constexpr uint32_t kCompareColumns = 4;    // se, ae, rel, ssim
constexpr uint32_t kCompareStageWords = 2 * 3 * kCompareBlock;  // LDS of the pixel kernel, in doubles
constexpr uint64_t kCompareNoIndex = ~0ull;
enum { kCompareNonfinite, kCompareMasked, kCompareDiffering, kCompareCounts };  // the counted columns
constexpr uint32_t kSsimRadius = 5, kSsimTaps = 2 * kSsimRadius + 1;
constexpr uint32_t kSsimTileW = 32, kSsimTileH = 16;  // the library's tile
constexpr uint32_t kSsimBlock = 256;

inline uint64_t compareBlocks(uint64_t n) { return (n + kCompareBlock - 1) / kCompareBlock; }
inline uint32_t compareVec(const double* rgb, const double* ref) { return (((uintptr_t)rgb | (uintptr_t)ref) & 15u) == 0 ? 1u : 0u; }
inline uint64_t ssimCentres(uint32_t width, uint32_t height) {
    return width < kSsimTaps || height < kSsimTaps ? 0 : (uint64_t)(width - 2 * kSsimRadius) * (height - 2 * kSsimRadius);
}
constexpr uint32_t ssimLdsWords(uint32_t tw, uint32_t th) { return 2 * (tw + 2 * kSsimRadius) * (th + 2 * kSsimRadius) + 5 * tw * (th + 2 * kSsimRadius); }

// Level 0. Block b writes out_sum[c][b] (c = 0 se, 1 ae, 2 rel), out_max[b], out_idx[b] and out_cnt[k][b] (k: the enum above).
struct ComparePixels {
    const double *rgb, *ref, *mask;        // mask may be nullptr
    double *map_se, *map_rel, *map_zero;   // nullptr = not wanted; map_zero: the ssim map, 0.0 written where there is no centre
    double* out_sum[3];
    double* out_max;
    uint64_t* out_idx;
    uint64_t* out_cnt[kCompareCounts];
    uint64_t pixels;
    uint32_t width, height;
    uint32_t vec;  // compareVec
    double eps;
};

// An upper level. Column c has n[c] values in[c] (0: absent) and writes compareBlocks(n[c]) values out[c]; the pairs and the counts
// have n[0] entries.
struct CompareLevel {
    const double* in[kCompareColumns];
    double* out[kCompareColumns];
    uint64_t n[kCompareColumns];
    const double* in_max;
    const uint64_t* in_idx;
    double* out_max;
    uint64_t* out_idx;
    const uint64_t* in_cnt[kCompareCounts];
    uint64_t* out_cnt[kCompareCounts];
};
constexpr uint32_t kCompareLevelWords = (kCompareColumns + 2 + kCompareCounts) * kCompareBlock;  // LDS of the level kernel, in doubles
constexpr uint32_t kCompareRecordWords = kCompareColumns + 2 + kCompareCounts;  // what the last level leaves side by side
inline uint64_t compareLevelBlocks(const CompareLevel& lv) {
    uint64_t blocks = 0;
    for (uint32_t c = 0; c < kCompareColumns; c++) blocks = compareBlocks(lv.n[c]) > blocks ? compareBlocks(lv.n[c]) : blocks;
    return blocks;
}

struct CompareSsim {
    const double *rgb, *ref;
    double* values;  // [centres], row-major over the (width - 10) x (height - 10) grid: the ssim, or 0.0 where it is not finite
    double* map;     // [height][width] or nullptr: the same at the centres
    unsigned long long* excluded;  // the call's count of centres whose ssim is not finite
    uint32_t width, height;
    double c1, c2;
};
inline uint64_t ssimTiles(uint32_t width, uint32_t height, uint32_t tw, uint32_t th) {
    return ssimCentres(width, height) ? (uint64_t)((width - 2 * kSsimRadius + tw - 1) / tw) * ((height - 2 * kSsimRadius + th - 1) / th) : 0;
}

MCRT_HD bool compareFinite(double v) { return v - v == 0.0; }
MCRT_HD double compareAbs(double d) { return d < 0 ? 0.0 - d : d; }
// (value, index) pairs: a wins over b. "Nothing yet" is (-1.0, kCompareNoIndex): every a_c is >= 0.
MCRT_HD bool compareMaxWins(double av, uint64_t ai, double bv, uint64_t bi) { return av > bv || (av == bv && ai < bi); }
// g[k - 5] of include/mcrt.h, k = 0 .. 10 (a constant once the tap loops are unrolled)
MCRT_HD double ssimWeight(uint32_t k) {
    const uint32_t a = k < kSsimRadius ? kSsimRadius - k : k - kSsimRadius;
    return a == 0 ? MCRT_SSIM_G0 : a == 1 ? MCRT_SSIM_G1 : a == 2 ? MCRT_SSIM_G2 : a == 3 ? MCRT_SSIM_G3 : a == 4 ? MCRT_SSIM_G4 : MCRT_SSIM_G5;
}

#if defined(__HIPCC__) || defined(MCRT_WAVE_EMU)

typedef double CompareVec2 __attribute__((vector_size(16)));  // (one 16-byte load)

// `words` consecutive words of a frame to LDS, lanes along words. kVec: src is 16-byte aligned.
template <bool kVec>
__device__ __forceinline__ void compareStage(const double* src, uint32_t words, uint32_t tid, double* dst) {
    if (kVec) {
        for (uint32_t i = tid; i < words / 2; i += kCompareBlock) {
            const CompareVec2 q = *reinterpret_cast<const CompareVec2*>(src + 2 * i);
            dst[2 * i] = q[0];
            dst[2 * i + 1] = q[1];
        }
        if (tid == 0 && (words & 1u)) dst[words - 1] = src[words - 1];
    } else {
        for (uint32_t i = tid; i < words; i += kCompareBlock) dst[i] = src[i];
    }
}

// One workgroup (kCompareBlock lanes, `tid` of them this one); stage: kCompareStageWords doubles of LDS, 16-byte aligned. Every lane
// reaches every barrier and every ballot.
__device__ __forceinline__ void comparePixelsBlock(const ComparePixels& cp, uint64_t block, uint32_t tid, double* stage) {
    const uint64_t first = block * kCompareBlock;
    const uint64_t left = cp.pixels - first;
    const uint32_t len = left < kCompareBlock ? (uint32_t)left : kCompareBlock;
    double* sx = stage;
    double* sr = stage + 3 * kCompareBlock;
    if (cp.vec) {
        compareStage<true>(cp.rgb + first * 3, len * 3, tid, sx);
        compareStage<true>(cp.ref + first * 3, len * 3, tid, sr);
    } else {
        compareStage<false>(cp.rgb + first * 3, len * 3, tid, sx);
        compareStage<false>(cp.ref + first * 3, len * 3, tid, sr);
    }
    __syncthreads();
    const bool live = tid < len;
    const uint64_t p = first + tid;
    double se = 0.0, ae = 0.0, rel = 0.0, mx = -1.0;
    uint64_t mi = kCompareNoIndex;
    bool masked = false, nonfinite = false, differs = false;
    if (live) {
        const double x_r = sx[3 * tid], x_g = sx[3 * tid + 1], x_b = sx[3 * tid + 2];
        const double r_r = sr[3 * tid], r_g = sr[3 * tid + 1], r_b = sr[3 * tid + 2];
        masked = cp.mask ? !(cp.mask[p] > 0) : false;
        const bool fin = compareFinite(x_r) && compareFinite(x_g) && compareFinite(x_b) && compareFinite(r_r) && compareFinite(r_g) && compareFinite(r_b);
        nonfinite = !masked && !fin;
        differs = !masked && (__double_as_longlong(x_r) != __double_as_longlong(r_r) || __double_as_longlong(x_g) != __double_as_longlong(r_g) ||
                              __double_as_longlong(x_b) != __double_as_longlong(r_b));
        if (!masked && fin) {
            const double d_r = x_r - r_r, d_g = x_g - r_g, d_b = x_b - r_b;
            const double a_r = compareAbs(d_r), a_g = compareAbs(d_g), a_b = compareAbs(d_b);
            se = (d_r * d_r + d_g * d_g) + d_b * d_b;
            ae = (a_r + a_g) + a_b;
            rel = ((d_r * d_r) / (r_r * r_r + cp.eps) + (d_g * d_g) / (r_g * r_g + cp.eps)) + (d_b * d_b) / (r_b * r_b + cp.eps);
            mx = a_r, mi = p * 3;
            if (a_g > mx) mx = a_g, mi = p * 3 + 1;
            if (a_b > mx) mx = a_b, mi = p * 3 + 2;
        }
        if (cp.map_se) cp.map_se[p] = se;
        if (cp.map_rel) cp.map_rel[p] = rel;
        if (cp.map_zero) {
            const uint32_t y = (uint32_t)(p / cp.width), x = (uint32_t)(p - (uint64_t)y * cp.width);
            const bool centre = x >= kSsimRadius && x + kSsimRadius < cp.width && y >= kSsimRadius && y + kSsimRadius < cp.height;
            if (!centre) cp.map_zero[p] = 0.0;
        }
    }
    const unsigned long long b_nonfinite = waveBallot(nonfinite), b_masked = waveBallot(masked), b_differs = waveBallot(differs);
    __syncthreads();  // the staged words are read: the area becomes the tree's
    double *t0 = stage, *t1 = stage + kCompareBlock, *t2 = stage + 2 * kCompareBlock, *tm = stage + 3 * kCompareBlock;
    uint64_t* ti = reinterpret_cast<uint64_t*>(stage + 4 * kCompareBlock);
    uint64_t* tc = reinterpret_cast<uint64_t*>(stage + 5 * kCompareBlock);  // [wavefront][kCompareCounts]
    if (live) t0[tid] = se, t1[tid] = ae, t2[tid] = rel, tm[tid] = mx, ti[tid] = mi;
    if ((tid & 63u) == 0) {
        uint64_t* mine = tc + (tid / 64u) * kCompareCounts;
        mine[kCompareNonfinite] = (uint64_t)__popcll(b_nonfinite);
        mine[kCompareMasked] = (uint64_t)__popcll(b_masked);
        mine[kCompareDiffering] = (uint64_t)__popcll(b_differs);
    }
    __syncthreads();
    for (uint32_t stride = kCompareBlock / 2; stride > 0; stride >>= 1) {
        if (tid < stride && tid + stride < len) {
            t0[tid] = t0[tid] + t0[tid + stride];
            t1[tid] = t1[tid] + t1[tid + stride];
            t2[tid] = t2[tid] + t2[tid + stride];
            if (compareMaxWins(tm[tid + stride], ti[tid + stride], tm[tid], ti[tid])) tm[tid] = tm[tid + stride], ti[tid] = ti[tid + stride];
        }
        __syncthreads();
    }
    if (tid == 0) {
        cp.out_sum[0][block] = t0[0];
        cp.out_sum[1][block] = t1[0];
        cp.out_sum[2][block] = t2[0];
        cp.out_max[block] = tm[0];
        cp.out_idx[block] = ti[0];
#pragma unroll
        for (uint32_t k = 0; k < kCompareCounts; k++) {
            uint64_t sum = 0;
            for (uint32_t w = 0; w < kCompareBlock / 64u; w++) sum += tc[w * kCompareCounts + k];
            cp.out_cnt[k][block] = sum;
        }
    }
}

// One workgroup of an upper level; t: kCompareLevelWords doubles of LDS. Every lane reaches every barrier.
__device__ __forceinline__ void compareLevelBlock(const CompareLevel& lv, uint64_t block, uint32_t tid, double* t) {
    const uint64_t first = block * kCompareBlock;
    uint32_t len[kCompareColumns];
#pragma unroll
    for (uint32_t c = 0; c < kCompareColumns; c++) {
        const uint64_t left = lv.n[c] > first ? lv.n[c] - first : 0;
        len[c] = left < kCompareBlock ? (uint32_t)left : kCompareBlock;
        if (tid < len[c]) t[c * kCompareBlock + tid] = lv.in[c][first + tid];
    }
    double* tm = t + kCompareColumns * kCompareBlock;
    uint64_t* ti = reinterpret_cast<uint64_t*>(t + (kCompareColumns + 1) * kCompareBlock);
    uint64_t* tc = reinterpret_cast<uint64_t*>(t + (kCompareColumns + 2) * kCompareBlock);  // [kCompareCounts][kCompareBlock]
    if (tid < len[0]) {
        tm[tid] = lv.in_max[first + tid], ti[tid] = lv.in_idx[first + tid];
#pragma unroll
        for (uint32_t k = 0; k < kCompareCounts; k++) tc[k * kCompareBlock + tid] = lv.in_cnt[k][first + tid];
    }
    __syncthreads();
    for (uint32_t stride = kCompareBlock / 2; stride > 0; stride >>= 1) {
        if (tid < stride) {
#pragma unroll
            for (uint32_t c = 0; c < kCompareColumns; c++)
                if (tid + stride < len[c]) t[c * kCompareBlock + tid] = t[c * kCompareBlock + tid] + t[c * kCompareBlock + tid + stride];
            if (tid + stride < len[0]) {
                if (compareMaxWins(tm[tid + stride], ti[tid + stride], tm[tid], ti[tid])) tm[tid] = tm[tid + stride], ti[tid] = ti[tid + stride];
#pragma unroll
                for (uint32_t k = 0; k < kCompareCounts; k++) tc[k * kCompareBlock + tid] += tc[k * kCompareBlock + tid + stride];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (uint32_t c = 0; c < kCompareColumns; c++)
            if (len[c]) lv.out[c][block] = t[c * kCompareBlock];
        if (len[0]) {
            lv.out_max[block] = tm[0], lv.out_idx[block] = ti[0];
#pragma unroll
            for (uint32_t k = 0; k < kCompareCounts; k++) lv.out_cnt[k][block] = tc[k * kCompareBlock];
        }
    }
}

// One workgroup (kSsimBlock lanes) and its tile of kTileW x kTileH centres; lds: ssimLdsWords(kTileW, kTileH) doubles.
template <uint32_t kTileW, uint32_t kTileH>
__device__ __forceinline__ void compareSsimBlock(const CompareSsim& cs, uint64_t block, uint32_t tid, double* lds) {
    constexpr uint32_t kStageW = kTileW + 2 * kSsimRadius, kStageH = kTileH + 2 * kSsimRadius;
    const uint32_t cw = cs.width - 2 * kSsimRadius, ch = cs.height - 2 * kSsimRadius;  // the centre grid
    const uint32_t tiles_x = (cw + kTileW - 1) / kTileW;
    const uint32_t x0 = (uint32_t)(block % tiles_x) * kTileW, y0 = (uint32_t)(block / tiles_x) * kTileH;  // the tile's first centre in the grid = its first staged pixel in the frame
    double* lx = lds;
    double* lr = lds + kStageW * kStageH;
    double* h = lds + 2 * kStageW * kStageH;  // [5][kStageH][kTileW]
    for (uint32_t i = tid; i < kStageW * kStageH; i += kSsimBlock) {
        const uint32_t sy = i / kStageW, sx = i % kStageW;
        const uint32_t x = x0 + sx, y = y0 + sy;
        double a = 0.0, b = 0.0;  // (past the frame: read by no centre of the grid)
        if (x < cs.width && y < cs.height) {
            const uint64_t q = ((uint64_t)y * cs.width + x) * 3;
            a = robustLuminance(cs.rgb[q], cs.rgb[q + 1], cs.rgb[q + 2]);
            b = robustLuminance(cs.ref[q], cs.ref[q + 1], cs.ref[q + 2]);
        }
        lx[i] = a;
        lr[i] = b;
    }
    __syncthreads();
    for (uint32_t i = tid; i < kStageH * kTileW; i += kSsimBlock) {
        const uint32_t row = i / kTileW, c = i % kTileW;
        if (x0 + c >= cw) continue;
        double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
#pragma unroll
        for (uint32_t k = 0; k < kSsimTaps; k++) {
            const double g = ssimWeight(k), a = lx[row * kStageW + c + k], b = lr[row * kStageW + c + k];
            h0 = h0 + g * a;
            h1 = h1 + g * b;
            h2 = h2 + g * (a * a);
            h3 = h3 + g * (b * b);
            h4 = h4 + g * (a * b);
        }
        h[i] = h0;
        h[kStageH * kTileW + i] = h1;
        h[2 * kStageH * kTileW + i] = h2;
        h[3 * kStageH * kTileW + i] = h3;
        h[4 * kStageH * kTileW + i] = h4;
    }
    __syncthreads();
    unsigned long long bad = 0;
    for (uint32_t i = tid; i < kTileH * kTileW; i += kSsimBlock) {
        const uint32_t r = i / kTileW, c = i % kTileW;
        const uint32_t cx = x0 + c, cy = y0 + r;
        if (cx >= cw || cy >= ch) continue;
        double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0, w4 = 0.0;
#pragma unroll
        for (uint32_t k = 0; k < kSsimTaps; k++) {
            const double g = ssimWeight(k);
            const uint32_t j = (r + k) * kTileW + c;
            w0 = w0 + g * h[j];
            w1 = w1 + g * h[kStageH * kTileW + j];
            w2 = w2 + g * h[2 * kStageH * kTileW + j];
            w3 = w3 + g * h[3 * kStageH * kTileW + j];
            w4 = w4 + g * h[4 * kStageH * kTileW + j];
        }
        const double mx = w0, mr = w1;
        const double sxx = w2 - mx * mx, srr = w3 - mr * mr, sxr = w4 - mx * mr;
        const double s = ((2.0 * (mx * mr) + cs.c1) * (2.0 * sxr + cs.c2)) / (((mx * mx + mr * mr) + cs.c1) * ((sxx + srr) + cs.c2));
        const bool fin = compareFinite(s);
        const double v = fin ? s : 0.0;
        if (!fin) bad++;
        cs.values[(uint64_t)cy * cw + cx] = v;
        if (cs.map) cs.map[(uint64_t)(cy + kSsimRadius) * cs.width + (cx + kSsimRadius)] = v;
    }
    if (bad) atomicAdd(cs.excluded, bad);
}

#endif  // __HIPCC__ || MCRT_WAVE_EMU

// The parameters with their defaults in, or the reason they are refused.
struct CompareSettings {
    double eps, peak, range;
    bool ssim;
};
inline int compareSettings(const mcrt_compare_params* params, CompareSettings* s, const char** why) {
    *s = CompareSettings{0.01, 1.0, 1.0, true};
    if (!params) return MCRT_OK;
    const double v[3] = {params->eps, params->peak, params->ssim_range};
    for (double x : v)
        if (!(x - x == 0.0) || x < 0.0) return *why = "eps, peak and ssim_range must be finite and positive (0 = the default)", MCRT_ERR_INVALID;
    if (params->eps != 0.0) s->eps = params->eps;
    if (params->peak != 0.0) s->peak = params->peak;
    if (params->ssim_range != 0.0) s->range = params->ssim_range;
    s->ssim = params->want_ssim != 0;
    return MCRT_OK;
}

// The host's part of the result: the derived figures from the sums and the counts (include/mcrt.h).
// max_index: the winning pair's pixel * 3 + channel, kCompareNoIndex when nothing was compared.
inline void compareFinish(mcrt_compare_result* r, const CompareSettings& s, uint64_t max_index) {
    r->compared = r->pixels - r->nonfinite - r->masked;
    r->max_abs_pixel = max_index == kCompareNoIndex ? kCompareNoIndex : max_index / 3;
    r->max_abs_channel = max_index == kCompareNoIndex ? 0xFFFFFFFFu : (uint32_t)(max_index % 3);
    r->reserved = 0;
    if (max_index == kCompareNoIndex) r->max_abs = 0.0;
    r->mse = r->mae = r->relmse = r->rmse = r->psnr = r->mean_ssim = 0.0;
    if (r->compared) {
        const double n = (double)(3 * r->compared);
        r->mse = r->sum_se / n;
        r->mae = r->sum_ae / n;
        r->relmse = r->sum_rel / n;
        r->rmse = std::sqrt(r->mse);
        r->psnr = r->mse == 0.0 ? HUGE_VAL : 10.0 * std::log10(s.peak * s.peak / r->mse);
    }
    if (r->ssim_centres > r->ssim_excluded) r->mean_ssim = r->sum_ssim / (double)(r->ssim_centres - r->ssim_excluded);
}

}  // namespace mcrt
