// Filtered planes (include/mcrt.h "Filtered planes"): the light groups' and the path classes' planes through the camera's film, as a
// GATHER in a fixed order over the samples' radiances, which the walk keeps until its resolve. The per-lane text of the three branches
// the feature adds to lightGroupsResolveKernel (csrc/mcrt_light_groups.hip) and pathClassesResolveKernel (csrc/mcrt_path_classes.hip),
// shared with the host emulation of the CPU tests (tests/emu/film_gather_emu.cpp): all three run this file. The film itself -
// filmFilterFunction, the table's index, the coverage window of filmDeposit - is mcrt_film.hpp's, the table and the view mcrt_launch.hpp's.
// Every operation is the one include/mcrt.h writes down, in that order, uncontracted.
//
// A sample's weight at output pixel (qx, qy) is filter(qy + 0.5 - py) * filter(qx + 0.5 - px): separable, and the 2H + 1 columns and
// 2H + 1 rows a sample can cover are known from its pixel alone. So the first branch writes, per sample, the filter's value for each of
// them - the ROWS, one lane per value - and the gather multiplies two of them per covering sample. The gather's loops then hold no
// filter at all: neither a polynomial's coefficients nor exp nor the sines of Lanczos live across them, and the kernels keep their
// eight waves a SIMD (profiles/NOTES_film_gather.md has the numbers of the shape that recomputed the weights in the gather).
// Both kernels state no LDS, so what the shading kernels read from there comes from memory here: the Sobol byte tables (filmGatherGet)
// and the sine table of the Lanczos filter (filmFilterFunction<false>).
#pragma once

#include "mcrt_film.hpp"
#include "mcrt_light_groups.hpp"

namespace mcrt {

enum : uint32_t {
    kFilmGatherNone = 0,       // the kernel's plain resolve: nothing of FilmGather is read
    kFilmGatherOffsets = 1,    // one lane per (row, sample of the chunk): the sample's film-position pair and its weight rows
    kFilmGatherGather = 2,     // one lane per (output pixel the chunk can reach, plane): S and W continued
    kFilmGatherNormalise = 3,  // one lane per output word, after the last chunk: S / W in place
};

// The launch-uniform argument. Zeroed: mode kFilmGatherNone.
struct FilmGather {
    uint32_t mode;
    uint32_t clamp;             // normalise: max(., 0) on every word
    FilmView film;              // makeFilmView of the camera; blob is not used
    const uint32_t* sobol_tab;  // the byte tables in memory (offsets)
    double* offset;             // [chunk samples][2] get(kDimPixel), get(kDimPixel + 1) of record i * c.pixels + p
    double* rows;               // [2][2H + 1][chunk samples]: x then y; entry k of a sample of pixel x is filter((x + k - H) + 0.5 - px),
                                // 0.0 where the sample does not cover that column (row); the stride is THIS chunk's sample count
    double* weight;             // [frame_pixels] W
    uint64_t first_out;         // gather: the packed output pixels [first_out, first_out + outs) ...
    uint32_t outs;
    uint32_t halo;              // ... the chunk's rows widened by H = ceil(radius + 0.5), clipped to the frame
};

// H of a radius: a sample of pixel x lies in [x, x + 1) and covers qx only if |qx - x| < radius + 0.5.
inline uint32_t filmGatherHalo(double radius) {
    const double h = radius + 0.5;
    uint32_t H = (uint32_t)h;
    if ((double)H < h) H++;
    return H;
}
// Doubles of `rows` per sample.
inline uint64_t filmGatherRowWords(double radius) { return 2ull * (2ull * filmGatherHalo(radius) + 1ull); }

// first_out, outs and halo of `g` for chunk c of a frame of cam.width x cam.height pixels (unsharded: packed pixel q is row q / width).
inline void filmGatherReach(FilmGather& g, const AovChunk& c) {
    const uint64_t width = c.cam.width, height = c.cam.height;
    const uint64_t y0 = c.first_pixel / width, y1 = (c.first_pixel + c.pixels - 1) / width;
    g.halo = filmGatherHalo(g.film.radius);
    const uint64_t r0 = y0 > g.halo ? y0 - g.halo : 0, r1 = y1 + g.halo < height - 1 ? y1 + g.halo : height - 1;
    g.first_out = r0 * width;
    g.outs = (uint32_t)((r1 + 1 - r0) * width);
}

// Sampler::get(dim) with the byte tables in memory: the same words, the same scramble.
MCRT_HD double filmGatherGet(const Sampler& smp, int dim, const uint32_t* tab) {
    uint32_t x = smp.shuffled_index;
    if (dim != 0) {
        const uint32_t* t = tab + (dim - 1) * 1024;
        const uint32_t i = smp.shuffled_index;
        x = t[i & 255u] ^ t[256 + ((i >> 8) & 255u)] ^ t[512 + ((i >> 16) & 255u)] ^ t[768 + (i >> 24)];
    }
    return owenScramble(x, hashCombine(smp.seed, hash32((uint32_t)dim))) * 0x1p-32;
}

// Would filmDeposit (mcrt_film.hpp) write a sample at film coordinate t (px or py) to the pixel column or row q of `size`? Its window,
// its clipping, one axis at a time. (Its truncations are to long long; a coordinate is below 2^31 here - filmGatherLaunchable - and
// the radius is what is left of an int's range: the same integers.)
MCRT_HD bool filmGatherCovers(double radius, double t, int q, int size) {
    const double a = t + 0.5 - radius, b = t - 0.5 + radius;
    int lo = a > 0.0 ? (a < 2147483520.0 ? (int)a : 2147483647) : 0;
    int hi = b > -1.0 ? (b < 2147483520.0 ? (int)b : 2147483647) : -1;
    if (hi > size - 1) hi = size - 1;
    return q >= lo && q <= hi;
}

// filmFilter (mcrt_film.hpp) of a film whose type is kType - a constant, so that a lane holds the constants of its own filter only.
template <uint32_t kType>
MCRT_HD double filmGatherFilter(const FilmView& f, double x) {
    if (f.cache_size == 0) return filmFilterFunction<false>(kType, f.two_inv_radius * fabs(x));
    return f.cache[(size_t)(f.inv_dx * fabs(x) + 0.5)];
}

// offsets, lane (row, r) over the n samples of the chunk (fewer than 2^32: one closest-hit search took their camera rays): row = axis *
// (2H + 1) + k. Record r is sample r / c.pixels of the chunk's pixel r % c.pixels; the lane draws that sample's coordinate of the axis - the camera ray's own pair -, the lanes of k == 0 store it,
// and every lane stores the filter's value at column (row) pixel + k - H, or 0.0 where the sample does not cover it.
template <uint32_t kType>
MCRT_HD void filmGatherOffsetLaneOf(const AovChunk& c, const FilmGather& g, uint32_t row, uint32_t r) {
    const uint32_t n = c.pixels * c.spp, per_axis = 2u * g.halo + 1u;
    const uint32_t axis = row >= per_axis ? 1u : 0u, k = row - axis * per_axis;
    const uint32_t p = r % c.pixels;
    const uint32_t q0 = (uint32_t)chunkPixel(c, p), x = q0 % c.cam.width, y = q0 / c.cam.width;  // (unsharded: the packed row is the frame's)
    Sampler smp;
    smp.initiate(chunkSeed(c, p), y * c.cam.width + x);
    smp.setIndex(r / c.pixels);
    const double u = filmGatherGet(smp, kDimPixel + (int)axis, g.sobol_tab);
    if (k == 0u) g.offset[2ull * r + axis] = u;
    const uint32_t pixel = axis == 0u ? x : y;
    const double t = (double)pixel + u;
    const int q = (int)pixel + (int)k - (int)g.halo, size = (int)(axis == 0u ? c.cam.width : c.cam.height);
    double w = 0.0;
    if (q >= 0 && filmGatherCovers(g.film.radius, t, q, size)) w = filmGatherFilter<kType>(g.film, (double)q + 0.5 - t);
    g.rows[(uint64_t)row * n + r] = w;
}
MCRT_HD void filmGatherOffsetLane(const AovChunk& c, const FilmGather& g, uint32_t row, uint32_t r) {
    switch (g.film.type) {  // (the launch's: every lane takes the same case)
        case MCRT_FILM_MITCHELL_NETRAVALI: return filmGatherOffsetLaneOf<MCRT_FILM_MITCHELL_NETRAVALI>(c, g, row, r);
        case MCRT_FILM_CATMULL_ROM: return filmGatherOffsetLaneOf<MCRT_FILM_CATMULL_ROM>(c, g, row, r);
        case MCRT_FILM_B_SPLINE: return filmGatherOffsetLaneOf<MCRT_FILM_B_SPLINE>(c, g, row, r);
        case MCRT_FILM_HERMITE: return filmGatherOffsetLaneOf<MCRT_FILM_HERMITE>(c, g, row, r);
        case MCRT_FILM_GAUSSIAN: return filmGatherOffsetLaneOf<MCRT_FILM_GAUSSIAN>(c, g, row, r);
        case MCRT_FILM_LANCZOS: return filmGatherOffsetLaneOf<MCRT_FILM_LANCZOS>(c, g, row, r);
        default: return filmGatherOffsetLaneOf<kFilmBoxSplat>(c, g, row, r);
    }
}

// gather, lane (plane, o): output pixel q = g.first_out + o of that plane. The window's pixels that lie in the
// chunk, in ascending packed order, their samples in ascending index: S of the plane's three words in `out` and - plane 0's lane
// alone reads and writes it - W in g.weight are continued where the chunk before left them. Consecutive lanes are consecutive pixels
// of one plane: every read of a neighbour's offsets, rows and radiances is one of consecutive words. The coverage test is the
// sample's own, from its film position; the weight is the product of its row's and its column's entry, y first as in filmDeposit.
// (32-bit coordinates: a frame has fewer than 2^32 pixels, a row fewer than 2^31 - filmGatherLaunchable. Loops not unrolled: registers.)
MCRT_HD void filmGatherLane(const AovChunk& c, const LgState& st, const FilmGather& g, uint32_t plane, uint32_t o, double* out, uint64_t frame_pixels) {
    const uint32_t q = (uint32_t)g.first_out + o;
    const int width = (int)c.cam.width, height = (int)c.cam.height, H = (int)g.halo;
    const int qx = (int)(q % c.cam.width), qy = (int)(q / c.cam.width);
    const uint32_t first = (uint32_t)c.first_pixel, last = first + (c.pixels - 1u);
    const uint32_t n = c.pixels * c.spp;
    // A sample of pixel s covers q only if |q - s| <= H - 1 = ceil(radius - 0.5): its coordinate is in [s, s + 1), and filmDeposit's window
    // ends at trunc(coordinate - 0.5 + radius) < s + 0.5 + radius and begins at trunc(coordinate + 0.5 - radius) >= s + 0.5 - radius
    // - 1 rounded up. So the loops walk (2H - 1)^2 pixels, 25 and not 49 at radius 2; H is what a chunk can reach, rounded up.
    int y0 = qy - (H - 1), y1 = qy + (H - 1), x0 = qx - (H - 1), x1 = qx + (H - 1);
    if (y0 < (int)(first / c.cam.width)) y0 = (int)(first / c.cam.width);  // (the chunk's rows: every other row of the window has no pixel of it)
    if (y1 > (int)(last / c.cam.width)) y1 = (int)(last / c.cam.width);
    if (x0 < 0) x0 = 0;
    if (x1 > width - 1) x1 = width - 1;
    double* s = out + ((uint64_t)plane * frame_pixels + q) * 3u;
    const double* r = st.radiance + (uint64_t)(3u * plane) * st.n;
    d3 S = ld3(s);
    double W = plane == 0u ? g.weight[q] : 0.0;
#pragma clang loop unroll(disable)
    for (int sy = y0; sy <= y1; sy++) {
        const double* wy = g.rows + (uint64_t)(2 * H + 1 + (qy - sy + H)) * n;
#pragma clang loop unroll(disable)
        for (int sx = x0; sx <= x1; sx++) {
            const uint32_t sq = (uint32_t)sy * c.cam.width + (uint32_t)sx;
            if (sq < first || sq > last) continue;
            const double* wx = g.rows + (uint64_t)(qx - sx + H) * n;
#pragma clang loop unroll(disable)
            for (uint32_t i = 0; i < c.spp; i++) {
                const uint32_t at = i * c.pixels + (sq - first);
                const double px = (double)sx + g.offset[2ull * at], py = (double)sy + g.offset[2ull * at + 1];
                if (!filmGatherCovers(g.film.radius, px, qx, width) || !filmGatherCovers(g.film.radius, py, qy, height)) continue;
                const double w = wy[at] * wx[at];
                S = S + d3{r[at], r[st.n + at], r[2 * st.n + at]} * w;
                W = W + w;
            }
        }
    }
    s[0] = S.x;
    s[1] = S.y;
    s[2] = S.z;
    if (plane == 0u) g.weight[q] = W;
}

// normalise, lane (plane, q): the three words of a pixel of a plane - Splat::get without its clamp, or with it.
MCRT_HD void filmGatherNormaliseLane(const FilmGather& g, uint32_t plane, uint32_t q, double* out, uint64_t frame_pixels) {
    const double w = g.weight[q];
    double* s = out + ((uint64_t)plane * frame_pixels + q) * 3u;
    for (int k = 0; k < 3; k++) {
        double v = w == 0.0 ? 0.0 : s[k] / w;
        if (g.clamp) v = gmax(v, 0.0);
        s[k] = v;
    }
}

// The lanes of a launch - rows (the kernels' blockIdx.y) of `x` lanes each, both below 2^32 - and what lane (row, x) does: the branch
// both resolve kernels and the emulation take for g.mode != 0.
MCRT_HD uint32_t filmGatherLaneRows(uint32_t planes, const FilmGather& g) { return g.mode == kFilmGatherOffsets ? 2u * (2u * g.halo + 1u) : planes; }
MCRT_HD uint32_t filmGatherLanesX(const AovChunk& c, const FilmGather& g, uint64_t frame_pixels) {
    return g.mode == kFilmGatherOffsets ? c.pixels * c.spp : g.mode == kFilmGatherGather ? g.outs : (uint32_t)frame_pixels;
}
MCRT_HD void filmGatherDo(const AovChunk& c, const LgState& st, const FilmGather& g, uint32_t row, uint32_t x, double* out, uint64_t frame_pixels) {
    if (g.mode == kFilmGatherOffsets) filmGatherOffsetLane(c, g, row, x);
    else if (g.mode == kFilmGatherGather) filmGatherLane(c, st, g, row, x, out, frame_pixels);
    else filmGatherNormaliseLane(g, row, x, out, frame_pixels);
}

// What a launch may not be asked: a mode that is none of the three, arrays that are missing, a chunk past the frame or the state, a
// halo that is not the radius's. (g.first_out, g.outs and g.halo are filmGatherReach's.)
inline bool filmGatherLaunchable(const AovChunk& c, const LgState& st, uint32_t planes, const FilmGather& g, const double* out, uint64_t frame_pixels) {
    if (g.mode < kFilmGatherOffsets || g.mode > kFilmGatherNormalise || planes == 0u || planes > kLgPlanesMax || !out || !g.weight) return false;
    if (g.mode == kFilmGatherNormalise) return frame_pixels <= 0xFFFFFFFFull;
    if (!g.offset || !g.rows || c.pixels == 0u || c.first_pixel + c.pixels > frame_pixels || (uint64_t)c.pixels * c.spp > st.n || (uint64_t)c.pixels * c.spp > 0xFFFFFFFFull) return false;
    if (g.halo > 16383u || c.cam.shard_count > 1) return false;
    if (frame_pixels != (uint64_t)c.cam.width * c.cam.height || g.film.width != c.cam.width || g.film.height != c.cam.height) return false;
    if (c.cam.width > 0x7FFFFFFFu || c.cam.height > 0x7FFFFFFFu || frame_pixels > 0xFFFFFFFFull) return false;  // (the 32-bit coordinates)
    if (!(g.film.radius > 0.0) || !(g.film.radius < 1e6) || g.halo != filmGatherHalo(g.film.radius)) return false;
    if (g.film.cache_size != 0u && !g.film.cache) return false;
    if (g.mode == kFilmGatherOffsets) return g.sobol_tab != nullptr;
    return g.outs != 0u && g.first_out + g.outs <= frame_pixels;
}

// ---------------------------------------------------------------------------------------------- the settings (host and emulation)
// What a call with the FILM flag does: MCRT_OK with *gather (false: the film does not splat, the plain resolve runs), or the status
// with *why set. force: option MCRT_FILM_GATHER=force - a film that does not splat goes through the gather too.
inline int filmGatherSettings(const mcrt_camera_desc& cam, bool has_ray_source, bool force, bool* gather, const char** why) {
    *gather = false;
    if (cam.shard_count > 1)
        return *why = "the FILM flag with a sharded camera (shard_count > 1) - the gather needs the neighbours' rows", MCRT_ERR_UNSUPPORTED;
    if (has_ray_source)
        return *why = "the FILM flag with a ray source set (mcrt_set_ray_source) - its pixels have no film position; mcrt_set_ray_source(ctx, NULL) takes it off",
               MCRT_ERR_UNSUPPORTED;
    if (cam.film_filter > MCRT_FILM_LANCZOS) return *why = "film_filter is more than MCRT_FILM_LANCZOS (6)", MCRT_ERR_INVALID;
    if (cam.film_cache_size == 1) return *why = "film_cache_size is 1 - the table's step 2 / (film_cache_size - 1) has no value", MCRT_ERR_INVALID;
    if (!(cam.film_radius >= 0.0) || !(cam.film_radius < 1e6)) return *why = "film_radius is negative, not a number or 1e6 and more", MCRT_ERR_INVALID;
    *gather = force || filmSplats(cam.film_filter, cam.film_radius);
    return MCRT_OK;
}

}  // namespace mcrt
