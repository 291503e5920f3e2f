// Ray sources (include/mcrt.h "Ray sources"): caller-supplied ray arrays and surface gathers for the passes that trace camera rays.
// The per-sample text of the source branches of aovRayKernel (csrc/mcrt_aov.hip), shared with the host emulation of the CPU tests
// (tests/emu/ray_source_emu.cpp): both run this file, as with mcrt_lens.hpp. Below it the settings and what mcrt_set_ray_source refuses,
// pure functions of the descriptor (host and emulation).
//
// A source replaces where a pixel sample's first ray comes from and nothing else: the camera of a call gives the frame's shape and the
// sampler keys (y * width + x), the passes read the 76-byte ray and hit records as they always do. Every ray ends in
// makeRay(start, direction, scene_ior); every operation is the one include/mcrt.h writes down, in that order, uncontracted.
#pragma once

#include "mcrt_lens.hpp"

namespace mcrt {

// The source's loops in aovRayKernel are two more values of LensSettings::model, internal ones: lensSettings refuses them (they are past
// MCRT_LENS_FISHEYE), so no descriptor of mcrt_set_lens reaches them - only launchSourceRays does.
constexpr uint32_t kLensModelSourceRays = 5, kLensModelSourceSurface = 6;

// A validated descriptor: what the kernel takes.
struct RaySource {
    uint32_t kind;       // MCRT_RAY_SOURCE_RAYS or _SURFACE (MCRT_RAY_SOURCE_NONE: none, nothing is read)
    uint32_t per_pixel;  // RAYS: the arrays are [pixels][3], every sample of a pixel takes the same record
    uint64_t pixels;     // packed pixels of the shard the arrays were made for: the stride between two samples of RAYS
    uint32_t spp;        // RAYS without per_pixel: the samples the arrays hold (checked against the camera, not read by the kernel)
    const double* a;     // RAYS: start,     SURFACE: position
    const double* b;     // RAYS: direction, SURFACE: normal
    double offset;       // SURFACE: start = P + Nn * offset
};

MCRT_HD bool sourceFinite(double v) { return v >= -kDblMax && v <= kDblMax; }  // (false for a NaN)
MCRT_HD bool sourceFinite3(d3 v) { return sourceFinite(v.x) && sourceFinite(v.y) && sourceFinite(v.z); }

// A record of RAYS is usable when its six words are finite and the direction is not all zero (-0 is a zero).
MCRT_HD bool sourceRayUsable(d3 start, d3 direction) {
    return sourceFinite3(start) && sourceFinite3(direction) && !(direction.x == 0.0 && direction.y == 0.0 && direction.z == 0.0);
}

// MCRT_RAY_SOURCE_RAYS, sample i of packed pixel q: record i * pixels + q (per_pixel: q), its words' bits copied; an unusable record
// becomes start (0,0,0), direction (0,0,1), so that nothing non-finite reaches the closest-hit search.
MCRT_HD Ray sourceRayOf(const RaySource& s, double scene_ior, uint64_t q, uint32_t i) {
    const uint64_t rec = s.per_pixel ? q : (uint64_t)i * s.pixels + q;
    d3 start = ld3(s.a + 3 * rec), direction = ld3(s.b + 3 * rec);
    if (!sourceRayUsable(start, direction)) {
        start = mk(0.0, 0.0, 0.0);
        direction = mk(0.0, 0.0, 1.0);
    }
    return makeRay(start, direction, scene_ior);
}

// MCRT_RAY_SOURCE_SURFACE: the direction `local` of the hemisphere about +z turned about the normal of packed pixel q, started `offset`
// along the normal above the position - the occlusion pass's construction (mcrt_occlusion.hpp).
MCRT_HD Ray sourceSurfaceRayOf(const RaySource& s, double scene_ior, uint64_t q, d3 local) {
    const d3 N = ld3(s.b + 3 * q);
    const double nn = (N.x * N.x + N.y * N.y) + N.z * N.z;
    const d3 Nn = (nn > 0.0 && nn <= kDblMax) ? N * (1.0 / sqrt(nn)) : mk(0.0, 0.0, 1.0);  // (a NaN fails both comparisons)
    const d3 direction = csFrom(orthonormalBasis(Nn), local);
    d3 P = ld3(s.a + 3 * q);
    if (!sourceFinite3(P)) P = mk(0.0, 0.0, 0.0);
    return makeRay(P + Nn * s.offset, direction, scene_ior);
}

// Dimension `dim` of sample i of the chunk's pixel p: aovCameraRay's sampler, at initiate(seed, y * width + x), setIndex(i).
template <class Chunk>
MCRT_HD double sourceSample(const Chunk& c, uint32_t p, uint32_t i, int dim, SobolTab tab) {
    uint32_t x, y;
    aovPixelOf(c, p, x, y);
    Sampler smp;
    smp.initiate(chunkSeed(c, p), y * c.cam.width + x);
    smp.setIndex(i);
    return smp.get(dim, tab);
}

// First ray of sample i of the chunk's pixel p under the source. SURFACE: cosWeightedHemi(u0, u1) of the camera's film-position pair,
// its operations (mcrt_shade.hpp) in another order - the sine and cosine of u1's azimuth first, u0 and the pixel's 48 bytes after
// them: what is drawn or read before sincos stays in registers through it, and on the device that spilled
// (profiles/NOTES_ray_source.md), so there p and i are handed on through an empty asm statement that waits for the sine and cosine.
// No value depends on the order.
template <bool kLdsTab, class Chunk>
MCRT_HD Ray sourceRay(const Chunk& c, const RaySource& s, double scene_ior, uint32_t p, uint32_t i, SobolTab tab) {
    if (s.kind == MCRT_RAY_SOURCE_RAYS) return sourceRayOf(s, scene_ior, chunkPixel(c, p), i);
    const double u1 = sourceSample(c, p, i, kDimPixel + 1, tab);
    const double azimuth = u1 * kTwoPi;
    double sin_a, cos_a;
    refSinCos<kLdsTab>(azimuth, sin_a, cos_a);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p), "+v"(i) : "v"(sin_a), "v"(cos_a));
#endif
    const double u0 = sourceSample(c, p, i, kDimPixel, tab);
    const double r = sqrt(u0);
    return sourceSurfaceRayOf(s, scene_ior, chunkPixel(c, p), d3{r * cos_a, r * sin_a, sqrt(1 - u0)});
}

// ---------------------------------------------------------------------------------------------- the settings (host and emulation)
// What mcrt_set_ray_source refuses about a descriptor: MCRT_OK, or the status with *why set. (The comparisons are written so that a
// NaN fails them.)
inline int raySourceSettings(const mcrt_ray_source_desc& d, RaySource& s, const char** why) {
    if (d.kind != MCRT_RAY_SOURCE_RAYS && d.kind != MCRT_RAY_SOURCE_SURFACE) return *why = "unknown kind", MCRT_ERR_INVALID;
    if (d.kind == MCRT_RAY_SOURCE_RAYS && (d.flags & ~(uint32_t)MCRT_RAY_SOURCE_PER_PIXEL) != 0) return *why = "unknown flag bits", MCRT_ERR_INVALID;
    if (d.kind == MCRT_RAY_SOURCE_SURFACE && d.flags != 0) return *why = "flags must be 0 for MCRT_RAY_SOURCE_SURFACE", MCRT_ERR_INVALID;
    if (d.reserved0 != 0 || d.reserved[0] != 0 || d.reserved[1] != 0) return *why = "reserved must be 0", MCRT_ERR_INVALID;
    if (!d.first || !d.second) return *why = "an array is NULL", MCRT_ERR_INVALID;
    if (d.pixels == 0) return *why = "pixels must be more than 0", MCRT_ERR_INVALID;
    s.kind = d.kind;
    s.per_pixel = d.kind == MCRT_RAY_SOURCE_RAYS && (d.flags & MCRT_RAY_SOURCE_PER_PIXEL) ? 1u : 0u;
    s.pixels = d.pixels;
    s.spp = d.spp;
    s.a = d.first;
    s.b = d.second;
    s.offset = d.offset;
    if (d.kind == MCRT_RAY_SOURCE_RAYS && !s.per_pixel && d.spp == 0) return *why = "spp must be more than 0", MCRT_ERR_INVALID;
    if (d.kind == MCRT_RAY_SOURCE_SURFACE && !(d.offset >= 0.0 && d.offset <= kDblMax)) return *why = "offset must be finite and at least 0", MCRT_ERR_INVALID;
    return MCRT_OK;
}

// Does the source read the sample count of its descriptor? (RAYS with per-sample arrays.)
inline bool raySourceReadsSpp(const RaySource& s) { return s.kind == MCRT_RAY_SOURCE_RAYS && !s.per_pixel; }

// The one thing a source refuses about a camera: a shard of another number of packed pixels (owned rows x width) or, where the
// arrays are per sample, another sample count. MCRT_OK, or which of the two: 1 = pixels, 2 = spp.
inline int raySourceTakesCamera(const RaySource& s, uint64_t cam_pixels, uint32_t cam_spp) {
    if (s.pixels != cam_pixels) return 1;
    if (raySourceReadsSpp(s) && s.spp != cam_spp) return 2;
    return 0;
}

// The records a host array holds that the kernel will replace (mcrt_set_ray_source_host counts them): RAYS' unusable records;
// SURFACE's positions that are not finite or normals whose squared length is not in (0, DBL_MAX].
inline uint64_t raySourceUnusable(const RaySource& s) {
    const uint64_t n = raySourceReadsSpp(s) ? s.pixels * s.spp : s.pixels;
    uint64_t bad = 0;
    for (uint64_t r = 0; r < n; r++) {
        const d3 a = ld3(s.a + 3 * r), b = ld3(s.b + 3 * r);
        if (s.kind == MCRT_RAY_SOURCE_RAYS) {
            bad += sourceRayUsable(a, b) ? 0 : 1;
        } else {
            const double nn = (b.x * b.x + b.y * b.y) + b.z * b.z;
            bad += (sourceFinite3(a) && nn > 0.0 && nn <= kDblMax) ? 0 : 1;
        }
    }
    return bad;
}

}  // namespace mcrt
