// Occlusion pass: ambient occlusion, sky visibility and bent normals per pixel (include/mcrt.h "Occlusion pass").
// The per-ray and per-pixel code, shared by the two gfx950 kernels of mcrt_occlusion.hip and the host emulation of the CPU tests
// (tests/emu/occlusion_emu.cpp): both run this text.
//
// The camera samples are the AOV pass's (mcrt_aov.hpp: aovCameraRay, aovSampleOf). From the first hit of sample i, occlusion ray j is
// the diffuse bounce the path tracer would draw there with the sampler j shuffles further on: restore(global_seed, pixel, i, 1 + j),
// the pair at kDimBsdf, a cosine-weighted direction around the shading normal, the start lifted off the surface along the geometric
// normal (ray/ray.cpp, rayFromInteraction's last branch). The closest-hit search between the two kernels is the one behind
// mcrt_intersect, unchanged: materials play no part.
#pragma once

#include "mcrt_aov.hpp"

namespace mcrt {

struct OcclusionSettings {
    uint32_t rays, flags;
    double max_distance;  // 0: unbounded
};

// The settings of `params` (nullptr: the defaults) into s; nullptr or why they are refused.
inline const char* occlusionSettingsOf(const mcrt_occlusion_params* params, OcclusionSettings& s) {
    s = OcclusionSettings{1u, 0u, 0.0};
    if (!params) return nullptr;
    if (params->rays) s.rays = params->rays;
    s.flags = params->flags;
    s.max_distance = params->max_distance;
    if (s.rays > MCRT_OCCLUSION_MAX_RAYS) return "rays must be 1 .. 64";
    if (s.flags & ~(uint32_t)MCRT_OCCLUSION_GEOMETRIC) return "unknown flag bits";
    if (!(s.max_distance >= 0.0) || !(s.max_distance <= kDblMax)) return "max_distance must be finite and >= 0";
    return nullptr;
}

// Occlusion ray j of sample i of pixel (x, y) from the sample's first hit `a` (normals already on the ray's side).
template <bool kLdsTab>
MCRT_HD void occlusionRayOf(const AovSample& a, uint32_t global_seed, uint32_t pixel_seed, uint32_t i, uint32_t j, uint32_t flags, SobolTab tab, d3& start,
                            d3& direction) {
    Sampler smp;
    smp.restore(global_seed, pixel_seed, i, 1u + j);
    const double u0 = smp.get(kDimBsdf, tab), u1 = smp.get(kDimBsdf + 1, tab);
    const d3 around = (flags & MCRT_OCCLUSION_GEOMETRIC) ? a.normal : a.shading_normal;
    direction = csFrom(orthonormalBasis(around), cosWeightedHemi<kLdsTab>(u0, u1));
    start = a.position + a.normal * kEpsilon;
}

// Occlusion ray r of the chunk: ray j of camera sample i of pixel p with r = (i * rays + j) * pixels + p, so that the resolve's lanes
// (one per pixel) read consecutive records. The slots of a camera sample that missed get the camera ray itself: finite, never read.
template <bool kLdsTab>
MCRT_HD void occlusionChunkRay(const AovChunk& c, const AovScene& s, const OcclusionSettings& o, const AovRays& cam, uint64_t r, SobolTab tab, d3& start,
                               d3& direction) {
    const uint32_t p = (uint32_t)(r % c.pixels);
    const uint64_t ij = r / c.pixels;
    const uint32_t i = (uint32_t)(ij / o.rays), j = (uint32_t)(ij % o.rays);
    const uint64_t cr = (uint64_t)i * c.pixels + p;
    start = ld3(cam.start + 3 * cr);
    direction = ld3(cam.direction + 3 * cr);
    const uint32_t surface = cam.surface[cr];
    if (surface == 0xFFFFFFFFu) return;
    const AovSample a = aovSampleOf(s, start, direction, cam.t[cr], surface, cam.uv[2 * cr], cam.uv[2 * cr + 1]);
    uint32_t x, y;
    aovPixelOf(c, p, x, y);
    occlusionRayOf<kLdsTab>(a, c.global_seed, y * c.cam.width + x, i, j, o.flags, tab, start, direction);
}

// One pixel's sums: one FP64 accumulator per word, fed in ascending (i, j) whatever the launch shape.
struct OcclusionAccum {
    double open, sky;
    d3 bent;
    uint32_t hits;
};

MCRT_HD void occlusionBegin(OcclusionAccum& acc) {
    acc.open = acc.sky = 0.0;
    acc.bent = splat(0.0);
    acc.hits = 0u;
}

// Occlusion ray r of the records `occ`, one of a camera sample that hit: it sees the sky when nothing is hit, and is open then or when
// its hit lies past max_distance. A miss's t and an occluded ray's direction are not read.
MCRT_HD void occlusionAddRay(OcclusionAccum& acc, const OcclusionSettings& o, const AovRays& occ, uint64_t r) {
    const bool sky = occ.surface[r] == 0xFFFFFFFFu;
    if (sky) acc.sky += 1.0;
    if (sky || (o.max_distance > 0.0 && occ.t[r] > o.max_distance)) {
        acc.open += 1.0;
        acc.bent = acc.bent + ld3(occ.direction + 3 * r);
    }
}

// The pixel from the chunk's records: camera hits `cam` (sample-major), occlusion rays and their hits `occ`.
MCRT_HD void occlusionPixel(OcclusionAccum& acc, const AovChunk& c, const OcclusionSettings& o, const AovRays& cam, const AovRays& occ, uint32_t p) {
    occlusionBegin(acc);
    for (uint32_t i = 0; i < c.spp; i++) {
        if (cam.surface[(uint64_t)i * c.pixels + p] == 0xFFFFFFFFu) continue;
        acc.hits++;
        for (uint32_t j = 0; j < o.rays; j++) occlusionAddRay(acc, o, occ, ((uint64_t)i * o.rays + j) * c.pixels + p);
    }
}

// The pixel's values into the requested channels at packed pixel q: fractions of the hits * rays occlusion rays drawn; a pixel whose
// camera samples all missed is open sky without a direction.
MCRT_HD void occlusionFinish(const OcclusionAccum& acc, uint32_t rays, const mcrt_occlusion_buffers& out, uint64_t q) {
    const double n = (double)((uint64_t)acc.hits * rays);
    if (out.ao) out.ao[q] = acc.hits ? acc.open / n : 1.0;
    if (out.sky) out.sky[q] = acc.hits ? acc.sky / n : 1.0;
    aovStore3(out.bent_normal, q, acc.hits ? acc.bent / n : splat(0.0));
}

}  // namespace mcrt
