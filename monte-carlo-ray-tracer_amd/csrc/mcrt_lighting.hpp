// Lighting passes: emission, sky, direct, sampled and unoccluded light per pixel (include/mcrt.h "Lighting passes").
// The per-ray and per-pixel code, shared by the two gfx950 kernels of mcrt_lighting.hip and the host emulation of the CPU tests
// (tests/emu/lighting_emu.cpp): both run this text.
//
// The camera samples are the AOV pass's (mcrt_aov.hpp: aovCameraRay). From the first hit of sample i the pass evaluates the path
// tracer's own path (pathTracerBounce, mcrt_integrator.hpp) cut after its second vertex, with the path tracer's own functions
// (mcrt_shade.hpp) in its order: interactionInit, sampleEmissive, sampleDirectSetup / sampleDirectFinish around the shadow ray's closest
// hit, interactionSampleBSDF, absorb's first test, and at the bounce ray's closest hit sampleEmissive or skyColor. The closest-hit search
// between the two kernels is the one behind mcrt_intersect, unchanged; both rays of a sample go through it in one launch.
#pragma once

#include "mcrt_aov.hpp"

namespace mcrt {

// Vertex 0 of a camera sample that hit, as the path tracer's first iteration has it: both kernels derive it from the camera record (the
// ray kernel for the two rays, the resolve for everything else), nothing of it is stored.
struct LightingVertex {
    InteractionT<false> ia;
    LightSample ls;   // as vertex 1 finds it: light and select_probability from sampleDirectSetup, bsdf_pdf from interactionSampleBSDF
    DirectQuery dq;
    Ray ray1;         // the bounce ray
    d3 T;             // f / bsdf_pdf: the throughput at vertex 1
    bool shadow;      // sampleDirectSetup built a shadow ray
    bool bounce;      // the path goes on to vertex 1
};

// Record cr of the camera samples `cam` (one that hit), sample i of the chunk's pixel p.
MCRT_HD void lightingVertex(LightingVertex& lv, const AovChunk& c, const AovScene& s, const AovRays& cam, uint64_t cr, uint32_t p, uint32_t i, SobolTab tab) {
    uint32_t x, y;
    aovPixelOf(c, p, x, y);
    Sampler smp;
    smp.restore(c.global_seed, y * c.cam.width + x, i, 1u);  // pathTracerBounce's first iteration: one shuffle (path-tracer.cpp:23)
    const Ray ray = makeRay(ld3(cam.start + 3 * cr), ld3(cam.direction + 3 * cr), s.sh.scene_ior);  // cameraRay's, depth 0
    Hit hit;
    hit.t = cam.t[cr];
    hit.surface = cam.surface[cr];
    hit.interpolate = s.prim[(size_t)hit.surface * kPrimStride + 9] >= 2.0;  // (intersectTriangle's tag)
    hit.u = hit.interpolate ? cam.uv[2 * cr] : 0.0;
    hit.v = hit.interpolate ? cam.uv[2 * cr + 1] : 0.0;
    interactionInit(lv.ia, s.sh, hit, ray, ray.medium_ior, smp, tab);  // RefractionHistory::init(camera_ray).externalIOR(camera_ray)
    lv.ls.bsdf_pdf = 0.0;  // pathBegin
    lv.ls.select_probability = 0.0;
    lv.ls.light = kNoSurface;
    lv.shadow = sampleDirectSetup(s.sh, lv.ia, lv.ls, lv.dq, smp, tab);
    d3 f = splat(0.0);
    lv.T = splat(0.0);
    lv.bounce = interactionSampleBSDF(lv.ia, f, lv.ls.bsdf_pdf, lv.ray1, false, smp, tab);
    if (lv.bounce) {
        lv.T = f / lv.ls.bsdf_pdf;
        lv.bounce = compMax(lv.T) * lv.ray1.refraction_scale != 0.0;  // absorb's first test (depth 1: its roulette does not play)
    }
}

// The two rays of camera sample i of pixel p into the 2n records `lit` at (2 i) * pixels + p (shadow ray) and (2 i + 1) * pixels + p
// (bounce ray): sample-major, so that the resolve's lanes (one per pixel) read consecutive records. A slot without a ray - the camera
// sample missed, no shadow ray was built, the bounce was cut - gets the camera ray itself: finite, traced, never read.
MCRT_HD void lightingChunkRays(const AovChunk& c, const AovScene& s, const AovRays& cam, const AovRays& lit, uint64_t r, SobolTab tab) {
    const uint32_t p = (uint32_t)(r % c.pixels), i = (uint32_t)(r / c.pixels);
    const d3 start = ld3(cam.start + 3 * r), direction = ld3(cam.direction + 3 * r);
    d3 s0 = start, d0 = direction, s1 = start, d1 = direction;
    if (cam.surface[r] != 0xFFFFFFFFu) {
        LightingVertex lv;
        lightingVertex(lv, c, s, cam, r, p, i, tab);
        if (lv.shadow) {
            s0 = lv.dq.shadow_ray.start;
            d0 = lv.dq.shadow_ray.direction;
        }
        if (lv.bounce) {
            s1 = lv.ray1.start;
            d1 = lv.ray1.direction;
        }
    }
    const uint64_t r0 = (uint64_t)(2u * i) * c.pixels + p, r1 = r0 + c.pixels;
    aovStore3(lit.start, r0, s0);
    aovStore3(lit.direction, r0, d0);
    aovStore3(lit.start, r1, s1);
    aovStore3(lit.direction, r1, d1);
}

// What sampleEmissive reads of the Interaction the path tracer would construct at the bounce ray's hit (interaction.cpp:12-36, depth 1).
MCRT_HD d3 lightingBounceEmission(const AovScene& s, const LightingVertex& lv, double t, uint32_t surface) {
    InteractionT<false> ia1;
    ia1.t = t;
    ia1.surface = surface;
    ia1.out = -lv.ray1.direction;
    ia1.position = lv.ray1.start + lv.ray1.direction * t;
    ia1.material = &s.sh.materials[s.sh.surf_material[surface]];
    ia1.normal = surfNormal(s.sh, surface, ia1.position);
    ia1.inside = dot(lv.ray1.direction, ia1.normal) > 0.0;
    if (ia1.inside) ia1.normal = -ia1.normal;
    ia1.ray_depth = lv.ray1.depth;
    ia1.ray_dirac_delta = lv.ray1.dirac_delta;
    return sampleEmissive(s.sh, ia1, lv.ls);
}

// One pixel's sums: one FP64 accumulator per word, fed in ascending sample index whatever the launch shape.
struct LightingAccum {
    d3 emission, sky, direct, light, unoccluded;
};

MCRT_HD void lightingBegin(LightingAccum& acc) { acc.emission = acc.sky = acc.direct = acc.light = acc.unoccluded = splat(0.0); }

// Sample i of pixel p from the chunk's records: camera hits `cam`, the two rays' hits `lit`. Every channel gets one addend per sample
// (zeros where the definition says 0), so the sums do not depend on which branches the other samples took.
MCRT_HD void lightingAddSample(LightingAccum& acc, const AovChunk& c, const AovScene& s, const AovRays& cam, const AovRays& lit, uint32_t p, uint32_t i, SobolTab tab) {
    const uint64_t cr = (uint64_t)i * c.pixels + p;
    d3 emission = splat(0.0), sky = splat(0.0), light = splat(0.0), unoccluded = splat(0.0), bounce = splat(0.0);
    if (cam.surface[cr] == 0xFFFFFFFFu) {
        sky = skyColor(makeRay(ld3(cam.start + 3 * cr), ld3(cam.direction + 3 * cr), s.sh.scene_ior));
    } else {
        LightingVertex lv;
        lightingVertex(lv, c, s, cam, cr, p, i, tab);
        LightSample ls0;  // as pathBegin leaves it
        ls0.bsdf_pdf = 0.0;
        ls0.select_probability = 0.0;
        ls0.light = kNoSurface;
        emission = sampleEmissive(s.sh, lv.ia, ls0);
        const uint64_t r0 = (uint64_t)(2u * i) * c.pixels + p, r1 = r0 + c.pixels;
        if (lv.shadow) {
            Hit h;
            h.surface = lit.surface[r0];
            h.t = lit.t[r0];
            h.u = h.v = 0.0;
            h.interpolate = false;
            light = sampleDirectFinish(s.sh, lv.ia, lv.ls, lv.dq, h);
            unoccluded = light;
            if (h.surface != lv.ls.light) {  // the light as if nothing stood before it: its hit at the distance the shadow ray was aimed at
                h.surface = lv.ls.light;
                h.t = lv.dq.sq.dist;
                unoccluded = sampleDirectFinish(s.sh, lv.ia, lv.ls, lv.dq, h);
            }
        }
        if (lv.bounce) {
            const uint32_t surface = lit.surface[r1];
            bounce = (surface == 0xFFFFFFFFu ? skyColor(lv.ray1) : lightingBounceEmission(s, lv, lit.t[r1], surface)) * lv.T;
        }
    }
    acc.emission = acc.emission + emission;
    acc.sky = acc.sky + sky;
    acc.direct = acc.direct + (light + bounce);
    acc.light = acc.light + light;
    acc.unoccluded = acc.unoccluded + unoccluded;
}

MCRT_HD void lightingPixel(LightingAccum& acc, const AovChunk& c, const AovScene& s, const AovRays& cam, const AovRays& lit, uint32_t p, SobolTab tab) {
    lightingBegin(acc);
    for (uint32_t i = 0; i < c.spp; i++) lightingAddSample(acc, c, s, cam, lit, p, i, tab);
}

// The pixel's means over ALL its samples into the requested channels at packed pixel q.
MCRT_HD void lightingFinish(const LightingAccum& acc, uint32_t spp, const mcrt_lighting_buffers& out, uint64_t q) {
    const double n = (double)spp;
    aovStore3(out.emission, q, acc.emission / n);
    aovStore3(out.sky, q, acc.sky / n);
    aovStore3(out.direct, q, acc.direct / n);
    aovStore3(out.light, q, acc.light / n);
    aovStore3(out.unoccluded, q, acc.unoccluded / n);
}

}  // namespace mcrt
