// First-hit AOV pass: depth, position, normals, albedo, coverage and ids of the camera samples' first hits, per pixel.
// The per-sample and per-pixel code, shared by the two gfx950 kernels of mcrt_aov.hip and the host emulation of the CPU tests
// (tests/emu/aov_emu.cpp): both run this text.
//
// A sample is the beauty frame's own: Camera::samplePixel's ray (camera/camera.cpp:79-95, cameraRay in mcrt_shade.hpp) with the
// sampler at initiate(y * width + x), setIndex(i) (camera.cpp:73-77), so an AOV frame lines up with a render of the same camera and
// seed sample for sample, depth of field included. What is kept of the hit is what Interaction's constructor derives before any
// material decision (ray/interaction.cpp:12-36): position, geometric normal, shading normal with its fall-back, both flipped
// towards the ray's side, and the material's reflectance.
#pragma once

#include "mcrt_shade.hpp"
#include "mcrt_wavefront.hpp"  // localToGlobalRow

namespace mcrt {

// What the pass reads of an uploaded scene, all in global memory (host emulation: the descriptor's arrays).
struct AovScene {
    ShadeViewT<false> sh;
    const double* prim;  // [n][kPrimStride] intersection records: word 9 == 2 marks a triangle that interpolates vertex normals
};

// A chunk of the frame: the pixels [first_pixel, first_pixel + pixels) of the shard's packed rows (pixel q = local row q / width,
// column q % width), every one with all its spp samples. Ray r of the chunk is sample r / pixels of pixel r % pixels: sample-major,
// so that the resolve's lanes (one per pixel) read consecutive records.
struct AovChunk {
    mcrt_camera_desc cam;
    uint32_t global_seed, spp;
    uint64_t first_pixel;
    uint32_t pixels;
};

// How a chunk names its pixels: pixel p of it is packed pixel chunkPixel(c, p) of the shard's rows. A chunk of the frame counts on
// from its first one; the adaptive pass's chunk of a pixel LIST (mcrt_adaptive.hpp: AdaptiveChunk) overloads this with one indirection.
// What follows - the camera rays here, the walk of mcrt_light_groups.hpp - takes the chunk's type as a parameter and asks this function.
// chunkSeed(c, p) is the global seed of that pixel's samples: the chunk's for a chunk of the frame; the adaptive pass counts a pixel's own
// batches.
MCRT_HD uint64_t chunkPixel(const AovChunk& c, uint32_t p) { return c.first_pixel + p; }
MCRT_HD uint32_t chunkSeed(const AovChunk& c, uint32_t) { return c.global_seed; }

template <class Chunk>
MCRT_HD void aovPixelOf(const Chunk& c, uint32_t p, uint32_t& x, uint32_t& y) {
    const uint64_t q = chunkPixel(c, p);
    x = (uint32_t)(q % c.cam.width);
    y = localToGlobalRow(c.cam, (uint32_t)(q / c.cam.width));
}

// Camera ray of sample i of the chunk's pixel p (camera.cpp:73-95).
template <bool kLdsTab, class Chunk>
MCRT_HD Ray aovCameraRay(const Chunk& c, double scene_ior, uint32_t p, uint32_t i, SobolTab tab) {
    uint32_t x, y;
    aovPixelOf(c, p, x, y);
    Sampler smp;
    smp.initiate(chunkSeed(c, p), y * c.cam.width + x);
    smp.setIndex(i);
    return cameraRay<kLdsTab>(c.cam, scene_ior, x, y, smp, tab);
}

struct AovSample {
    d3 position, normal, shading_normal, albedo;
    uint32_t material;
};

// The first hit of a sample (interaction.cpp:12-36): `surface` hit at `t` with barycentrics (u, v) by the ray (start, direction).
MCRT_HD AovSample aovSampleOf(const AovScene& s, d3 start, d3 direction, double t, uint32_t surface, double u, double v) {
    AovSample a;
    a.position = start + direction * t;  // Ray::operator() ray.cpp:69-72
    a.material = s.sh.surf_material[surface];
    a.albedo = ld3(s.sh.materials[a.material].reflectance);
    a.normal = surfNormal(s.sh, surface, a.position);
    const double cos_theta = dot(direction, a.normal);
    a.shading_normal = a.normal;
    if (s.prim[(size_t)surface * kPrimStride + 9] == 2.0) {  // Triangle::N != nullptr (triangle.cpp:56)
        a.shading_normal = surfInterpolatedNormal(s.sh, surface, u, v);
        if ((cos_theta < 0.0) != (dot(direction, a.shading_normal) < 0.0)) a.shading_normal = a.normal;
    }
    if (cos_theta > 0.0) {
        a.normal = -a.normal;
        a.shading_normal = -a.shading_normal;
    }
    return a;
}

// One pixel's sums: one FP64 accumulator per channel word, fed in ascending sample index whatever the launch shape.
struct AovAccum {
    double depth;
    d3 position, normal, shading_normal, albedo;
    uint32_t hits, surface0, material0;
};

MCRT_HD void aovBegin(AovAccum& acc) {
    acc.depth = 0.0;
    acc.position = acc.normal = acc.shading_normal = acc.albedo = splat(0.0);
    acc.hits = 0u;
    acc.surface0 = acc.material0 = 0xFFFFFFFFu;
}

// Sample i of the pixel: t == DBL_MAX / surface == 0xFFFFFFFF is a miss and adds nothing.
MCRT_HD void aovAdd(AovAccum& acc, const AovScene& s, uint32_t i, d3 start, d3 direction, double t, uint32_t surface, double u, double v) {
    if (surface == 0xFFFFFFFFu) return;
    const AovSample a = aovSampleOf(s, start, direction, t, surface, u, v);
    acc.hits++;
    acc.depth += t;
    acc.position = acc.position + a.position;
    acc.normal = acc.normal + a.normal;
    acc.shading_normal = acc.shading_normal + a.shading_normal;
    acc.albedo = acc.albedo + a.albedo;
    if (i == 0u) {
        acc.surface0 = surface;
        acc.material0 = a.material;
    }
}

// A chunk's rays and their closest hits (the shape ArrayRays takes, csrc/mcrt_kernels.hpp).
struct AovRays {
    double* start;      // [n][3]
    double* direction;  // [n][3]
    double* t;          // [n]
    uint32_t* surface;  // [n]
    double* uv;         // [n][2]
};

// Sample i of the pixel from record r of the chunk: a missed ray's other words are not read (the hit kernels need not have written them).
MCRT_HD void aovAddRay(AovAccum& acc, const AovScene& s, uint32_t i, const AovRays& rays, uint64_t r) {
    const uint32_t surface = rays.surface[r];
    if (surface == 0xFFFFFFFFu) return;
    aovAdd(acc, s, i, ld3(rays.start + 3 * r), ld3(rays.direction + 3 * r), rays.t[r], surface, rays.uv[2 * r], rays.uv[2 * r + 1]);
}

MCRT_HD void aovStore3(double* out, uint64_t q, d3 v) {
    if (!out) return;
    out[3 * q] = v.x;
    out[3 * q + 1] = v.y;
    out[3 * q + 2] = v.z;
}

// The pixel's values into the requested channels at packed pixel q: normals and albedo are means over ALL samples (a miss counts as
// zero, so they are already weighted by coverage), position and depth means over the hits (zeros / DBL_MAX where nothing was hit).
MCRT_HD void aovFinish(const AovAccum& acc, uint32_t spp, const mcrt_aov_buffers& out, uint64_t q) {
    const double n = (double)spp, h = (double)acc.hits;
    if (out.coverage) out.coverage[q] = h / n;
    if (out.depth) out.depth[q] = acc.hits ? acc.depth / h : kDblMax;
    aovStore3(out.position, q, acc.hits ? acc.position / h : splat(0.0));
    aovStore3(out.normal, q, acc.normal / n);
    aovStore3(out.shading_normal, q, acc.shading_normal / n);
    aovStore3(out.albedo, q, acc.albedo / n);
    if (out.surface) out.surface[q] = acc.surface0;
    if (out.material) out.material[q] = acc.material0;
}

}  // namespace mcrt
