// Light groups: the path-traced frame split by emitter, every bounce (include/mcrt.h "Light groups").
// The per-sample and per-pixel code, shared by the four gfx950 kernels of mcrt_light_groups.hip and the host emulation of the CPU tests
// (tests/emu/light_groups_emu.cpp): both run this text.
//
// The camera samples are the AOV pass's (mcrt_aov.hpp: aovCameraRay). From there the pass follows PathTracer::sampleRay's own loop as
// pathTracerBounce (mcrt_integrator.hpp) restates it - the same functions of mcrt_shade.hpp in the same order, the same throughput -
// one iteration per launch group, over the samples that are still alive. The lighting passes (mcrt_lighting.hpp) are its iteration 0; as
// there, a vertex is rebuilt from the stored ray and hit in both kernels around the closest-hit search, and nothing of the
// interaction is stored. What IS stored per sample (LgState, structure of arrays over the chunk's samples) is what sampleRay carries
// from one iteration to the next: the ray, its hit, the throughput, the light sample, the refraction history and one radiance per plane.
#pragma once

#include "mcrt_aov.hpp"

namespace mcrt {

constexpr uint32_t kLgPlanesMax = MCRT_LIGHT_GROUPS_MAX + 1u;  // the groups and a plane of its own for the sky
constexpr uint32_t kLgMaxIterations = 4096;                    // the host loop's bound (MCRT_ERR_UNSUPPORTED beyond it)

// Sample s of a chunk is sample s / pixels of pixel s % pixels (the AOV pass's record order). `n` is the chunk's number of samples and
// the stride of every array that has more than one word per sample, so that the lanes of a wave read consecutive words.
struct LgState {
    AovRays ray;         // start, direction of the ray that arrives at the vertex and its closest hit (iteration 0: the camera records)
    double* medium;      // [2][n] Ray::medium_ior, refraction_scale
    double* throughput;  // [3][n]
    double* pdf;         // [2][n] LightSample::bsdf_pdf, select_probability
    uint32_t* word;      // [5][n] Ray::refraction_level, depth | diffuse_depth << 16, dirac_delta, LightSample::light, RefractionHistory::size
    double* iors;        // [kMaxIors][n] RefractionHistory's entries
    double* radiance;    // [planes][3][n] R_p
    uint64_t n;
};
constexpr uint64_t kLgStateBytes = 76 + 16 + 24 + 16 + 20 + 8 * kMaxIors;  // per sample, without the planes' 24 each

// What does not change over a call: the plane of every surface (emitters: their group's; everything else 0, never added to with a
// value other than zero), the sky's plane, the number of planes, and the depth the paths are cut at (0 = not cut).
struct LgParams {
    const uint8_t* plane;  // [num_surfaces]
    uint32_t planes, sky_plane, max_depth;
};

// ---------------------------------------------------------------------------------------------- the settings (host and emulation)
// What the calls resolve from mcrt_light_group_params, here and nowhere else: host-only text, nothing of it is device code.
struct LgSettings {
    uint32_t groups, sky_plane, planes, max_depth;
    const uint32_t* surface_group;
};

// The parameters with their defaults filled in; -> the number of planes, or 0 when the numbers are out of range (more than
// MCRT_LIGHT_GROUPS_MAX groups - sky_plane is then not looked at - or a sky_plane above the groups).
inline uint32_t lgSettingsOf(const mcrt_light_group_params* p, LgSettings& s) {
    s.groups = p && p->num_groups ? p->num_groups : 1u;
    s.max_depth = p ? p->max_depth : 0u;
    s.surface_group = p ? p->surface_group : nullptr;
    if (s.groups > MCRT_LIGHT_GROUPS_MAX) return 0u;
    s.sky_plane = p && (p->flags & MCRT_LIGHT_GROUPS_SKY_PLANE) ? p->sky_plane : s.groups;
    if (s.sky_plane > s.groups) return 0u;
    s.planes = s.groups > s.sky_plane + 1u ? s.groups : s.sky_plane + 1u;
    return s.planes;
}

// LgParams::plane for the scene's surfaces into plane[0 .. num_surfaces): an emitter's (a surface whose material carries
// MCRT_MAT_EMISSIVE) is its group, every other surface's 0 - also one whose surf_material names no material. false: *bad is the first
// emitter whose group is not one of the s.groups.
inline bool lgSurfacePlanes(const LgSettings& s, const uint32_t* surf_material, uint32_t num_surfaces, const mcrt_material* materials, uint32_t num_materials,
                            uint8_t* plane, uint32_t* bad) {
    for (uint32_t i = 0; i < num_surfaces; i++) {
        plane[i] = 0;
        if (surf_material[i] >= num_materials || !(materials[surf_material[i]].flags & MCRT_MAT_EMISSIVE)) continue;
        const uint32_t g = s.surface_group ? s.surface_group[i] : 0u;
        if (g >= s.groups) {
            *bad = i;
            return false;
        }
        plane[i] = (uint8_t)g;
    }
    return true;
}

// The live list's counters and the pass's error word, in device memory; the host reads them after every step kernel.
struct LgCounters {
    uint32_t live[2];   // entries of the two lists (ping-pong: iteration k reads list k & 1 and appends to the other)
    uint32_t too_deep;  // a path entered a dielectric medium at nesting depth kMaxIors
    uint32_t pad;
};

MCRT_HD Ray lgLoadRay(const LgState& st, uint64_t s) {
    Ray r = makeRay(ld3(st.ray.start + 3 * s), ld3(st.ray.direction + 3 * s), st.medium[s]);  // inv_direction: rcp3(direction), as every Ray has it
    r.refraction_scale = st.medium[st.n + s];
    r.refraction_level = (int)st.word[s];
    const uint32_t depths = st.word[st.n + s];
    r.depth = (uint16_t)(depths & 0xFFFFu);
    r.diffuse_depth = (uint16_t)(depths >> 16);
    r.dirac_delta = st.word[2 * st.n + s] != 0u;
    return r;
}

MCRT_HD void lgStoreRay(const LgState& st, uint64_t s, const Ray& r) {
    aovStore3(st.ray.start, s, r.start);
    aovStore3(st.ray.direction, s, r.direction);
    st.medium[s] = r.medium_ior;
    st.medium[st.n + s] = r.refraction_scale;
    st.word[s] = (uint32_t)r.refraction_level;
    st.word[st.n + s] = (uint32_t)r.depth | ((uint32_t)r.diffuse_depth << 16);
    st.word[2 * st.n + s] = r.dirac_delta ? 1u : 0u;
}

// The sample's refraction history into the lane's column (LDS on the GPU) and back.
MCRT_HD void lgLoadHistory(const LgState& st, uint64_t s, RefractionHistory& rh) {
    rh.size = (int)st.word[4 * st.n + s];
    for (int e = 0; e < kMaxIors; e++)
        if (e < rh.size) rh.put(e, st.iors[(uint64_t)e * st.n + s]);
    rh.overflow = false;
}
MCRT_HD void lgStoreHistory(const LgState& st, uint64_t s, const RefractionHistory& rh) {
    st.word[4 * st.n + s] = (uint32_t)rh.size;
    for (int e = 0; e < kMaxIors; e++)
        if (e < rh.size) st.iors[(uint64_t)e * st.n + s] = rh.at(e);
}

// R_p = R_p + c * throughput: the lane owns its sample's words.
MCRT_HD void lgAdd(const LgState& st, uint64_t s, uint32_t plane, d3 c, d3 throughput) {
    double* r = st.radiance + (uint64_t)(3u * plane) * st.n + s;
    const d3 sum = d3{r[0], r[st.n], r[2 * st.n]} + c * throughput;
    r[0] = sum.x;
    r[st.n] = sum.y;
    r[2 * st.n] = sum.z;
}

// pathBegin for sample s, whose camera ray and hit the AOV pass's ray kernel and the search have written into st.ray. A camera ray that
// missed is iteration 0's miss (path-tracer.cpp:27-30): its sky goes to the sky's plane here and the path has ended. Returns true when
// the sample is alive. (A live sample's stored hit is therefore always a hit: lgStep treats the bounce ray's miss the same way.)
MCRT_HD bool lgBegin(const LgState& st, uint64_t s, double scene_ior, const LgParams& par) {
    st.medium[s] = scene_ior;  // cameraRay's makeRay
    st.medium[st.n + s] = 1.0;
    st.word[s] = 0u;
    st.word[st.n + s] = 0u;
    st.word[2 * st.n + s] = 0u;
    st.word[3 * st.n + s] = kNoSurface;
    st.word[4 * st.n + s] = 1u;  // RefractionHistory::init(camera_ray)
    st.iors[s] = scene_ior;
    for (int c = 0; c < 3; c++) st.throughput[(uint64_t)c * st.n + s] = 1.0;
    st.pdf[s] = 0.0;
    st.pdf[st.n + s] = 0.0;
    for (uint32_t w = 0; w < 3u * par.planes; w++) st.radiance[(uint64_t)w * st.n + s] = 0.0;
    if (st.ray.surface[s] != kNoSurface) return true;
    lgAdd(st, s, par.sky_plane, skyColor(lgLoadRay(st, s)), splat(1.0));
    return false;
}

// Vertex k of sample s, as iteration k of sampleRay's loop has it (path-tracer.cpp:23-47 without the additions to the radiance):
// both kernels derive it from the stored ray and hit. `rh` holds the sample's history and is not changed. (Chunk: how the chunk names
// its pixels, mcrt_aov.hpp chunkPixel - the frame's chunks here and in the path classes, a pixel list in the adaptive pass.)
struct LgVertex {
    InteractionT<false> ia;
    LightSample ls;   // in: as vertex k finds it; out: as vertex k + 1 finds it
    DirectQuery dq;
    Ray ray;          // in: the ray that arrives; out: the bounce ray
    d3 emission;      // sampleEmissive(ia, ls as vertex k finds it)
    d3 throughput;    // of vertex k
    d3 next;          // of vertex k + 1 (after absorb's division)
    bool shadow;      // sampleDirectSetup built a shadow ray
    bool bounce;      // the path goes on to vertex k + 1
};

template <class Chunk>
MCRT_HD void lgVertex(LgVertex& v, const Chunk& c, const AovScene& s, const LgState& st, uint64_t sample, uint32_t k, const RefractionHistory& rh, SobolTab tab) {
    uint32_t x, y;
    const uint32_t p = (uint32_t)(sample % c.pixels);
    aovPixelOf(c, p, x, y);
    Sampler smp;
    smp.restore(chunkSeed(c, p), y * c.cam.width + x, (uint32_t)(sample / c.pixels), k + 1u);  // iteration k begins with one shuffle (path-tracer.cpp:23)
    v.ray = lgLoadRay(st, sample);
    Hit hit;
    hit.t = st.ray.t[sample];
    hit.surface = st.ray.surface[sample];
    hit.interpolate = s.prim[(size_t)hit.surface * kPrimStride + 9] == 2.0;  // primIntersect's tag: a triangle with vertex normals (3 is a quadric)
    hit.u = hit.interpolate ? st.ray.uv[2 * sample] : 0.0;
    hit.v = hit.interpolate ? st.ray.uv[2 * sample + 1] : 0.0;
    interactionInit(v.ia, s.sh, hit, v.ray, rh.externalIOR(v.ray), smp, tab);
    v.ls.bsdf_pdf = st.pdf[sample];
    v.ls.select_probability = st.pdf[st.n + sample];
    v.ls.light = st.word[3 * st.n + sample];
    v.emission = sampleEmissive(s.sh, v.ia, v.ls);
    v.shadow = sampleDirectSetup(s.sh, v.ia, v.ls, v.dq, smp, tab);
    v.throughput = d3{st.throughput[sample], st.throughput[st.n + sample], st.throughput[2 * st.n + sample]};
    v.next = v.throughput;
    d3 f = splat(0.0);
    v.bounce = interactionSampleBSDF(v.ia, f, v.ls.bsdf_pdf, v.ray, false, smp, tab);
    if (v.bounce) {
        v.next = v.throughput * (f / v.ls.bsdf_pdf);
        v.bounce = !absorb(v.ray, v.next, smp, tab);
    }
}

// Ray kernel, entry j of the n_live entries of `list`: the shadow ray of the sample's vertex k into record j of `lit`, its bounce ray
// into record n_live + j. A slot without a ray - no shadow ray was built, the path ends here - gets the ray that
// arrived: finite, traced, never read.
template <class Chunk>
MCRT_HD void lgRays(const Chunk& c, const AovScene& s, const LgState& st, const uint32_t* list, uint32_t n_live, uint32_t j, uint32_t k, const AovRays& lit,
                    RefractionHistory& rh, SobolTab tab) {
    const uint64_t sample = list[j];
    const d3 start = ld3(st.ray.start + 3 * sample), direction = ld3(st.ray.direction + 3 * sample);
    d3 s0 = start, d0 = direction, s1 = start, d1 = direction;
    lgLoadHistory(st, sample, rh);
    LgVertex v;
    lgVertex(v, c, s, st, sample, k, rh, tab);
    if (v.shadow) {
        s0 = v.dq.shadow_ray.start;
        d0 = v.dq.shadow_ray.direction;
    }
    if (v.bounce) {
        s1 = v.ray.start;
        d1 = v.ray.direction;
    }
    aovStore3(lit.start, j, s0);
    aovStore3(lit.direction, j, d0);
    aovStore3(lit.start, (uint64_t)n_live + j, s1);
    aovStore3(lit.direction, (uint64_t)n_live + j, d1);
}

// What the step kernels (this pass's and the path classes', mcrt_path_classes.hpp) share around their additions: the shadow ray's closest
// hit from record j, and the state of vertex k + 1 - the bounce ray, its hit from record b of `lit`, the throughput, the light sample and
// the history `rh` after its update.
MCRT_HD Hit lgShadowHit(const AovRays& lit, uint64_t j) {
    Hit h;
    h.surface = lit.surface[j];
    h.t = lit.t[j];
    h.u = h.v = 0.0;
    h.interpolate = false;
    return h;
}
MCRT_HD void lgStoreNext(const LgState& st, uint64_t sample, const LgVertex& v, const AovRays& lit, uint64_t b, const RefractionHistory& rh) {
    lgStoreRay(st, sample, v.ray);
    st.ray.t[sample] = lit.t[b];
    st.ray.surface[sample] = lit.surface[b];
    st.ray.uv[2 * sample] = lit.uv[2 * b];
    st.ray.uv[2 * sample + 1] = lit.uv[2 * b + 1];
    st.throughput[sample] = v.next.x;
    st.throughput[st.n + sample] = v.next.y;
    st.throughput[2 * st.n + sample] = v.next.z;
    st.pdf[sample] = v.ls.bsdf_pdf;
    st.pdf[st.n + sample] = v.ls.select_probability;
    st.word[3 * st.n + sample] = v.ls.light;
    lgStoreHistory(st, sample, rh);
}

// Step kernel, entry j: the terms of vertex k into their planes in the path tracer's order, then the state of vertex k + 1. `last`: this
// is iteration max_depth, which takes its emission and ends (its miss was taken where the ray was found to miss; no rays were traced for
// it, lit is not read). Returns true when
// the path goes on; too_deep: the history would have needed a ninth entry (the sample is dropped, the host refuses the frame).
template <class Chunk>
MCRT_HD bool lgStep(const Chunk& c, const AovScene& s, const LgState& st, const LgParams& par, const uint32_t* list, uint32_t n_live, uint32_t j, uint32_t k, bool last,
                    const AovRays& lit, RefractionHistory& rh, bool& too_deep, SobolTab tab) {
    const uint64_t sample = list[j];
    too_deep = false;
    lgLoadHistory(st, sample, rh);
    LgVertex v;
    lgVertex(v, c, s, st, sample, k, rh, tab);
    if (v.ia.material->flags & MCRT_MAT_EMISSIVE) lgAdd(st, sample, par.plane[v.ia.surface], v.emission, v.throughput);  // :34 (zeros otherwise)
    if (last) return false;
    if (v.shadow) {  // :35
        const Hit h = lgShadowHit(lit, j);
        if (h.surface == v.ls.light) lgAdd(st, sample, par.plane[v.ls.light], sampleDirectFinish(s.sh, v.ia, v.ls, v.dq, h), v.throughput);  // (zeros otherwise)
    }
    if (!v.bounce) return false;  // :37-47
    rh.update(v.ray);             // :49
    if (rh.overflow) {
        too_deep = true;
        return false;
    }
    const uint64_t b = (uint64_t)n_live + j;
    const uint32_t surface = lit.surface[b];
    if (surface == kNoSurface) {  // iteration k + 1 would find the miss and end (:27-30): its sky now, with the throughput it would have
        lgAdd(st, sample, par.sky_plane, skyColor(v.ray), v.next);
        return false;
    }
    lgStoreNext(st, sample, v, lit, b, rh);
    return true;
}

// Resolve kernel, pixel p of the chunk: per plane and word (((0.0 + R_p(0)) + R_p(1)) + ...) / spp over the pixel's samples in
// ascending order, into plane-major frames of `frame_pixels` pixels at packed pixel first_pixel + p.
MCRT_HD void lgResolvePixel(const AovChunk& c, const LgState& st, uint32_t planes, uint32_t p, double* out, uint64_t frame_pixels) {
    const double n = (double)c.spp;
    for (uint32_t plane = 0; plane < planes; plane++) {
        d3 acc = splat(0.0);
        const double* r = st.radiance + (uint64_t)(3u * plane) * st.n + p;
        for (uint32_t i = 0; i < c.spp; i++) {
            const uint64_t at = (uint64_t)i * c.pixels;
            acc = acc + d3{r[at], r[st.n + at], r[2 * st.n + at]};
        }
        aovStore3(out + (uint64_t)plane * frame_pixels * 3u, c.first_pixel + p, acc / n);
    }
}

// The arrays of LgState over one allocation `base` for chunks of up to n samples and `planes` planes (ray.* 8-byte words first).
inline void lgPlaceState(LgState& st, void* base, uint64_t n) {
    double* d = (double*)base;
    st.ray.start = d; d += 3 * n;
    st.ray.direction = d; d += 3 * n;
    st.ray.t = d; d += n;
    st.ray.uv = d; d += 2 * n;
    st.medium = d; d += 2 * n;
    st.throughput = d; d += 3 * n;
    st.pdf = d; d += 2 * n;
    st.iors = d; d += (uint64_t)kMaxIors * n;
    st.ray.surface = (uint32_t*)d;
    st.word = st.ray.surface + n;
    st.radiance = nullptr;
    st.n = n;
}

}  // namespace mcrt
