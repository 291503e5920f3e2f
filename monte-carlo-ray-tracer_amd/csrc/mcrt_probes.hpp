// Light probes (include/mcrt.h "Light probes"): spherical-harmonic radiance at points, split per lamp. The per-sample text of the two
// kernel branches a probe call adds - the probe-ray loop of aovRayKernel (csrc/mcrt_aov.hip) and the projection of
// lightGroupsResolveKernel (csrc/mcrt_light_groups.hip) -, shared with the host emulation of the CPU tests (tests/emu/probes_emu.cpp):
// both run this file, as with mcrt_ray_source.hpp. The walk between the two is the light groups' own (mcrt_light_groups.hpp), unchanged.
// Every operation is the one include/mcrt.h writes down, in that order, uncontracted.
#pragma once

#include "mcrt_light_groups.hpp"
#include "mcrt_ray_source.hpp"

namespace mcrt {

// The probe rays' loop in aovRayKernel is one more internal value of LensSettings::model, beside the ray source's two: lensSettings
// refuses it, only launchProbeRays reaches it.
constexpr uint32_t kLensModelProbe = 7;

constexpr uint32_t kProbeOrderMax = MCRT_PROBE_ORDER_MAX;
constexpr uint32_t kProbeCoefficientsMax = (kProbeOrderMax + 1u) * (kProbeOrderMax + 1u);

// K of an order: (L + 1)^2; 0 when it is out of range.
MCRT_HD uint32_t probeCoefficients(uint32_t order) { return order <= kProbeOrderMax ? (order + 1u) * (order + 1u) : 0u; }

// First ray of sample i of the chunk's pixel p of a probe call with positions ([pixels][3], packed pixels of the shard): a direction
// uniform over the sphere from the camera's film-position pair, started at the pixel's position. As in sourceRay the sine and cosine
// of u1's azimuth come first and p and i are handed on through an empty asm statement that waits for them: what is drawn or read before
// sincos stays in registers through it (profiles/NOTES_ray_source.md). No value depends on the order.
template <bool kLdsTab, class Chunk>
MCRT_HD Ray probeRay(const Chunk& c, const double* positions, double scene_ior, uint32_t p, uint32_t i, SobolTab tab) {
    const double u1 = sourceSample(c, p, i, kDimPixel + 1, tab);
    const double azimuth = u1 * kTwoPi;
    double sin_a, cos_a;
    refSinCos<kLdsTab>(azimuth, sin_a, cos_a);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p), "+v"(i) : "v"(sin_a), "v"(cos_a));
#endif
    const double u0 = sourceSample(c, p, i, kDimPixel, tab);
    const double z = 1.0 - (u0 + u0);
    const double rr = 1.0 - z * z;
    const double r = sqrt(rr > 0.0 ? rr : 0.0);
    d3 start = ld3(positions + 3 * chunkPixel(c, p));
    if (!sourceFinite3(start)) start = mk(0.0, 0.0, 0.0);
    return makeRay(start, d3{r * cos_a, r * sin_a, z}, scene_ior);
}

// The un-normalised basis b_k of direction d, k < 9 (k = 0 is 1 and multiplies nothing: probeTerm).
MCRT_HD double probeBasis(uint32_t k, d3 d) {
    switch (k) {
        case 1: return d.y;
        case 2: return d.z;
        case 3: return d.x;
        case 4: return d.x * d.y;
        case 5: return d.y * d.z;
        case 6: return 3.0 * (d.z * d.z) - 1.0;
        case 7: return d.x * d.z;
        default: return (d.x * d.x) - (d.y * d.y);
    }
}

// What the projection reads beside the samples' state. coefficients == 0: no projection - lightGroupsResolveKernel runs the plain
// mean, lgResolvePixel, and reads nothing of this.
struct ProbeProjection {
    uint32_t coefficients;    // K
    uint32_t pad;
    const double* direction;  // [chunk samples][3]: the first rays' directions as the search took them, record i * c.pixels + p
    const double* weight;     // [spp][frame_pixels] or nullptr
};

// t(i) of one output word: sample i of the chunk's pixel p, word `w` = 3 * plane + channel of the samples' radiances, coefficient k.
template <bool kWeighted>
MCRT_HD double probeTerm(const AovChunk& c, const LgState& st, const ProbeProjection& proj, uint32_t w, uint32_t k, uint32_t p, uint32_t i, uint64_t frame_pixels) {
    const uint64_t at = (uint64_t)i * c.pixels + p;
    double t = st.radiance[(uint64_t)w * st.n + at];
    if (kWeighted) t = t * proj.weight[(uint64_t)i * frame_pixels + c.first_pixel + p];
    if (k != 0u) t = t * probeBasis(k, ld3(proj.direction + 3 * at));
    return t;
}

// One word of the output: (((0.0 + t(0)) + t(1)) + ...) / spp, ascending i, one accumulator. Four terms are fetched before the four
// additions that depend on each other: the addresses do not depend on the sum.
template <bool kWeighted>
MCRT_HD double probeWordOf(const AovChunk& c, const LgState& st, const ProbeProjection& proj, uint32_t w, uint32_t k, uint32_t p, uint64_t frame_pixels) {
    double acc = 0.0;
    uint32_t i = 0;
    for (; i + 4u <= c.spp; i += 4u) {
        double t[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) t[u] = probeTerm<kWeighted>(c, st, proj, w, k, p, i + u, frame_pixels);
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) acc = acc + t[u];
    }
    for (; i < c.spp; i++) acc = acc + probeTerm<kWeighted>(c, st, proj, w, k, p, i, frame_pixels);
    return acc / (double)c.spp;
}

// Lane `lane` of the projection's launch, lane = word * c.pixels + p with word = (plane * K + k) * 3 + channel: consecutive lanes
// consecutive pixels of one word, all lanes of a pixel the same radiances' samples and directions. The word goes to
// out[plane][k][first_pixel + p][channel] of frames of frame_pixels pixels. lanes: probeLanes.
MCRT_HD uint64_t probeLanes(const AovChunk& c, uint32_t planes, const ProbeProjection& proj) { return (uint64_t)planes * proj.coefficients * 3u * c.pixels; }
MCRT_HD void probeResolveLane(const AovChunk& c, const LgState& st, const ProbeProjection& proj, uint64_t lane, double* out, uint64_t frame_pixels) {
    const uint32_t p = (uint32_t)(lane % c.pixels), word = (uint32_t)(lane / c.pixels);
    const uint32_t channel = word % 3u, k = (word / 3u) % proj.coefficients, plane = word / (3u * proj.coefficients);
    const uint32_t w = 3u * plane + channel;
    const double v = proj.weight ? probeWordOf<true>(c, st, proj, w, k, p, frame_pixels) : probeWordOf<false>(c, st, proj, w, k, p, frame_pixels);
    out[(((uint64_t)plane * proj.coefficients + k) * frame_pixels + c.first_pixel + p) * 3u + channel] = v;
}

// ---------------------------------------------------------------------------------------------- the settings (host and emulation)
// What the probe calls refuse about their own fields (the groups' are the light groups': lgSettingsOf): MCRT_OK, or the status with
// *why set.
inline int probeSettings(const mcrt_probe_params& p, const char** why) {
    if (p.order > kProbeOrderMax) return *why = "order is more than MCRT_PROBE_ORDER_MAX (2)", MCRT_ERR_INVALID;
    if (p.flags != 0) return *why = "flags must be 0", MCRT_ERR_INVALID;
    if (p.reserved[0] != 0 || p.reserved[1] != 0) return *why = "reserved must be 0", MCRT_ERR_INVALID;
    if (p.groups.flags & (MCRT_LIGHT_GROUPS_FILM | MCRT_LIGHT_GROUPS_FILM_CLAMP))
        return *why = "groups.flags carries MCRT_LIGHT_GROUPS_FILM or MCRT_LIGHT_GROUPS_FILM_CLAMP - a probe has no film", MCRT_ERR_INVALID;
    return MCRT_OK;
}

}  // namespace mcrt
