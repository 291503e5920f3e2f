// Path classes: the path-traced frame split by what the FIRST surface did with the light - diffuse, glossy, transmission - and by whether
// the light arrived there directly or after further bounces, plus emission and background (include/mcrt.h "Path classes"). The per-sample
// code shared by the four gfx950 kernels of mcrt_path_classes.hip and the host emulation of the CPU tests
// (tests/emu/path_classes_emu.cpp): both run this text.
//
// The walk is the light groups' (mcrt_light_groups.hpp): the same state, lgVertex, lgRays, the same history and resolve. What differs is
// the key of a term: there the emitter it came from, here the class of the path. Interaction's selectType picks ONE lobe per vertex
// before any light is gathered (interactionInit), so the lobe of iteration 0 is a property of the sample: step 0 stores it in one more
// word of state, the later steps read it.
#pragma once

#include "mcrt_light_groups.hpp"

namespace mcrt {

// The classes in the order of MCRT_PATH_CLASS_*: emission, background, then direct and indirect of the lobes diffuse, glossy, transmission.
constexpr uint32_t kPcEmission = 0, kPcBackground = 1;
MCRT_HD uint32_t pcLobe(int type) { return type == kDiffuse ? 0u : type == kReflect ? 1u : 2u; }  // (a reflect on a Dirac surface is glossy too)
// Light that arrives along the ray of iteration m >= 1 - its sampleEmissive, the skyColor of its miss -: direct when the ray left the
// first vertex (m == 1), indirect after that.
MCRT_HD uint32_t pcArrivingClass(uint32_t lobe, uint32_t m) { return 2u + 2u * lobe + (m >= 2u ? 1u : 0u); }
// sampleDirect of iteration m: direct at the first vertex, indirect at every later one.
MCRT_HD uint32_t pcSampledClass(uint32_t lobe, uint32_t m) { return 2u + 2u * lobe + (m >= 1u ? 1u : 0u); }

struct PcState {
    LgState lg;
    uint32_t* lobe;  // [n] pcLobe of iteration 0's interaction; written by step 0 for the samples that go on, read by the later steps
};
constexpr uint64_t kPcStateBytes = kLgStateBytes + 4;  // per sample, without the planes' 24 each

struct PcParams {
    uint8_t class_plane[MCRT_PATH_CLASSES];
    uint32_t planes, max_depth;
};

// The settings (host and emulation), resolved here and nowhere else - host-only text, nothing of it is device code: the parameters with
// their defaults filled in (no map: the identity); -> P, or 0 when an entry is out of range (*bad: the first such class).
inline uint32_t pcSettingsOf(const mcrt_path_class_params* p, PcParams& r, uint32_t* bad = nullptr) {
    const bool mapped = p && (p->flags & MCRT_PATH_CLASSES_MAP);
    r.max_depth = p ? p->max_depth : 0u;
    r.planes = 0u;
    for (uint32_t c = 0; c < MCRT_PATH_CLASSES; c++) {
        r.class_plane[c] = mapped ? p->class_plane[c] : (uint8_t)c;
        if (r.class_plane[c] >= MCRT_PATH_CLASSES) {
            if (bad) *bad = c;
            return 0u;
        }
        if (r.class_plane[c] + 1u > r.planes) r.planes = r.class_plane[c] + 1u;
    }
    return r.planes;
}

// pathBegin for sample s: the light groups', the sky of a camera ray that missed (iteration 0's miss) going to the background's plane.
MCRT_HD bool pcBegin(const PcState& st, uint64_t s, double scene_ior, const PcParams& par) {
    LgParams lg;
    lg.plane = nullptr;  // (lgBegin reads the number of planes and the sky's)
    lg.planes = par.planes;
    lg.sky_plane = par.class_plane[kPcBackground];
    lg.max_depth = par.max_depth;
    return lgBegin(st.lg, s, scene_ior, lg);
}

// Step kernel, entry j: lgStep with the plane of every term chosen by the path's class. The sky of a bounce ray that misses is added
// here, in step k, with the throughput of vertex k + 1: it is iteration k + 1's miss and takes that iteration's class.
MCRT_HD bool pcStep(const AovChunk& c, const AovScene& s, const PcState& st, const PcParams& par, const uint32_t* list, uint32_t n_live, uint32_t j, uint32_t k, bool last,
                    const AovRays& lit, RefractionHistory& rh, bool& too_deep, SobolTab tab) {
    const uint64_t sample = list[j];
    too_deep = false;
    lgLoadHistory(st.lg, sample, rh);
    LgVertex v;
    lgVertex(v, c, s, st.lg, sample, k, rh, tab);
    const uint32_t lobe = k == 0u ? pcLobe(v.ia.type) : st.lobe[sample];
    if (v.ia.material->flags & MCRT_MAT_EMISSIVE)  // path-tracer.cpp:34 (zeros otherwise)
        lgAdd(st.lg, sample, par.class_plane[k == 0u ? kPcEmission : pcArrivingClass(lobe, k)], v.emission, v.throughput);
    if (last) return false;
    if (v.shadow) {  // :35
        const Hit h = lgShadowHit(lit, j);
        if (h.surface == v.ls.light)  // (zeros otherwise)
            lgAdd(st.lg, sample, par.class_plane[pcSampledClass(lobe, k)], sampleDirectFinish(s.sh, v.ia, v.ls, v.dq, h), v.throughput);
    }
    if (!v.bounce) return false;  // :37-47
    rh.update(v.ray);             // :49
    if (rh.overflow) {
        too_deep = true;
        return false;
    }
    const uint64_t b = (uint64_t)n_live + j;
    if (lit.surface[b] == kNoSurface) {  // :27-30 of iteration k + 1
        lgAdd(st.lg, sample, par.class_plane[pcArrivingClass(lobe, k + 1u)], skyColor(v.ray), v.next);
        return false;
    }
    if (k == 0u) st.lobe[sample] = lobe;
    lgStoreNext(st.lg, sample, v, lit, b, rh);
    return true;
}

// The arrays of PcState over one allocation of kPcStateBytes * n bytes (the light groups' layout, the lobes behind its words).
inline void pcPlaceState(PcState& st, void* base, uint64_t n) {
    lgPlaceState(st.lg, base, n);
    st.lobe = st.lg.word + 5 * n;
}

}  // namespace mcrt
