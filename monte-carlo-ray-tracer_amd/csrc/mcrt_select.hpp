// Kernel selection of a frame (mcrt_hip.hip: launchRender) and the decision to render a frame again (mcrt_render_finish), as pure
// functions of small structs: no HIP, no mcrt_ctx. Plain host C++ like mcrt_plan.hpp, built into tests/emu so that the rules are
// checked without a GPU (tests/test_kernel_selection.py). The table that maps a RenderInstance to its kernel's address, and to its
// lean twin, is in mcrt_hip.hip.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>

#include "../../include/mcrt.h"
#include "mcrt_plan.hpp"
#include "mcrt_stats_words.hpp"

namespace mcrt {

// What the rules below need to know of the kernels' headers, by value: mcrt_hip.hip asserts each against the header that owns it.
constexpr uint32_t kSelBlock = 512;           // kBlock
constexpr uint32_t kSelWfBlock = 256;         // kWfBlock
constexpr uint32_t kSelLdsStack = 16;         // kLdsStackDepth
constexpr uint32_t kSelIorsDeep = 32;         // kMaxIorsDeep
constexpr uint32_t kSelIorsDepthLimit = 1u << 15;  // (32 768 nested media - a slot keeps the history's size in 16 bits; beyond it something other than a scene is going on)
constexpr uint32_t kSelWaveK = 128;           // waveMaxK(kWaveRows): what the narrow candidate buffer of a wave-cooperative search serves
constexpr uint32_t kSelWaveKMax = 768;        // waveMaxK(kWaveRowsLarge): ... the widest
constexpr uint32_t kSelWaveKnnBytes = 3584;        // waveKnnBytes(kWaveRows)
constexpr uint32_t kSelWaveKnnBytesLarge = 12800;  // waveKnnBytes(kWaveRowsLarge)
constexpr uint32_t kSelWaveStateBytes = 16;   // kWaveStateBytes
constexpr uint32_t kSelFlatArgFloats = 704;   // kFlatPreArgFloats
constexpr uint32_t kSelVisit = 160;           // kMaxVisit
constexpr uint32_t kSelVisitLimit = 1u << 15; // kMaxVisitLimit
constexpr uint64_t kSelKnnOverflow = 0x10000u;  // kKnnOverflowFlag
static_assert(kSelKnnOverflow == kStatKnnOverflowBit && kKnnOverflowUnit >= kSelKnnOverflow, "the overflow word, mcrt_stats_words.hpp");
constexpr uint32_t kSelLeanFeaturesOff = (1u << 0) | (1u << 1) | (1u << 6);  // MCRT_LEAN_FEATURES_OFF

// ------------------------------------------------------------------------------------------------
// options
// ------------------------------------------------------------------------------------------------
enum KernelOption : int { kKernelAuto = 0, kKernelWf, kKernelSm, kKernelLegacy, kKernelOther };

// The MCRT_* options a launch reads (include/mcrt.h), parsed once per launch by parseRenderOptions.
struct RenderOptions {
    int kernel = kKernelAuto;          // MCRT_KERNEL: wf / sm / legacy (any other value: set, and none of the three)
    bool flat_karg = true;             // MCRT_FLAT_KARG
    uint32_t wf_min_nodes = 65536u;    // MCRT_WF_MIN_NODES
    uint64_t wf_min_paths = 32000000ull;     // MCRT_WF_MIN_PATHS
    uint64_t wf_pm_min_paths = 32000000ull;  // MCRT_WF_PM_MIN_PATHS
    uint64_t wf_slots = 1ull << 24;    // MCRT_WF_SLOTS
    int wf_lean = 1;                   // MCRT_WF_LEAN
    int wf_leaf = 16;                  // MCRT_WF_LEAF
    bool wf_pm_eval = true;            // MCRT_WF_PM_EVAL
    bool wf_log = false;               // MCRT_WF_LOG
    long long chunks = -1;             // MCRT_CHUNKS: units per pixel; -1: the planners decide
    double sample_store_gb = 64.0;     // MCRT_SAMPLE_STORE_GB
    bool lean_kernels = true;          // MCRT_LEAN_KERNELS
    bool count_tests = false;          // MCRT_COUNT_TESTS
    bool profile_phases = false;       // MCRT_PROFILE_PHASES
    bool device_order = true;          // MCRT_DEVICE_ORDER
};

inline RenderOptions parseRenderOptions(const std::map<std::string, std::string>& options) {
    auto get = [&options](const char* key) -> const char* {
        auto it = options.find(key);
        return it == options.end() ? nullptr : it->second.c_str();
    };
    auto num = [&get](const char* key, long dflt) { const char* v = get(key); return v ? atol(v) : dflt; };
    RenderOptions o;
    if (const char* v = get("MCRT_KERNEL")) {
        const std::string k = v;
        o.kernel = k == "wf" ? kKernelWf : k == "sm" ? kKernelSm : k == "legacy" ? kKernelLegacy : kKernelOther;
    }
    o.flat_karg = num("MCRT_FLAT_KARG", 1) != 0;
    if (const char* v = get("MCRT_WF_MIN_NODES")) o.wf_min_nodes = (uint32_t)strtoul(v, nullptr, 0);
    if (const char* v = get("MCRT_WF_MIN_PATHS")) o.wf_min_paths = strtoull(v, nullptr, 0);
    if (const char* v = get("MCRT_WF_PM_MIN_PATHS")) o.wf_pm_min_paths = strtoull(v, nullptr, 0);
    o.wf_slots = (uint64_t)num("MCRT_WF_SLOTS", 1l << 24);
    o.wf_lean = (int)num("MCRT_WF_LEAN", 1);
    o.wf_leaf = (int)num("MCRT_WF_LEAF", 16);
    o.wf_pm_eval = num("MCRT_WF_PM_EVAL", 1) != 0;
    o.wf_log = num("MCRT_WF_LOG", 0) != 0;
    if (const char* v = get("MCRT_CHUNKS")) o.chunks = (long long)std::min<unsigned long long>(strtoull(v, nullptr, 0), 0x7FFFFFFFFFFFFFFFull);
    o.sample_store_gb = sampleStoreGb(get("MCRT_SAMPLE_STORE_GB"));
    o.lean_kernels = num("MCRT_LEAN_KERNELS", 1) != 0;
    o.count_tests = num("MCRT_COUNT_TESTS", 0) != 0;
    o.profile_phases = num("MCRT_PROFILE_PHASES", 0) != 0;
    o.device_order = num("MCRT_DEVICE_ORDER", 1) != 0;
    return o;
}

// ------------------------------------------------------------------------------------------------
// inputs
// ------------------------------------------------------------------------------------------------
struct SceneFacts {  // what mcrt_upload_scene computes
    bool flat = false;          // DeviceScene::flat: all lanes test all primitives in one wave-uniform loop
    bool cull = false;          // the flat loop's FP32 cull records exist (DeviceScene::flat_pre)
    uint32_t cull_floats = 0;   // ... their float count, when a kernel argument can carry them (0: it cannot)
    bool stage_all = false;     // the whole scene is LDS-resident
    uint32_t num_nodes = 0;     // BVH nodes of the descriptor
    uint32_t q_nodes = 0;       // nodes of the tree the pipeline's trace kernel walks (0: none could be built)
    bool q_single = false;      // HostLayout::q_single: no node of that tree has more than four children
    uint32_t material_flags = 0xFFFFFFFFu;  // OR of the materials' flags
    // planLds's totals (mcrt_kernels.hpp) of the photon-mapping kernel's plans, computed by the caller: [512 / 1024 lanes][2, 4 .. 16 stack
    // entries per lane in LDS] with two refraction-history entries per lane in LDS, and 512 lanes with all 16 and all 8 of them
    uint32_t pm_lds[2][8] = {};
    uint32_t pm_lds_full = 0;
};

struct FrameFacts {
    bool photon = false;        // integrator == MCRT_INTEGRATOR_PHOTON_MAPPER
    uint64_t paths = 0;         // path samples in this call's rows
    bool filtered = false;      // per-sample splats (a reconstruction filter)
    bool film_out = false;      // mcrt_render_film_device: the splats stay in the caller's buffer
    uint32_t k_nearest = 50;
    uint32_t max_lds = 0;       // dynamic LDS a kernel that shades may ask for
    bool force_wf = false;      // mcrt_render_finish renders the frame again: through the pipeline
    bool force_pm_lane = false; // ... by the per-lane photon-mapping kernel
};

// ------------------------------------------------------------------------------------------------
// output
// ------------------------------------------------------------------------------------------------
// Every kernel instance a frame or a photon pass is rendered by. Suffixes: Count = MCRT_COUNT_TESTS, All = whole scene in LDS, Prof = MCRT_PROFILE_PHASES.
enum RenderInstance : int {
    kInstNone = -1,
    // renderKernel<integrator, count, all, prof, flat>: the wave-synchronous megakernel
    kInstPT = 0, kInstPT_All, kInstPT_Count, kInstPT_CountAll, kInstPT_Prof, kInstPT_ProfAll,
    kInstPMLane, kInstPMLane_All, kInstPMLane_Count, kInstPMLane_CountAll,
    kInstFlat512,   // renderKernel<PT, false, true, false, 1>: the flat loop, cull records in LDS
    kInstFlatK512,  // renderKernelFlatK<512>: ... in the argument block
    kInstFlatK768,
    // renderKernelSM<count, all, prof>: the lane state machine
    kInstSM, kInstSM_All, kInstSM_Count, kInstSM_CountAll, kInstSM_Prof, kInstSM_ProfAll,
    // renderKernelPM<count, all, lanes, rows>: photon mapping with wave-cooperative estimates
    kInstPM512, kInstPM512_All, kInstPM512_Count, kInstPM512_CountAll,
    kInstPM1024, kInstPM1024_All, kInstPM1024_Count, kInstPM1024_CountAll,
    kInstPMWide, kInstPMWide_All, kInstPMWide_Count, kInstPMWide_CountAll,
    // the pipeline: wfShadeKernel<photon>, wfTraceKernel<PoolRays, count, visit>, wfKnnKernel<eval, rows>
    kInstShadePT, kInstShadePM,
    kInstTrace, kInstTrace_Count, kInstTraceLean, kInstTraceLeanSingle,
    kInstKnnEval, kInstKnnEvalWide, kInstKnnRaw, kInstKnnRawWide,
    // the photon pass: emitKernel<all>
    kInstEmit, kInstEmit_All,
    kInstCount
};

// The enumerator's name without its prefix ("-" for kInstNone): what the read-only option MCRT_INSTANCES_USED reports.
inline const char* instanceName(int id) {
    static const char* const names[] = {
        "PT", "PT_All", "PT_Count", "PT_CountAll", "PT_Prof", "PT_ProfAll",
        "PMLane", "PMLane_All", "PMLane_Count", "PMLane_CountAll",
        "Flat512", "FlatK512", "FlatK768",
        "SM", "SM_All", "SM_Count", "SM_CountAll", "SM_Prof", "SM_ProfAll",
        "PM512", "PM512_All", "PM512_Count", "PM512_CountAll",
        "PM1024", "PM1024_All", "PM1024_Count", "PM1024_CountAll",
        "PMWide", "PMWide_All", "PMWide_Count", "PMWide_CountAll",
        "ShadePT", "ShadePM",
        "Trace", "Trace_Count", "TraceLean", "TraceLeanSingle",
        "KnnEval", "KnnEvalWide", "KnnRaw", "KnnRawWide",
        "Emit", "Emit_All"};
    static_assert(sizeof(names) / sizeof(names[0]) == kInstCount && kInstFlat512 == 10 && kInstSM == 13 && kInstPM512 == 19 && kInstShadePT == 31 &&
                      kInstTrace == 33 && kInstKnnEval == 37 && kInstEmit == 41,
                  "names follow the enumeration");
    return id >= 0 && id < kInstCount ? names[id] : "-";
}

// Which words 8.. of a frame's statistics the instance wrote: the phase clocks (MCRT_PROFILE_PHASES), the trace kernel's step counters
// and the photon-mapping kernel's estimate clocks (MCRT_COUNT_TESTS). mcrt_render_finish prints a readout only for what was measured.
inline bool instanceProfiles(int id) { return id == kInstPT_Prof || id == kInstPT_ProfAll || id == kInstSM_Prof || id == kInstSM_ProfAll; }
inline bool instanceClocksEstimates(int id) {
    return id == kInstPM512_Count || id == kInstPM512_CountAll || id == kInstPM1024_Count || id == kInstPM1024_CountAll || id == kInstPMWide_Count ||
           id == kInstPMWide_CountAll;
}

// The inner visit of the pipeline's trace kernel (wfTraceKernel's third template argument; launchWavefront and mcrt_intersect):
// MCRT_WF_LEAN (default 1) 1: travInnerStepQLean - with one block per visit (3) when the tree has no node with more than four children
// (every quaternary tree); 0 (and MCRT_COUNT_TESTS): the earlier visit; 2: the block loop kept on a quaternary tree.
inline int traceVisit(const RenderOptions& o, bool q_single, bool count_tests) {
    if (count_tests || o.wf_lean == 0) return 0;
    return q_single && o.wf_lean != 2 ? 3 : 1;
}

struct KernelChoice {
    uint32_t form = MCRT_KERNEL_NONE;  // MCRT_KERNEL_*
    int instance = kInstNone;          // megakernel; pipeline: its shade kernel
    int knn_instance = kInstNone;      // pipeline of a photon-mapped frame: its kNN kernel
    bool lean = false;                 // `instance` runs as its lean twin (mcrt_hip_lean.hip)
    bool knn_lean = false;             // ... and `knn_instance`
    uint32_t block = kSelBlock;        // workgroup size of `instance`
    uint32_t stack_depth = kSelLdsStack;  // traversal-stack entries per lane kept in LDS (sm_depth / pm_stack_depth)
    int trace_visit = 0;               // pipeline: traceVisit() ...
    int trace_instance = kInstNone;    // ... and the trace kernel that has it
    int err = MCRT_OK;                 // refusal: the code and the text
    std::string message;
};

inline bool leanScene(const SceneFacts& s, const RenderOptions& o) { return (s.material_flags & kSelLeanFeaturesOff) == 0u && o.lean_kernels; }

inline KernelChoice selectKernel(const SceneFacts& s, const FrameFacts& f, const RenderOptions& o) {
    KernelChoice c;
    auto refuse = [&c](int code, const char* text) {
        c.err = code;
        c.message = text;
        return c;
    };
    const bool photon = f.photon, all = s.stage_all, count = o.count_tests, prof = o.profile_phases;
    // Lean instances (mcrt_hip_lean.hip: the default path's kernels compiled without Oren-Nayar, GGX and conductor Fresnel): a scene whose
    // materials carry none of those flags renders through them - same bits, fewer registers (mcrt_shade.hpp) - unless MCRT_LEAN_KERNELS=0.
    // The counting and profiling instances have no lean twin: with MCRT_COUNT_TESTS or MCRT_PROFILE_PHASES every kernel is the full one.
    const bool lean = leanScene(s, o) && !count && !prof;
    const bool has_tree = s.q_nodes > 0;  // (a scene without a BVH is walked through a tree over index ranges by the pipeline's trace kernel, mcrt_layout.hpp)
    const bool legacy = o.kernel == kKernelLegacy, auto_kernel = o.kernel == kKernelAuto;

    if (f.film_out && !f.filtered)
        return refuse(MCRT_ERR_INVALID, "mcrt_render_film_device is for splatted frames (a reconstruction filter, or the box filter with a radius other than 0.5)");
    // per-sample splats: only the pipeline's shade kernel has them
    if (f.filtered && !has_tree)
        return refuse(MCRT_ERR_UNSUPPORTED, "reconstruction filters need the wavefront pipeline, and this scene has neither a BVH nor finite surface bounds to build its stand-in from");
    if (f.filtered && photon && f.k_nearest > kSelWaveKMax)
        return refuse(MCRT_ERR_UNSUPPORTED, "reconstruction filters on photon-mapped frames need k_nearest_photons <= 768 (wavefront pipeline)");

    // Path tracing of scenes whose BVH is walked: the lane-state-machine kernel (MCRT_KERNEL=legacy keeps the wave-synchronous one for
    // A/B runs) and, when the tree lives in HBM, the wavefront pipeline (MCRT_KERNEL=sm keeps the megakernel, MCRT_KERNEL=wf forces the
    // pipeline for any scene that has a tree).
    const bool use_sm = !photon && !s.flat && !legacy;
    const bool want_wf = f.filtered || o.kernel == kKernelWf || f.force_wf;
    // Measured: the pipeline wins on deep trees (metal_bunnies 169 k nodes +28 %, spaceship with hulls 154 k nodes +7 %), the
    // megakernel on small ones (spaceship cockpit 23 k nodes: 1352 vs 940 Mray/s): MCRT_WF_MIN_NODES, default 65 536 ...
    // ... and the pipeline wins on ANY tree in memory once the frame is large enough to amortise its launches (spaceship cockpit, 23 k nodes,
    // 1080p, ms per frame megakernel / pipeline: 2 M paths 9.4 / 19.1, 8 M 24.5 / 35.3, 33 M 80.9 / 77.3, 133 M 311 / 228):
    // MCRT_WF_MIN_PATHS path samples in this call's rows, default 32 M.
    const bool pt_pipeline = use_sm && !all && auto_kernel && (s.num_nodes >= o.wf_min_nodes || f.paths >= o.wf_min_paths);
    // Photon-mapped frames go through the pipeline (trace / kNN / shade launches) on request - k must fit the per-wave candidate buffer -
    // and by themselves for a scene whose tree stays in memory, whose materials allow the lean instances and whose k fits the narrow
    // buffers, once the frame is large enough (MCRT_WF_PM_MIN_PATHS path samples in this call's rows, default 32 M). With the lean kNN
    // launch (17 instead of 61 spilled registers, 6 waves per SIMD) and the lean shade launch (8 instead of 192) C5 renders in 739 ms per
    // 64-spp frame against the megakernel's 817 (profiles/r06_ab_lean_knn_occupancy.log): the pipeline's kernels each run at their own
    // register budget, the megakernel's estimates at the budget of its bounce code. With the full instances the megakernel wins (C5 9.3
    // vs 7.4 s per frame, hexagon_room map 308 vs 242 ms), and LDS-resident scenes stay with it (hexagon_room_pm 93.7 ms against 136).
    const bool pm_pipeline = has_tree && !all && auto_kernel && !count && leanScene(s, o) && f.k_nearest <= kSelWaveK && f.paths >= o.wf_pm_min_paths;
    if (has_tree && (photon ? f.k_nearest <= kSelWaveKMax && (want_wf || pm_pipeline) && !f.force_pm_lane : want_wf || pt_pipeline)) {
        c.form = photon ? MCRT_KERNEL_WAVEFRONT_PM : MCRT_KERNEL_WAVEFRONT;
        c.instance = photon ? kInstShadePM : kInstShadePT;
        c.lean = lean;
        c.block = kSelWfBlock;
        c.trace_visit = traceVisit(o, s.q_single, count);
        c.trace_instance = c.trace_visit == 3 ? kInstTraceLeanSingle : c.trace_visit == 1 ? kInstTraceLean : count ? kInstTrace_Count : kInstTrace;
        if (photon) {
            // MCRT_WF_PM_EVAL (default 1): the kNN launch evaluates the estimates from staged Interactions; 0: it hands the k photons
            // back and the shade launch sums them per lane. The wide candidate buffer (k > 128) has no lean twin.
            const bool large_k = f.k_nearest > kSelWaveK;
            c.knn_instance = o.wf_pm_eval ? (large_k ? kInstKnnEvalWide : kInstKnnEval) : (large_k ? kInstKnnRawWide : kInstKnnRaw);
            c.knn_lean = lean && c.knn_instance == kInstKnnEval;
        }
        return c;
    }

    if (photon) {
        // Wave-cooperative estimates unless k is too large for the widest per-wave buffer (k <= 128: 256 candidates per wave; k <= 768:
        // 1024 candidates per wave, 512 lanes per workgroup).
        bool pm_wave = f.k_nearest <= kSelWaveKMax && !legacy && !f.force_pm_lane;
        const bool large_k = pm_wave && f.k_nearest > kSelWaveK;
        if (large_k) {
            // the wide buffers take 100 KB of a 512-lane workgroup's LDS: a BVH staged whole with its 16 stack entries per lane may not
            // leave that (a tree in HBM keeps as few as 2 entries per lane in LDS, a flat scene has no stack) - then the per-lane kernel
            const uint32_t least = s.pm_lds[0][all ? 7 : 0] + (kSelBlock / 64) * (kSelWaveKnnBytesLarge + kSelWaveStateBytes);
            if (least > f.max_lds) pm_wave = false;
        }
        if (!pm_wave) {
            static const int lane[2][2] = {{kInstPMLane, kInstPMLane_All}, {kInstPMLane_Count, kInstPMLane_CountAll}};
            c.form = MCRT_KERNEL_PM_LANE;
            c.instance = lane[count][all];
            return c;
        }
        const uint32_t knn_bytes = (large_k ? kSelWaveKnnBytesLarge : kSelWaveKnnBytes) + (all ? 0u : kSelWaveStateBytes);
        // (the 1024-lane and the wide instances keep two refraction-history entries per lane in LDS, the deeper ones in global memory)
        auto ldsBytes = [&](uint32_t block, uint32_t depth) {
            return (block == 1024u || large_k ? s.pm_lds[block == 1024u][depth / 2 - 1] : s.pm_lds_full) + (block / 64) * knn_bytes;
        };
        c.block = kSelBlock;
        c.stack_depth = kSelLdsStack;
        if (large_k) {
            if (!all) {
                c.stack_depth = 2;
                for (uint32_t depth = 16u; depth > 2u; depth -= 2)
                    if (ldsBytes(kSelBlock, depth) <= f.max_lds) {
                        c.stack_depth = depth;
                        break;
                    }
            }
        } else if (s.flat && ldsBytes(1024u, kSelLdsStack) <= f.max_lds) {
            // 1024 lanes per workgroup (4 waves per SIMD) when the LDS plan allows it: flat scenes have no traversal stack; a tree in HBM
            // is walked with the state machine's stack, of which then only a few entries per lane stay in LDS (the rest spills to
            // HBM); a staged BVH walked by the wave-synchronous code needs its 16 entries (512 lanes).
            // (a 768-lane instance - 3 waves per SIMD, 168 VGPRs, 639 instead of 769 spill instructions - measured 895 ms against 762 on
            // the C5 probe and 112 against 101 on pm, profiles/r05_ab_pm768.log: this kernel wants its four waves)
            c.block = 1024u;
        } else if (!all) {
            for (uint32_t depth = 16u; depth >= 2 && c.block == kSelBlock; depth -= 2)
                if (ldsBytes(1024u, depth) <= f.max_lds) {
                    c.block = 1024u;
                    c.stack_depth = depth;
                }
        }
        static const int wave[3][2][2] = {{{kInstPM512, kInstPM512_All}, {kInstPM512_Count, kInstPM512_CountAll}},
                                          {{kInstPM1024, kInstPM1024_All}, {kInstPM1024_Count, kInstPM1024_CountAll}},
                                          {{kInstPMWide, kInstPMWide_All}, {kInstPMWide_Count, kInstPMWide_CountAll}}};
        c.form = MCRT_KERNEL_PM_WAVE;
        c.instance = wave[large_k ? 2 : c.block == 1024u ? 1 : 0][count][all];
        // (the kernel of trees in MEMORY keeps its full instance: lean it spills 883 registers instead of 769 and a C5 frame takes 845 ms
        // instead of 815 - that kernel's frame time follows its spill placement, not its instruction count, DESIGN 4.4 - while the
        // LDS-resident scenes' instance gains 7 %: profiles/r06_ab_lean_kernels.log)
        c.lean = lean && (c.instance == kInstPM512_All || c.instance == kInstPM1024_All);
        if (ldsBytes(c.block, c.stack_depth) > f.max_lds) return refuse(MCRT_ERR_INVALID, "LDS plan exceeds the device limit");
        return c;
    }

    if (use_sm) {
        static const int sm[2][2] = {{kInstSM, kInstSM_All}, {kInstSM_Count, kInstSM_CountAll}};
        c.form = MCRT_KERNEL_LANE_SM;
        c.instance = prof ? (all ? kInstSM_ProfAll : kInstSM_Prof) : sm[count][all];
        c.lean = lean;
        return c;
    }

    // Flat-mode scenes get their own instance of the kernel: without the BVH walk in the code it needs no traversal stack (64 KB of LDS
    // at 512 lanes), so a CU can hold more waves. With the FP32 cull in front of the FP64 tests (mcrt_scene.hpp) and the records in LDS,
    // 512 lanes are fastest: C2 448.7 ms, 768 lanes 455.8, 1024 lanes 485.2 - the spills of the narrow instances (107 / 169 VGPRs)
    // cost more than the extra waves hide.
    if (s.flat && s.cull && all && !count && !prof) {
        // MCRT_FLAT_KARG (default 1): the cull records travel in the kernel's argument block and are read with scalar loads
        // (renderKernelFlatK) - when they fit it. With the records in SGPRs the 768-lane shape (3 waves per SIMD, 168 VGPRs) is the
        // fastest: C2 439.6 ms against 442.8 at 512 lanes and 478 at 1024, C2-GGX 596.9 against 614.6 and 649
        // (profiles/r05_ab_c2_flat_karg.log) ...
        // ... of the full instance. The lean one spills NOTHING at 512 lanes and is fastest there: C2 108.2 ms per 64-spp frame against
        // 111.0 at 768 lanes and the full instance's 112.0, profiles/r06_ab_feature_strip_probe.log.
        const bool karg = o.flat_karg && s.cull_floats > 0 && s.cull_floats <= kSelFlatArgFloats;
        c.form = MCRT_KERNEL_FLAT;
        c.block = karg && !lean ? 768u : 512u;
        c.instance = !karg ? kInstFlat512 : c.block == 768u ? kInstFlatK768 : kInstFlatK512;
        c.lean = lean;
        return c;
    }

    static const int sync[2][2] = {{kInstPT, kInstPT_All}, {kInstPT_Count, kInstPT_CountAll}};
    c.form = MCRT_KERNEL_WAVESYNC;
    c.instance = prof ? (all ? kInstPT_ProfAll : kInstPT_Prof) : sync[count][all];
    return c;
}

// ------------------------------------------------------------------------------------------------
// rendering a frame again (mcrt_render_finish)
// ------------------------------------------------------------------------------------------------
struct RetryState {  // what of the context decides how the frame is rendered again
    bool force_wf = false, force_pm_lane = false;  // hold until the frame is delivered or refused
    uint32_t knn_visit_cap = kSelVisit;   // frontier entries per lane of the per-lane photon search; stays with the context
    uint32_t iors_depth = kSelIorsDeep;   // RefractionHistory entries per pipeline slot; stays with the context
};

struct FrameOutcome {
    uint32_t kernel_id = MCRT_KERNEL_NONE;  // the form that rendered the frame
    uint64_t overflow = 0;       // the word kStatOverflow: statsStackOverflows / statsKnnOverflowed (mcrt_stats_words.hpp)
    bool iors_overflow = false;  // the word kStatIorsOverflow: a path nested deeper than its refraction history holds
    bool splats = false;         // (only the pipeline splats: no second kernel for such a frame)
    bool can_pipeline = false;   // the scene has a tree and, photon-mapped, k fits the widest per-wave buffer
};

enum RetryAction : int { kRetryDone = 0, kRetryError, kRetryAgain };

struct RetryStep {
    int action = kRetryDone;
    int err = MCRT_OK;
    std::string message;
    RetryState next;  // kRetryAgain: render the frame with these
};

inline RetryStep nextRender(const RetryState& st, const FrameOutcome& r) {
    RetryStep step;
    step.next = st;
    auto refuse = [&step](const std::string& text) {
        step.action = kRetryError;
        step.err = MCRT_ERR_UNSUPPORTED;
        step.message = text;
        return step;
    };
    const bool pm_wave_frame = r.kernel_id == MCRT_KERNEL_PM_WAVE || r.kernel_id == MCRT_KERNEL_WAVEFRONT_PM;
    const bool lane_frame = r.kernel_id == MCRT_KERNEL_PM_LANE;
    const bool was_pipeline = r.kernel_id == MCRT_KERNEL_WAVEFRONT || r.kernel_id == MCRT_KERNEL_WAVEFRONT_PM;
    if (statsKnnOverflowed(r.overflow)) {
        // The reference's frontier is an unbounded priority queue (linear-octree.cpp:33). A wave-cooperative search keeps 128 entries
        // in registers and 1 024 in a list in memory; a frame in which one of them ran out is rendered AGAIN by the per-lane kernel (the
        // reference's two queues per lane, in memory), whose own frontier - 160 entries per lane to begin with - grows eightfold per
        // attempt, up to kMaxVisitLimit. Slower, and correct.
        if (r.splats)
            return refuse("kNN frontier overflow in a splatted frame: a wave-cooperative search had more than 128 + 1 024 octants pending at once, and only the "
                          "pipeline splats - the per-lane kernel cannot render this frame again (the reference's queue is unbounded, linear-octree.cpp:33)");
        if ((pm_wave_frame && !st.force_pm_lane) || (lane_frame && st.knn_visit_cap < kSelVisitLimit)) {
            step.next.knn_visit_cap = lane_frame ? std::min<uint32_t>(st.knn_visit_cap * 8u, kSelVisitLimit) : std::max<uint32_t>(st.knn_visit_cap, 2048u);
            step.next.force_pm_lane = true;
            step.action = kRetryAgain;
            return step;
        }
        return refuse("kNN frontier overflow: a search had more than " + std::to_string(kSelVisitLimit) + " octants pending at once in the per-lane "
                      "kernel's frontier (the reference's queue is unbounded, linear-octree.cpp:33)");
    }
    if (statsStackOverflows(r.overflow)) return refuse("traversal stack overflow (internal error: the stacks are sized to the tree's own bound, HostLayout::stack_bound)");
    if (r.iors_overflow) {
        // RefractionHistory (ray.cpp:74-98) is an unbounded vector. The megakernels keep kMaxIors (8) entries per lane, the pipeline
        // iors_depth per slot (32 to begin with). A frame that nested deeper is rendered AGAIN: a megakernel frame through the
        // pipeline, a pipeline frame with four times the rows - slower, and correct. The rows a scene needed stay with the context.
        // (No scene of the reference nests deeper than 4.)
        // A per-lane frame that stands in for overflowed wave-cooperative searches has nowhere to go: the pipeline searches wave-cooperatively.
        const bool lane_only = lane_frame && st.force_pm_lane;
        if (!lane_only && r.can_pipeline && (was_pipeline ? st.iors_depth < kSelIorsDepthLimit : !st.force_wf)) {
            if (was_pipeline) step.next.iors_depth = st.iors_depth * 4u;
            step.next.force_wf = true;
            step.action = kRetryAgain;
            return step;
        }
        return refuse("a path entered more nested dielectric media than this frame can keep (RefractionHistory, ray.cpp:74-98: 8 per lane in the "
                      "megakernels of scenes the pipeline cannot take; 32 768 per slot in the pipeline)");
    }
    return step;
}

}  // namespace mcrt
