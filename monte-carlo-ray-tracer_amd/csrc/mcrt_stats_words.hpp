// The 64-bit words a render and a photon pass report through: which kernel adds to which word (mcrt_kernels.hpp), and which word
// mcrt_render_finish / emitOnDevice (mcrt_hip.hip, mcrt_stats_readout.hpp) and the host emulation (tests/emu) read. Host and device
// code, nothing of HIP: plain g++ includes it.
// THE NUMBERING IS FROZEN: the Python tests index the words by number (tests/test_stats_words.py holds them to this header).
#pragma once

#include <cstdint>

namespace mcrt {

// The phases of the optional phase profiler (PhaseProf, mcrt_integrator.hpp), in the order of their words and of the [mcrt phase] lines.
enum : int { kPhRegen = 0, kPhTraverse = 1, kPhShade = 2, kPhShadow = 3, kPhSample = 4, kPhLoop = 5, kNumPhases = 6 };

// ---- a render's statistics (RenderParams::stats, WfTraceArgs::stats, ...: one buffer per context, zeroed per frame)
enum : int {
    // every kernel of a frame adds to these
    kStatPaths = 0,
    kStatRays = 1,
    kStatNodeTests = 2,      // MCRT_COUNT_TESTS instances only
    kStatPrimTests = 3,      // ... likewise
    kStatKnnSearches = 4,
    kStatOverflow = 5,       // two meanings in one word: statsStackOverflows / statsKnnOverflowed below
    kStatKnnOctants = 6,     // octants the searches visited
    kStatIorsOverflow = 7,   // lanes a path of which nested deeper than its refraction history holds
    // From here on three OVERLAYS share the words; at most one kernel of a frame writes them, and the readout is printed only for the
    // instance that did (statsReadout).
    kStatOverlay = 8,
    // 1. the profiling instances (PT_Prof*, SM_Prof*): per phase the wave's clocks, then per phase the lanes'
    kStatPhaseWave = kStatOverlay,
    kStatPhaseLane = kStatPhaseWave + kNumPhases,
    kStatPhaseEnd = kStatPhaseLane + kNumPhases,
    // 2. the counting trace kernel (Trace_Count), named after what [mcrt trace] prints from each
    kStatTraceIters = kStatOverlay,   // wave iterations
    kStatTraceHave,                   // lanes that hold a ray, summed over the iterations
    kStatTraceInnerSteps,             // iterations with an inner step
    kStatTraceInnerLanes,             // ... the lanes in them (inner lane steps)
    kStatTraceLeafSteps,              // iterations with a leaf step
    kStatTraceLeafLanes,              // ... the lanes in them (leaf lane steps)
    kStatTraceLeafWait,               // leaf lanes that waited, summed over the iterations
    kStatTraceInnerCycles,            // wave cycles in inner steps
    kStatTraceLeafCycles,             // ... in leaf steps
    kStatTraceKernelCycles,           // ... in the kernel
    kStatTraceRefillCycles,           // ... in refills
    kStatTracePopCycles,              // ... at the pop site
    kStatTraceEnd,
    // 3. the counting wave-cooperative photon-mapping kernels (PM512 / PM1024 / PMWide _Count*)
    kStatPmEstimateCycles = kStatOverlay,  // wave cycles inside the radiance estimates
    kStatPmKernelCycles,                   // ... in the kernel
    kStatPmEnd,
};
constexpr int statsMax(int a, int b) { return a > b ? a : b; }
constexpr uint32_t kStatsWords = (uint32_t)statsMax(kStatPhaseEnd, statsMax(kStatTraceEnd, kStatPmEnd));
static_assert(kStatPhaseWave >= kStatOverlay && kStatPhaseEnd <= (int)kStatsWords, "the phase clocks fit the statistics buffer");
static_assert(kStatTraceIters >= kStatOverlay && kStatTraceEnd - kStatTraceIters == 12 && kStatTraceEnd <= (int)kStatsWords, "the trace kernel's words fit the statistics buffer");
static_assert(kStatPmEstimateCycles >= kStatOverlay && kStatPmEnd - kStatPmEstimateCycles == 2 && kStatPmEnd <= (int)kStatsWords, "the photon-mapping kernel's words fit the statistics buffer");
static_assert(kStatIorsOverflow == 7 && kStatOverlay == 8, "the numbering is frozen");

// kStatOverflow counts two things the host tells apart: lanes whose traversal stack overflowed (one each; cannot happen - the stacks are
// sized to the tree's own bound) and searches whose kNN frontier did (octrees with leaves far smaller than k): a lane of a megakernel
// adds kStatKnnOverflowBit (kKnnOverflowFlag, mcrt_waveknn.hpp; kLaneKnnOverflow, mcrt_integrator.hpp), the pipeline's kNN launch
// kKnnOverflowUnit per wave.
constexpr unsigned long long kStatKnnOverflowBit = 0x10000ull;
constexpr unsigned long long kKnnOverflowUnit = 1ull << 32;
static_assert(kKnnOverflowUnit >= kStatKnnOverflowBit, "both read as a kNN overflow");
constexpr unsigned long long statsStackOverflows(unsigned long long overflow_word) { return overflow_word & (kStatKnnOverflowBit - 1ull); }
constexpr bool statsKnnOverflowed(unsigned long long overflow_word) { return overflow_word >= kStatKnnOverflowBit; }

// ---- the emission pass's counters (EmitParams::counters)
enum : int {
    kEmitWork = 0,           // the next path to hand out
    kEmitGlobalCount = 1,    // photons counted for the global list ...
    kEmitCausticCount = 2,   // ... and the caustic list, which follows it (list `which` counts at kEmitGlobalCount + which)
    kEmitPaths = 3,
    kEmitRays = 4,
    kEmitOverflow = 5,       // lanes whose traversal stack overflowed
    kEmitIorsOverflow = 6,   // lanes a photon path of which nested deeper than kMaxIors media
    kEmitWords = 8,
};
static_assert(kEmitCausticCount == kEmitGlobalCount + 1 && kEmitIorsOverflow < kEmitWords, "the emission counters");

}  // namespace mcrt
