// What mcrt_render_finish makes of a frame's statistics words (mcrt_stats_words.hpp), as pure functions of the words: the counters of
// mcrt_stats, the readouts it prints on stderr, and the outcome nextRender (mcrt_select.hpp) decides on. No HIP, no mcrt_ctx: built
// into tests/emu so that the readouts are checked without a GPU (tests/test_stats_words.py).
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "mcrt_select.hpp"
#include "mcrt_stats_words.hpp"

namespace mcrt {

inline void statsCounters(const unsigned long long* w, mcrt_stats& s) {
    s.paths = w[kStatPaths];
    s.rays = w[kStatRays];
    s.node_tests = w[kStatNodeTests];
    s.prim_tests = w[kStatPrimTests];
    s.knn_searches = w[kStatKnnSearches];
}

// ... what nextRender reads of the words; splats and can_pipeline are the caller's
inline FrameOutcome statsOutcome(const unsigned long long* w, uint32_t kernel_id) {
    FrameOutcome frame;
    frame.kernel_id = kernel_id;
    frame.overflow = w[kStatOverflow];
    frame.iors_overflow = w[kStatIorsOverflow] != 0;
    return frame;
}

inline void statsAppendf(std::string& text, const char* fmt, ...) {
    va_list ap, ap2;
    va_start(ap, fmt);
    va_copy(ap2, ap);
    const int n = vsnprintf(nullptr, 0, fmt, ap);
    va_end(ap);
    if (n > 0) {
        const size_t at = text.size();
        text.resize(at + (size_t)n + 1);
        vsnprintf(&text[at], (size_t)n + 1, fmt, ap2);
        text.resize(at + (size_t)n);
    }
    va_end(ap2);
}

// Readouts of the overlay words - only of what the instances that ran measured (noteInstances, mcrt_hip.hip). The phase clocks, the
// trace kernel's step counters and the photon-mapping kernel's estimate clocks share those words: a line is printed for the kernel that
// wrote them and never from the option alone (MCRT_PROFILE_PHASES on a form without a profiling instance - pipeline, photon kernels - or
// next to MCRT_COUNT_TESTS, which a profiling instance does not carry, used to print another kernel's words as phases), and never with a
// zero divisor (a frame whose launches found no work leaves every clock at 0).
inline std::string statsReadout(const unsigned long long* w, int used_instance, int used_trace, uint32_t kernel_id) {
    std::string text;
    if (instanceProfiles(used_instance)) {
        static const char* names[kNumPhases] = {"regen", "trav/inner", "shade", "shadow/leaf", "sample", "loop"};
        const unsigned long long *wave = w + kStatPhaseWave, *lane = w + kStatPhaseLane;
        unsigned long long tw = 0;
        for (int i = 0; i < kNumPhases; i++) tw += wave[i];
        for (int i = 0; tw && i < kNumPhases; i++)
            statsAppendf(text, "[mcrt phase] %-9s wave-cycles %6.2f%%  lane utilisation %5.1f%%\n", names[i], 100.0 * wave[i] / (double)tw,
                         wave[i] ? 100.0 * lane[i] / (64.0 * wave[i]) : 0.0);
    }
    if (kernel_id == MCRT_KERNEL_WAVEFRONT && used_trace == kInstTrace_Count && w[kStatTraceIters] && w[kStatTraceKernelCycles]) {
        const double iters = (double)w[kStatTraceIters], cyc = (double)w[kStatTraceKernelCycles], rays = (double)(w[kStatRays] ? w[kStatRays] : 1);
        const unsigned long long in_steps = w[kStatTraceInnerSteps], in_lanes = w[kStatTraceInnerLanes], lf_steps = w[kStatTraceLeafSteps], lf_lanes = w[kStatTraceLeafLanes];
        const unsigned long long stepped = std::min(w[kStatTraceInnerCycles] + w[kStatTraceLeafCycles], w[kStatTraceKernelCycles]);
        statsAppendf(text, "[mcrt trace] per wave iteration: %.1f lanes hold a ray; inner step in %.1f%% of the iterations with %.1f lanes, leaf step in %.1f%% with %.1f lanes, "
                           "%.1f leaf lanes wait; wave cycles: inner %.1f%%, leaf %.1f%%, rest %.1f%% (of the kernel: refills %.1f%%, pop site %.1f%%); per ray: %.2f inner steps, %.2f leaf steps "
                           "(%llu inner and %llu leaf lane steps of %llu rays)\n",
                     (double)w[kStatTraceHave] / iters, 100.0 * in_steps / iters, in_steps ? (double)in_lanes / in_steps : 0.0, 100.0 * lf_steps / iters,
                     lf_steps ? (double)lf_lanes / lf_steps : 0.0, (double)w[kStatTraceLeafWait] / iters, 100.0 * w[kStatTraceInnerCycles] / cyc,
                     100.0 * w[kStatTraceLeafCycles] / cyc, 100.0 * (w[kStatTraceKernelCycles] - stepped) / cyc, 100.0 * w[kStatTraceRefillCycles] / cyc,
                     100.0 * w[kStatTracePopCycles] / cyc, (double)in_lanes / rays, (double)lf_lanes / rays, in_lanes, lf_lanes, w[kStatRays]);
    }
    if (kernel_id == MCRT_KERNEL_PM_WAVE && instanceClocksEstimates(used_instance) && w[kStatPmKernelCycles])
        statsAppendf(text, "[mcrt pm] wave cycles inside the radiance estimates: %.1f%% of the kernel (%llu searches, %.1f octants per search)\n",
                     100.0 * (double)std::min(w[kStatPmEstimateCycles], w[kStatPmKernelCycles]) / (double)w[kStatPmKernelCycles], w[kStatKnnSearches],
                     w[kStatKnnSearches] ? (double)w[kStatKnnOctants] / (double)w[kStatKnnSearches] : 0.0);
    return text;
}

}  // namespace mcrt
