// The bounce loop of the passes that walk whole paths over live lists - the light groups, the path classes and adaptive sampling
// (mcrt_{light_groups,path_classes,adaptive}_host.hip) - behind the camera-ray passes' chunk loop (mcrt_camera_pass.hpp): per chunk begin, then
// per iteration rays -> intersectDeviceArrays over 2 rays per LIVE sample -> step, the host reading the next list's count (and the
// pass's error word) after every step; resolve when no sample is alive. Each pass hands in its own four launches. Scratch of the family:
// slot 2 the shadow and bounce records, 3 the two live lists and the counters.
// With `log` one JSON line per chunk on stderr, keyed `log_key` - the live samples of every iteration and the host-clock milliseconds of
// the chunk and of its searches, the stream drained before each bounce search so that the kernels queued before it are not counted as
// search (the camera rays' kernel is counted with their search). It changes no result.
#pragma once

#include <chrono>
#include <cstdio>

#include "mcrt_camera_pass.hpp"
#include "mcrt_light_groups.hpp"

namespace mcrt {

constexpr uint64_t kLivePathRecordBytes = 76;  // start, direction, t, surface, uv of one ray

struct LivePathScratch {
    AovRays lit;  // 2 * max_n records
    LgCounters* counters;
    uint32_t* list[2];
};

// false: an allocation failed
inline bool livePathScratch(mcrt_ctx* ctx, PassFamily family, uint64_t max_n, LivePathScratch& sc) {
    double* records = (double*)ctxPassScratch(ctx, family, 2, 2 * max_n * kLivePathRecordBytes);
    uint32_t* lists = (uint32_t*)ctxPassScratch(ctx, family, 3, sizeof(LgCounters) + 2 * max_n * 4);
    if (!records || !lists) return false;
    sc.lit.start = records;
    sc.lit.direction = sc.lit.start + 6 * max_n;
    sc.lit.t = sc.lit.direction + 6 * max_n;
    sc.lit.uv = sc.lit.t + 2 * max_n;
    sc.lit.surface = (uint32_t*)(sc.lit.uv + 4 * max_n);
    sc.counters = (LgCounters*)lists;
    sc.list[0] = lists + sizeof(LgCounters) / 4;
    sc.list[1] = sc.list[0] + max_n;
    return true;
}

// begin(c, n, list, counters), rays(c, list, live, k, lit, counters, next), step(c, list, live, k, last, lit, next_list, counters, next)
// and resolve(c) queue one kernel each and return its hipError_t as an int. camera_rays: where the chunk loop writes the camera rays
// and their hits (the samples' state). naming: how the chunks name their pixels (mcrt_camera_pass.hpp FramePixels; c is its chunk).
template <class Naming, class Begin, class Rays, class Step, class Resolve>
int runLivePathsOf(const Naming& naming, mcrt_ctx* ctx, const char* what, const CameraPass& cp, PassTimer& timer, const mcrt_camera_desc* cam, uint32_t global_seed, const PixelChunks& plan,
                 const AovRays& camera_rays, mcrt_stats* stats, const LivePathScratch& sc, uint32_t max_depth, bool log, const char* log_key, Begin begin, Rays rays_of,
                 Step step, Resolve resolve) {
    const hipStream_t stream = cp.stream;
    const AovRays& lit = sc.lit;
    LgCounters* counters = sc.counters;
    auto clock_ms = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto search = [&](uint64_t count, const AovRays& rays_, double& ms) {
        if (!log) return intersectDeviceArrays(ctx, count, rays_.start, rays_.direction, rays_.t, rays_.surface, rays_.uv);
        (void)hipStreamSynchronize(stream);
        const double t0 = clock_ms();
        const int rc = intersectDeviceArrays(ctx, count, rays_.start, rays_.direction, rays_.t, rays_.surface, rays_.uv);
        ms += clock_ms() - t0;
        return rc;
    };
    double chunk_t0 = log ? clock_ms() : 0.0;  // (a chunk's clock starts where the one before it ended: the stream is drained there)
    return runChunksOf(naming, ctx, cp, timer, cam, global_seed, plan, camera_rays, stats, [&](const auto& c, uint32_t& launches, uint64_t& rays) {
        const uint64_t n = (uint64_t)c.pixels * c.spp;
        double search_ms = log ? clock_ms() - chunk_t0 : 0.0;  // the camera rays and their search
        std::string curve;
        MCRT_HIP_TRY(ctx, hipMemsetAsync(counters, 0, sizeof(LgCounters), stream));
        MCRT_HIP_TRY(ctx, (hipError_t)begin(c, n, sc.list[0], counters));
        LgCounters now;
        MCRT_HIP_TRY(ctx, hipMemcpyAsync(&now, counters, sizeof(now), hipMemcpyDeviceToHost, stream));
        MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
        launches++;
        uint32_t live = now.live[0];
        for (uint32_t k = 0; live != 0u; k++) {
            if (k >= kLgMaxIterations)
                return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": " + std::to_string(live) + " paths are still alive after " +
                                                              std::to_string(kLgMaxIterations) + " iterations (max_depth cuts them)");
            const uint32_t cur = k & 1u, next = cur ^ 1u;
            if (log) curve += (k ? "," : "") + std::to_string(live);
            const bool last = max_depth != 0u && k == max_depth;
            if (!last) {
                MCRT_HIP_TRY(ctx, (hipError_t)rays_of(c, sc.list[cur], live, k, lit, counters, next));
                if (int rc = search(2ull * live, lit, search_ms)) return rc;
                launches += 2;
                rays += 2ull * live;
            }
            if (last) MCRT_HIP_TRY(ctx, hipMemsetAsync(&counters->live[next], 0, 4, stream));  // (otherwise the ray kernel did)
            MCRT_HIP_TRY(ctx, (hipError_t)step(c, sc.list[cur], live, k, last, lit, sc.list[next], counters, next));
            launches++;
            MCRT_HIP_TRY(ctx, hipMemcpyAsync(&now, counters, sizeof(now), hipMemcpyDeviceToHost, stream));
            MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
            if (now.too_deep)
                return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": a path nests more than " + std::to_string(kMaxIors) +
                                                              " dielectric media (mcrt_render renders such frames through the pipeline's deep rows; this pass does not)");
            if (now.live[next] > live) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the live list grew");  // (cannot happen: a sample is appended once)
            live = now.live[next];
        }
        MCRT_HIP_TRY(ctx, (hipError_t)resolve(c));
        launches++;
        if (log) {
            (void)hipStreamSynchronize(stream);
            const double now_ms = clock_ms();
            std::fprintf(stderr, "{\"%s\":%llu,\"samples\":%llu,\"live\":[%s],\"chunk_ms\":%.3f,\"search_ms\":%.3f}\n", log_key, (unsigned long long)c.first_pixel,
                         (unsigned long long)n, curve.c_str(), now_ms - chunk_t0, search_ms);
            chunk_t0 = now_ms;
        }
        return (int)MCRT_OK;
    });
}

template <class Begin, class Rays, class Step, class Resolve>
int runLivePaths(mcrt_ctx* ctx, const char* what, const CameraPass& cp, PassTimer& timer, const mcrt_camera_desc* cam, uint32_t global_seed, const PixelChunks& plan,
                 const AovRays& camera_rays, mcrt_stats* stats, const LivePathScratch& sc, uint32_t max_depth, bool log, const char* log_key, Begin begin, Rays rays_of,
                 Step step, Resolve resolve) {
    if (const mcrt_lens_desc* lens = ctxLens(ctx))
        return runLivePathsOf(LensPixels(*lens), ctx, what, cp, timer, cam, global_seed, plan, camera_rays, stats, sc, max_depth, log, log_key, begin, rays_of, step, resolve);
    if (const mcrt_ray_source_desc* source = ctxRaySource(ctx))
        return runLivePathsOf(SourcePixels(*source), ctx, what, cp, timer, cam, global_seed, plan, camera_rays, stats, sc, max_depth, log, log_key, begin, rays_of, step, resolve);
    return runLivePathsOf(FramePixels{}, ctx, what, cp, timer, cam, global_seed, plan, camera_rays, stats, sc, max_depth, log, log_key, begin, rays_of, step, resolve);
}

}  // namespace mcrt
