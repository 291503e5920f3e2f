// Adaptive sampling (include/mcrt.h mcrt_render_adaptive*), host side: validation, defaults, the accumulators, the loop over the batches
// and the host-pointer form. No kernel here: they are libmcrt_adaptive.so (csrc/mcrt_adaptive.hip; DESIGN.md "Image passes" says why).
// Per batch: the rule and the list (launchAdaptiveFlags, Count, Scan, Scatter), the host reading ONE word, the list's length; then either
// mcrt_render_pixel_stats_device and launchAdaptiveMerge (the list is the whole frame and option MCRT_ADAPTIVE_FULL_BATCH is not "walk")
// or the light groups' bounce loop (runLivePathsOf, mcrt_live_paths_host.hpp) behind the camera-ray passes' chunk loop, both taking
// their pixels from the list (ListPixels below) and ending in launchAdaptiveResolve. The family's scratch: slot 0 the samples' state,
// 1 their radiances - before the first walk the four frames of a rendered full batch: rendered batches all come before it -, 2 the
// shadow and bounce records, 3 the two live lists and the counters, 4 the accumulators, the counts, the flags, the pixel list and the block counts, 5 the host-pointer form's frames. Option MCRT_AOV_CHUNK_RAYS bounds the shadow
// and bounce SLOTS of iteration 0 of a chunk of the list: pixels * spp * 2, as in the light groups.
// Option MCRT_ADAPTIVE_LOG (tools/adaptive_probe.py sets it): one JSON line per batch on stderr - the list's length, the form and the
// host-clock milliseconds of the rule with the list and of the batch. It changes no result.
#include <cstring>
#include <vector>

#include "mcrt_adaptive_launch.hpp"
#include "mcrt_film.hpp"
#include "mcrt_live_paths_host.hpp"

using namespace mcrt;

namespace {

// The chunks of a pixel list: chunk(...) cuts entries [first, first + chunk_pixels) of it, rays(...) is this library's camera-ray kernel.
struct ListPixels {
    const uint32_t* list;
    const uint32_t* count;
    AdaptiveChunk chunk(const mcrt_camera_desc& cam, uint32_t global_seed, uint32_t spp, uint64_t first, uint64_t chunk_pixels, uint64_t total_pixels) const {
        AdaptiveChunk c;
        static_cast<AovChunk&>(c) = chunkAt(cam, global_seed, spp, first, chunk_pixels, total_pixels);
        c.list = list;
        c.count = count;
        return c;
    }
    int rays(hipStream_t stream, const AdaptiveChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays_) const {
        return launchAdaptiveCameraRays(stream, c, scene_ior, sobol_tab, rays_);
    }
};

void addStats(mcrt_stats& sum, const mcrt_stats& st) {
    sum.paths += st.paths;
    sum.rays += st.rays;
    sum.node_tests += st.node_tests;
    sum.prim_tests += st.prim_tests;
    sum.knn_searches += st.knn_searches;
    sum.kernel_ms += st.kernel_ms;
    sum.kernel_launches += st.kernel_launches;
}

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_adaptive_params* params, const void* frame, AdaptiveSettings& s, const char* what) {
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (ctxLens(ctx))  // (the lists' camera rays are this library's own kernel, the perspective camera's)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": a lens is set (mcrt_set_lens): adaptive sampling traces the camera's own rays only");
    if (ctxRaySource(ctx))
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": a ray source is set (mcrt_set_ray_source): adaptive sampling traces the camera's own rays only");
    if (!cam) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": camera is NULL");
    if (!frame) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": the frame (out_rgb) is NULL");
    if (int rc = ctxNeedScene(ctx, what)) return rc;
    if (int rc = checkCamera(ctx, cam, true, what)) return rc;
    const char* why = nullptr;
    if (int rc = adaptiveSettings(params, cam->sqrtspp, s, &why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);
    if (cam->shard_count > 1)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": a sharded camera - the window of the rule needs the neighbouring rows");
    if (filmSplats(cam->film_filter, cam->film_radius))
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": a frame whose film splats (a reconstruction filter, or a box of another radius) keeps no "
                                                      "samples per pixel: there is nothing to take a pixel's statistics of");
    return checkPixelSlots(ctx, cam, 2, "rays", what);
}

}  // namespace

extern "C" int mcrt_render_adaptive_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_adaptive_params* params, double* d_out_rgb,
                                           const mcrt_pixel_stats_buffers* d_stats, uint32_t* d_count, mcrt_adaptive_result* result, mcrt_stats* stats) {
    const char* what = "mcrt_render_adaptive_device";
    if (!ctx) return MCRT_ERR_INVALID;
    AdaptiveSettings s;
    if (int rc = validate(ctx, cam, params, d_out_rgb, s, what)) return rc;
    const char* form = ctxOpt(ctx, "MCRT_ADAPTIVE_FULL_BATCH");
    if (form && *form && std::strcmp(form, "render") != 0 && std::strcmp(form, "walk") != 0)
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": option MCRT_ADAPTIVE_FULL_BATCH is render or walk");
    const bool render_full = !(form && std::strcmp(form, "walk") == 0);
    const bool log = ctxOptOn(ctx, "MCRT_ADAPTIVE_LOG");

    PassTimer whole(ctx);
    const CameraPass cp(ctx);
    const hipStream_t stream = cp.stream;
    const AovScene& scene = cp.scene;
    const uint32_t* sobol_tab = cp.sobol_tab;
    const uint64_t pixels = (uint64_t)cam->width * cam->height;
    const uint32_t n = cam->sqrtspp * cam->sqrtspp, blocks = adaptiveBlocks(pixels);
    uint32_t num_surfaces = 0, num_materials = 0;
    ctxSceneCounts(ctx, &num_surfaces, &num_materials);

    // slot 4: the accumulators' four frames, then the 4-byte arrays, then the bytes
    const size_t frame = (size_t)pixels * 24;
    const size_t words = (size_t)pixels * 2 + (size_t)blocks * 2 + 2;  // count, list, block counts, offsets, length (and a word of padding)
    const size_t plane_bytes = std::max<uint32_t>(num_surfaces, 1u);
    unsigned char* base = (unsigned char*)ctxPassScratch(ctx, kPassAdaptive, 4, 4 * frame + words * 4 + (size_t)pixels + plane_bytes);
    if (!base) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the accumulators could not be allocated");
    double* frames = (double*)base;
    uint32_t* word = (uint32_t*)(base + 4 * frame);
    AdaptiveFrame acc{frames, frames + 3 * pixels, frames + 6 * pixels, frames + 9 * pixels, word};
    uint32_t* list = word + pixels;
    uint32_t* block_counts = list + pixels;
    uint32_t* offsets = block_counts + blocks;
    uint32_t* d_length = offsets + blocks;
    uint8_t* flags = (uint8_t*)(word + words);
    uint8_t* plane = flags + pixels;  // the walk's one plane: every surface's is 0
    MCRT_HIP_TRY(ctx, hipMemsetAsync(acc.count, 0, (size_t)pixels * 4, stream));
    MCRT_HIP_TRY(ctx, hipMemsetAsync(plane, 0, plane_bytes, stream));

    LgParams par;
    par.plane = plane;
    par.planes = 1u;
    par.sky_plane = 0u;
    par.max_depth = 0u;

    // the walk's scratch, sized at the first walk for the largest list there can be (the frame) and kept
    const uint64_t sample_bytes = kLgStateBytes + 24ull + 2 * kLivePathRecordBytes + 8;
    const uint64_t chunk_dflt = lightGroupsDefaultChunkSlots((uint64_t)n * 2, sample_bytes);
    const long chunk_opt = ctxOptL(ctx, "MCRT_AOV_CHUNK_RAYS", 0);
    const uint64_t chunk_want = chunk_opt > 0 ? (uint64_t)chunk_opt : 0;
    LgState st{};
    LivePathScratch sc{};
    bool walk_ready = false;

    AdaptiveRule rule;
    rule.t2 = s.target * s.target;
    rule.f2 = s.floor < 0.0 ? 0.0 : s.floor * s.floor;  // (the default: after batch 0, below; batch 0's list does not read it)
    rule.width = cam->width;
    rule.height = cam->height;
    rule.n = n;
    rule.max_spp = s.max_spp;
    rule.window = s.window;

    mcrt_adaptive_result res{};
    bool uniform = true;
    mcrt_stats sum{};
    sum.kernel_id = MCRT_KERNEL_NONE;
    auto clock_ms = [&] { return whole.hostMs(); };
    for (uint32_t j = 0;; j++) {
        const double t0 = log ? clock_ms() : 0.0;
        rule.force = j < s.min_batches || s.target == 0.0 ? 1u : 0u;
        MCRT_HIP_TRY(ctx, (hipError_t)launchAdaptiveFlags(stream, acc, rule, flags));
        MCRT_HIP_TRY(ctx, (hipError_t)launchAdaptiveCount(stream, flags, pixels, block_counts));
        MCRT_HIP_TRY(ctx, (hipError_t)launchAdaptiveScan(stream, block_counts, blocks, offsets, d_length));
        uint32_t listed = 0;
        MCRT_HIP_TRY(ctx, hipMemcpyAsync(&listed, d_length, 4, hipMemcpyDeviceToHost, stream));
        MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
        sum.kernel_launches += 3;
        if (listed > pixels) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the list is longer than the frame");  // (cannot happen)
        if (listed == 0u) break;
        // a batch over the whole frame is a render when every pixel is at ITS batch j: no batch before it left a pixel out
        const bool rendered = listed == pixels && uniform && render_full;
        uniform = uniform && listed == pixels;
        if (!rendered) {
            MCRT_HIP_TRY(ctx, (hipError_t)launchAdaptiveScatter(stream, flags, pixels, offsets, list));
            sum.kernel_launches += 1;
        }
        const double t1 = log ? ((void)hipStreamSynchronize(stream), clock_ms()) : 0.0;
        if (j < MCRT_CONVERGE_TRACE) res.active[j] = listed;
        mcrt_stats bst;
        if (rendered) {
            // the batch's four frames: only a rendered batch has them. Rendered batches come before the first walk (`uniform`), so
            // they borrow the slot of the walk's radiances, which is sized anew when the walk is set up.
            double* batch = walk_ready ? nullptr : (double*)ctxPassScratch(ctx, kPassAdaptive, 1, 4 * frame);
            if (!batch) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the batch frames could not be allocated");
            const AdaptiveFrame bat{batch, batch + 3 * pixels, batch + 6 * pixels, batch + 9 * pixels, nullptr};
            const mcrt_pixel_stats_buffers ds{bat.variance, bat.half_a, bat.half_b};
            if (int rc = mcrt_render_pixel_stats_device(ctx, cam, global_seed + j, MCRT_INTEGRATOR_PATH_TRACER, bat.rgb, &ds, &bst)) return rc;
            MCRT_HIP_TRY(ctx, (hipError_t)launchAdaptiveMerge(stream, acc, bat, pixels, n));
            MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
            bst.kernel_launches += 1;
            sum.kernel_id = bst.kernel_id;
        } else {
            const PixelChunks plan = pixelChunks(listed, n, (uint64_t)n * 2, chunk_want, chunk_dflt);
            if (!walk_ready) {
                const uint64_t max_n = pixelChunks(pixels, n, (uint64_t)n * 2, chunk_want, chunk_dflt).max_rays;
                void* state = ctxPassScratch(ctx, kPassAdaptive, 0, max_n * kLgStateBytes);
                double* radiance = (double*)ctxPassScratch(ctx, kPassAdaptive, 1, max_n * 24);
                if (!state || !radiance || !livePathScratch(ctx, kPassAdaptive, max_n, sc))
                    return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string((max_n * sample_bytes) >> 20) +
                                                          " MiB of path state could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
                lgPlaceState(st, state, max_n);
                st.radiance = radiance;
                walk_ready = true;
            }
            PassTimer timer(ctx);
            const int rc = runLivePathsOf(
                ListPixels{list, acc.count}, ctx, what, cp, timer, cam, global_seed, plan, st.ray, &bst, sc, 0u, false, "adaptive_chunk",
                [&](const AdaptiveChunk&, uint64_t samples, uint32_t* live_list, LgCounters* counters) {
                    return launchAdaptiveBegin(stream, st, samples, scene.sh.scene_ior, par, live_list, counters);
                },
                [&](const AdaptiveChunk& c, const uint32_t* live_list, uint32_t live, uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next) {
                    return launchAdaptiveRays(stream, c, scene, sobol_tab, st, live_list, live, k, lit, counters, next);
                },
                [&](const AdaptiveChunk& c, const uint32_t* live_list, uint32_t live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters,
                    uint32_t next) { return launchAdaptiveStep(stream, c, scene, sobol_tab, st, par, live_list, live, k, last, lit, next_list, counters, next); },
                [&](const AdaptiveChunk& c) { return launchAdaptiveResolve(stream, c, st, acc); });
            if (rc) return rc;
        }
        addStats(sum, bst);
        res.batches = j + 1;
        if (j == 0 && s.floor < 0.0) {  // the default floor, from the frame after batch 0
            mcrt_frame_noise_result noise;
            if (int rc = mcrt_frame_noise_device(ctx, pixels, n, acc.rgb, acc.variance, &noise)) return rc;
            const double floor = adaptiveDefaultFloor(noise.signal, pixels);
            rule.f2 = floor * floor;
        }
        if (log)
            std::fprintf(stderr, "{\"adaptive_batch\":%u,\"listed\":%u,\"form\":\"%s\",\"list_ms\":%.3f,\"batch_ms\":%.3f}\n", j, listed, rendered ? "render" : "walk", t1 - t0,
                         clock_ms() - t1);
    }

    // the counts: to the caller, and to the host for the result
    std::vector<uint32_t> counts((size_t)pixels);
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(counts.data(), acc.count, (size_t)pixels * 4, hipMemcpyDeviceToHost, stream));
    if (d_count) MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_count, acc.count, (size_t)pixels * 4, hipMemcpyDeviceToDevice, stream));
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_out_rgb, acc.rgb, frame, hipMemcpyDeviceToDevice, stream));
    if (d_stats && d_stats->variance) MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_stats->variance, acc.variance, frame, hipMemcpyDeviceToDevice, stream));
    if (d_stats && d_stats->half_a) MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_stats->half_a, acc.half_a, frame, hipMemcpyDeviceToDevice, stream));
    if (d_stats && d_stats->half_b) MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_stats->half_b, acc.half_b, frame, hipMemcpyDeviceToDevice, stream));
    MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
    res.min_count = 0xFFFFFFFFu;
    for (uint32_t c : counts) {
        res.min_count = std::min(res.min_count, c);
        res.max_count = std::max(res.max_count, c);
        res.samples += c;
    }
    sum.total_ms = whole.hostMs();
    if (result) *result = res;
    if (stats) *stats = sum;
    return MCRT_OK;
}

extern "C" int mcrt_render_adaptive(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_adaptive_params* params, double* out_rgb,
                                    const mcrt_pixel_stats_buffers* stats_buffers, uint32_t* count, mcrt_adaptive_result* result, mcrt_stats* stats) {
    const char* what = "mcrt_render_adaptive";
    if (!ctx) return MCRT_ERR_INVALID;
    AdaptiveSettings s;
    if (int rc = validate(ctx, cam, params, out_rgb, s, what)) return rc;
    PassTimer whole(ctx);
    FrameChannel ch[5] = {{nullptr, out_rgb, 24},
                          {nullptr, stats_buffers ? stats_buffers->variance : nullptr, 24},
                          {nullptr, stats_buffers ? stats_buffers->half_a : nullptr, 24},
                          {nullptr, stats_buffers ? stats_buffers->half_b : nullptr, 24},
                          {nullptr, count, 4}};
    const size_t pixels = (size_t)cam->width * cam->height;
    StagedFrames frames{{ctx, what, kPassAdaptive, 5, kPackedWanted, ch, 5}};
    if (int rc = frames.place(pixels)) return rc;
    const mcrt_pixel_stats_buffers ds{(double*)ch[1].dev, (double*)ch[2].dev, (double*)ch[3].dev};
    mcrt_stats st;
    if (int rc = mcrt_render_adaptive_device(ctx, cam, global_seed, params, (double*)ch[0].dev, &ds, (uint32_t*)ch[4].dev, result, &st)) return rc;
    if (int rc = frames.down(pixels)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}

extern "C" int mcrt_adaptive_list(mcrt_ctx* ctx, uint64_t pixels, const uint8_t* flags, uint32_t* list, uint32_t* length) {
    const char* what = "mcrt_adaptive_list";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (!flags || !list || !length) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": the flags, the list or the length is NULL");
    if (pixels == 0 || pixels > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": pixels must be non-zero and below 2^32");
    const hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const uint32_t blocks = adaptiveBlocks(pixels);
    // the words first: the list, the block counts, the offsets, the length; then the flags
    uint32_t* d_list = (uint32_t*)ctxPassScratch(ctx, kPassAdaptive, 5, ((size_t)pixels + 2 * (size_t)blocks + 1) * 4 + (size_t)pixels);
    if (!d_list) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": scratch could not be allocated");
    uint32_t* block_counts = d_list + pixels;
    uint32_t* offsets = block_counts + blocks;
    uint32_t* d_length = offsets + blocks;
    uint8_t* d_flags = (uint8_t*)(d_length + 1);
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_flags, flags, (size_t)pixels, hipMemcpyHostToDevice, stream));
    MCRT_HIP_TRY(ctx, (hipError_t)launchAdaptiveCount(stream, d_flags, pixels, block_counts));
    MCRT_HIP_TRY(ctx, (hipError_t)launchAdaptiveScan(stream, block_counts, blocks, offsets, d_length));
    MCRT_HIP_TRY(ctx, (hipError_t)launchAdaptiveScatter(stream, d_flags, pixels, offsets, d_list));
    uint32_t n = 0;
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(&n, d_length, 4, hipMemcpyDeviceToHost, stream));
    MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (n > pixels) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the list is longer than the flags");  // (cannot happen)
    if (n) MCRT_HIP_TRY(ctx, hipMemcpy(list, d_list, (size_t)n * 4, hipMemcpyDeviceToHost));
    *length = n;
    return MCRT_OK;
}
