// Firefly suppression (include/mcrt.h mcrt_render_highlights*, mcrt_robust_resolve*), host side: the entry points, validation, defaults,
// the host-pointer forms and scratch. No kernel here: the two kernels are a code object of their own (libmcrt_robust.so,
// csrc/mcrt_robust.hip), so that the device code of libmcrt_hip.so stays what tests/golden/device_code_hashes.json lists. A render's
// highlights are launched by the pass loops of csrc/mcrt_hip.hip, which find their targets in the context: this file sets them for the
// length of a call (ctxHighlightsBegin / End), so a frame that mcrt_render_finish renders again fills them again.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "mcrt_internal.hpp"
#include "mcrt_robust.hpp"
#include "mcrt_robust_launch.hpp"

using namespace mcrt;

namespace {

#define ROBUST_HIP_TRY(ctx, call)                                                                            \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return ctxFail(ctx, MCRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Events {  // the call's own pair: the context's belong to renders and to the operators' timing option
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

struct RobustSettings {
    double kappa, floor;
    uint32_t radius;
};
RobustSettings robustSettings(const mcrt_robust_params* p) {
    RobustSettings s{8.0, 0.0, 1};
    if (p) {
        if (p->kappa != 0.0) s.kappa = p->kappa;
        if (p->floor != 0.0) s.floor = p->floor;
        if (p->radius != 0) s.radius = p->radius;
    }
    return s;
}

int validate(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* rgb, const double* tops, const double* level,
             const RobustSettings& s, const double* out, const char* what) {
    const std::string w(what);
    if ((uint64_t)width * height == 0 || (uint64_t)width * height > 0xFFFFFFFFull)
        return ctxFail(ctx, MCRT_ERR_INVALID, w + ": width * height must be non-zero and below 2^32");
    if (spp == 0) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": spp is 0");
    if (!rgb || !tops || !level || !out) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": the frame, its tops, its level or the output frame is NULL");
    if (!std::isfinite(s.kappa) || s.kappa < 1.0) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": kappa must be finite and at least 1");
    if (!std::isfinite(s.floor) || s.floor < 0.0) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": floor must be finite and not negative");
    if (s.radius > kRobustMaxRadius)
        return ctxFail(ctx, MCRT_ERR_INVALID, w + ": radius " + std::to_string(s.radius) + ", at most " + std::to_string(kRobustMaxRadius));
    return MCRT_OK;
}

}  // namespace

extern "C" int mcrt_render_highlights_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_out_rgb,
                                             const mcrt_highlight_buffers* d_highlights, const mcrt_pixel_stats_buffers* d_stats_buffers,
                                             mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!d_out_rgb) return ctxFail(ctx, MCRT_ERR_INVALID, "d_out_rgb is NULL");
    if (int rc = ctxHighlightsBegin(ctx, cam, d_highlights, "mcrt_render_highlights_device")) return rc;
    int rc = ctxPixelStatsBegin(ctx, cam, d_stats_buffers, "mcrt_render_highlights_device");
    if (rc == MCRT_OK) rc = mcrt_render_device(ctx, cam, global_seed, integrator, d_out_rgb, nullptr);
    if (rc == MCRT_OK) rc = mcrt_render_finish(ctx, stats);  // (renders again when it has to: the targets are still set)
    ctxPixelStatsEnd(ctx);
    ctxHighlightsEnd(ctx);
    return rc;
}

extern "C" int mcrt_render_highlights(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* out_rgb,
                                      const mcrt_highlight_buffers* highlights, const mcrt_pixel_stats_buffers* stats_buffers, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!out_rgb) return ctxFail(ctx, MCRT_ERR_INVALID, "out_rgb is NULL");
    if (int rc = ctxPixelStatsReady(ctx, "mcrt_render_highlights")) return rc;
    if (!cam || cam->width == 0) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_render_highlights: camera is NULL or has no columns");
    if (cam->shard_count > 1 && cam->shard_index >= cam->shard_count) return ctxFail(ctx, MCRT_ERR_INVALID, "shard_index >= shard_count");
    const uint32_t rows = mcrt_shard_rows(cam, nullptr);
    // the frames of the call: host pointer and doubles per pixel; the owned rows packed on the device
    const struct {
        double* host;
        size_t per_pixel;
    } fr[6] = {{out_rgb, 3},
               {highlights ? highlights->tops : nullptr, MCRT_ROBUST_TOPS * 3},
               {highlights ? highlights->level : nullptr, 1},
               {stats_buffers ? stats_buffers->variance : nullptr, 3},
               {stats_buffers ? stats_buffers->half_a : nullptr, 3},
               {stats_buffers ? stats_buffers->half_b : nullptr, 3}};
    double* dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t pixels = (size_t)rows * cam->width;
    for (int i = 0; i < 6; i++)
        if (fr[i].host && !(dev[i] = (double*)ctxRobustScratch(ctx, i, pixels * fr[i].per_pixel * sizeof(double))))
            return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_render_highlights: the frames' device copy could not be allocated");
    const mcrt_highlight_buffers dh{dev[1], dev[2]};
    const mcrt_pixel_stats_buffers ds{dev[3], dev[4], dev[5]};
    mcrt_stats st;
    if (int rc = mcrt_render_highlights_device(ctx, cam, global_seed, integrator, dev[0], &dh, &ds, &st)) return rc;
    if (rows) {
        std::vector<uint32_t> idx(rows);
        mcrt_shard_rows(cam, idx.data());
        std::vector<double> packed;
        for (int i = 0; i < 6; i++) {
            if (!fr[i].host) continue;
            const size_t row_words = (size_t)cam->width * fr[i].per_pixel;
            packed.resize((size_t)rows * row_words);
            ROBUST_HIP_TRY(ctx, hipMemcpy(packed.data(), dev[i], packed.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (uint32_t r = 0; r < rows; r++)
                memcpy(fr[i].host + (size_t)idx[r] * row_words, &packed[(size_t)r * row_words], row_words * sizeof(double));
        }
    }
    if (stats) *stats = st;
    return MCRT_OK;
}

extern "C" int mcrt_robust_resolve_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* d_rgb, const double* d_tops,
                                          const double* d_level, const mcrt_robust_params* params, double* d_out_rgb,
                                          const mcrt_robust_buffers* d_buffers, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxPixelStatsReady(ctx, "mcrt_robust_resolve_device")) return rc;
    const RobustSettings s = robustSettings(params);
    if (int rc = validate(ctx, width, height, spp, d_rgb, d_tops, d_level, s, d_out_rgb, "mcrt_robust_resolve_device")) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    RobustResolve rr;
    rr.rgb = d_rgb;
    rr.tops = d_tops;
    rr.level = d_level;
    rr.out = d_out_rgb;
    rr.removed = d_buffers ? d_buffers->removed : nullptr;
    rr.clamped = d_buffers ? d_buffers->clamped : nullptr;
    rr.width = width;
    rr.height = height;
    rr.spp = spp;
    rr.radius = s.radius;
    rr.kappa = s.kappa;
    rr.floor = s.floor;
    Events ev;
    ROBUST_HIP_TRY(ctx, hipEventCreate(&ev.e0));
    ROBUST_HIP_TRY(ctx, hipEventCreate(&ev.e1));
    ROBUST_HIP_TRY(ctx, hipEventRecord(ev.e0, stream));
    ROBUST_HIP_TRY(ctx, (hipError_t)launchRobustResolve(stream, rr));
    ROBUST_HIP_TRY(ctx, hipEventRecord(ev.e1, stream));
    ROBUST_HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (stats) {
        float ms = 0.f;
        ROBUST_HIP_TRY(ctx, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        memset(stats, 0, sizeof(*stats));
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        stats->kernel_launches = 1;
        stats->kernel_id = MCRT_KERNEL_NONE;  // (names the integrator's kernel form: none ran)
    }
    return MCRT_OK;
}

extern "C" int mcrt_robust_resolve(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* rgb, const double* tops,
                                   const double* level, const mcrt_robust_params* params, double* out_rgb, const mcrt_robust_buffers* buffers,
                                   mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxPixelStatsReady(ctx, "mcrt_robust_resolve")) return rc;
    const RobustSettings s = robustSettings(params);
    if (int rc = validate(ctx, width, height, spp, rgb, tops, level, s, out_rgb, "mcrt_robust_resolve")) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    const size_t pixels = (size_t)width * height;
    double* d_rgb = (double*)ctxRobustScratch(ctx, 0, pixels * 24);  // (resolved in place)
    double* d_tops = (double*)ctxRobustScratch(ctx, 1, pixels * MCRT_ROBUST_TOPS * 24);
    double* d_level = (double*)ctxRobustScratch(ctx, 2, pixels * 8);
    mcrt_robust_buffers d{nullptr, nullptr};
    if (buffers && buffers->removed) d.removed = (double*)ctxRobustScratch(ctx, 3, pixels * 24);
    if (buffers && buffers->clamped) d.clamped = (uint32_t*)ctxRobustScratch(ctx, 4, pixels * 4);
    if (!d_rgb || !d_tops || !d_level || (buffers && buffers->removed && !d.removed) || (buffers && buffers->clamped && !d.clamped))
        return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_robust_resolve: the frames' device copy could not be allocated");
    ROBUST_HIP_TRY(ctx, hipMemcpy(d_rgb, rgb, pixels * 24, hipMemcpyHostToDevice));
    ROBUST_HIP_TRY(ctx, hipMemcpy(d_tops, tops, pixels * MCRT_ROBUST_TOPS * 24, hipMemcpyHostToDevice));
    ROBUST_HIP_TRY(ctx, hipMemcpy(d_level, level, pixels * 8, hipMemcpyHostToDevice));
    mcrt_stats st;
    if (int rc = mcrt_robust_resolve_device(ctx, width, height, spp, d_rgb, d_tops, d_level, params, d_rgb, &d, &st)) return rc;
    ROBUST_HIP_TRY(ctx, hipMemcpy(out_rgb, d_rgb, pixels * 24, hipMemcpyDeviceToHost));
    if (d.removed) ROBUST_HIP_TRY(ctx, hipMemcpy(buffers->removed, d.removed, pixels * 24, hipMemcpyDeviceToHost));
    if (d.clamped) ROBUST_HIP_TRY(ctx, hipMemcpy(buffers->clamped, d.clamped, pixels * 4, hipMemcpyDeviceToHost));
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = st;
    return MCRT_OK;
}
