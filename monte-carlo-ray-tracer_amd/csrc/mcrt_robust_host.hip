// Firefly suppression (include/mcrt.h mcrt_render_highlights*, mcrt_robust_resolve*), host side: the entry points, validation, defaults,
// the host-pointer forms and scratch. No kernel here: they are libmcrt_robust.so (csrc/mcrt_robust.hip; DESIGN.md "Image passes" says
// why, and what mcrt_pass_host.hpp shares). A render's highlights are launched by the pass loops of csrc/mcrt_hip.hip, which find their
// targets in the context: the render's two forms (mcrt_summary_host.hpp, shared with the sample statistics) set them for the length of
// a call, so a frame that mcrt_render_finish renders again fills them again.
#include <cmath>

#include "mcrt_robust.hpp"
#include "mcrt_robust_launch.hpp"
#include "mcrt_summary_host.hpp"

using namespace mcrt;

namespace {

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
    return renderSummaryDevice(ctx, "mcrt_render_highlights_device", cam, global_seed, integrator, summaryOf(d_out_rgb, d_stats_buffers, d_highlights), stats);
}

extern "C" int mcrt_render_highlights(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* out_rgb,
                                      const mcrt_highlight_buffers* highlights, const mcrt_pixel_stats_buffers* stats_buffers, mcrt_stats* stats) {
    return renderSummaryHost(ctx, "mcrt_render_highlights", kPassRobust, cam, global_seed, integrator, summaryOf(out_rgb, stats_buffers, highlights), stats);
}

extern "C" int mcrt_robust_resolve_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* d_rgb, const double* d_tops,
                                          const double* d_level, const mcrt_robust_params* params, double* d_out_rgb,
                                          const mcrt_robust_buffers* d_buffers, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_robust_resolve_device")) return rc;
    const RobustSettings s = robustSettings(params);
    if (int rc = validate(ctx, width, height, spp, d_rgb, d_tops, d_level, s, d_out_rgb, "mcrt_robust_resolve_device")) return rc;
    PassTimer timer(ctx);
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
    if (int rc = timer.begin(stream)) return rc;
    MCRT_HIP_TRY(ctx, (hipError_t)launchRobustResolve(stream, rr));
    if (int rc = timer.end(stream)) return rc;
    return timer.finish(stats, 1);
}

extern "C" int mcrt_robust_resolve(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* rgb, const double* tops,
                                   const double* level, const mcrt_robust_params* params, double* out_rgb, const mcrt_robust_buffers* buffers,
                                   mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_robust_resolve")) return rc;
    const RobustSettings s = robustSettings(params);
    if (int rc = validate(ctx, width, height, spp, rgb, tops, level, s, out_rgb, "mcrt_robust_resolve")) return rc;
    PassTimer whole(ctx);
    const size_t pixels = (size_t)width * height;
    FrameChannel ch[5] = {{rgb, out_rgb, 24},  // (resolved in place)
                          {tops, nullptr, MCRT_ROBUST_TOPS * 24},
                          {level, nullptr, 8},
                          {nullptr, buffers ? buffers->removed : nullptr, 24},
                          {nullptr, buffers ? buffers->clamped : nullptr, 4}};
    StagedFrames frames{{ctx, "mcrt_robust_resolve", kPassRobust, 0, kSlotEach, ch, 5}};
    if (int rc = frames.up(pixels)) return rc;
    const mcrt_robust_buffers d{(double*)ch[3].dev, (uint32_t*)ch[4].dev};
    mcrt_stats st;
    if (int rc = mcrt_robust_resolve_device(ctx, width, height, spp, (double*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev, params,
                                            (double*)ch[0].dev, &d, &st))
        return rc;
    if (int rc = frames.down(pixels)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
