// Per-pixel sample statistics and the frame summary (include/mcrt.h mcrt_render_pixel_stats*, mcrt_frame_noise*), host side: the
// entry points, validation, the host-pointer forms and scratch. No kernel here: they are libmcrt_pixel_stats.so (csrc/mcrt_pixel_stats.hip;
// DESIGN.md "Image passes" says why, and what mcrt_pass_host.hpp shares). A render's statistics are launched by the pass loops of
// csrc/mcrt_hip.hip, which find their targets in the context: the render's two forms (mcrt_summary_host.hpp, shared with the firefly
// suppression) set them for the length of a call. Scratch slots: 0 .. 3 the host forms (the summary's channels in order), 4 and 5 the noise levels.
#include <cmath>

#include "mcrt_pixel_stats.hpp"
#include "mcrt_pixel_stats_launch.hpp"
#include "mcrt_summary_host.hpp"

using namespace mcrt;

extern "C" int mcrt_render_pixel_stats_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_out_rgb,
                                              const mcrt_pixel_stats_buffers* d_buffers, mcrt_stats* stats) {
    return renderSummaryDevice(ctx, "mcrt_render_pixel_stats_device", cam, global_seed, integrator, summaryOf(d_out_rgb, d_buffers, nullptr), stats);
}

extern "C" int mcrt_render_pixel_stats(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* out_rgb,
                                       const mcrt_pixel_stats_buffers* buffers, mcrt_stats* stats) {
    return renderSummaryHost(ctx, "mcrt_render_pixel_stats", kPassPixelStats, cam, global_seed, integrator, summaryOf(out_rgb, buffers, nullptr), stats);
}

extern "C" int mcrt_frame_noise_device(mcrt_ctx* ctx, uint64_t pixels, uint32_t spp, const double* d_rgb, const double* d_variance,
                                       mcrt_frame_noise_result* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_frame_noise_device")) return rc;
    if (!d_rgb || !d_variance || !out) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise_device: the frame, the variance or the result is NULL");
    if (pixels == 0 || pixels >= kFrameNoiseMaxPixels) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise_device: pixels must be non-zero and below 2^38");
    if (spp == 0) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise_device: spp is 0");
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    // the block values of the levels, ping-ponged: [0] holds level 0's (and every second one's), [1] the others'; e first, then g
    const uint64_t blocks0 = frameNoiseBlocks(pixels);
    double* buf[2] = {(double*)ctxPassScratch(ctx, kPassPixelStats, 4, blocks0 * 2 * sizeof(double)),
                      (double*)ctxPassScratch(ctx, kPassPixelStats, 5, frameNoiseBlocks(blocks0) * 2 * sizeof(double))};
    if (!buf[0] || !buf[1]) return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_frame_noise_device: scratch could not be allocated");
    FrameNoiseLevel lv{};
    lv.rgb = d_rgb;
    lv.variance = d_variance;
    lv.spp = (double)spp;
    lv.n = pixels;
    int which = 0;
    for (;;) {
        const uint64_t blocks = frameNoiseBlocks(lv.n);
        lv.out_e = buf[which];
        lv.out_g = buf[which] + blocks;
        MCRT_HIP_TRY(ctx, (hipError_t)launchFrameNoiseLevel(stream, lv));
        if (blocks == 1) break;
        lv.rgb = lv.variance = nullptr;
        lv.in_e = lv.out_e;
        lv.in_g = lv.out_g;
        lv.n = blocks;
        which ^= 1;
    }
    double r[2];
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(r, buf[which], sizeof(r), hipMemcpyDeviceToHost, stream));
    MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
    out->noise = r[0];
    out->signal = r[1];
    out->relative_error = r[1] > 0.0 ? std::sqrt(r[0] / r[1]) : 0.0;
    out->pixels = pixels;
    return MCRT_OK;
}

extern "C" int mcrt_frame_noise(mcrt_ctx* ctx, uint64_t pixels, uint32_t spp, const double* rgb, const double* variance,
                                mcrt_frame_noise_result* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_frame_noise")) return rc;
    if (!rgb || !variance || !out) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise: the frame, the variance or the result is NULL");
    if (pixels == 0 || pixels >= kFrameNoiseMaxPixels) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise: pixels must be non-zero and below 2^38");
    FrameChannel ch[2] = {{rgb, nullptr, 24}, {variance, nullptr, 24}};
    StagedFrames frames{{ctx, "mcrt_frame_noise", kPassPixelStats, 0, kSlotEach, ch, 2}};
    if (int rc = frames.up(pixels)) return rc;
    return mcrt_frame_noise_device(ctx, pixels, spp, (double*)ch[0].dev, (double*)ch[1].dev, out);
}
