// Per-pixel sample statistics and the frame summary (include/mcrt.h mcrt_render_pixel_stats*, mcrt_frame_noise*), host side: the
// entry points, validation, the host-pointer forms and scratch. No kernel here: the two kernels are a code object of their own
// (libmcrt_pixel_stats.so, csrc/mcrt_pixel_stats.hip), so that the device code of libmcrt_hip.so stays what
// tests/golden/device_code_hashes.json lists. A render's statistics are launched by the pass loops of csrc/mcrt_hip.hip, which find
// their targets in the context: this file sets them for the length of a call (ctxPixelStatsBegin / End), so a frame that
// mcrt_render_finish renders again fills them again.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "mcrt_internal.hpp"
#include "mcrt_pixel_stats.hpp"
#include "mcrt_pixel_stats_launch.hpp"

using namespace mcrt;

namespace {

#define STATS_HIP_TRY(ctx, call)                                                                             \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return ctxFail(ctx, MCRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

}  // namespace

extern "C" int mcrt_render_pixel_stats_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_out_rgb,
                                              const mcrt_pixel_stats_buffers* d_buffers, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!d_out_rgb) return ctxFail(ctx, MCRT_ERR_INVALID, "d_out_rgb is NULL");
    if (int rc = ctxPixelStatsBegin(ctx, cam, d_buffers, "mcrt_render_pixel_stats_device")) return rc;
    int rc = mcrt_render_device(ctx, cam, global_seed, integrator, d_out_rgb, nullptr);
    if (rc == MCRT_OK) rc = mcrt_render_finish(ctx, stats);  // (renders again when it has to: the targets are still set)
    ctxPixelStatsEnd(ctx);
    return rc;
}

extern "C" int mcrt_render_pixel_stats(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* out_rgb,
                                       const mcrt_pixel_stats_buffers* buffers, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!out_rgb) return ctxFail(ctx, MCRT_ERR_INVALID, "out_rgb is NULL");
    if (int rc = ctxPixelStatsReady(ctx, "mcrt_render_pixel_stats")) return rc;
    if (!cam || cam->width == 0) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_render_pixel_stats: camera is NULL or has no columns");
    if (cam->shard_count > 1 && cam->shard_index >= cam->shard_count) return ctxFail(ctx, MCRT_ERR_INVALID, "shard_index >= shard_count");
    const uint32_t rows = mcrt_shard_rows(cam, nullptr);
    const size_t frame = (size_t)rows * cam->width * 3;  // doubles of the owned rows, packed
    double* host[4] = {out_rgb, buffers ? buffers->variance : nullptr, buffers ? buffers->half_a : nullptr, buffers ? buffers->half_b : nullptr};
    double* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; i++)
        if (host[i] && !(dev[i] = (double*)ctxPixelStatsScratch(ctx, i, frame * sizeof(double))))
            return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_render_pixel_stats: the frames' device copy could not be allocated");
    const mcrt_pixel_stats_buffers d{dev[1], dev[2], dev[3]};
    mcrt_stats st;
    if (int rc = mcrt_render_pixel_stats_device(ctx, cam, global_seed, integrator, dev[0], &d, &st)) return rc;
    if (rows) {
        std::vector<double> packed(frame);
        std::vector<uint32_t> idx(rows);
        mcrt_shard_rows(cam, idx.data());
        const size_t row_words = (size_t)cam->width * 3;
        for (int i = 0; i < 4; i++) {
            if (!host[i]) continue;
            STATS_HIP_TRY(ctx, hipMemcpy(packed.data(), dev[i], frame * sizeof(double), hipMemcpyDeviceToHost));
            for (uint32_t r = 0; r < rows; r++) memcpy(host[i] + (size_t)idx[r] * row_words, &packed[(size_t)r * row_words], row_words * sizeof(double));
        }
    }
    if (stats) *stats = st;
    return MCRT_OK;
}

extern "C" int mcrt_frame_noise_device(mcrt_ctx* ctx, uint64_t pixels, uint32_t spp, const double* d_rgb, const double* d_variance,
                                       mcrt_frame_noise_result* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxPixelStatsReady(ctx, "mcrt_frame_noise_device")) return rc;
    if (!d_rgb || !d_variance || !out) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise_device: the frame, the variance or the result is NULL");
    if (pixels == 0 || pixels >= kFrameNoiseMaxPixels) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise_device: pixels must be non-zero and below 2^38");
    if (spp == 0) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise_device: spp is 0");
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    // the block values of the levels, ping-ponged: [0] holds level 0's (and every second one's), [1] the others'; e first, then g
    const uint64_t blocks0 = frameNoiseBlocks(pixels);
    double* buf[2] = {(double*)ctxPixelStatsScratch(ctx, 4, blocks0 * 2 * sizeof(double)),
                      (double*)ctxPixelStatsScratch(ctx, 5, frameNoiseBlocks(blocks0) * 2 * sizeof(double))};
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
        STATS_HIP_TRY(ctx, (hipError_t)launchFrameNoiseLevel(stream, lv));
        if (blocks == 1) break;
        lv.rgb = lv.variance = nullptr;
        lv.in_e = lv.out_e;
        lv.in_g = lv.out_g;
        lv.n = blocks;
        which ^= 1;
    }
    double r[2];
    STATS_HIP_TRY(ctx, hipMemcpyAsync(r, buf[which], sizeof(r), hipMemcpyDeviceToHost, stream));
    STATS_HIP_TRY(ctx, hipStreamSynchronize(stream));
    out->noise = r[0];
    out->signal = r[1];
    out->relative_error = r[1] > 0.0 ? std::sqrt(r[0] / r[1]) : 0.0;
    out->pixels = pixels;
    return MCRT_OK;
}

extern "C" int mcrt_frame_noise(mcrt_ctx* ctx, uint64_t pixels, uint32_t spp, const double* rgb, const double* variance,
                                mcrt_frame_noise_result* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxPixelStatsReady(ctx, "mcrt_frame_noise")) return rc;
    if (!rgb || !variance || !out) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise: the frame, the variance or the result is NULL");
    if (pixels == 0 || pixels >= kFrameNoiseMaxPixels) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_frame_noise: pixels must be non-zero and below 2^38");
    double* d_rgb = (double*)ctxPixelStatsScratch(ctx, 0, pixels * 24);
    double* d_var = (double*)ctxPixelStatsScratch(ctx, 1, pixels * 24);
    if (!d_rgb || !d_var) return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_frame_noise: the frames' device copy could not be allocated");
    STATS_HIP_TRY(ctx, hipMemcpy(d_rgb, rgb, pixels * 24, hipMemcpyHostToDevice));
    STATS_HIP_TRY(ctx, hipMemcpy(d_var, variance, pixels * 24, hipMemcpyHostToDevice));
    return mcrt_frame_noise_device(ctx, pixels, spp, d_rgb, d_var, out);
}
