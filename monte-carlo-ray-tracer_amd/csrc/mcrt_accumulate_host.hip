// Accumulated rendering (include/mcrt.h mcrt_frame_merge*, mcrt_render_converged*), host side: the entry points, validation, defaults,
// the host-pointer forms, scratch and the stopping loop. No kernel here: the merge is libmcrt_accumulate.so (csrc/mcrt_accumulate.hip;
// DESIGN.md "Image passes" says why, and what mcrt_pass_host.hpp shares). The loop is built from the library's own calls - a batch is a
// mcrt_render_highlights_device or mcrt_render_pixel_stats_device, the summary a mcrt_frame_noise_device - so no render kernel knows of it.
// Everything here works on mcrt_frame_summary, by the channel table and the conversions of mcrt_summary_channels.hpp.
// Scratch slots of the family: 0 the host form of the merge, 1 the accumulators and the batch, 2 the host form of the converged render.
#include <cmath>

#include "mcrt_accumulate.hpp"
#include "mcrt_accumulate_launch.hpp"
#include "mcrt_pass_host.hpp"
#include "mcrt_summary_channels.hpp"

using namespace mcrt;

namespace {

int mergeCheck(mcrt_ctx* ctx, const char* what, uint64_t pixels, const mcrt_frame_summary* a, uint32_t n_a, const mcrt_frame_summary* b,
               uint32_t n_b, const mcrt_frame_summary* out) {
    const char* why = nullptr;
    if (int rc = frameMergeCheck(pixels, a, n_a, b, n_b, out, &why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);
    return MCRT_OK;
}

struct ConvergeSettings {
    double target;
    uint32_t max_spp, min_batches;
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

}  // namespace

extern "C" int mcrt_frame_merge_device(mcrt_ctx* ctx, uint64_t pixels, const mcrt_frame_summary* d_a, uint32_t n_a, const mcrt_frame_summary* d_b,
                                       uint32_t n_b, const mcrt_frame_summary* d_out, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_frame_merge_device")) return rc;
    if (int rc = mergeCheck(ctx, "mcrt_frame_merge_device", pixels, d_a, n_a, d_b, n_b, d_out)) return rc;
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    FrameMerge fm;
    fm.a = *d_a;
    fm.b = *d_b;
    fm.out = *d_out;
    fm.pixels = pixels;
    fm.n_a = n_a;
    fm.n_b = n_b;
    if (int rc = timer.begin(stream)) return rc;
    MCRT_HIP_TRY(ctx, (hipError_t)launchFrameMerge(stream, fm));
    if (int rc = timer.end(stream)) return rc;
    return timer.finish(stats, 1);
}

extern "C" int mcrt_frame_merge(mcrt_ctx* ctx, uint64_t pixels, const mcrt_frame_summary* a, uint32_t n_a, const mcrt_frame_summary* b, uint32_t n_b,
                                const mcrt_frame_summary* out, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_frame_merge")) return rc;
    if (int rc = mergeCheck(ctx, "mcrt_frame_merge", pixels, a, n_a, b, n_b, out)) return rc;
    PassTimer whole(ctx);
    // A's device copies are merged into in place and come back as the outputs; only the channels of wanted groups travel
    FrameChannel ch[2 * kSummaryChannels];
    for (int i = 0; i < kSummaryChannels; i++) {
        double* po = summaryChannel(*out, i);
        ch[i] = FrameChannel{po ? summaryChannel(*a, i) : nullptr, po, kSummaryChannel[i].pixel_bytes};
        ch[kSummaryChannels + i] = FrameChannel{po ? summaryChannel(*b, i) : nullptr, nullptr, kSummaryChannel[i].pixel_bytes};
    }
    StagedFrames frames{{ctx, "mcrt_frame_merge", kPassAccumulate, 0, kPackedWanted, ch, 2 * kSummaryChannels}};
    if (int rc = frames.up((size_t)pixels)) return rc;
    const mcrt_frame_summary d_a = summaryOfDevice(ch), d_b = summaryOfDevice(ch + kSummaryChannels);
    mcrt_stats st;
    if (int rc = mcrt_frame_merge_device(ctx, pixels, &d_a, n_a, &d_b, n_b, &d_a, &st)) return rc;
    if (int rc = frames.down((size_t)pixels)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}

extern "C" int mcrt_render_converged_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                                            const mcrt_converge_params* params, double* d_out_rgb, const mcrt_pixel_stats_buffers* d_stats_buffers,
                                            const mcrt_highlight_buffers* d_highlights, mcrt_converge_result* result, mcrt_stats* stats) {
    const char* what = "mcrt_render_converged_device";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (!cam) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": camera is NULL");
    if (!d_out_rgb) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": d_out_rgb is NULL");
    if (int rc = ctxNeedScene(ctx, what)) return rc;
    const uint64_t pixels = (uint64_t)cam->width * cam->height;
    if (pixels == 0 || pixels > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": width * height must be non-zero and below 2^32");
    const uint64_t batch64 = (uint64_t)cam->sqrtspp * cam->sqrtspp;
    if (batch64 == 0 || batch64 > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": sqrtspp must be 1 .. 65535");
    const uint32_t batch = (uint32_t)batch64;
    if (cam->shard_count > 1)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": a sharded camera - the summary needs the whole frame: merge per shard with mcrt_frame_merge_device");
    ConvergeSettings s{0.0, batch > 1024u ? batch : 1024u, cam->sqrtspp == 1 ? 2u : 1u};
    if (params) {
        if (params->target_relative_error != 0.0) s.target = params->target_relative_error;
        if (params->max_spp != 0) s.max_spp = params->max_spp;
        if (params->min_batches != 0) s.min_batches = params->min_batches;
    }
    if (!std::isfinite(s.target) || s.target < 0.0) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": target_relative_error must be finite and not negative");
    if (s.max_spp < batch) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": max_spp is less than one batch");
    if (cam->sqrtspp == 1 && s.min_batches < 2) s.min_batches = 2;  // a 1-sample batch has variance 0
    const mcrt_frame_summary dst = summaryOf(d_out_rgb, d_stats_buffers, d_highlights);
    const bool want_halves = dst.half_a || dst.half_b, want_tops = summaryWantsHighlights(dst);
    if (want_tops && batch < kFrameMergeTopsMin)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": highlights need 16 samples per batch");

    PassTimer whole(ctx);
    // the accumulators [0 .. 5] and the batch [6 .. 11], whole groups, in one allocation
    const bool want[kSummaryChannels] = {true, true, want_halves, want_halves, want_tops, want_tops};
    size_t at[2 * kSummaryChannels], total = 0;
    for (int i = 0; i < 2 * kSummaryChannels; i++) {
        at[i] = total;
        if (want[i % kSummaryChannels]) total += (size_t)pixels * kSummaryChannel[i % kSummaryChannels].pixel_bytes;
    }
    unsigned char* base = (unsigned char*)ctxPassScratch(ctx, kPassAccumulate, 1, total);
    if (!base) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the accumulators could not be allocated");
    mcrt_frame_summary acc{}, bat{};
    for (int i = 0; i < kSummaryChannels; i++)
        if (want[i]) summaryChannel(acc, i) = (double*)(base + at[i]), summaryChannel(bat, i) = (double*)(base + at[kSummaryChannels + i]);

    mcrt_converge_result res{};
    mcrt_stats sum{};
    uint32_t spp = 0;
    for (uint32_t j = 0;; j++) {
        const mcrt_frame_summary& to = j == 0 ? acc : bat;  // (batch 0 is the accumulators' first content)
        const mcrt_pixel_stats_buffers ds = summaryStats(to);
        const mcrt_highlight_buffers dh = summaryHighlights(to);
        mcrt_stats st;
        const int rc = want_tops ? mcrt_render_highlights_device(ctx, cam, global_seed + j, integrator, to.rgb, &dh, &ds, &st)
                                 : mcrt_render_pixel_stats_device(ctx, cam, global_seed + j, integrator, to.rgb, &ds, &st);
        if (rc) return rc;
        addStats(sum, st);
        sum.kernel_id = st.kernel_id;
        if (j > 0) {
            if (int rc2 = mcrt_frame_merge_device(ctx, pixels, &acc, spp, &bat, batch, &acc, nullptr)) return rc2;
            sum.kernel_launches += 1;
        }
        spp += batch;
        if (int rc2 = mcrt_frame_noise_device(ctx, pixels, spp, acc.rgb, acc.variance, &res.final)) return rc2;
        res.batches = j + 1;
        res.spp = spp;
        if (j < MCRT_CONVERGE_TRACE) res.relative_error[j] = res.final.relative_error;
        if (res.batches >= s.min_batches && res.final.relative_error <= s.target) break;
        if ((uint64_t)spp + batch > s.max_spp) break;
    }

    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    for (int i = 0; i < kSummaryChannels; i++)
        if (summaryChannel(dst, i))
            MCRT_HIP_TRY(ctx, hipMemcpyAsync(summaryChannel(dst, i), summaryChannel(acc, i), (size_t)pixels * kSummaryChannel[i].pixel_bytes, hipMemcpyDeviceToDevice, stream));
    MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
    sum.total_ms = whole.hostMs();
    if (result) *result = res;
    if (stats) *stats = sum;
    return MCRT_OK;
}

extern "C" int mcrt_render_converged(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                                     const mcrt_converge_params* params, double* out_rgb, const mcrt_pixel_stats_buffers* stats_buffers,
                                     const mcrt_highlight_buffers* highlights, mcrt_converge_result* result, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_render_converged")) return rc;
    if (!cam) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_render_converged: camera is NULL");
    if (!out_rgb) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_render_converged: out_rgb is NULL");
    PassTimer whole(ctx);
    FrameChannel ch[kSummaryChannels];
    summaryFrameChannels(summaryOf(out_rgb, stats_buffers, highlights), ch);
    const size_t pixels = (size_t)cam->width * cam->height;
    if (pixels == 0 || pixels > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_render_converged: width * height must be non-zero and below 2^32");
    StagedFrames frames{{ctx, "mcrt_render_converged", kPassAccumulate, 2, kPackedWanted, ch, kSummaryChannels}};
    if (int rc = frames.place(pixels)) return rc;
    const mcrt_frame_summary d = summaryOfDevice(ch);
    const mcrt_pixel_stats_buffers ds = summaryStats(d);
    const mcrt_highlight_buffers dh = summaryHighlights(d);
    mcrt_stats st;
    if (int rc = mcrt_render_converged_device(ctx, cam, global_seed, integrator, params, d.rgb, &ds, &dh, result, &st)) return rc;
    if (int rc = frames.down(pixels)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
