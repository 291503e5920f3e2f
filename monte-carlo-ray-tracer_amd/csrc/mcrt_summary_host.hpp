// A render that also delivers channels of its per-sample summary (mcrt_summary_channels.hpp): the one device form and the one host-pointer
// form behind mcrt_render_pixel_stats[_device] and mcrt_render_highlights[_device], which differ in the name that the messages carry
// (`what`), in the channels they can ask for and in the scratch family of their host form.
#pragma once

#include "mcrt_pass_host.hpp"
#include "mcrt_summary_channels.hpp"

namespace mcrt {

// d.rgb: the frame; the other channels of d that are not NULL are the sample targets of this render (ctxSampleTargetsBegin).
inline int renderSummaryDevice(mcrt_ctx* ctx, const char* what, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                               const mcrt_frame_summary& d, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!d.rgb) return ctxFail(ctx, MCRT_ERR_INVALID, "d_out_rgb is NULL");
    if (int rc = ctxSampleTargetsBegin(ctx, cam, &d, what)) return rc;
    SampleTargetsScope targets{ctx};
    if (int rc = mcrt_render_device(ctx, cam, global_seed, integrator, d.rgb, nullptr)) return rc;
    return mcrt_render_finish(ctx, stats);  // (renders again when it has to: the targets are still set)
}

// host: FULL frames, of which the rows of cam's shard are written. The render is `what`_device's, under that name.
inline int renderSummaryHost(mcrt_ctx* ctx, const char* what, PassFamily family, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                             const mcrt_frame_summary& host, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!host.rgb) return ctxFail(ctx, MCRT_ERR_INVALID, "out_rgb is NULL");
    if (int rc = ctxIdle(ctx, what)) return rc;
    FrameChannel ch[kSummaryChannels];
    summaryFrameChannels(host, ch);
    ShardFrames frames{{ctx, what, family, 0, kSlotEach, ch, kSummaryChannels}};
    if (int rc = frames.place(cam)) return rc;
    mcrt_stats st;
    if (int rc = renderSummaryDevice(ctx, (std::string(what) + "_device").c_str(), cam, global_seed, integrator, summaryOfDevice(ch), &st)) return rc;
    if (int rc = frames.down(cam)) return rc;
    if (stats) *stats = st;
    return MCRT_OK;
}

}  // namespace mcrt
