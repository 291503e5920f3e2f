// The guide channels that both a-trous filters (mcrt_denoise_host.hip, mcrt_denoise_var_host.hip) read from a first-hit AOV frame: one
// table for the check of a call's guides and for the host-pointer forms' device copies.
#pragma once

#include "mcrt_pass_host.hpp"

namespace mcrt {

struct DenoiseGuide {
    double* mcrt_aov_buffers::*field;
    const char* name;
    size_t pixel_bytes;
    bool optional;  // not read with MCRT_DENOISE_NO_ALBEDO
};
// In the order the host-pointer forms stage them.
constexpr int kDenoiseGuides = 5;
const DenoiseGuide kDenoiseGuide[kDenoiseGuides] = {{&mcrt_aov_buffers::shading_normal, "shading_normal", 24, false},
                                                    {&mcrt_aov_buffers::normal, "normal", 24, false},
                                                    {&mcrt_aov_buffers::position, "position", 24, false},
                                                    {&mcrt_aov_buffers::albedo, "albedo", 24, true},
                                                    {&mcrt_aov_buffers::coverage, "coverage", 8, false}};

// Refuses guides that miss a channel the call reads: the channels every call reads first, then the optional one. what: the call's name.
inline int denoiseCheckGuides(mcrt_ctx* ctx, const std::string& what, const mcrt_aov_buffers* guides, bool with_albedo) {
    if (!guides) return ctxFail(ctx, MCRT_ERR_INVALID, what + ": guides is NULL");
    for (const bool optional : {false, true})
        for (const DenoiseGuide& g : kDenoiseGuide)
            if (g.optional == optional && (with_albedo || !optional) && !(guides->*g.field))
                return ctxFail(ctx, MCRT_ERR_INVALID, what + ": guide channel " + g.name + " is NULL");
    return MCRT_OK;
}

// The guides' host frames as the kDenoiseGuides entries ch[0 ..] of a host-pointer form's table (inputs only), and the guides of the
// _device call from those entries once they are placed.
inline void denoiseGuideChannels(const mcrt_aov_buffers& guides, bool with_albedo, FrameChannel* ch) {
    for (const DenoiseGuide& g : kDenoiseGuide) *ch++ = FrameChannel{g.optional && !with_albedo ? nullptr : guides.*g.field, nullptr, g.pixel_bytes};
}
inline mcrt_aov_buffers denoiseDeviceGuides(const FrameChannel* ch) {
    mcrt_aov_buffers d{};
    for (const DenoiseGuide& g : kDenoiseGuide) d.*g.field = (double*)(ch++)->dev;
    return d;
}

}  // namespace mcrt
