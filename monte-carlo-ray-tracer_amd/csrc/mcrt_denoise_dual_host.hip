// Dual-buffer denoised output (include/mcrt.h mcrt_denoise_dual*), host side: validation, defaults, scratch, the two launches,
// statistics and the host-pointer form. No kernel here: they are libmcrt_denoise_dual.so (csrc/mcrt_denoise_dual.hip; DESIGN.md "Image
// passes" says why, and what mcrt_pass_host.hpp shares).
// Scratch per pixel, kept in the context and grown on demand: 72 B of packed records {A, B, V0}; the host-pointer form stages the three
// input frames and the frame in another 96 B per pixel and filters the halves and the variance in place.
#include "mcrt_denoise_dual.hpp"
#include "mcrt_denoise_dual_launch.hpp"
#include "mcrt_pass_host.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* half_a, const double* half_b, const double* variance,
             const DenoiseDualSettings& s, const mcrt_denoise_dual_buffers* out, const char* what) {
    const std::string w(what);
    if ((uint64_t)width * height == 0 || (uint64_t)width * height > 0xFFFFFFFFull)
        return ctxFail(ctx, MCRT_ERR_INVALID, w + ": width * height must be non-zero and below 2^32");
    if (spp < 2) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": spp must be at least 2 (half_b of one sample is not a mean)");
    if (!half_a || !half_b) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": a half-buffer is NULL");
    if (!variance) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": the variance frame is NULL");
    if (!out || !out->rgb) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": the output buffers or their rgb frame are NULL");
    if (const char* why = denoiseDualSettingsError(s)) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": " + why);
    return MCRT_OK;
}

// Which form the filter runs: option MCRT_DENOISE_DUAL_FORM ("tile" / "plain") or, unset, the measured choice - the tile form, 4 - 11 times
// faster at 1080p (profiles/NOTES_denoise_dual.md). Both give the same bits.
// The tile form's workgroup: option MCRT_DENOISE_DUAL_LANES (256 / 512 / 1024 lanes on one tile) or, unset, denoiseDualTileLanes(R, F).
// -> the lanes, 0 for the plain form.
uint32_t tileLanes(const mcrt_ctx* ctx, const DenoiseDualSettings& s) {
    const char* form = ctxOpt(ctx, "MCRT_DENOISE_DUAL_FORM");
    if (form && !strcmp(form, "plain")) return 0;
    const long lanes = ctxOptL(ctx, "MCRT_DENOISE_DUAL_LANES", 0);
    return lanes == 256 || lanes == 512 || lanes == 1024 ? (uint32_t)lanes : denoiseDualTileLanes(s.window_radius, s.patch_radius);
}

}  // namespace

extern "C" int mcrt_denoise_dual_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* d_half_a, const double* d_half_b,
                                        const double* d_variance, const mcrt_denoise_dual_params* params, const mcrt_denoise_dual_buffers* d_out,
                                        mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_denoise_dual_device")) return rc;
    const DenoiseDualSettings s = denoiseDualSettings(params);
    if (int rc = validate(ctx, width, height, spp, d_half_a, d_half_b, d_variance, s, d_out, "mcrt_denoise_dual_device")) return rc;
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const size_t pixels = (size_t)width * height;

    DenoiseDualFrame f;
    f.width = width;
    f.height = height;
    f.half_a = d_half_a;
    f.half_b = d_half_b;
    f.variance = d_variance;
    f.rec = (double*)ctxPassScratch(ctx, kPassDenoiseDual, 0, pixels * kDenoiseDualRecWords * 8);
    if (!f.rec)
        return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_denoise_dual_device: " + std::to_string((pixels * 72) >> 20) + " MiB of scratch could not be allocated");
    DenoiseDualStep st;
    st.width = width;
    st.height = height;
    denoiseDualStepConstants(s, spp, st);
    st.rec = f.rec;
    st.out_rgb = d_out->rgb;
    st.out_variance = d_out->variance;
    st.out_half_a = d_out->half_a;
    st.out_half_b = d_out->half_b;

    if (int rc = timer.begin(stream)) return rc;
    MCRT_HIP_TRY(ctx, (hipError_t)launchDenoiseDualPrep(stream, f));
    MCRT_HIP_TRY(ctx, (hipError_t)launchDenoiseDualFilter(stream, st, tileLanes(ctx, s)));
    if (int rc = timer.end(stream)) return rc;
    return timer.finish(stats, 2);
}

extern "C" int mcrt_denoise_dual(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* half_a, const double* half_b,
                                 const double* variance, const mcrt_denoise_dual_params* params, const mcrt_denoise_dual_buffers* out, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_denoise_dual")) return rc;
    const DenoiseDualSettings s = denoiseDualSettings(params);
    if (int rc = validate(ctx, width, height, spp, half_a, half_b, variance, s, out, "mcrt_denoise_dual")) return rc;
    PassTimer whole(ctx);
    const size_t pixels = (size_t)width * height;
    // the three input frames (the halves and the variance filtered in place) and the frame as one device allocation of 96 B per pixel
    FrameChannel ch[4] = {{half_a, out->half_a, 24}, {half_b, out->half_b, 24}, {variance, out->variance, 24}, {nullptr, out->rgb, 24}};
    StagedFrames frames{{ctx, "mcrt_denoise_dual", kPassDenoiseDual, 1, kPackedAll, ch, 4}};
    if (int rc = frames.up(pixels)) return rc;
    mcrt_denoise_dual_buffers d{};
    d.rgb = (double*)ch[3].dev;
    d.variance = out->variance ? (double*)ch[2].dev : nullptr;
    d.half_a = out->half_a ? (double*)ch[0].dev : nullptr;
    d.half_b = out->half_b ? (double*)ch[1].dev : nullptr;
    mcrt_stats st;
    if (int rc = mcrt_denoise_dual_device(ctx, width, height, spp, (double*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev, params, &d, &st)) return rc;
    if (int rc = frames.down(pixels)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
