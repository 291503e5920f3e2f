// Variance-guided denoised output (include/mcrt.h mcrt_denoise_variance*), host side: validation, defaults, scratch, the iteration loop,
// statistics and the host-pointer form. No kernel here: they are libmcrt_denoise_var.so (csrc/mcrt_denoise_var.hip; DESIGN.md "Image
// passes" says why, and what mcrt_pass_host.hpp shares).
// Scratch per pixel, kept in the context and grown on demand: 80 B of packed guides + 2 x 48 B of {irradiance, variance} = 176 B; the
// host-pointer form stages its seven input frames in another 152 B per pixel and filters the beauty and the variance frame in place.
#include "mcrt_denoise_var.hpp"
#include "mcrt_denoise_var_launch.hpp"
#include "mcrt_denoise_guides.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* rgb, const double* variance, const mcrt_aov_buffers* guides,
             const DenoiseVarSettings& s, const double* out, const char* what) {
    const std::string w(what);
    if ((uint64_t)width * height == 0 || (uint64_t)width * height > 0xFFFFFFFFull)
        return ctxFail(ctx, MCRT_ERR_INVALID, w + ": width * height must be non-zero and below 2^32");
    if (spp == 0) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": spp must not be 0");
    if (!rgb || !out) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": the beauty frame or the output frame is NULL");
    if (!variance) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": the variance frame is NULL");
    if (int rc = denoiseCheckGuides(ctx, w, guides, !(s.flags & MCRT_DENOISE_NO_ALBEDO))) return rc;
    if (const char* why = denoiseVarSettingsError(s)) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": " + why);
    return MCRT_OK;
}

// Which form an iteration of step s runs: option MCRT_DENOISE_VAR_FORM ("tile" / "plain") or, unset, the measured choice - the tile form
// at every step: at 1080p it takes 0.22 - 0.27 ms an iteration at steps 2 .. 16 where the plain form takes 0.38 - 0.59 ms
// (profiles/NOTES_denoise_variance.md). Both give the same bits.
bool tileForm(const mcrt_ctx* ctx, uint32_t step) {
    (void)step;  // (no step at which the plain form won)
    const char* form = ctxOpt(ctx, "MCRT_DENOISE_VAR_FORM");
    return !(form && !strcmp(form, "plain"));
}

}  // namespace

extern "C" int mcrt_denoise_variance_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* d_rgb, const double* d_variance,
                                            const mcrt_aov_buffers* guides, const mcrt_denoise_variance_params* params, double* d_out_rgb,
                                            double* d_out_variance, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_denoise_variance_device")) return rc;
    const DenoiseVarSettings s = denoiseVarSettings(params);
    if (int rc = validate(ctx, width, height, spp, d_rgb, d_variance, guides, s, d_out_rgb, "mcrt_denoise_variance_device")) return rc;
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const size_t pixels = (size_t)width * height;
    const bool with_albedo = !(s.flags & MCRT_DENOISE_NO_ALBEDO);

    DenoiseVarFrame f;
    f.width = width;
    f.height = height;
    f.spp = (double)spp;
    f.rgb = d_rgb;
    f.variance = d_variance;
    f.shading_normal = guides->shading_normal;
    f.normal = guides->normal;
    f.position = guides->position;
    f.coverage = guides->coverage;
    f.albedo = with_albedo ? guides->albedo : nullptr;
    f.albedo_floor = s.albedo_floor;
    f.guide = (double*)ctxPassScratch(ctx, kPassDenoiseVar, 0, pixels * kDenoiseGuideWords * 8);
    f.iv = (double*)ctxPassScratch(ctx, kPassDenoiseVar, 1, pixels * kDenoiseVarIvWords * 8);
    double* other = (double*)ctxPassScratch(ctx, kPassDenoiseVar, 2, pixels * kDenoiseVarIvWords * 8);
    if (!f.guide || !f.iv || !other)
        return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_denoise_variance_device: " + std::to_string((pixels * 176) >> 20) + " MiB of scratch could not be allocated");

    if (int rc = timer.begin(stream)) return rc;
    MCRT_HIP_TRY(ctx, (hipError_t)launchDenoiseVarPrep(stream, f));
    DenoiseVarStep st;
    st.width = width;
    st.height = height;
    st.guide = f.guide;
    denoiseVarStepConstants(s, spp, st);
    const double* in = f.iv;
    for (uint32_t i = 0; i < s.iterations; i++) {
        const bool last = i + 1 == s.iterations;
        st.step = 1u << i;
        st.in = in;
        st.out = last ? nullptr : (in == f.iv ? other : f.iv);
        st.out_rgb = last ? d_out_rgb : nullptr;
        st.out_variance = last ? d_out_variance : nullptr;
        st.albedo = last ? f.albedo : nullptr;
        MCRT_HIP_TRY(ctx, (hipError_t)launchDenoiseVarStep(stream, st, tileForm(ctx, st.step)));
        in = st.out;
    }
    if (int rc = timer.end(stream)) return rc;
    return timer.finish(stats, 1 + s.iterations);
}

extern "C" int mcrt_denoise_variance(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* rgb, const double* variance,
                                     const mcrt_aov_buffers* guides, const mcrt_denoise_variance_params* params, double* out_rgb, double* out_variance,
                                     mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_denoise_variance")) return rc;
    const DenoiseVarSettings s = denoiseVarSettings(params);
    if (int rc = validate(ctx, width, height, spp, rgb, variance, guides, s, out_rgb, "mcrt_denoise_variance")) return rc;
    PassTimer whole(ctx);
    const size_t pixels = (size_t)width * height;
    // the seven input frames as one device allocation of 152 B per pixel: beauty and variance (both filtered in place), Ns, N, P, albedo,
    // coverage
    const bool with_albedo = !(s.flags & MCRT_DENOISE_NO_ALBEDO);
    FrameChannel ch[2 + kDenoiseGuides] = {{rgb, out_rgb, 24}, {variance, out_variance, 24}};
    denoiseGuideChannels(*guides, with_albedo, ch + 2);
    StagedFrames frames{{ctx, "mcrt_denoise_variance", kPassDenoiseVar, 3, kPackedAll, ch, 2 + kDenoiseGuides}};
    if (int rc = frames.up(pixels)) return rc;
    const mcrt_aov_buffers d = denoiseDeviceGuides(ch + 2);
    mcrt_stats st;
    if (int rc = mcrt_denoise_variance_device(ctx, width, height, spp, (double*)ch[0].dev, (double*)ch[1].dev, &d, params, (double*)ch[0].dev,
                                              out_variance ? (double*)ch[1].dev : nullptr, &st))
        return rc;
    if (int rc = frames.down(pixels)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
