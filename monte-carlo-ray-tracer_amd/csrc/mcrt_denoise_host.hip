// Denoised output (include/mcrt.h mcrt_denoise*), host side: validation, defaults, scratch, the iteration loop, statistics and the
// host-pointer form. No kernel here: they are libmcrt_denoise.so (csrc/mcrt_denoise.hip; DESIGN.md "Image passes" says why, and what
// mcrt_pass_host.hpp shares).
// Scratch per pixel, kept in the context and grown on demand: 80 B of packed guides + 2 x 24 B of irradiance = 128 B; the host-pointer
// form stages its six input frames in another 128 B per pixel and filters the beauty frame in place.
#include "mcrt_denoise.hpp"
#include "mcrt_denoise_launch.hpp"
#include "mcrt_denoise_guides.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* rgb, const mcrt_aov_buffers* guides, const DenoiseSettings& s,
             const double* out, const char* what) {
    const std::string w(what);
    if ((uint64_t)width * height == 0 || (uint64_t)width * height > 0xFFFFFFFFull)
        return ctxFail(ctx, MCRT_ERR_INVALID, w + ": width * height must be non-zero and below 2^32");
    if (!rgb || !out) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": the beauty frame or the output frame is NULL");
    if (int rc = denoiseCheckGuides(ctx, w, guides, !(s.flags & MCRT_DENOISE_NO_ALBEDO))) return rc;
    if (s.iterations > kDenoiseMaxIterations)
        return ctxFail(ctx, MCRT_ERR_INVALID, w + ": " + std::to_string(s.iterations) + " iterations, at most " + std::to_string(kDenoiseMaxIterations));
    if (s.normal_power_log2 > kDenoiseMaxNormalPowerLog2)
        return ctxFail(ctx, MCRT_ERR_INVALID, w + ": normal_power_log2 " + std::to_string(s.normal_power_log2) + ", at most " + std::to_string(kDenoiseMaxNormalPowerLog2));
    return MCRT_OK;
}

// Which form the iterations run: option MCRT_DENOISE_FORM ("tile" / "plain") or, unset, the measured choice - the tile form at every
// step: at 1080p it takes 0.19 - 0.23 ms an iteration at steps 1 .. 16 where the plain form takes 0.31 - 0.47 ms
// (profiles/NOTES_denoise.md). Both give the same bits.
bool tileForm(const mcrt_ctx* ctx) {
    const char* form = ctxOpt(ctx, "MCRT_DENOISE_FORM");
    return !(form && !strcmp(form, "plain"));
}

}  // namespace

extern "C" int mcrt_denoise_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* d_rgb, const mcrt_aov_buffers* guides,
                                   const mcrt_denoise_params* params, double* d_out_rgb, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_denoise_device")) return rc;
    const DenoiseSettings s = denoiseSettings(params);
    if (int rc = validate(ctx, width, height, d_rgb, guides, s, d_out_rgb, "mcrt_denoise_device")) return rc;
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const size_t pixels = (size_t)width * height;
    const bool with_albedo = !(s.flags & MCRT_DENOISE_NO_ALBEDO);

    DenoiseFrame f;
    f.width = width;
    f.height = height;
    f.rgb = d_rgb;
    f.shading_normal = guides->shading_normal;
    f.normal = guides->normal;
    f.position = guides->position;
    f.coverage = guides->coverage;
    f.albedo = with_albedo ? guides->albedo : nullptr;
    f.albedo_floor = s.albedo_floor;
    f.guide = (double*)ctxPassScratch(ctx, kPassDenoise, 0, pixels * kDenoiseGuideWords * 8);
    f.irr = (double*)ctxPassScratch(ctx, kPassDenoise, 1, pixels * 24);
    double* other = (double*)ctxPassScratch(ctx, kPassDenoise, 2, pixels * 24);
    if (!f.guide || !f.irr || !other)
        return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_denoise_device: " + std::to_string((pixels * 128) >> 20) + " MiB of scratch could not be allocated");

    if (int rc = timer.begin(stream)) return rc;
    MCRT_HIP_TRY(ctx, (hipError_t)launchDenoisePrep(stream, f));
    DenoiseStep st;
    st.width = width;
    st.height = height;
    st.guide = f.guide;
    const double* in = f.irr;
    const bool tile = tileForm(ctx);
    for (uint32_t i = 0; i < s.iterations; i++) {
        const bool last = i + 1 == s.iterations;
        denoiseStepConstants(s, i, st);
        st.in = in;
        st.out = last ? d_out_rgb : (in == f.irr ? other : f.irr);
        st.albedo = last ? f.albedo : nullptr;
        MCRT_HIP_TRY(ctx, (hipError_t)launchDenoiseStep(stream, st, tile));
        in = st.out;
    }
    if (int rc = timer.end(stream)) return rc;
    return timer.finish(stats, 1 + s.iterations);
}

extern "C" int mcrt_denoise(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* rgb, const mcrt_aov_buffers* guides,
                            const mcrt_denoise_params* params, double* out_rgb, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, "mcrt_denoise")) return rc;
    const DenoiseSettings s = denoiseSettings(params);
    if (int rc = validate(ctx, width, height, rgb, guides, s, out_rgb, "mcrt_denoise")) return rc;
    PassTimer whole(ctx);
    const size_t pixels = (size_t)width * height;
    // the six input frames as one device allocation of 128 B per pixel: beauty (filtered in place), Ns, N, P, albedo, coverage
    const bool with_albedo = !(s.flags & MCRT_DENOISE_NO_ALBEDO);
    FrameChannel ch[1 + kDenoiseGuides] = {{rgb, out_rgb, 24}};
    denoiseGuideChannels(*guides, with_albedo, ch + 1);
    StagedFrames frames{{ctx, "mcrt_denoise", kPassDenoise, 3, kPackedAll, ch, 1 + kDenoiseGuides}};
    if (int rc = frames.up(pixels)) return rc;
    const mcrt_aov_buffers d = denoiseDeviceGuides(ch + 1);
    mcrt_stats st;
    if (int rc = mcrt_denoise_device(ctx, width, height, (double*)ch[0].dev, &d, params, (double*)ch[0].dev, &st)) return rc;
    if (int rc = frames.down(pixels)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
