// Denoised output (include/mcrt.h mcrt_denoise*), host side: validation, defaults, scratch, the iteration loop, statistics and the
// host-pointer form. No kernel here: the filter's three kernels are a code object of their own (libmcrt_denoise.so,
// csrc/mcrt_denoise.hip), so that the device code of libmcrt_hip.so stays what tests/golden/device_code_hashes.json lists.
// Scratch per pixel, kept in the context and grown on demand: 80 B of packed guides + 2 x 24 B of irradiance = 128 B; the host-pointer
// form stages its six input frames in another 128 B per pixel and filters the beauty frame in place.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>

#include "mcrt_denoise.hpp"
#include "mcrt_denoise_launch.hpp"
#include "mcrt_internal.hpp"

using namespace mcrt;

namespace {

#define DENOISE_HIP_TRY(ctx, call)                                                                           \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return ctxFail(ctx, MCRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Events {  // the pass's own pair: the context's belong to renders and to the operators' timing option
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

int validate(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* rgb, const mcrt_aov_buffers* guides, const DenoiseSettings& s,
             const double* out, const char* what) {
    const std::string w(what);
    if ((uint64_t)width * height == 0 || (uint64_t)width * height > 0xFFFFFFFFull)
        return ctxFail(ctx, MCRT_ERR_INVALID, w + ": width * height must be non-zero and below 2^32");
    if (!rgb || !out) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": the beauty frame or the output frame is NULL");
    if (!guides) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": guides is NULL");
    const struct {
        const double* p;
        const char* name;
        bool needed;
    } ch[5] = {{guides->shading_normal, "shading_normal", true},
               {guides->normal, "normal", true},
               {guides->position, "position", true},
               {guides->coverage, "coverage", true},
               {guides->albedo, "albedo", !(s.flags & MCRT_DENOISE_NO_ALBEDO)}};
    for (const auto& c : ch)
        if (c.needed && !c.p) return ctxFail(ctx, MCRT_ERR_INVALID, w + ": guide channel " + c.name + " is NULL");
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
    if (int rc = ctxDenoiseReady(ctx, "mcrt_denoise_device")) return rc;
    const DenoiseSettings s = denoiseSettings(params);
    if (int rc = validate(ctx, width, height, d_rgb, guides, s, d_out_rgb, "mcrt_denoise_device")) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
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
    f.guide = (double*)ctxDenoiseScratch(ctx, 0, pixels * kDenoiseGuideWords * 8);
    f.irr = (double*)ctxDenoiseScratch(ctx, 1, pixels * 24);
    double* other = (double*)ctxDenoiseScratch(ctx, 2, pixels * 24);
    if (!f.guide || !f.irr || !other)
        return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_denoise_device: " + std::to_string((pixels * 128) >> 20) + " MiB of scratch could not be allocated");

    Events ev;
    DENOISE_HIP_TRY(ctx, hipEventCreate(&ev.e0));
    DENOISE_HIP_TRY(ctx, hipEventCreate(&ev.e1));
    DENOISE_HIP_TRY(ctx, hipEventRecord(ev.e0, stream));
    DENOISE_HIP_TRY(ctx, (hipError_t)launchDenoisePrep(stream, f));
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
        DENOISE_HIP_TRY(ctx, (hipError_t)launchDenoiseStep(stream, st, tile));
        in = st.out;
    }
    DENOISE_HIP_TRY(ctx, hipEventRecord(ev.e1, stream));
    DENOISE_HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (stats) {
        float ms = 0.f;
        DENOISE_HIP_TRY(ctx, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        memset(stats, 0, sizeof(*stats));
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        stats->kernel_launches = 1 + s.iterations;
        stats->kernel_id = MCRT_KERNEL_NONE;  // (names the integrator's kernel form: none ran)
    }
    return MCRT_OK;
}

extern "C" int mcrt_denoise(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* rgb, const mcrt_aov_buffers* guides,
                            const mcrt_denoise_params* params, double* out_rgb, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxDenoiseReady(ctx, "mcrt_denoise")) return rc;
    const DenoiseSettings s = denoiseSettings(params);
    if (int rc = validate(ctx, width, height, rgb, guides, s, out_rgb, "mcrt_denoise")) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    const size_t pixels = (size_t)width * height;
    // the six input frames as one device allocation, in units of 8 bytes per pixel: beauty (filtered in place), Ns, N, P, albedo, coverage
    double* base = (double*)ctxDenoiseScratch(ctx, 3, pixels * 128);
    if (!base) return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_denoise: the frames' device copy could not be allocated");
    mcrt_aov_buffers d{};
    d.shading_normal = base + pixels * 3;
    d.normal = base + pixels * 6;
    d.position = base + pixels * 9;
    d.albedo = (s.flags & MCRT_DENOISE_NO_ALBEDO) ? nullptr : base + pixels * 12;
    d.coverage = base + pixels * 15;
    DENOISE_HIP_TRY(ctx, hipMemcpy(base, rgb, pixels * 24, hipMemcpyHostToDevice));
    DENOISE_HIP_TRY(ctx, hipMemcpy(d.shading_normal, guides->shading_normal, pixels * 24, hipMemcpyHostToDevice));
    DENOISE_HIP_TRY(ctx, hipMemcpy(d.normal, guides->normal, pixels * 24, hipMemcpyHostToDevice));
    DENOISE_HIP_TRY(ctx, hipMemcpy(d.position, guides->position, pixels * 24, hipMemcpyHostToDevice));
    if (d.albedo) DENOISE_HIP_TRY(ctx, hipMemcpy(d.albedo, guides->albedo, pixels * 24, hipMemcpyHostToDevice));
    DENOISE_HIP_TRY(ctx, hipMemcpy(d.coverage, guides->coverage, pixels * 8, hipMemcpyHostToDevice));
    mcrt_stats st;
    if (int rc = mcrt_denoise_device(ctx, width, height, base, &d, params, base, &st)) return rc;
    DENOISE_HIP_TRY(ctx, hipMemcpy(out_rgb, base, pixels * 24, hipMemcpyDeviceToHost));
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = st;
    return MCRT_OK;
}
