// Ray sources (include/mcrt.h mcrt_set_ray_source, mcrt_set_ray_source_host, mcrt_get_ray_source), host side: the descriptor into and
// out of the context. No kernel here: the sources are branches of aovRayKernel (csrc/mcrt_aov.hip, libmcrt_aov.so; launchSourceRays).
// The passes take a source through the chunk loop (mcrt_camera_pass.hpp SourcePixels), mcrt_camera_rays* in mcrt_lens_host.hip; the
// render calls' guard is where the lens has its own (mcrt_hip.hip launchRender, mcrt_adaptive_host.hip).
#include "mcrt_camera_pass.hpp"

using namespace mcrt;

namespace {

// What both forms refuse before they look at the arrays: the status, and the settings.
int validate(mcrt_ctx* ctx, const mcrt_ray_source_desc* source, RaySource& s, const char* what) {
    if (ctxLens(ctx))
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": a lens is set (mcrt_set_lens) - a lens and a ray source exclude each other; mcrt_set_lens(ctx, NULL) takes it off");
    const char* why = nullptr;
    if (int rc = raySourceSettings(*source, s, &why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);
    return MCRT_OK;
}

}  // namespace

extern "C" int mcrt_set_ray_source(mcrt_ctx* ctx, const mcrt_ray_source_desc* source) {
    const char* what = "mcrt_set_ray_source";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (!source || source->kind == MCRT_RAY_SOURCE_NONE) {
        ctxSetRaySource(ctx, mcrt_ray_source_desc{}, nullptr, nullptr);
        return MCRT_OK;
    }
    RaySource s;
    if (int rc = validate(ctx, source, s, what)) return rc;
    ctxSetRaySource(ctx, *source, nullptr, nullptr);
    return MCRT_OK;
}

extern "C" int mcrt_set_ray_source_host(mcrt_ctx* ctx, const mcrt_ray_source_desc* source, uint64_t* sanitised) {
    const char* what = "mcrt_set_ray_source_host";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (sanitised) *sanitised = 0;
    if (!source || source->kind == MCRT_RAY_SOURCE_NONE) {
        ctxSetRaySource(ctx, mcrt_ray_source_desc{}, nullptr, nullptr);
        return MCRT_OK;
    }
    RaySource s;
    if (int rc = validate(ctx, source, s, what)) return rc;
    const uint64_t records = raySourceReadsSpp(s) ? s.pixels * s.spp : s.pixels;
    if (records > kClosestHitMaxRays)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": more records than one closest-hit launch takes (" + std::to_string(kClosestHitMaxRays) + ")");
    const size_t bytes = (size_t)records * 24;
    void *d_first = nullptr, *d_second = nullptr;
    if (hipMalloc(&d_first, bytes) != hipSuccess || hipMalloc(&d_second, bytes) != hipSuccess) {
        (void)hipGetLastError();
        if (d_first) (void)hipFree(d_first);
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string((2 * bytes) >> 20) + " MiB for the arrays' device copy could not be allocated");
    }
    if (hipMemcpy(d_first, source->first, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_second, source->second, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d_first);
        (void)hipFree(d_second);
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the arrays could not be copied to the device");
    }
    if (sanitised) *sanitised = raySourceUnusable(s);
    mcrt_ray_source_desc owned = *source;
    owned.first = (const double*)d_first;
    owned.second = (const double*)d_second;
    ctxSetRaySource(ctx, owned, d_first, d_second);
    return MCRT_OK;
}

extern "C" int mcrt_get_ray_source(mcrt_ctx* ctx, mcrt_ray_source_desc* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!out) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_get_ray_source: out is NULL");
    const mcrt_ray_source_desc* source = ctxRaySource(ctx);
    *out = source ? *source : mcrt_ray_source_desc{};
    return MCRT_OK;
}
