// Camera models (include/mcrt.h mcrt_set_lens, mcrt_get_lens, mcrt_camera_rays*), host side: the descriptor into and out of the context,
// and the rays of a whole shard in one launch. No kernel here: the models are branches of aovRayKernel (csrc/mcrt_aov.hip,
// libmcrt_aov.so; launchLensRays). The passes take a lens through the chunk loop (mcrt_camera_pass.hpp LensPixels); the render calls' guard is where they bottom out
// (mcrt_hip.hip launchRender) and in mcrt_adaptive_host.hip. The host-pointer form borrows the AOV family's ray scratch, slots 0 and 1:
// the passes of a context run one after the other.
#include "mcrt_camera_pass.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const void* start, const void* direction, uint64_t& pixels, const char* what) {
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (int rc = checkCamera(ctx, cam, start && direction, what, "cam, start or direction is NULL")) return rc;
    pixels = (uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width;
    if (pixels * cam->sqrtspp * cam->sqrtspp > kClosestHitMaxRays)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": more rays than one closest-hit launch takes (" + std::to_string(kClosestHitMaxRays) + ")");
    return MCRT_OK;
}

}  // namespace

extern "C" int mcrt_set_lens(mcrt_ctx* ctx, const mcrt_lens_desc* lens) {
    const char* what = "mcrt_set_lens";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (!lens || lens->model == MCRT_LENS_NONE) {
        ctxSetLens(ctx, mcrt_lens_desc{});
        return MCRT_OK;
    }
    if (ctxRaySource(ctx))
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": a ray source is set (mcrt_set_ray_source) - a lens and a ray source exclude each other; "
                                                                 "mcrt_set_ray_source(ctx, NULL) takes it off");
    LensSettings s;
    const char* why = nullptr;
    if (int rc = lensSettings(*lens, s, &why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);
    ctxSetLens(ctx, *lens);
    return MCRT_OK;
}

extern "C" int mcrt_get_lens(mcrt_ctx* ctx, mcrt_lens_desc* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!out) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_get_lens: out is NULL");
    const mcrt_lens_desc* lens = ctxLens(ctx);
    *out = lens ? *lens : mcrt_lens_desc{};
    return MCRT_OK;
}

extern "C" int mcrt_camera_rays_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, double* d_start, double* d_direction, mcrt_stats* stats) {
    const char* what = "mcrt_camera_rays_device";
    if (!ctx) return MCRT_ERR_INVALID;
    uint64_t pixels = 0;
    if (int rc = validate(ctx, cam, d_start, d_direction, pixels, what)) return rc;
    PassTimer timer(ctx);
    const CameraPass cp(ctx);
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    const AovRays rays{d_start, d_direction, nullptr, nullptr, nullptr};
    if (int rc = timer.begin(cp.stream)) return rc;
    if (pixels) {  // one chunk: the shard's packed pixels
        const AovChunk c = chunkAt(*cam, global_seed, spp, 0, pixels, pixels);
        const mcrt_lens_desc* lens = ctxLens(ctx);
        const mcrt_ray_source_desc* source = ctxRaySource(ctx);
        MCRT_HIP_TRY(ctx, (hipError_t)(lens     ? LensPixels(*lens).rays(cp.stream, c, cp.scene.sh.scene_ior, cp.sobol_tab, rays)
                                       : source ? SourcePixels(*source).rays(cp.stream, c, cp.scene.sh.scene_ior, cp.sobol_tab, rays)
                                                : FramePixels{}.rays(cp.stream, c, cp.scene.sh.scene_ior, cp.sobol_tab, rays)));
    }
    if (int rc = timer.end(cp.stream)) return rc;
    if (int rc = timer.finish(stats, pixels ? 1 : 0)) return rc;
    if (stats) stats->paths = stats->rays = pixels * spp;
    return MCRT_OK;
}

extern "C" int mcrt_camera_rays(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, double* start, double* direction, mcrt_stats* stats) {
    const char* what = "mcrt_camera_rays";
    if (!ctx) return MCRT_ERR_INVALID;
    uint64_t pixels = 0;
    if (int rc = validate(ctx, cam, start, direction, pixels, what)) return rc;
    PassTimer whole(ctx);
    const size_t bytes = (size_t)pixels * cam->sqrtspp * cam->sqrtspp * 24;
    double* d_start = (double*)ctxPassScratch(ctx, kPassAov, 0, bytes);
    double* d_direction = (double*)ctxPassScratch(ctx, kPassAov, 1, bytes);
    if (!d_start || !d_direction) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the rays' device copy could not be allocated");
    mcrt_stats st;
    if (int rc = mcrt_camera_rays_device(ctx, cam, global_seed, d_start, d_direction, &st)) return rc;
    if (bytes) {
        MCRT_HIP_TRY(ctx, hipMemcpy(start, d_start, bytes, hipMemcpyDeviceToHost));
        MCRT_HIP_TRY(ctx, hipMemcpy(direction, d_direction, bytes, hipMemcpyDeviceToHost));
    }
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
