// Occlusion pass (include/mcrt.h mcrt_render_occlusion*), host side: validation, the chunk loop, statistics and the host-pointer form. No
// kernel here: they are libmcrt_occlusion.so (csrc/mcrt_occlusion.hip; DESIGN.md "Image passes" says why, and what mcrt_pass_host.hpp
// shares). The chunk loop is the AOV pass's with a second search in it: launchAovRays -> intersectDeviceArrays -> launchOcclusionRays ->
// intersectDeviceArrays -> launchOcclusionResolve, the camera rays on the AOV pass's ray scratch (kPassAov slots 0 .. 4: the passes of a
// context run one after the other), the occlusion rays on the family's own: slots 0 .. 4 start, direction, t, surface, uv - 76 B per
// occlusion ray, of which the resolve reads direction, t and surface (the search wants room for uv) -, slot 5 the host-pointer form's
// frames. Option MCRT_AOV_CHUNK_RAYS bounds the OCCLUSION rays of a chunk: pixels * spp * rays, whole pixels, one pixel at least.
#include <algorithm>

#include "mcrt_aov.hpp"
#include "mcrt_aov_launch.hpp"
#include "mcrt_occlusion.hpp"
#include "mcrt_occlusion_launch.hpp"
#include "mcrt_pass_host.hpp"

using namespace mcrt;

namespace {

constexpr uint64_t kOcclusionDefaultChunkRays = 1ull << 24;  // (the AOV pass's: the option is shared)
constexpr uint64_t kOcclusionMaxChunkRays = 0xFFF00000ull;   // mcrt_intersect's queue limit (32-bit cursors)

int ready(mcrt_ctx* ctx, const char* what) {  // (the scene first: a context without one says so, whatever else is wrong)
    if (int rc = ctxNeedScene(ctx, what)) return rc;
    return ctxIdle(ctx, what);
}

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_occlusion_params* params, const mcrt_occlusion_buffers* buffers, OcclusionSettings& s,
             const char* what) {
    if (!cam || !buffers) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": cam or buffers is NULL");
    if (cam->width == 0 || cam->height == 0 || cam->sqrtspp == 0)
        return ctxFail(ctx, MCRT_ERR_INVALID, "camera: width, height and sqrtspp must be non-zero");
    if (cam->shard_count > 1 && cam->shard_index >= cam->shard_count) return ctxFail(ctx, MCRT_ERR_INVALID, "camera: shard_index >= shard_count");
    if ((uint64_t)cam->width * cam->height > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, "camera: more than 2^32 pixels");
    if (const char* why = occlusionSettingsOf(params, s)) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": " + why);
    if (!buffers->ao && !buffers->sky && !buffers->bent_normal) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": no channel is wanted (ao, sky and bent_normal are NULL)");
    if ((uint64_t)cam->sqrtspp * cam->sqrtspp * s.rays > kOcclusionMaxChunkRays)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": more occlusion rays per pixel than one closest-hit launch takes");
    return MCRT_OK;
}

}  // namespace

extern "C" int mcrt_render_occlusion_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_occlusion_params* params,
                                            const mcrt_occlusion_buffers* d_buffers, mcrt_stats* stats) {
    const char* what = "mcrt_render_occlusion_device";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ready(ctx, what)) return rc;
    OcclusionSettings s;
    if (int rc = validate(ctx, cam, params, d_buffers, s, what)) return rc;
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    const uint64_t per_pixel = (uint64_t)spp * s.rays;
    const uint64_t total_pixels = (uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width;
    // a chunk is a whole number of pixels, at least one, and never more occlusion rays than one closest-hit launch takes
    const long want = ctxOptL(ctx, "MCRT_AOV_CHUNK_RAYS", (long)kOcclusionDefaultChunkRays);
    const uint64_t chunk_rays = std::min<uint64_t>(want > 0 ? (uint64_t)want : kOcclusionDefaultChunkRays, kOcclusionMaxChunkRays);
    const uint64_t chunk_pixels = std::min<uint64_t>(std::max<uint64_t>(chunk_rays / per_pixel, 1), std::max<uint64_t>(total_pixels, 1));
    const uint64_t max_cam = chunk_pixels * spp, max_occ = chunk_pixels * per_pixel;

    AovRays cam_rays, occ;
    cam_rays.start = (double*)ctxPassScratch(ctx, kPassAov, 0, max_cam * 24);
    cam_rays.direction = (double*)ctxPassScratch(ctx, kPassAov, 1, max_cam * 24);
    cam_rays.t = (double*)ctxPassScratch(ctx, kPassAov, 2, max_cam * 8);
    cam_rays.surface = (uint32_t*)ctxPassScratch(ctx, kPassAov, 3, max_cam * 4);
    cam_rays.uv = (double*)ctxPassScratch(ctx, kPassAov, 4, max_cam * 16);
    occ.start = (double*)ctxPassScratch(ctx, kPassOcclusion, 0, max_occ * 24);
    occ.direction = (double*)ctxPassScratch(ctx, kPassOcclusion, 1, max_occ * 24);
    occ.t = (double*)ctxPassScratch(ctx, kPassOcclusion, 2, max_occ * 8);
    occ.surface = (uint32_t*)ctxPassScratch(ctx, kPassOcclusion, 3, max_occ * 4);
    occ.uv = (double*)ctxPassScratch(ctx, kPassOcclusion, 4, max_occ * 16);
    if (!cam_rays.start || !cam_rays.direction || !cam_rays.t || !cam_rays.surface || !cam_rays.uv || !occ.start || !occ.direction || !occ.t || !occ.surface || !occ.uv)
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string(((max_cam + max_occ) * 76) >> 20) +
                                              " MiB of ray scratch could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
    AovScene scene;
    const uint32_t* sobol_tab = nullptr;
    ctxAovScene(ctx, &scene, &sobol_tab);

    if (int rc = timer.begin(stream)) return rc;
    uint32_t launches = 0;
    for (uint64_t first = 0; first < total_pixels; first += chunk_pixels) {
        AovChunk c;
        c.cam = *cam;
        c.global_seed = global_seed;
        c.spp = spp;
        c.first_pixel = first;
        c.pixels = (uint32_t)std::min<uint64_t>(chunk_pixels, total_pixels - first);
        const uint64_t n = (uint64_t)c.pixels * spp;
        MCRT_HIP_TRY(ctx, (hipError_t)launchAovRays(stream, c, scene.sh.scene_ior, sobol_tab, cam_rays));
        if (int rc = intersectDeviceArrays(ctx, n, cam_rays.start, cam_rays.direction, cam_rays.t, cam_rays.surface, cam_rays.uv)) return rc;
        MCRT_HIP_TRY(ctx, (hipError_t)launchOcclusionRays(stream, c, scene, s, sobol_tab, cam_rays, occ));
        if (int rc = intersectDeviceArrays(ctx, n * s.rays, occ.start, occ.direction, occ.t, occ.surface, occ.uv)) return rc;
        MCRT_HIP_TRY(ctx, (hipError_t)launchOcclusionResolve(stream, c, s, cam_rays, occ, *d_buffers));
        launches += 5;
    }
    if (int rc = timer.end(stream)) return rc;
    if (int rc = timer.finish(stats, launches)) return rc;
    if (stats) {
        stats->paths = total_pixels * spp;
        stats->rays = total_pixels * spp * (1 + (uint64_t)s.rays);  // (the slots of missed camera samples are traced too)
    }
    return MCRT_OK;
}

extern "C" int mcrt_render_occlusion(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_occlusion_params* params,
                                     const mcrt_occlusion_buffers* buffers, mcrt_stats* stats) {
    const char* what = "mcrt_render_occlusion";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ready(ctx, what)) return rc;
    OcclusionSettings s;
    if (int rc = validate(ctx, cam, params, buffers, s, what)) return rc;
    PassTimer whole(ctx);
    FrameChannel ch[3] = {{nullptr, buffers->ao, 8}, {nullptr, buffers->sky, 8}, {nullptr, buffers->bent_normal, 24}};  // the requested channels as one device allocation
    ShardFrames frames{{ctx, what, kPassOcclusion, 5, kPackedWanted, ch, 3}};
    if (int rc = frames.place(cam, "channels'")) return rc;
    const mcrt_occlusion_buffers d{(double*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev};
    mcrt_stats st;
    if (int rc = mcrt_render_occlusion_device(ctx, cam, global_seed, params, &d, &st)) return rc;
    if (int rc = frames.down(cam)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
