// Occlusion pass (include/mcrt.h mcrt_render_occlusion*), host side: the settings, and behind the camera-ray passes' chunk loop
// (mcrt_camera_pass.hpp) the second search and the resolve: launchOcclusionRays -> intersectDeviceArrays -> launchOcclusionResolve. No
// kernel here: they are libmcrt_occlusion.so (csrc/mcrt_occlusion.hip; DESIGN.md "Image passes" says why). The family's scratch: slots
// 0 .. 4 the occlusion rays' records, of which the resolve reads direction, t and surface (the search wants room for uv), slot 5 the
// host-pointer form's frames. Option MCRT_AOV_CHUNK_RAYS bounds the OCCLUSION rays of a chunk: pixels * spp * rays.
#include "mcrt_camera_pass.hpp"
#include "mcrt_occlusion.hpp"
#include "mcrt_occlusion_launch.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_occlusion_params* params, const mcrt_occlusion_buffers* buffers, OcclusionSettings& s,
             const char* what) {
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (int rc = checkCamera(ctx, cam, buffers != nullptr, what)) return rc;
    if (const char* why = occlusionSettingsOf(params, s)) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": " + why);
    if (!buffers->ao && !buffers->sky && !buffers->bent_normal) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": no channel is wanted (ao, sky and bent_normal are NULL)");
    return checkPixelSlots(ctx, cam, s.rays, "occlusion rays", what);
}

}  // namespace

extern "C" int mcrt_render_occlusion_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_occlusion_params* params,
                                            const mcrt_occlusion_buffers* d_buffers, mcrt_stats* stats) {
    const char* what = "mcrt_render_occlusion_device";
    if (!ctx) return MCRT_ERR_INVALID;
    OcclusionSettings s;
    if (int rc = validate(ctx, cam, params, d_buffers, s, what)) return rc;
    PassTimer timer(ctx);
    const PixelChunks plan = pixelChunksOf(ctx, cam, s.rays, defaultChunkSlots());
    AovRays cam_rays, occ;
    if (int rc = rayScratch(ctx, what, kPassAov, plan.max_rays, plan.max_rays + plan.max_slots, cam_rays)) return rc;
    if (int rc = rayScratch(ctx, what, kPassOcclusion, plan.max_slots, plan.max_rays + plan.max_slots, occ)) return rc;
    const CameraPass cp(ctx);
    return runChunks(ctx, cp, timer, cam, global_seed, plan, cam_rays, stats, [&](const AovChunk& c, uint32_t& launches, uint64_t& traced) {
        const uint64_t n = (uint64_t)c.pixels * c.spp * s.rays;  // (the slots of missed camera samples are traced too)
        MCRT_HIP_TRY(ctx, (hipError_t)launchOcclusionRays(cp.stream, c, cp.scene, s, cp.sobol_tab, cam_rays, occ));
        if (int rc = intersectDeviceArrays(ctx, n, occ.start, occ.direction, occ.t, occ.surface, occ.uv)) return rc;
        MCRT_HIP_TRY(ctx, (hipError_t)launchOcclusionResolve(cp.stream, c, s, cam_rays, occ, *d_buffers));
        launches += 3;
        traced += n;
        return (int)MCRT_OK;
    });
}

extern "C" int mcrt_render_occlusion(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_occlusion_params* params,
                                     const mcrt_occlusion_buffers* buffers, mcrt_stats* stats) {
    const char* what = "mcrt_render_occlusion";
    if (!ctx) return MCRT_ERR_INVALID;
    OcclusionSettings s;
    if (int rc = validate(ctx, cam, params, buffers, s, what)) return rc;
    FrameChannel ch[3] = {{nullptr, buffers->ao, 8}, {nullptr, buffers->sky, 8}, {nullptr, buffers->bent_normal, 24}};
    return hostPointerForm(ctx, what, cam, kPassOcclusion, 5, ch, 3, "channels'", stats, [&](mcrt_stats* st) {
        const mcrt_occlusion_buffers d{(double*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev};
        return mcrt_render_occlusion_device(ctx, cam, global_seed, params, &d, st);
    });
}
