// First-hit AOV pass (include/mcrt.h mcrt_render_aov*), host side: the resolve launch behind the camera-ray passes' chunk loop
// (mcrt_camera_pass.hpp) and the channel table of the host-pointer form. No kernel here: they are libmcrt_aov.so (csrc/mcrt_aov.hip;
// DESIGN.md "Image passes" says why). Scratch: the camera-ray records (kPassAov slots 0 .. 4), slot 5 the host-pointer form's frames.
#include "mcrt_camera_pass.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_aov_buffers* buffers, const char* what) {
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (int rc = checkCamera(ctx, cam, buffers != nullptr, what)) return rc;
    return checkPixelSlots(ctx, cam, 1, "samples", what);
}

}  // namespace

extern "C" int mcrt_render_aov_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_aov_buffers* buffers,
                                      mcrt_stats* stats) {
    const char* what = "mcrt_render_aov_device";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = validate(ctx, cam, buffers, what)) return rc;
    PassTimer timer(ctx);
    const PixelChunks plan = pixelChunksOf(ctx, cam, 1, defaultChunkSlots());
    AovRays rays;
    if (int rc = rayScratch(ctx, what, kPassAov, plan.max_rays, plan.max_rays, rays)) return rc;
    const CameraPass cp(ctx);
    return runChunks(ctx, cp, timer, cam, global_seed, plan, rays, stats, [&](const AovChunk& c, uint32_t& launches, uint64_t&) {
        MCRT_HIP_TRY(ctx, (hipError_t)launchAovResolve(cp.stream, c, cp.scene, rays, *buffers));
        launches++;
        return (int)MCRT_OK;
    });
}

extern "C" int mcrt_render_aov(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_aov_buffers* buffers,
                               mcrt_stats* stats) {
    const char* what = "mcrt_render_aov";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = validate(ctx, cam, buffers, what)) return rc;
    // the requested channels: depth, position, normal, shading normal, albedo, coverage, then the two id channels
    FrameChannel ch[8] = {{nullptr, buffers->depth, 8},  {nullptr, buffers->position, 24},       {nullptr, buffers->normal, 24},
                          {nullptr, buffers->shading_normal, 24}, {nullptr, buffers->albedo, 24}, {nullptr, buffers->coverage, 8},
                          {nullptr, buffers->surface, 4}, {nullptr, buffers->material, 4}};
    return hostPointerForm(ctx, what, cam, kPassAov, 5, ch, 8, "channels'", stats, [&](mcrt_stats* st) {
        const mcrt_aov_buffers d{(double*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev, (double*)ch[3].dev,
                                 (double*)ch[4].dev, (double*)ch[5].dev, (uint32_t*)ch[6].dev, (uint32_t*)ch[7].dev};
        return mcrt_render_aov_device(ctx, cam, global_seed, &d, st);
    });
}
