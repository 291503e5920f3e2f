// Lighting passes (include/mcrt.h mcrt_render_lighting*), host side: behind the camera-ray passes' chunk loop (mcrt_camera_pass.hpp)
// the second search and the resolve: launchLightingRays -> intersectDeviceArrays -> launchLightingResolve. No kernel here: they are
// libmcrt_lighting.so (csrc/mcrt_lighting.hip; DESIGN.md "Image passes" says why). The shadow and bounce rays are ONE array of two per
// camera sample, one search for both, on the family's scratch: slots 0 .. 4 their records, of which the resolve reads t and surface (the
// search wants room for uv), slot 5 the host-pointer form's frames. Option MCRT_AOV_CHUNK_RAYS bounds the shadow and bounce SLOTS of a
// chunk: pixels * spp * 2; its default grows with the sample count (lightingDefaultChunkSlots).
#include "mcrt_camera_pass.hpp"
#include "mcrt_lighting.hpp"
#include "mcrt_lighting_launch.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_lighting_buffers* b, const char* what) {
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (int rc = checkCamera(ctx, cam, b != nullptr, what)) return rc;
    if (!b->emission && !b->sky && !b->direct && !b->light && !b->unoccluded)
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": no channel is wanted (emission, sky, direct, light and unoccluded are NULL)");
    return checkPixelSlots(ctx, cam, 2, "rays", what);
}

}  // namespace

extern "C" int mcrt_render_lighting_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_lighting_buffers* d_buffers,
                                           mcrt_stats* stats) {
    const char* what = "mcrt_render_lighting_device";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = validate(ctx, cam, d_buffers, what)) return rc;
    PassTimer timer(ctx);
    const PixelChunks plan = pixelChunksOf(ctx, cam, 2, lightingDefaultChunkSlots((uint64_t)cam->sqrtspp * cam->sqrtspp * 2));
    AovRays cam_rays, lit;
    if (int rc = rayScratch(ctx, what, kPassAov, plan.max_rays, plan.max_rays + plan.max_slots, cam_rays)) return rc;
    if (int rc = rayScratch(ctx, what, kPassLighting, plan.max_slots, plan.max_rays + plan.max_slots, lit)) return rc;
    const CameraPass cp(ctx);
    return runChunks(ctx, cp, timer, cam, global_seed, plan, cam_rays, stats, [&](const AovChunk& c, uint32_t& launches, uint64_t& traced) {
        const uint64_t n = 2ull * c.pixels * c.spp;  // (the slots of samples without a shadow or a bounce ray are traced too)
        MCRT_HIP_TRY(ctx, (hipError_t)launchLightingRays(cp.stream, c, cp.scene, cp.sobol_tab, cam_rays, lit));
        if (int rc = intersectDeviceArrays(ctx, n, lit.start, lit.direction, lit.t, lit.surface, lit.uv)) return rc;
        MCRT_HIP_TRY(ctx, (hipError_t)launchLightingResolve(cp.stream, c, cp.scene, cp.sobol_tab, cam_rays, lit, *d_buffers));
        launches += 3;
        traced += n;
        return (int)MCRT_OK;
    });
}

extern "C" int mcrt_render_lighting(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_lighting_buffers* buffers, mcrt_stats* stats) {
    const char* what = "mcrt_render_lighting";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = validate(ctx, cam, buffers, what)) return rc;
    FrameChannel ch[5] = {{nullptr, buffers->emission, 24}, {nullptr, buffers->sky, 24}, {nullptr, buffers->direct, 24}, {nullptr, buffers->light, 24},
                          {nullptr, buffers->unoccluded, 24}};
    return hostPointerForm(ctx, what, cam, kPassLighting, 5, ch, 5, "channels'", stats, [&](mcrt_stats* st) {
        const mcrt_lighting_buffers d{(double*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev, (double*)ch[3].dev, (double*)ch[4].dev};
        return mcrt_render_lighting_device(ctx, cam, global_seed, &d, st);
    });
}
