// Lighting passes (include/mcrt.h mcrt_render_lighting*), host side: validation, the chunk loop, statistics and the host-pointer form. No
// kernel here: they are libmcrt_lighting.so (csrc/mcrt_lighting.hip; DESIGN.md "Image passes" says why, and what mcrt_pass_host.hpp
// shares). The chunk loop is the occlusion pass's: launchAovRays -> intersectDeviceArrays -> launchLightingRays -> intersectDeviceArrays
// -> launchLightingResolve, the camera rays on the AOV pass's ray scratch (kPassAov slots 0 .. 4: the passes of a context run one after
// the other), the shadow and bounce rays - ONE array of two per camera sample, one search for both - on the family's own: slots 0 .. 4
// start, direction, t, surface, uv - 76 B per slot, of which the resolve reads t and surface (the search wants room for uv) -, slot 5 the
// host-pointer form's frames. Option MCRT_AOV_CHUNK_RAYS bounds the shadow and bounce SLOTS of a chunk: pixels * spp * 2, whole pixels,
// one pixel at least. Its default here grows with the sample count: the resolve kernel is one lane per PIXEL, and the AOV pass's 2^24
// slots are 32 768 pixels at 256 samples a pixel - 512 waves on 1024 SIMDs, each alone on its SIMD, and the resolve 3.2 times as slow
// per sample as at 16 samples a pixel (profiles/NOTES_lighting.md). So the default is what 2^17 pixels take, between 2^24 and 2^26 slots.
#include <algorithm>

#include "mcrt_aov.hpp"
#include "mcrt_aov_launch.hpp"
#include "mcrt_lighting.hpp"
#include "mcrt_lighting_launch.hpp"
#include "mcrt_pass_host.hpp"

using namespace mcrt;

namespace {

constexpr uint64_t kLightingDefaultChunkRays = 1ull << 24;  // (the AOV pass's: the option is shared) - the least the default is
constexpr uint64_t kLightingDefaultChunkRaysMost = 1ull << 26;  // ... and the most: 5.1 GB of slots and 2.5 GB of camera records
constexpr uint64_t kLightingDefaultChunkPixels = 1ull << 17;  // what the default aims at: two waves of the resolve on every SIMD
constexpr uint64_t kLightingMaxChunkRays = 0xFFF00000ull;   // mcrt_intersect's queue limit (32-bit cursors)

int ready(mcrt_ctx* ctx, const char* what) {  // (the scene first: a context without one says so, whatever else is wrong)
    if (int rc = ctxNeedScene(ctx, what)) return rc;
    return ctxIdle(ctx, what);
}

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_lighting_buffers* b, const char* what) {
    if (!cam || !b) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": cam or buffers is NULL");
    if (cam->width == 0 || cam->height == 0 || cam->sqrtspp == 0)
        return ctxFail(ctx, MCRT_ERR_INVALID, "camera: width, height and sqrtspp must be non-zero");
    if (cam->shard_count > 1 && cam->shard_index >= cam->shard_count) return ctxFail(ctx, MCRT_ERR_INVALID, "camera: shard_index >= shard_count");
    if ((uint64_t)cam->width * cam->height > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, "camera: more than 2^32 pixels");
    if (!b->emission && !b->sky && !b->direct && !b->light && !b->unoccluded)
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": no channel is wanted (emission, sky, direct, light and unoccluded are NULL)");
    if ((uint64_t)cam->sqrtspp * cam->sqrtspp * 2 > kLightingMaxChunkRays)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": more rays per pixel than one closest-hit launch takes");
    return MCRT_OK;
}

}  // namespace

extern "C" int mcrt_render_lighting_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_lighting_buffers* d_buffers,
                                           mcrt_stats* stats) {
    const char* what = "mcrt_render_lighting_device";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ready(ctx, what)) return rc;
    if (int rc = validate(ctx, cam, d_buffers, what)) return rc;
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    const uint64_t per_pixel = (uint64_t)spp * 2;
    const uint64_t total_pixels = (uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width;
    // a chunk is a whole number of pixels, at least one, and never more slots than one closest-hit launch takes
    const uint64_t dflt = std::min(std::max(kLightingDefaultChunkPixels * per_pixel, kLightingDefaultChunkRays), kLightingDefaultChunkRaysMost);
    const long want = ctxOptL(ctx, "MCRT_AOV_CHUNK_RAYS", (long)dflt);
    const uint64_t chunk_rays = std::min<uint64_t>(want > 0 ? (uint64_t)want : dflt, kLightingMaxChunkRays);
    const uint64_t chunk_pixels = std::min<uint64_t>(std::max<uint64_t>(chunk_rays / per_pixel, 1), std::max<uint64_t>(total_pixels, 1));
    const uint64_t max_cam = chunk_pixels * spp, max_lit = chunk_pixels * per_pixel;

    AovRays cam_rays, lit;
    cam_rays.start = (double*)ctxPassScratch(ctx, kPassAov, 0, max_cam * 24);
    cam_rays.direction = (double*)ctxPassScratch(ctx, kPassAov, 1, max_cam * 24);
    cam_rays.t = (double*)ctxPassScratch(ctx, kPassAov, 2, max_cam * 8);
    cam_rays.surface = (uint32_t*)ctxPassScratch(ctx, kPassAov, 3, max_cam * 4);
    cam_rays.uv = (double*)ctxPassScratch(ctx, kPassAov, 4, max_cam * 16);
    lit.start = (double*)ctxPassScratch(ctx, kPassLighting, 0, max_lit * 24);
    lit.direction = (double*)ctxPassScratch(ctx, kPassLighting, 1, max_lit * 24);
    lit.t = (double*)ctxPassScratch(ctx, kPassLighting, 2, max_lit * 8);
    lit.surface = (uint32_t*)ctxPassScratch(ctx, kPassLighting, 3, max_lit * 4);
    lit.uv = (double*)ctxPassScratch(ctx, kPassLighting, 4, max_lit * 16);
    if (!cam_rays.start || !cam_rays.direction || !cam_rays.t || !cam_rays.surface || !cam_rays.uv || !lit.start || !lit.direction || !lit.t || !lit.surface || !lit.uv)
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string(((max_cam + max_lit) * 76) >> 20) +
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
        MCRT_HIP_TRY(ctx, (hipError_t)launchLightingRays(stream, c, scene, sobol_tab, cam_rays, lit));
        if (int rc = intersectDeviceArrays(ctx, 2 * n, lit.start, lit.direction, lit.t, lit.surface, lit.uv)) return rc;
        MCRT_HIP_TRY(ctx, (hipError_t)launchLightingResolve(stream, c, scene, sobol_tab, cam_rays, lit, *d_buffers));
        launches += 5;
    }
    if (int rc = timer.end(stream)) return rc;
    if (int rc = timer.finish(stats, launches)) return rc;
    if (stats) {
        stats->paths = total_pixels * spp;
        stats->rays = 3 * stats->paths;  // (the slots of samples without a shadow or a bounce ray are traced too)
    }
    return MCRT_OK;
}

extern "C" int mcrt_render_lighting(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_lighting_buffers* buffers, mcrt_stats* stats) {
    const char* what = "mcrt_render_lighting";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ready(ctx, what)) return rc;
    if (int rc = validate(ctx, cam, buffers, what)) return rc;
    PassTimer whole(ctx);
    FrameChannel ch[5] = {{nullptr, buffers->emission, 24}, {nullptr, buffers->sky, 24}, {nullptr, buffers->direct, 24}, {nullptr, buffers->light, 24},
                          {nullptr, buffers->unoccluded, 24}};  // the requested channels as one device allocation
    ShardFrames frames{{ctx, what, kPassLighting, 5, kPackedWanted, ch, 5}};
    if (int rc = frames.place(cam, "channels'")) return rc;
    const mcrt_lighting_buffers d{(double*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev, (double*)ch[3].dev, (double*)ch[4].dev};
    mcrt_stats st;
    if (int rc = mcrt_render_lighting_device(ctx, cam, global_seed, &d, &st)) return rc;
    if (int rc = frames.down(cam)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
