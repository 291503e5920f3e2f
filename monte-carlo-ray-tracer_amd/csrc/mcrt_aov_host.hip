// First-hit AOV pass (include/mcrt.h mcrt_render_aov*), host side: chunking, scratch, the closest-hit search mcrt_intersect already has
// (intersectDeviceArrays, mcrt_hip.hip) between the two launches of csrc/mcrt_aov.hip, statistics, and the host-pointer form. No kernel
// here: they are libmcrt_aov.so (csrc/mcrt_aov.hip; DESIGN.md "Image passes" says why, and what mcrt_pass_host.hpp shares).
// Scratch per ray: 48 B of ray + 28 B of hit = 76 B, kept in the context and grown on demand (2^24 rays per chunk by default = 1.2 GiB;
// option MCRT_AOV_CHUNK_RAYS).
#include <algorithm>

#include "mcrt_aov.hpp"
#include "mcrt_aov_launch.hpp"
#include "mcrt_pass_host.hpp"

using namespace mcrt;

namespace {

constexpr uint64_t kAovDefaultChunkRays = 1ull << 24;
constexpr uint64_t kAovMaxChunkRays = 0xFFF00000ull;  // mcrt_intersect's queue limit (32-bit cursors)

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_aov_buffers* buffers, const char* what) {
    if (!cam || !buffers) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": cam or buffers is NULL");
    if (cam->width == 0 || cam->height == 0 || cam->sqrtspp == 0)
        return ctxFail(ctx, MCRT_ERR_INVALID, "camera: width, height and sqrtspp must be non-zero");
    if (cam->shard_count > 1 && cam->shard_index >= cam->shard_count) return ctxFail(ctx, MCRT_ERR_INVALID, "camera: shard_index >= shard_count");
    if ((uint64_t)cam->width * cam->height > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, "camera: more than 2^32 pixels");
    if ((uint64_t)cam->sqrtspp * cam->sqrtspp > kAovMaxChunkRays)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": more samples per pixel than one closest-hit launch takes");
    return MCRT_OK;
}

int ready(mcrt_ctx* ctx, const char* what) {  // (the scene first: a context without one says so, whatever else is wrong)
    if (int rc = ctxNeedScene(ctx, what)) return rc;
    return ctxIdle(ctx, what);
}

}  // namespace

extern "C" int mcrt_render_aov_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_aov_buffers* buffers,
                                      mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ready(ctx, "mcrt_render_aov_device")) return rc;
    if (int rc = validate(ctx, cam, buffers, "mcrt_render_aov_device")) return rc;
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    const uint64_t total_pixels = (uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width;
    // a chunk is a whole number of pixels, at least one, and never more rays than one closest-hit launch takes
    const long want = ctxOptL(ctx, "MCRT_AOV_CHUNK_RAYS", (long)kAovDefaultChunkRays);
    const uint64_t chunk_rays = std::min<uint64_t>(want > 0 ? (uint64_t)want : kAovDefaultChunkRays, kAovMaxChunkRays);
    const uint64_t chunk_pixels = std::min<uint64_t>(std::max<uint64_t>(chunk_rays / spp, 1), std::max<uint64_t>(total_pixels, 1));
    const uint64_t max_rays = chunk_pixels * spp;

    AovRays rays;
    rays.start = (double*)ctxPassScratch(ctx, kPassAov, 0, max_rays * 24);
    rays.direction = (double*)ctxPassScratch(ctx, kPassAov, 1, max_rays * 24);
    rays.t = (double*)ctxPassScratch(ctx, kPassAov, 2, max_rays * 8);
    rays.surface = (uint32_t*)ctxPassScratch(ctx, kPassAov, 3, max_rays * 4);
    rays.uv = (double*)ctxPassScratch(ctx, kPassAov, 4, max_rays * 16);
    if (!rays.start || !rays.direction || !rays.t || !rays.surface || !rays.uv)
        return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_render_aov_device: " + std::to_string((max_rays * 76) >> 20) +
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
        MCRT_HIP_TRY(ctx, (hipError_t)launchAovRays(stream, c, scene.sh.scene_ior, sobol_tab, rays));
        if (int rc = intersectDeviceArrays(ctx, n, rays.start, rays.direction, rays.t, rays.surface, rays.uv)) return rc;
        MCRT_HIP_TRY(ctx, (hipError_t)launchAovResolve(stream, c, scene, rays, *buffers));
        launches += 3;
    }
    if (int rc = timer.end(stream)) return rc;
    if (int rc = timer.finish(stats, launches)) return rc;
    if (stats) stats->paths = stats->rays = total_pixels * spp;
    return MCRT_OK;
}

extern "C" int mcrt_render_aov(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_aov_buffers* buffers,
                               mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ready(ctx, "mcrt_render_aov")) return rc;
    if (int rc = validate(ctx, cam, buffers, "mcrt_render_aov")) return rc;
    PassTimer whole(ctx);
    // the requested channels as one device allocation: depth, position, normal, shading normal, albedo, coverage, then the two id channels
    FrameChannel ch[8] = {{nullptr, buffers->depth, 8},  {nullptr, buffers->position, 24},       {nullptr, buffers->normal, 24},
                          {nullptr, buffers->shading_normal, 24}, {nullptr, buffers->albedo, 24}, {nullptr, buffers->coverage, 8},
                          {nullptr, buffers->surface, 4}, {nullptr, buffers->material, 4}};
    ShardFrames frames{{ctx, "mcrt_render_aov", kPassAov, 5, kPackedWanted, ch, 8}};
    if (int rc = frames.place(cam, "channels'")) return rc;
    const mcrt_aov_buffers d{(double*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev, (double*)ch[3].dev,
                             (double*)ch[4].dev, (double*)ch[5].dev, (uint32_t*)ch[6].dev, (uint32_t*)ch[7].dev};
    mcrt_stats st;
    if (int rc = mcrt_render_aov_device(ctx, cam, global_seed, &d, &st)) return rc;
    if (int rc = frames.down(cam)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
