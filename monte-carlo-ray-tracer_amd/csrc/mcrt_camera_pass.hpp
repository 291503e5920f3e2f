// What the passes that trace camera rays share (DESIGN.md "Image passes"): the first-hit AOV pass, the ID mattes, the occlusion pass, the
// lighting passes, the light groups, the path classes and adaptive sampling (mcrt_{aov,matte,occlusion,lighting,light_groups,path_classes,adaptive}_host.hip). Two layers. The PURE one - no HIP, no
// context - is the chunk plan, its defaults, a chunk's record and a shard's rows: the host sides and the emulations of the CPU tests
// (tests/emu/*_emu.cpp, which include this file the way they include mcrt_aov.hpp) run the same text. The HOST one, on top of
// mcrt_pass_host.hpp and compiled by hipcc only, is the calls' guard, the camera checks, the five arrays of a family's ray scratch, the
// chunk loop around the camera rays and their closest hits, and the host-pointer form.
//
// Every such pass keeps its camera-ray records - 48 B of ray + 28 B of hit = 76 B per ray: start, direction, t, surface, uv - in
// kPassAov slots 0 .. 4 (the light groups and the path classes in their samples' state): the passes of a context run one after the other, and each sizes the
// slots for its own chunk. A pass with a second search keeps those rays in slots 0 .. 4 of its own family.
#pragma once

#include <algorithm>

#include "mcrt_aov.hpp"

namespace mcrt {

// The most rays one closest-hit search takes: mcrt_intersect's queue limit (32-bit cursors with room for the waves' overshoot).
constexpr uint64_t kClosestHitMaxRays = 0xFFF00000ull;

// A chunk is a whole number of pixels, at least one, and never more slots than one closest-hit launch takes. A slot is what option
// MCRT_AOV_CHUNK_RAYS counts: a camera ray (AOV, mattes), an occlusion ray, a shadow or bounce ray (lighting, light groups' iteration 0).
struct PixelChunks {
    uint64_t total_pixels;
    uint32_t spp;
    uint64_t chunk_pixels, max_rays, max_slots;  // of a chunk: pixels, camera rays, slots
};

// per_pixel: the slots of a pixel; wanted: the option's value, 0 = unset, then dflt.
inline PixelChunks pixelChunks(uint64_t total_pixels, uint32_t spp, uint64_t per_pixel, uint64_t wanted, uint64_t dflt) {
    const uint64_t chunk_slots = std::min<uint64_t>(wanted ? wanted : dflt, kClosestHitMaxRays);
    PixelChunks p;
    p.total_pixels = total_pixels;
    p.spp = spp;
    p.chunk_pixels = std::min<uint64_t>(std::max<uint64_t>(chunk_slots / per_pixel, 1), std::max<uint64_t>(total_pixels, 1));
    p.max_rays = p.chunk_pixels * spp;
    p.max_slots = p.chunk_pixels * per_pixel;
    return p;
}

// The default of the AOV pass, the mattes and the occlusion pass: 2^24 slots, 1.2 GiB of records.
inline uint64_t defaultChunkSlots() { return 1ull << 24; }

// The lighting passes' grows with the sample count: their resolve kernel is one lane per PIXEL, and 2^24 slots are 32 768 pixels at 256
// samples a pixel - 512 waves on 1024 SIMDs, each alone on its SIMD, and the resolve 3.2 times as slow per sample as at 16 samples a pixel
// (profiles/NOTES_lighting.md). So the default is what 2^17 pixels take - two waves of the resolve on every SIMD - between 2^24 and 2^26
// slots (the most: 5.1 GB of slots and 2.5 GB of camera records).
inline uint64_t lightingDefaultChunkSlots(uint64_t per_pixel, uint64_t least = 1ull << 24) {
    return std::min<uint64_t>(std::max<uint64_t>((1ull << 17) * per_pixel, least), 1ull << 26);
}

// The light groups' is sized like that, between 2^25 and 2^26 slots, and cut down to what 8 GiB of state, radiances and records hold
// (sample_bytes per sample: 216 bytes of state, 24 per plane and 152 of records where the lighting passes take 228 in all; a sample is two
// slots). Large chunks matter more here than there: every chunk runs its own tail of iterations with a handful of live samples, each
// about 0.08 ms of launches and waits whatever it shades (profiles/NOTES_light_groups.md: hexagon_room at 16 samples a pixel takes 98 ms
// in one chunk, 118 in four, 175 in sixteen).
inline uint64_t lightGroupsDefaultChunkSlots(uint64_t per_pixel, uint64_t sample_bytes) {
    return std::min<uint64_t>(lightingDefaultChunkSlots(per_pixel, 1ull << 25), (8ull << 30) / sample_bytes * 2);
}

// The chunk of chunk_pixels pixels (fewer at the frame's end) that starts at packed pixel `first`.
inline AovChunk chunkAt(const mcrt_camera_desc& cam, uint32_t global_seed, uint32_t spp, uint64_t first, uint64_t chunk_pixels, uint64_t total_pixels) {
    AovChunk c;
    c.cam = cam;
    c.global_seed = global_seed;
    c.spp = spp;
    c.first_pixel = first;
    c.pixels = (uint32_t)std::min<uint64_t>(chunk_pixels, total_pixels - first);
    return c;
}

// Owned rows of the camera's shard: what mcrt_shard_rows counts, for the emulations, which do not link it.
inline uint32_t ownedRows(const mcrt_camera_desc& cam) {
    uint32_t rows = 0;
    for (uint32_t ly = 0; localToGlobalRow(cam, ly) < cam.height; ly++) rows++;
    return rows;
}

}  // namespace mcrt

#if defined(__HIPCC__)

#include "mcrt_aov_launch.hpp"
#include "mcrt_lens_launch.hpp"
#include "mcrt_pass_host.hpp"

namespace mcrt {

inline int cameraPassReady(mcrt_ctx* ctx, const char* what) {  // (the scene first: a context without one says so, whatever else is wrong)
    if (int rc = ctxNeedScene(ctx, what)) return rc;
    return ctxIdle(ctx, what);
}

// The frame's order under the context's ray source ("Ray sources" in mcrt.h): the same chunks, the rays from the source's loops of
// aovRayKernel (launchSourceRays, csrc/mcrt_aov.hip).
struct SourcePixels {
    RaySource source{};  // (kind MCRT_RAY_SOURCE_NONE, which the launch refuses, should the descriptor not be a valid one)
    explicit SourcePixels(const mcrt_ray_source_desc& d) {
        const char* why = nullptr;
        if (raySourceSettings(d, source, &why) != MCRT_OK) source = RaySource{};  // (cannot happen: mcrt_set_ray_source lets no other descriptor into the context)
    }
    AovChunk chunk(const mcrt_camera_desc& cam, uint32_t global_seed, uint32_t spp, uint64_t first, uint64_t chunk_pixels, uint64_t total_pixels) const {
        return chunkAt(cam, global_seed, spp, first, chunk_pixels, total_pixels);
    }
    int rays(hipStream_t stream, const AovChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays_) const {
        return launchSourceRays(stream, c, source, scene_ior, sobol_tab, rays_);
    }
};

// The frame's order of a probe call with positions ("Light probes" in mcrt.h): the same chunks, the rays from the probe loop of
// aovRayKernel (launchProbeRays, csrc/mcrt_aov.hip). The call itself names it (mcrt_probes_host.hip): nothing of it is on the context.
struct ProbePixels {
    const double* positions;  // DEVICE [pixels][3]
    uint64_t pixels;          // the shard's packed pixels
    AovChunk chunk(const mcrt_camera_desc& cam, uint32_t global_seed, uint32_t spp, uint64_t first, uint64_t chunk_pixels, uint64_t total_pixels) const {
        return chunkAt(cam, global_seed, spp, first, chunk_pixels, total_pixels);
    }
    int rays(hipStream_t stream, const AovChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays_) const {
        return launchProbeRays(stream, c, positions, pixels, scene_ior, sobol_tab, rays_);
    }
};

// The camera's own checks. given: the call's other pointers are there; missing: what the message names when they or cam are not.
inline int checkCamera(mcrt_ctx* ctx, const mcrt_camera_desc* cam, bool given, const char* what, const char* missing = "cam or buffers is NULL") {
    if (!cam || !given) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": " + missing);
    if (cam->width == 0 || cam->height == 0 || cam->sqrtspp == 0)
        return ctxFail(ctx, MCRT_ERR_INVALID, "camera: width, height and sqrtspp must be non-zero");
    if (cam->shard_count > 1 && cam->shard_index >= cam->shard_count) return ctxFail(ctx, MCRT_ERR_INVALID, "camera: shard_index >= shard_count");
    if ((uint64_t)cam->width * cam->height > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, "camera: more than 2^32 pixels");
    if (const mcrt_lens_desc* lens = ctxLens(ctx))
        if (!lensTakesCamera(*lens, *cam))
            return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": a thin-lens camera under the lens of mcrt_set_lens - only MCRT_LENS_PERSPECTIVE has a thin lens");
    if (const mcrt_ray_source_desc* source = ctxRaySource(ctx)) {  // the arrays were made for this shard's packed pixels (and samples)
        const SourcePixels sp(*source);
        const uint64_t pixels = (uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width;
        const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
        const int which = raySourceTakesCamera(sp.source, pixels, spp);
        if (which == 1)
            return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": the ray source of mcrt_set_ray_source was made for " + std::to_string(sp.source.pixels) +
                                                      " packed pixels, the camera's shard has " + std::to_string(pixels) + " (owned rows x width)");
        if (which == 2)
            return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": the ray source of mcrt_set_ray_source holds " + std::to_string(sp.source.spp) +
                                                      " samples per pixel, the camera takes " + std::to_string(spp) + " (sqrtspp squared)");
    }
    return MCRT_OK;
}

// ... and the last one, after the pass's settings where the factor comes from them: a pixel's slots (`factor` `noun` per camera sample)
// fit one closest-hit search.
inline int checkPixelSlots(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint64_t factor, const char* noun, const char* what) {
    if ((uint64_t)cam->sqrtspp * cam->sqrtspp * factor > kClosestHitMaxRays)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": more " + noun + " per pixel than one closest-hit launch takes");
    return MCRT_OK;
}

// The plan of a call: `factor` slots per camera sample, option MCRT_AOV_CHUNK_RAYS or dflt slots a chunk.
inline PixelChunks pixelChunksOf(const mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint64_t factor, uint64_t dflt) {
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    const long want = ctxOptL(ctx, "MCRT_AOV_CHUNK_RAYS", 0);
    return pixelChunks((uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width, spp, spp * factor, want > 0 ? (uint64_t)want : 0, dflt);
}

// Records for n rays in slots 0 .. 4 of `family`. all_rays: the records of every family the call allocates, for the message.
inline int rayScratch(mcrt_ctx* ctx, const char* what, PassFamily family, uint64_t n, uint64_t all_rays, AovRays& rays) {
    rays.start = (double*)ctxPassScratch(ctx, family, 0, n * 24);
    rays.direction = (double*)ctxPassScratch(ctx, family, 1, n * 24);
    rays.t = (double*)ctxPassScratch(ctx, family, 2, n * 8);
    rays.surface = (uint32_t*)ctxPassScratch(ctx, family, 3, n * 4);
    rays.uv = (double*)ctxPassScratch(ctx, family, 4, n * 16);
    if (!rays.start || !rays.direction || !rays.t || !rays.surface || !rays.uv)
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string((all_rays * 76) >> 20) +
                                              " MiB of ray scratch could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
    return MCRT_OK;
}

// What every launch of a call takes.
struct CameraPass {
    hipStream_t stream;
    AovScene scene;
    const uint32_t* sobol_tab = nullptr;
    explicit CameraPass(mcrt_ctx* ctx) : stream((hipStream_t)ctxStream(ctx)) { ctxAovScene(ctx, &scene, &sobol_tab); }
};

// How the chunks of a call name their pixels, as the chunk loop needs it: chunk(...) is the record of a chunk, rays(...) queues the
// kernel that writes its camera rays. Here the frame's own order - pixel p of a chunk is packed pixel first_pixel + p, the rays are
// libmcrt_aov.so's -; under a lens LensPixels below, under a ray source SourcePixels above, a probe call's positions ProbePixels; the adaptive pass has a naming through a pixel list (mcrt_adaptive_host.hip).
struct FramePixels {
    AovChunk chunk(const mcrt_camera_desc& cam, uint32_t global_seed, uint32_t spp, uint64_t first, uint64_t chunk_pixels, uint64_t total_pixels) const {
        return chunkAt(cam, global_seed, spp, first, chunk_pixels, total_pixels);
    }
    int rays(hipStream_t stream, const AovChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays_) const {
        return launchAovRays(stream, c, scene_ior, sobol_tab, rays_);
    }
};

// The frame's order under the context's lens ("Camera models" in mcrt.h): the same chunks, the rays from the lens branches of
// aovRayKernel (launchLensRays, csrc/mcrt_aov.hip).
struct LensPixels {
    LensSettings lens{};  // (model MCRT_LENS_NONE - the camera's own rays - should the descriptor not be a valid one)
    explicit LensPixels(const mcrt_lens_desc& d) {
        const char* why = nullptr;
        if (lensSettings(d, lens, &why) != MCRT_OK) lens = LensSettings{};  // (cannot happen: mcrt_set_lens lets no other descriptor into the context)
    }
    AovChunk chunk(const mcrt_camera_desc& cam, uint32_t global_seed, uint32_t spp, uint64_t first, uint64_t chunk_pixels, uint64_t total_pixels) const {
        return FramePixels{}.chunk(cam, global_seed, spp, first, chunk_pixels, total_pixels);
    }
    int rays(hipStream_t stream, const AovChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays_) const {
        return launchLensRays(stream, c, lens, scene_ior, sobol_tab, rays_);
    }
};

// The chunk loop. Per chunk: the camera rays into `rays` and their closest hits (2 launches, n rays), then body(chunk, launches, traced)
// -> rc, which adds its own launches and rays to the two counts. Around the loop the call's events; after it the statistics.
template <class Naming, class Body>
int runChunksOf(const Naming& naming, mcrt_ctx* ctx, const CameraPass& cp, PassTimer& timer, const mcrt_camera_desc* cam, uint32_t global_seed, const PixelChunks& plan,
                const AovRays& rays, mcrt_stats* stats, Body body) {
    if (int rc = timer.begin(cp.stream)) return rc;
    uint32_t launches = 0;
    uint64_t traced = 0;
    for (uint64_t first = 0; first < plan.total_pixels; first += plan.chunk_pixels) {
        const auto c = naming.chunk(*cam, global_seed, plan.spp, first, plan.chunk_pixels, plan.total_pixels);
        const uint64_t n = (uint64_t)c.pixels * plan.spp;
        MCRT_HIP_TRY(ctx, (hipError_t)naming.rays(cp.stream, c, cp.scene.sh.scene_ior, cp.sobol_tab, rays));
        if (int rc = intersectDeviceArrays(ctx, n, rays.start, rays.direction, rays.t, rays.surface, rays.uv)) return rc;
        launches += 2;
        traced += n;
        if (int rc = body(c, launches, traced)) return rc;
    }
    if (int rc = timer.end(cp.stream)) return rc;
    if (int rc = timer.finish(stats, launches)) return rc;
    if (stats) {
        stats->paths = plan.total_pixels * plan.spp;
        stats->rays = traced;
    }
    return MCRT_OK;
}
template <class Body>
int runChunks(mcrt_ctx* ctx, const CameraPass& cp, PassTimer& timer, const mcrt_camera_desc* cam, uint32_t global_seed, const PixelChunks& plan, const AovRays& rays,
              mcrt_stats* stats, Body body) {
    if (const mcrt_lens_desc* lens = ctxLens(ctx)) return runChunksOf(LensPixels(*lens), ctx, cp, timer, cam, global_seed, plan, rays, stats, body);
    if (const mcrt_ray_source_desc* source = ctxRaySource(ctx)) return runChunksOf(SourcePixels(*source), ctx, cp, timer, cam, global_seed, plan, rays, stats, body);
    return runChunksOf(FramePixels{}, ctx, cp, timer, cam, global_seed, plan, rays, stats, body);
}

// The host-pointer form of a pass: the frames of `ch` (n of them, the wanted ones one allocation in the family's `slot`) as device
// copies of the shard's rows, device(&stats) - the _device call on ch[i].dev -, the rows back into the host frames, and the call's whole
// time in total_ms.
template <class Device>
int hostPointerForm(mcrt_ctx* ctx, const char* what, const mcrt_camera_desc* cam, PassFamily family, int slot, FrameChannel* ch, int n, const char* noun,
                    mcrt_stats* stats, Device device) {
    PassTimer whole(ctx);
    ShardFrames frames{{ctx, what, family, slot, kPackedWanted, ch, n}};
    if (int rc = frames.place(cam, noun)) return rc;
    mcrt_stats st;
    if (int rc = device(&st)) return rc;
    if (int rc = frames.down(cam)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}

}  // namespace mcrt

#endif  // __HIPCC__
