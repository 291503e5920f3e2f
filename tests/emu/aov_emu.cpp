// tests/emu/aov_emu.cpp — TEST HARNESS ONLY (built by tests/test_aov_emulation.py into tests/emu/_build/).
//
// The first-hit AOV pass on the host: csrc/mcrt_aov.hpp unchanged - the text the two kernels of csrc/mcrt_aov.hip run - driven chunk by
// chunk the way mcrt_render_aov_device drives them (mcrt_emu.cpp's chunk plan and emuCameraRays), with the closest hits from the
// emulation's sceneIntersect (emu_intersect). Not a CPU fallback: nothing in the product links or loads it.
#include "mcrt_emu.cpp"

extern "C" {

// The camera rays of the frame, [pixel][sample][3] over the packed owned rows.
int aov_emu_rays(const mcrt_scene_desc* scene, const mcrt_camera_desc* cam, uint32_t global_seed, double* start, double* direction) {
    std::vector<uint32_t> tab(kSobolTableWords);
    buildSobolByteTables(tab.data());
    const uint64_t pixels = (uint64_t)ownedRows(*cam) * cam->width;
    const AovChunk c = chunkAt(*cam, global_seed, cam->sqrtspp * cam->sqrtspp, 0, pixels, pixels);
    for (uint64_t p = 0; p < pixels; p++)
        for (uint32_t i = 0; i < c.spp; i++) {
            const Ray ray = aovCameraRay<true>(c, scene->scene_ior, (uint32_t)p, i, tab.data());
            aovStore3(start, p * c.spp + i, ray.start);
            aovStore3(direction, p * c.spp + i, ray.direction);
        }
    return 0;
}

// The AOV frame into `out` (host arrays over the packed owned rows, null = channel not wanted), in chunks of chunk_rays rays (0 = one
// chunk). hit_t / hit_surface / hit_uv (may be null): every sample's hit, [pixel][sample]. stage_lds: emu_intersect's flavour of the walk.
int aov_emu_frame(const mcrt_scene_desc* scene, const mcrt_camera_desc* cam, uint32_t global_seed, int stage_lds, uint64_t chunk_rays,
                  const mcrt_aov_buffers* out, double* hit_t, uint32_t* hit_surface, double* hit_uv) {
    Emu E;
    if (int rc = setup(E, scene, 0)) return rc;
    const AovScene as = aovSceneOf(E);
    const PixelChunks plan = emuPixelChunks(cam, 1, chunk_rays);
    const uint32_t spp = plan.spp;
    EmuRays records(plan.max_rays);
    const AovRays rays = records.view();
    for (uint64_t first = 0; first < plan.total_pixels; first += plan.chunk_pixels) {
        const AovChunk c = chunkAt(*cam, global_seed, spp, first, plan.chunk_pixels, plan.total_pixels);
        if (int rc = emuCameraRays(scene, E, c, stage_lds, rays)) return rc;
        for (uint32_t p = 0; p < c.pixels; p++) {  // aovResolveKernel
            AovAccum acc;
            aovBegin(acc);
            for (uint32_t i = 0; i < spp; i++) {
                const uint64_t r = (uint64_t)i * c.pixels + p;
                aovAddRay(acc, as, i, rays, r);
                if (hit_t) hit_t[(first + p) * spp + i] = rays.t[r];
                if (hit_surface) hit_surface[(first + p) * spp + i] = rays.surface[r];
                if (hit_uv) {
                    hit_uv[((first + p) * spp + i) * 2] = rays.uv[2 * r];
                    hit_uv[((first + p) * spp + i) * 2 + 1] = rays.uv[2 * r + 1];
                }
            }
            aovFinish(acc, spp, *out, first + p);
        }
    }
    return 0;
}

}  // extern "C"
