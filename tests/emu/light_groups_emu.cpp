// tests/emu/light_groups_emu.cpp — TEST HARNESS ONLY (built by tests/test_light_groups_emulation.py into tests/emu/_build/).
//
// The light groups on the host: csrc/mcrt_light_groups.hpp (and csrc/mcrt_aov.hpp, csrc/mcrt_shade.hpp below it) unchanged - the text the
// kernels of csrc/mcrt_light_groups.hip run - driven chunk by chunk and iteration by iteration the way mcrt_render_light_groups_device
// drives them (mcrt_emu.cpp's chunk plan and emuCameraRays, live_paths_emu.hpp's loop), live lists included, with the closest hits from
// the emulation's sceneIntersect (emu_intersect). Not a CPU fallback: nothing in the product links or loads it.
#include "mcrt_emu.cpp"

#include "live_paths_emu.hpp"

extern "C" {

// What the calls resolve from the parameters and a scene's surfaces (lgSettingsOf, lgSurfacePlanes), without a render: the status;
// out[0 .. 3] = groups, sky_plane, planes, max_depth; plane: [num_surfaces]; *bad: the first offending surface (0xFFFFFFFF: none).
int light_groups_emu_settings(const mcrt_light_group_params* params, const uint32_t* surf_material, uint32_t num_surfaces, const mcrt_material* materials,
                              uint32_t num_materials, uint32_t* out, uint8_t* plane, uint32_t* bad) {
    LgSettings set;
    *bad = 0xFFFFFFFFu;
    if (!lgSettingsOf(params, set)) return MCRT_ERR_INVALID;
    out[0] = set.groups, out[1] = set.sky_plane, out[2] = set.planes, out[3] = set.max_depth;
    return lgSurfacePlanes(set, surf_material, num_surfaces, materials, num_materials, plane, bad) ? MCRT_OK : MCRT_ERR_INVALID;
}

// The planes into `out` (host array [planes][owned pixels][3]), in chunks of chunk_rays shadow and bounce slots of iteration 0 (0 = one
// chunk). stage_lds, list_order: EmuLivePaths'. info: [0] rays handed to the search, [1] the most iterations a chunk took, [2] live
// samples summed over all iterations. Returns mcrt_status values for what the call refuses.
int light_groups_emu_frame(const mcrt_scene_desc* scene, const mcrt_camera_desc* cam, uint32_t global_seed, int stage_lds, uint64_t chunk_rays,
                           const mcrt_light_group_params* params, int list_order, double* out, uint64_t* info) {
    Emu E;
    if (int rc = setup(E, scene, 0)) return rc;
    const AovScene as = aovSceneOf(E);
    LgSettings set;
    if (!lgSettingsOf(params, set)) return MCRT_ERR_INVALID;
    std::vector<uint8_t> plane(scene->num_surfaces, 0);
    uint32_t bad = 0;
    if (!lgSurfacePlanes(set, scene->surf_material, scene->num_surfaces, scene->materials, scene->num_materials, plane.data(), &bad)) return MCRT_ERR_INVALID;
    const LgParams par{plane.data(), set.planes, set.sky_plane, set.max_depth};

    const PixelChunks plan = emuPixelChunks(cam, 2, chunk_rays);
    const uint64_t max_n = plan.max_rays, total = plan.total_pixels;
    std::vector<double> state((max_n * kLgStateBytes + 7) / 8), radiance(max_n * 3 * par.planes);
    LgState st;
    lgPlaceState(st, state.data(), max_n);
    st.radiance = radiance.data();
    EmuLivePaths paths(scene, stage_lds, plan.max_slots, list_order, par.max_depth);
    if (info) info[0] = info[1] = info[2] = 0;
    for (uint64_t first = 0; first < total; first += plan.chunk_pixels) {
        const AovChunk c = chunkAt(*cam, global_seed, plan.spp, first, plan.chunk_pixels, total);
        if (int rc = emuCameraRays(scene, E, c, stage_lds, st.ray)) return rc;
        const int rc = paths.run(
            c, [&](const AovChunk&, uint64_t s) { return lgBegin(st, s, as.sh.scene_ior, par); },  // lightGroupsBeginKernel
            [&](const AovChunk& c_, const uint32_t* list, uint32_t live, uint32_t j, uint32_t k, const AovRays& lit, RefractionHistory& rh) {
                lgRays(c_, as, st, list, live, j, k, lit, rh, E.tab.data());  // lightGroupsRayKernel
            },
            [&](const AovChunk& c_, const uint32_t* list, uint32_t live, uint32_t j, uint32_t k, bool last, const AovRays& lit, RefractionHistory& rh, bool& too_deep) {
                return lgStep(c_, as, st, par, list, live, j, k, last, lit, rh, too_deep, E.tab.data());  // lightGroupsStepKernel
            },
            [&](const AovChunk& c_, uint32_t p) { lgResolvePixel(c_, st, par.planes, p, out, total); });  // lightGroupsResolveKernel
        if (rc) return rc;
    }
    if (info) info[0] = paths.rays, info[1] = paths.iterations, info[2] = paths.live;
    return 0;
}

}  // extern "C"
