// Light groups (include/mcrt.h mcrt_render_light_groups*), host side: the group map, the samples' state, and behind the camera-ray
// passes' chunk loop (mcrt_camera_pass.hpp), which writes the camera rays and their hits straight into that state, the bounce loop
// (runLivePaths, mcrt_live_paths_host.hpp, which the path classes run too):
// launchLightGroupsBegin starts the paths, then per iteration launchLightGroupsRays -> intersectDeviceArrays over 2 rays per LIVE sample
// -> launchLightGroupsStep, the host reading the next list's count (and the pass's error word) after every step;
// launchLightGroupsResolve when no sample is alive. No kernel here: they are libmcrt_light_groups.so (csrc/mcrt_light_groups.hip;
// DESIGN.md "Image passes" says why). The family's scratch: slot 0 the samples' state, 1 the planes' radiances, 2 the shadow and bounce
// records, 3 the two live lists and the counters, 4 the surfaces' planes, 5 the host-pointer form's frames. Option MCRT_AOV_CHUNK_RAYS
// bounds the shadow and bounce SLOTS of iteration 0: pixels * spp * 2 (its default: lightGroupsDefaultChunkSlots).
// Option MCRT_LIGHT_GROUPS_LOG (tools/light_groups_probe.py sets it): one JSON line per chunk on stderr - the live samples of every
// iteration and the host-clock milliseconds of the chunk and of its searches, the stream drained before each bounce search so that the
// kernels queued before it are not counted as search (the camera rays' kernel is counted with their search). It changes no result.
#include <vector>

#include "mcrt_live_paths_host.hpp"
#include "mcrt_light_groups_launch.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_light_group_params* params, const void* planes, LgSettings& r, const char* what) {
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (int rc = checkCamera(ctx, cam, true, what, "cam is NULL")) return rc;
    if (!planes) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": planes is NULL");
    if (params && params->num_groups > MCRT_LIGHT_GROUPS_MAX)
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": num_groups " + std::to_string(params->num_groups) + " is more than MCRT_LIGHT_GROUPS_MAX (" +
                                                  std::to_string(MCRT_LIGHT_GROUPS_MAX) + ")");
    if (!lgSettingsOf(params, r))
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": sky_plane " + std::to_string(params->sky_plane) + " is more than num_groups (" +
                                                  std::to_string(r.groups) + "): the sky takes a group's plane or the one after them");
    return checkPixelSlots(ctx, cam, 2, "rays", what);
}

// The plane of every surface of the uploaded scene (lgSurfacePlanes) into scratch slot 4. The scene's own arrays are read back from the
// device: the context keeps no host copy.
int uploadPlanes(mcrt_ctx* ctx, const AovScene& scene, const LgSettings& r, const char* what, const uint8_t** d_plane) {
    uint32_t num_surfaces = 0, num_materials = 0;
    ctxSceneCounts(ctx, &num_surfaces, &num_materials);
    std::vector<uint32_t> surf_material(num_surfaces);
    std::vector<mcrt_material> materials(num_materials);
    MCRT_HIP_TRY(ctx, hipMemcpy(surf_material.data(), scene.sh.surf_material, (size_t)num_surfaces * 4, hipMemcpyDeviceToHost));
    MCRT_HIP_TRY(ctx, hipMemcpy(materials.data(), scene.sh.materials, (size_t)num_materials * sizeof(mcrt_material), hipMemcpyDeviceToHost));
    std::vector<uint8_t> plane(std::max<uint32_t>(num_surfaces, 1u), 0);
    uint32_t i = 0;
    if (!lgSurfacePlanes(r, surf_material.data(), num_surfaces, materials.data(), num_materials, plane.data(), &i))
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": surface_group[" + std::to_string(i) + "] = " + std::to_string(r.surface_group[i]) + ", but surface " +
                                                  std::to_string(i) + " is an emitter and there are " + std::to_string(r.groups) + " groups");
    uint8_t* d = (uint8_t*)ctxPassScratch(ctx, kPassLightGroups, 4, plane.size());
    if (!d) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the surfaces' planes could not be allocated");
    MCRT_HIP_TRY(ctx, hipMemcpy(d, plane.data(), plane.size(), hipMemcpyHostToDevice));
    *d_plane = d;
    return MCRT_OK;
}

}  // namespace

extern "C" uint32_t mcrt_light_group_planes(const mcrt_light_group_params* params) {
    LgSettings r;
    return lgSettingsOf(params, r);
}

extern "C" int mcrt_render_light_groups_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_light_group_params* params,
                                               double* d_planes, mcrt_stats* stats) {
    const char* what = "mcrt_render_light_groups_device";
    if (!ctx) return MCRT_ERR_INVALID;
    LgSettings r;
    if (int rc = validate(ctx, cam, params, d_planes, r, what)) return rc;
    PassTimer timer(ctx);
    const CameraPass cp(ctx);
    const hipStream_t stream = cp.stream;
    const AovScene& scene = cp.scene;
    const uint32_t* sobol_tab = cp.sobol_tab;
    LgParams par;
    par.planes = r.planes;
    par.sky_plane = r.sky_plane;
    par.max_depth = r.max_depth;
    if (int rc = uploadPlanes(ctx, scene, r, what, &par.plane)) return rc;

    const uint64_t sample_bytes = kLgStateBytes + 24ull * r.planes + 2 * kLivePathRecordBytes + 8;
    const PixelChunks plan = pixelChunksOf(ctx, cam, 2, lightGroupsDefaultChunkSlots((uint64_t)cam->sqrtspp * cam->sqrtspp * 2, sample_bytes));
    const uint64_t max_n = plan.max_rays, total_pixels = plan.total_pixels;

    LgState st;
    void* state = ctxPassScratch(ctx, kPassLightGroups, 0, max_n * kLgStateBytes);
    double* radiance = (double*)ctxPassScratch(ctx, kPassLightGroups, 1, max_n * 24 * r.planes);
    LivePathScratch sc;
    if (!state || !radiance || !livePathScratch(ctx, kPassLightGroups, max_n, sc))
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string((max_n * sample_bytes) >> 20) +
                                              " MiB of path state could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
    lgPlaceState(st, state, max_n);
    st.radiance = radiance;
    return runLivePaths(
        ctx, what, cp, timer, cam, global_seed, plan, st.ray, stats, sc, r.max_depth, ctxOptOn(ctx, "MCRT_LIGHT_GROUPS_LOG"), "light_groups_chunk",
        [&](const AovChunk&, uint64_t n, uint32_t* list, LgCounters* counters) { return launchLightGroupsBegin(stream, st, n, scene.sh.scene_ior, par, list, counters); },
        [&](const AovChunk& c, const uint32_t* list, uint32_t live, uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next) {
            return launchLightGroupsRays(stream, c, scene, sobol_tab, st, list, live, k, lit, counters, next);
        },
        [&](const AovChunk& c, const uint32_t* list, uint32_t live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next) {
            return launchLightGroupsStep(stream, c, scene, sobol_tab, st, par, list, live, k, last, lit, next_list, counters, next);
        },
        [&](const AovChunk& c) { return launchLightGroupsResolve(stream, c, st, r.planes, d_planes, total_pixels); });
}

extern "C" int mcrt_render_light_groups(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_light_group_params* params, double* planes,
                                        mcrt_stats* stats) {
    const char* what = "mcrt_render_light_groups";
    if (!ctx) return MCRT_ERR_INVALID;
    LgSettings r;
    if (int rc = validate(ctx, cam, params, planes, r, what)) return rc;
    FrameChannel ch[kLgPlanesMax];  // the planes, one behind the other
    const size_t frame = (size_t)cam->width * cam->height * 3;
    for (uint32_t p = 0; p < r.planes; p++) ch[p] = FrameChannel{nullptr, planes + p * frame, 24};
    return hostPointerForm(ctx, what, cam, kPassLightGroups, 5, ch, (int)r.planes, "planes'", stats,
                           [&](mcrt_stats* st) { return mcrt_render_light_groups_device(ctx, cam, global_seed, params, (double*)ch[0].dev, st); });
}
