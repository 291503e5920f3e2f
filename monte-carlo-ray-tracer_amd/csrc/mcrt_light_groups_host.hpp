// What the calls that walk the light groups' paths share on the host - mcrt_render_light_groups* (mcrt_light_groups_host.hip) and the
// light probes (mcrt_probes_host.hip), whose walk is the light groups' own: what both refuse, the plane of every surface, and the
// samples' state in the family's scratch (kPassLightGroups slots 0 .. 4: the passes of a context run one after the other).
#pragma once

#include <vector>

#include "mcrt_live_paths_host.hpp"
#include "mcrt_light_groups_launch.hpp"

namespace mcrt {

inline int lgValidate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_light_group_params* params, const void* planes, LgSettings& r, const char* what) {
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
inline int lgUploadPlanes(mcrt_ctx* ctx, const AovScene& scene, const LgSettings& r, const char* what, const uint8_t** d_plane) {
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

// A call's walk: the parameters the kernels take, the chunk plan, the samples' state and the bounce loop's scratch.
struct LgWalk {
    LgParams par;
    PixelChunks plan;
    LgState st;
    LivePathScratch sc;
};

// After lgValidate, with the call's PassTimer running: everything of `w`.
inline int lgWalkPrepare(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const AovScene& scene, const LgSettings& r, const char* what, LgWalk& w) {
    w.par.planes = r.planes;
    w.par.sky_plane = r.sky_plane;
    w.par.max_depth = r.max_depth;
    if (int rc = lgUploadPlanes(ctx, scene, r, what, &w.par.plane)) return rc;

    const uint64_t sample_bytes = kLgStateBytes + 24ull * r.planes + 2 * kLivePathRecordBytes + 8;
    w.plan = pixelChunksOf(ctx, cam, 2, lightGroupsDefaultChunkSlots((uint64_t)cam->sqrtspp * cam->sqrtspp * 2, sample_bytes));
    const uint64_t max_n = w.plan.max_rays;

    void* state = ctxPassScratch(ctx, kPassLightGroups, 0, max_n * kLgStateBytes);
    double* radiance = (double*)ctxPassScratch(ctx, kPassLightGroups, 1, max_n * 24 * r.planes);
    if (!state || !radiance || !livePathScratch(ctx, kPassLightGroups, max_n, w.sc))
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string((max_n * sample_bytes) >> 20) +
                                              " MiB of path state could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
    lgPlaceState(w.st, state, max_n);
    w.st.radiance = radiance;
    return MCRT_OK;
}

}  // namespace mcrt
