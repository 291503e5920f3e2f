// What the calls that walk the light groups' paths share on the host - mcrt_render_light_groups* (mcrt_light_groups_host.hip) and the
// light probes (mcrt_probes_host.hip), whose walk is the light groups' own: what both refuse, the plane of every surface, and the
// samples' state in the family's scratch (kPassLightGroups slots 0 .. 4: the passes of a context run one after the other). And what the
// light groups and the path classes (mcrt_path_classes_host.hip) share for their filtered planes (include/mcrt.h "Filtered planes"):
// FilmPlanes below.
#pragma once

#include <cstring>
#include <vector>

#include "mcrt_launch.hpp"
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

// ---------------------------------------------------------------------------------------------- filtered planes
// A call with the FILM flag whose film goes through the gather (filmGatherSettings). Its memory: S is the caller's planes; W, the
// filter's table and the samples' weight rows lie behind the samples' radiances in the family's slot 1 (filmPlanesFrameBytes and, per
// sample of a chunk, filmPlanesSampleBytes more of it - the chunk plan counts the latter); the samples' film positions take the first
// words of the shadow and bounce records (slot 2), which no kernel reads once a chunk's walk has ended.
struct FilmPlanes {
    bool on = false;
    FilmGather g{};
    uint32_t extra_launches = 0;  // what the chunks' resolves launched beyond one kernel each (filmPlanesFinish)
};

// The FILM flag's refusals, before anything is allocated or written. -> f.on
inline int filmPlanesValidate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, bool film_flag, const char* what, FilmPlanes& f) {
    f = FilmPlanes{};
    if (!film_flag) return MCRT_OK;
    const char* why = nullptr;
    const char* opt = ctxOpt(ctx, "MCRT_FILM_GATHER");
    if (int rc = filmGatherSettings(*cam, ctxRaySource(ctx) != nullptr, opt && std::strcmp(opt, "force") == 0, &f.on, &why))
        return ctxFail(ctx, rc, std::string(what) + ": " + why);
    return MCRT_OK;
}
inline size_t filmPlanesFrameBytes(const FilmPlanes& f, const mcrt_camera_desc* cam) {
    return f.on ? ((size_t)cam->width * cam->height + cam->film_cache_size) * 8 : 0;
}
inline uint64_t filmPlanesSampleBytes(const FilmPlanes& f, const mcrt_camera_desc* cam) {
    return f.on ? filmGatherRowWords(makeFilmView(*cam, nullptr, nullptr).radius) * 8 : 0;
}
// The table up, W and the planes' S zeroed on the stream. extra: filmPlanesFrameBytes + max_n * filmPlanesSampleBytes of device memory;
// offsets: 16 bytes per sample of a chunk.
inline int filmPlanesPrepare(mcrt_ctx* ctx, const mcrt_camera_desc* cam, bool clamp, const CameraPass& cp, double* extra, double* offsets, double* d_planes, uint32_t planes,
                             FilmPlanes& f) {
    const size_t frame = (size_t)cam->width * cam->height;
    double* table = extra + frame;
    const std::vector<double> host_table = filmCacheTable(*cam);
    if (!host_table.empty()) MCRT_HIP_TRY(ctx, hipMemcpy(table, host_table.data(), host_table.size() * 8, hipMemcpyHostToDevice));
    f.g.film = makeFilmView(*cam, table, nullptr);
    f.g.clamp = clamp ? 1u : 0u;
    f.g.sobol_tab = cp.sobol_tab;
    f.g.offset = offsets;
    f.g.rows = table + cam->film_cache_size;
    f.g.weight = extra;
    f.g.halo = filmGatherHalo(f.g.film.radius);
    MCRT_HIP_TRY(ctx, hipMemsetAsync(extra, 0, frame * 8, cp.stream));
    MCRT_HIP_TRY(ctx, hipMemsetAsync(d_planes, 0, frame * 24 * planes, cp.stream));
    return MCRT_OK;
}
// A chunk's resolve: its film positions and weight rows, then the gather over the pixels it reaches, and after the frame's last chunk the division.
// launch(g) queues the pass's resolve kernel in g's mode and returns its hipError_t as an int.
template <class Launch>
int filmPlanesChunk(FilmPlanes& f, const AovChunk& c, uint64_t total_pixels, Launch launch) {
    filmGatherReach(f.g, c);
    f.g.mode = kFilmGatherOffsets;
    if (int e = launch(f.g)) return e;
    f.g.mode = kFilmGatherGather;
    if (int e = launch(f.g)) return e;
    f.extra_launches++;
    if (c.first_pixel + c.pixels < total_pixels) return 0;
    f.g.mode = kFilmGatherNormalise;
    f.extra_launches++;
    return launch(f.g);
}
// After the chunk loop, which counts a chunk's resolve as one launch: the call's status handed on, its statistics completed.
inline int filmPlanesFinish(const FilmPlanes& f, int rc, mcrt_stats* stats) {
    if (rc == MCRT_OK && stats) stats->kernel_launches += f.extra_launches;
    return rc;
}

// A call's walk: the parameters the kernels take, the chunk plan, the samples' state and the bounce loop's scratch.
struct LgWalk {
    LgParams par;
    PixelChunks plan;
    LgState st;
    LivePathScratch sc;
    double* extra;  // extra_frame_bytes + max_n * extra_sample_bytes behind the radiances
};

// After lgValidate, with the call's PassTimer running: everything of `w`.
inline int lgWalkPrepare(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const AovScene& scene, const LgSettings& r, const char* what, LgWalk& w, size_t extra_frame_bytes = 0,
                         uint64_t extra_sample_bytes = 0) {
    w.par.planes = r.planes;
    w.par.sky_plane = r.sky_plane;
    w.par.max_depth = r.max_depth;
    if (int rc = lgUploadPlanes(ctx, scene, r, what, &w.par.plane)) return rc;

    const uint64_t sample_bytes = kLgStateBytes + 24ull * r.planes + 2 * kLivePathRecordBytes + 8 + extra_sample_bytes;
    w.plan = pixelChunksOf(ctx, cam, 2, lightGroupsDefaultChunkSlots((uint64_t)cam->sqrtspp * cam->sqrtspp * 2, sample_bytes));
    const uint64_t max_n = w.plan.max_rays;

    void* state = ctxPassScratch(ctx, kPassLightGroups, 0, max_n * kLgStateBytes);
    double* radiance = (double*)ctxPassScratch(ctx, kPassLightGroups, 1, max_n * 24 * r.planes + extra_frame_bytes + max_n * extra_sample_bytes);
    if (!state || !radiance || !livePathScratch(ctx, kPassLightGroups, max_n, w.sc))
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string((max_n * sample_bytes) >> 20) +
                                              " MiB of path state could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
    lgPlaceState(w.st, state, max_n);
    w.st.radiance = radiance;
    w.extra = radiance + max_n * 3 * r.planes;
    return MCRT_OK;
}

}  // namespace mcrt
