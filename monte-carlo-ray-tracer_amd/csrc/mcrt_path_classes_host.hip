// Path classes (include/mcrt.h mcrt_render_path_classes*), host side: the class map, the samples' state, and behind the camera-ray
// passes' chunk loop (mcrt_camera_pass.hpp), which writes the camera rays and their hits straight into that state, the light groups'
// bounce loop (runLivePaths, mcrt_live_paths_host.hpp) with this pass's four launches. No kernel here: they are libmcrt_path_classes.so
// (csrc/mcrt_path_classes.hip). The family's scratch: slot 0 the samples' state, 1 the planes' radiances, 2 the shadow and bounce records,
// 3 the two live lists and the counters, 5 the host-pointer form's frames. Options: MCRT_AOV_CHUNK_RAYS as in the light groups;
// With MCRT_PATH_CLASSES_FILM the resolve is the filtered planes' (FilmPlanes, mcrt_light_groups_host.hpp), as in the light groups.
// MCRT_PATH_CLASSES_LOG (tools/path_classes_probe.py sets it) their per-chunk line on stderr, keyed "path_classes_chunk".
#include "mcrt_light_groups_host.hpp"
#include "mcrt_path_classes.hpp"
#include "mcrt_path_classes_launch.hpp"

using namespace mcrt;

namespace {

const char* const kClassNames[MCRT_PATH_CLASSES] = {"emission",      "background",      "diffuse_direct",      "diffuse_indirect",
                                                    "glossy_direct", "glossy_indirect", "transmission_direct", "transmission_indirect"};

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_path_class_params* params, const void* planes, PcParams& r, const char* what) {
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (int rc = checkCamera(ctx, cam, true, what, "cam is NULL")) return rc;
    if (!planes) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": planes is NULL");
    uint32_t bad = 0;
    if (!pcSettingsOf(params, r, &bad))
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": class_plane[" + std::to_string(bad) + "] (" + kClassNames[bad] + ") = " +
                                                  std::to_string(params->class_plane[bad]) + ", but there are at most " + std::to_string(MCRT_PATH_CLASSES) + " planes");
    return checkPixelSlots(ctx, cam, 2, "rays", what);
}

}  // namespace

extern "C" uint32_t mcrt_path_class_planes(const mcrt_path_class_params* params) {
    PcParams r;
    return pcSettingsOf(params, r);
}

extern "C" int mcrt_render_path_classes_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_path_class_params* params,
                                               double* d_planes, mcrt_stats* stats) {
    const char* what = "mcrt_render_path_classes_device";
    if (!ctx) return MCRT_ERR_INVALID;
    PcParams par;
    if (int rc = validate(ctx, cam, params, d_planes, par, what)) return rc;
    const uint32_t flags = params ? params->flags : 0u;
    FilmPlanes film;
    if (int rc = filmPlanesValidate(ctx, cam, (flags & MCRT_PATH_CLASSES_FILM) != 0u, what, film)) return rc;
    PassTimer timer(ctx);
    const CameraPass cp(ctx);
    const hipStream_t stream = cp.stream;
    const AovScene& scene = cp.scene;
    const uint32_t* sobol_tab = cp.sobol_tab;

    const uint64_t sample_bytes = kPcStateBytes + 24ull * par.planes + 2 * kLivePathRecordBytes + 8 + filmPlanesSampleBytes(film, cam);
    const PixelChunks plan = pixelChunksOf(ctx, cam, 2, lightGroupsDefaultChunkSlots((uint64_t)cam->sqrtspp * cam->sqrtspp * 2, sample_bytes));
    const uint64_t max_n = plan.max_rays, total_pixels = plan.total_pixels;

    PcState st;
    void* state = ctxPassScratch(ctx, kPassPathClasses, 0, max_n * kPcStateBytes);
    double* radiance = (double*)ctxPassScratch(ctx, kPassPathClasses, 1, max_n * 24 * par.planes + filmPlanesFrameBytes(film, cam) + max_n * filmPlanesSampleBytes(film, cam));
    LivePathScratch sc;
    if (!state || !radiance || !livePathScratch(ctx, kPassPathClasses, max_n, sc))
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string((max_n * sample_bytes) >> 20) +
                                              " MiB of path state could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
    pcPlaceState(st, state, max_n);
    st.lg.radiance = radiance;
    if (film.on)  // (W and the table behind the radiances, the film positions in the records: FilmPlanes, mcrt_light_groups_host.hpp)
        if (int rc = filmPlanesPrepare(ctx, cam, (flags & MCRT_PATH_CLASSES_FILM_CLAMP) != 0u, cp, radiance + max_n * 3 * par.planes, sc.lit.start, d_planes, par.planes, film))
            return rc;
    const int rc = runLivePaths(
        ctx, what, cp, timer, cam, global_seed, plan, st.lg.ray, stats, sc, par.max_depth, ctxOptOn(ctx, "MCRT_PATH_CLASSES_LOG"), "path_classes_chunk",
        [&](const AovChunk&, uint64_t n, uint32_t* list, LgCounters* counters) { return launchPathClassesBegin(stream, st, n, scene.sh.scene_ior, par, list, counters); },
        [&](const AovChunk& c, const uint32_t* list, uint32_t live, uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next) {
            return launchPathClassesRays(stream, c, scene, sobol_tab, st, list, live, k, lit, counters, next);
        },
        [&](const AovChunk& c, const uint32_t* list, uint32_t live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next) {
            return launchPathClassesStep(stream, c, scene, sobol_tab, st, par, list, live, k, last, lit, next_list, counters, next);
        },
        [&](const AovChunk& c) {
            if (!film.on) return launchPathClassesResolve(stream, c, st, par.planes, d_planes, total_pixels);
            return filmPlanesChunk(film, c, total_pixels, [&](const FilmGather& g) { return launchPathClassesFilm(stream, c, st, par.planes, g, d_planes, total_pixels); });
        });
    return filmPlanesFinish(film, rc, stats);
}

extern "C" int mcrt_render_path_classes(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_path_class_params* params, double* planes,
                                        mcrt_stats* stats) {
    const char* what = "mcrt_render_path_classes";
    if (!ctx) return MCRT_ERR_INVALID;
    PcParams par;
    if (int rc = validate(ctx, cam, params, planes, par, what)) return rc;
    FrameChannel ch[MCRT_PATH_CLASSES];  // the planes, one behind the other
    const size_t frame = (size_t)cam->width * cam->height * 3;
    for (uint32_t p = 0; p < par.planes; p++) ch[p] = FrameChannel{nullptr, planes + p * frame, 24};
    return hostPointerForm(ctx, what, cam, kPassPathClasses, 5, ch, (int)par.planes, "planes'", stats,
                           [&](mcrt_stats* st) { return mcrt_render_path_classes_device(ctx, cam, global_seed, params, (double*)ch[0].dev, st); });
}
