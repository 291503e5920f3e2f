// ID mattes (include/mcrt.h mcrt_render_matte*, mcrt_matte_rank_device, mcrt_matte_code, mcrt_matte_manifest), host side: the settings,
// the key map and the code table, the ranking's form, the manifest, and behind the camera-ray passes' chunk loop (mcrt_camera_pass.hpp)
// launchMatteRank (which maps surfaces to keys as it loads them) [-> launchAovResolve when the AOV channels are wanted too]. No kernel
// here: the ranking is libmcrt_matte.so (csrc/mcrt_matte.hip; DESIGN.md "Image passes" says why). Scratch slots of the family: 0 the
// uploaded key map (MCRT_MATTE_CUSTOM), 1 the code table, 2 the memory form's work arrays, 3 the host-pointer form's frames. The map and
// the codes are made and uploaded by every call that needs them: a snprintf and a hash per key, next to a closest-hit search per sample.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcrt_camera_pass.hpp"
#include "mcrt_matte.hpp"
#include "mcrt_matte_launch.hpp"

using namespace mcrt;

namespace {

static_assert(kMatteMaxSamples == kClosestHitMaxRays, "a ranking takes what one closest-hit search gives it");

struct MatteSettings {
    uint32_t key, ranks, num_keys;
    const uint32_t* surface_key;
    const char* const* names;
};

// The settings of `params` for a scene of num_surfaces / num_materials; nullptr or why they are refused.
const char* settingsOf(const mcrt_matte_params* params, uint32_t num_surfaces, uint32_t num_materials, MatteSettings& s, std::string& detail) {
    s = MatteSettings{MCRT_MATTE_MATERIAL, MCRT_MATTE_DEFAULT_RANKS, 0, nullptr, nullptr};
    if (params) {
        s.key = params->key;
        if (params->ranks) s.ranks = params->ranks;
        s.surface_key = params->surface_key;
        s.names = params->names;
    }
    if (s.key > MCRT_MATTE_CUSTOM) return "key must be MCRT_MATTE_MATERIAL, MCRT_MATTE_SURFACE or MCRT_MATTE_CUSTOM";
    if (const char* why = matteRanksError(s.ranks)) return why;
    s.num_keys = s.key == MCRT_MATTE_MATERIAL ? num_materials : s.key == MCRT_MATTE_SURFACE ? num_surfaces : params->num_keys;
    if (s.key == MCRT_MATTE_CUSTOM) {
        if (!s.surface_key) return "MCRT_MATTE_CUSTOM without surface_key";
        if (s.num_keys == 0) return "MCRT_MATTE_CUSTOM with num_keys 0";
        for (uint32_t i = 0; i < num_surfaces; i++)
            if (s.surface_key[i] >= s.num_keys) {
                detail = "surface_key[" + std::to_string(i) + "] = " + std::to_string(s.surface_key[i]) + " is not below num_keys " + std::to_string(s.num_keys);
                return detail.c_str();
            }
    }
    if (s.names)
        for (uint32_t k = 0; k < s.num_keys; k++)
            if (!matteNameOk(s.names[k])) {
                detail = "names[" + std::to_string(k) + "] is not 1 .. 255 bytes of printable ASCII";
                return detail.c_str();
            }
    return nullptr;
}

// Key k's name: the caller's, or the default of the key mode written into buf (16 bytes at least).
const char* nameOf(uint32_t key_mode, const char* const* names, uint32_t k, char* buf, size_t cap) {
    if (names) return names[k];
    snprintf(buf, cap, matteDefaultNameFormat(key_mode), k);
    return buf;
}

// Which form ranks spp samples per pixel: option MCRT_MATTE_FORM ("tile" / "memory") or, unset, the tile form up to
// kMatteTileAutoMaxSpp samples per pixel - there a workgroup's LDS leaves four workgroups a CU - and the memory form past it
// (profiles/NOTES_matte.md has the two measured at 256 and 1024 samples per pixel). Both give the same bits. 0: "tile" pinned where it
// cannot run.
int formOf(const mcrt_ctx* ctx, uint32_t spp) {
    const char* form = ctxOpt(ctx, "MCRT_MATTE_FORM");
    const bool fits = matteTilePixels(spp) != 0;
    if (form && !strcmp(form, "memory")) return kMatteFormMemory;
    if (form && !strcmp(form, "tile")) return fits ? kMatteFormTile : 0;
    return fits && spp <= kMatteTileAutoMaxSpp ? kMatteFormTile : kMatteFormMemory;
}

// mr (keys, map, codes, out, first_pixel, pixels, spp, ranks set) queued on `stream` in `form`.
int rankLaunch(mcrt_ctx* ctx, hipStream_t stream, MatteRank& mr, int form, const char* what) {
    mr.tile = form == kMatteFormTile ? matteTilePixels(mr.spp) : 0;
    mr.work = nullptr;
    if (form == kMatteFormMemory) {
        mr.work = (uint32_t*)ctxPassScratch(ctx, kPassMatte, 2, (size_t)mr.pixels * mr.spp * 8);
        if (!mr.work) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the memory form's 8 bytes per sample could not be allocated");
    }
    MCRT_HIP_TRY(ctx, (hipError_t)launchMatteRank(stream, mr, form));
    return MCRT_OK;
}

int validateCamera(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_matte_buffers* buffers, const char* what) {  // (as mcrt_render_aov*)
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (int rc = checkCamera(ctx, cam, buffers != nullptr, what)) return rc;
    return checkPixelSlots(ctx, cam, 1, "samples", what);
}

int settingsFor(mcrt_ctx* ctx, const mcrt_matte_params* params, MatteSettings& s, const char* what) {
    uint32_t num_surfaces = 0, num_materials = 0;
    ctxSceneCounts(ctx, &num_surfaces, &num_materials);
    std::string detail;
    if (const char* why = settingsOf(params, num_surfaces, num_materials, s, detail)) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": " + why);
    return MCRT_OK;
}

}  // namespace

extern "C" uint32_t mcrt_matte_code(const char* name) { return name ? matteCodeOf((const unsigned char*)name, strlen(name)) : matteCodeOf(nullptr, 0); }

extern "C" int64_t mcrt_matte_manifest(const mcrt_matte_params* params, uint32_t num_keys, char* buf, uint64_t cap) {
    const uint32_t key_mode = params ? params->key : (uint32_t)MCRT_MATTE_MATERIAL;
    const char* const* names = params ? params->names : nullptr;
    if (key_mode > MCRT_MATTE_CUSTOM || (cap && !buf)) return MCRT_ERR_INVALID;
    uint64_t at = 0;
    auto put = [&](char c) {
        if (at < cap) buf[at] = c;
        at++;
    };
    put('{');
    for (uint32_t k = 0; k < num_keys; k++) {
        char dflt[24], hex[12];
        const char* name = nameOf(key_mode, names, k, dflt, sizeof dflt);
        if (!matteNameOk(name)) return MCRT_ERR_INVALID;
        if (k) put(',');
        put('"');
        for (const char* c = name; *c; c++) {
            if (*c == '"' || *c == '\\') put('\\');
            put(*c);
        }
        put('"');
        put(':');
        snprintf(hex, sizeof hex, "\"%08x\"", matteCodeOf((const unsigned char*)name, strlen(name)));
        for (const char* c = hex; *c; c++) put(*c);
    }
    put('}');
    put('\0');
    return (int64_t)at;
}

extern "C" int mcrt_matte_rank_device(mcrt_ctx* ctx, uint64_t pixels, uint32_t spp, const uint32_t* d_keys, uint32_t ranks, const uint32_t* d_codes,
                                      const mcrt_matte_buffers* d_buffers, mcrt_stats* stats) {
    const char* what = "mcrt_matte_rank_device";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (pixels == 0 || pixels > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": pixels must be non-zero and below 2^32");
    if (spp == 0 || pixels * spp > kMatteMaxSamples) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": spp must be non-zero and pixels * spp below 2^32");
    if (!d_keys || !d_buffers) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": d_keys or d_buffers is NULL");
    if (!ranks) ranks = MCRT_MATTE_DEFAULT_RANKS;
    if (const char* why = matteRanksError(ranks)) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": " + why);
    if (d_buffers->layer && !d_codes) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": layer wanted without d_codes");
    const int form = formOf(ctx, spp);
    if (!form) return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": option MCRT_MATTE_FORM pins the tile form, which takes 2048 samples per pixel at most");
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    MatteRank mr{};
    mr.keys = d_keys;
    mr.codes = d_codes;
    mr.out = *d_buffers;
    mr.pixels = (uint32_t)pixels;
    mr.spp = spp;
    mr.ranks = ranks;
    if (int rc = timer.begin(stream)) return rc;
    if (int rc = rankLaunch(ctx, stream, mr, form, what)) return rc;
    if (int rc = timer.end(stream)) return rc;
    return timer.finish(stats, 1);
}

extern "C" int mcrt_render_matte_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_matte_params* params,
                                        const mcrt_matte_buffers* d_buffers, const mcrt_aov_buffers* d_aov, mcrt_stats* stats) {
    const char* what = "mcrt_render_matte_device";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = validateCamera(ctx, cam, d_buffers, what)) return rc;
    MatteSettings s;
    if (int rc = settingsFor(ctx, params, s, what)) return rc;
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    const int form = formOf(ctx, spp);
    if (!form) return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": option MCRT_MATTE_FORM pins the tile form, which takes 2048 samples per pixel at most");
    PassTimer timer(ctx);
    const PixelChunks plan = pixelChunksOf(ctx, cam, 1, defaultChunkSlots());
    AovRays rays;
    if (int rc = rayScratch(ctx, what, kPassAov, plan.max_rays, plan.max_rays, rays)) return rc;
    const CameraPass cp(ctx);

    // the key map and, when the layer is wanted, the code table
    const uint32_t* d_map = nullptr;
    const uint32_t* d_codes = nullptr;
    if (s.key == MCRT_MATTE_MATERIAL) d_map = cp.scene.sh.surf_material;
    if (s.key == MCRT_MATTE_CUSTOM) {
        uint32_t num_surfaces = 0, num_materials = 0;
        ctxSceneCounts(ctx, &num_surfaces, &num_materials);
        void* up = ctxPassScratch(ctx, kPassMatte, 0, (size_t)num_surfaces * 4);
        if (!up) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the key map could not be allocated");
        MCRT_HIP_TRY(ctx, hipMemcpy(up, s.surface_key, (size_t)num_surfaces * 4, hipMemcpyHostToDevice));
        d_map = (const uint32_t*)up;
    }
    if (d_buffers->layer) {
        std::vector<uint32_t> codes(s.num_keys);
        char dflt[24];
        for (uint32_t k = 0; k < s.num_keys; k++) codes[k] = mcrt_matte_code(nameOf(s.key, s.names, k, dflt, sizeof dflt));
        void* up = ctxPassScratch(ctx, kPassMatte, 1, (size_t)s.num_keys * 4);
        if (!up) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the code table could not be allocated");
        MCRT_HIP_TRY(ctx, hipMemcpy(up, codes.data(), (size_t)s.num_keys * 4, hipMemcpyHostToDevice));
        d_codes = (const uint32_t*)up;
    }

    return runChunks(ctx, cp, timer, cam, global_seed, plan, rays, stats, [&](const AovChunk& c, uint32_t& launches, uint64_t&) {
        MatteRank mr{};
        mr.keys = rays.surface;
        mr.map = d_map;
        mr.codes = d_codes;
        mr.out = *d_buffers;
        mr.first_pixel = c.first_pixel;
        mr.pixels = c.pixels;
        mr.spp = spp;
        mr.ranks = s.ranks;
        if (int rc = rankLaunch(ctx, cp.stream, mr, form, what)) return rc;
        launches++;
        if (d_aov) {
            MCRT_HIP_TRY(ctx, (hipError_t)launchAovResolve(cp.stream, c, cp.scene, rays, *d_aov));
            launches++;
        }
        return (int)MCRT_OK;
    });
}

extern "C" int mcrt_render_matte(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_matte_params* params,
                                 const mcrt_matte_buffers* buffers, const mcrt_aov_buffers* aov, mcrt_stats* stats) {
    const char* what = "mcrt_render_matte";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = validateCamera(ctx, cam, buffers, what)) return rc;
    MatteSettings s;
    if (int rc = settingsFor(ctx, params, s, what)) return rc;
    // the wanted buffers: the four of the mattes, then the AOV pass's eight
    const size_t r = s.ranks;
    const mcrt_aov_buffers none{};
    const mcrt_aov_buffers& a = aov ? *aov : none;
    FrameChannel ch[12] = {{nullptr, buffers->id, 4 * r}, {nullptr, buffers->coverage, 8 * r}, {nullptr, buffers->layer, 16 * r}, {nullptr, buffers->distinct, 4},
                           {nullptr, a.depth, 8},  {nullptr, a.position, 24}, {nullptr, a.normal, 24}, {nullptr, a.shading_normal, 24},
                           {nullptr, a.albedo, 24}, {nullptr, a.coverage, 8}, {nullptr, a.surface, 4}, {nullptr, a.material, 4}};
    return hostPointerForm(ctx, what, cam, kPassMatte, 3, ch, 12, "buffers'", stats, [&](mcrt_stats* st) {
        const mcrt_matte_buffers d{(uint32_t*)ch[0].dev, (double*)ch[1].dev, (double*)ch[2].dev, (uint32_t*)ch[3].dev};
        const mcrt_aov_buffers da{(double*)ch[4].dev, (double*)ch[5].dev, (double*)ch[6].dev, (double*)ch[7].dev,
                                  (double*)ch[8].dev, (double*)ch[9].dev, (uint32_t*)ch[10].dev, (uint32_t*)ch[11].dev};
        return mcrt_render_matte_device(ctx, cam, global_seed, params, &d, aov ? &da : nullptr, st);
    });
}
