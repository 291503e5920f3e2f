// First-hit AOV pass (include/mcrt.h mcrt_render_aov*), host side: chunking, scratch, the closest-hit search mcrt_intersect already has
// (intersectDeviceArrays, mcrt_hip.hip) between the two launches of csrc/mcrt_aov.hip, statistics, and the host-pointer form. No kernel
// here: the pass's two kernels are a code object of their own (libmcrt_aov.so, csrc/mcrt_aov.hip), so that the device code of
// libmcrt_hip.so - the render path's, listed function by function in tests/golden/device_code_hashes.json - is exactly what it was.
// Scratch per ray: 48 B of ray + 28 B of hit = 76 B, kept in the context and grown on demand (2^24 rays per chunk by default = 1.2 GiB;
// option MCRT_AOV_CHUNK_RAYS).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "mcrt_aov.hpp"
#include "mcrt_aov_launch.hpp"
#include "mcrt_internal.hpp"

using namespace mcrt;

namespace {

constexpr uint64_t kAovDefaultChunkRays = 1ull << 24;
constexpr uint64_t kAovMaxChunkRays = 0xFFF00000ull;  // mcrt_intersect's queue limit (32-bit cursors)

#define AOV_HIP_TRY(ctx, call)                                                                               \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return ctxFail(ctx, MCRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Events {  // the pass's own pair: the context's belong to renders and to the operators' timing option
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

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

}  // namespace

extern "C" int mcrt_render_aov_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_aov_buffers* buffers,
                                      mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxAovReady(ctx, "mcrt_render_aov_device")) return rc;
    if (int rc = validate(ctx, cam, buffers, "mcrt_render_aov_device")) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    const uint64_t total_pixels = (uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width;
    // a chunk is a whole number of pixels, at least one, and never more rays than one closest-hit launch takes
    const long want = ctxOptL(ctx, "MCRT_AOV_CHUNK_RAYS", (long)kAovDefaultChunkRays);
    const uint64_t chunk_rays = std::min<uint64_t>(want > 0 ? (uint64_t)want : kAovDefaultChunkRays, kAovMaxChunkRays);
    const uint64_t chunk_pixels = std::min<uint64_t>(std::max<uint64_t>(chunk_rays / spp, 1), std::max<uint64_t>(total_pixels, 1));
    const uint64_t max_rays = chunk_pixels * spp;

    AovRays rays;
    rays.start = (double*)ctxAovScratch(ctx, 0, max_rays * 24);
    rays.direction = (double*)ctxAovScratch(ctx, 1, max_rays * 24);
    rays.t = (double*)ctxAovScratch(ctx, 2, max_rays * 8);
    rays.surface = (uint32_t*)ctxAovScratch(ctx, 3, max_rays * 4);
    rays.uv = (double*)ctxAovScratch(ctx, 4, max_rays * 16);
    if (!rays.start || !rays.direction || !rays.t || !rays.surface || !rays.uv)
        return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_render_aov_device: " + std::to_string((max_rays * 76) >> 20) +
                                              " MiB of ray scratch could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
    AovScene scene;
    const uint32_t* sobol_tab = nullptr;
    ctxAovScene(ctx, &scene, &sobol_tab);

    Events ev;
    AOV_HIP_TRY(ctx, hipEventCreate(&ev.e0));
    AOV_HIP_TRY(ctx, hipEventCreate(&ev.e1));
    AOV_HIP_TRY(ctx, hipEventRecord(ev.e0, stream));
    uint32_t launches = 0;
    for (uint64_t first = 0; first < total_pixels; first += chunk_pixels) {
        AovChunk c;
        c.cam = *cam;
        c.global_seed = global_seed;
        c.spp = spp;
        c.first_pixel = first;
        c.pixels = (uint32_t)std::min<uint64_t>(chunk_pixels, total_pixels - first);
        const uint64_t n = (uint64_t)c.pixels * spp;
        AOV_HIP_TRY(ctx, (hipError_t)launchAovRays(stream, c, scene.sh.scene_ior, sobol_tab, rays));
        if (int rc = intersectDeviceArrays(ctx, n, rays.start, rays.direction, rays.t, rays.surface, rays.uv)) return rc;
        AOV_HIP_TRY(ctx, (hipError_t)launchAovResolve(stream, c, scene, rays, *buffers));
        launches += 3;
    }
    AOV_HIP_TRY(ctx, hipEventRecord(ev.e1, stream));
    AOV_HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (stats) {
        float ms = 0.f;
        AOV_HIP_TRY(ctx, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        memset(stats, 0, sizeof(*stats));
        stats->paths = stats->rays = total_pixels * spp;
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        stats->kernel_launches = launches;
        stats->kernel_id = MCRT_KERNEL_NONE;  // (names the integrator's kernel form: none ran)
    }
    return MCRT_OK;
}

extern "C" int mcrt_render_aov(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_aov_buffers* buffers,
                               mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxAovReady(ctx, "mcrt_render_aov")) return rc;
    if (int rc = validate(ctx, cam, buffers, "mcrt_render_aov")) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    const uint32_t rows = mcrt_shard_rows(cam, nullptr);
    const size_t pixels = (size_t)rows * cam->width;
    // the requested channels as one device allocation, in units of 8 bytes per pixel: depth, position, normal, shading normal, albedo,
    // coverage, then the two id channels (4 bytes per pixel each) in a word of their own
    struct Channel {
        void* host;
        size_t elem, per_pixel;
        void** dev;
    };
    mcrt_aov_buffers d{};
    const Channel ch[8] = {{buffers->depth, 8, 1, (void**)&d.depth},
                           {buffers->position, 8, 3, (void**)&d.position},
                           {buffers->normal, 8, 3, (void**)&d.normal},
                           {buffers->shading_normal, 8, 3, (void**)&d.shading_normal},
                           {buffers->albedo, 8, 3, (void**)&d.albedo},
                           {buffers->coverage, 8, 1, (void**)&d.coverage},
                           {buffers->surface, 4, 1, (void**)&d.surface},
                           {buffers->material, 4, 1, (void**)&d.material}};
    size_t bytes = 0;
    for (const Channel& c : ch)
        if (c.host) bytes += (pixels * c.elem * c.per_pixel + 7) / 8 * 8;
    unsigned char* base = (unsigned char*)ctxAovScratch(ctx, 5, bytes);
    if (!base) return ctxFail(ctx, MCRT_ERR_HIP, "mcrt_render_aov: the channels' device copy could not be allocated");
    size_t off = 0;
    for (const Channel& c : ch)
        if (c.host) {
            *c.dev = base + off;
            off += (pixels * c.elem * c.per_pixel + 7) / 8 * 8;
        }
    mcrt_stats st;
    if (int rc = mcrt_render_aov_device(ctx, cam, global_seed, &d, &st)) return rc;
    if (rows) {
        std::vector<uint32_t> idx(rows);
        mcrt_shard_rows(cam, idx.data());
        std::vector<unsigned char> packed;
        for (const Channel& c : ch)
            if (c.host) {
                const size_t row_bytes = (size_t)cam->width * c.elem * c.per_pixel;
                packed.resize(rows * row_bytes);
                AOV_HIP_TRY(ctx, hipMemcpy(packed.data(), *c.dev, packed.size(), hipMemcpyDeviceToHost));
                for (uint32_t r = 0; r < rows; r++) memcpy((unsigned char*)c.host + (size_t)idx[r] * row_bytes, &packed[(size_t)r * row_bytes], row_bytes);
            }
    }
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = st;
    return MCRT_OK;
}
