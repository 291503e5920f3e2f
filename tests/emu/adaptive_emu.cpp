// tests/emu/adaptive_emu.cpp — TEST HARNESS ONLY (built by tests/test_adaptive_emulation.py into tests/emu/_build/).
//
// Adaptive sampling on the host: csrc/mcrt_adaptive.hpp (and csrc/mcrt_light_groups.hpp, csrc/mcrt_aov.hpp, csrc/mcrt_shade.hpp below it)
// unchanged - the text the kernels of csrc/mcrt_adaptive.hip run - driven batch by batch, chunk by chunk and iteration by iteration the way
// mcrt_render_adaptive_device drives them (mcrt_emu.cpp's chunk plan, the closest hits from the emulation's sceneIntersect). The rule is
// a loop over its lanes; the three launches of the list run workgroup by workgroup on wave_emu.hpp's emulated workgroup (4 wavefronts of
// 64 fibers, ballots served from a snapshot of the wave, __syncthreads a rendezvous of all of them), their LDS arrays here; the default
// floor comes from frameNoiseBlock (csrc/mcrt_pixel_stats.hpp) on the same workgroup. Not a CPU fallback: nothing in the product links
// or loads it.
#define MCRT_WAVE_EMU 1
#include "wave_emu.hpp"

#include "mcrt_emu.cpp"

#include "live_paths_emu.hpp"

#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_adaptive.hpp"
#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_pixel_stats.hpp"

namespace {

// adaptiveCountKernel, adaptiveScanKernel, adaptiveScatterKernel: the list of the set flags and its length.
uint32_t emuCompact(const uint8_t* flags, uint64_t pixels, uint32_t* list) {
    static uint32_t wave_sums[kAdaptiveWaves], sums[2 * kAdaptiveBlock];
    const uint32_t blocks = adaptiveBlocks(pixels);
    std::vector<uint32_t> block_counts(blocks, 0xABABABABu), offsets(blocks, 0xABABABABu);
    uint32_t length = 0xABABABABu;
    wemu::launch().block_dim = kAdaptiveBlock;
    wemu::launch().grid_dim = blocks;
    for (uint32_t b = 0; b < blocks; b++) {
        wemu::launch().block_idx = b;
        for (uint32_t w = 0; w < kAdaptiveWaves; w++) wave_sums[w] = 0xABABABABu;
        wemu::runGroup(kAdaptiveWaves, [&](int tid) { adaptiveCountBlock(flags, pixels, b, (uint32_t)tid, wave_sums, block_counts.data()); });
    }
    wemu::launch().block_idx = 0;
    wemu::launch().grid_dim = 1;
    for (uint32_t k = 0; k < 2 * kAdaptiveBlock; k++) sums[k] = 0xABABABABu;
    wemu::runGroup(kAdaptiveWaves, [&](int tid) { adaptiveScanBlocks(block_counts.data(), blocks, (uint32_t)tid, sums, offsets.data(), &length); });
    wemu::launch().grid_dim = blocks;
    for (uint32_t b = 0; b < blocks; b++) {
        wemu::launch().block_idx = b;
        for (uint32_t w = 0; w < kAdaptiveWaves; w++) wave_sums[w] = 0xABABABABu;
        wemu::runGroup(kAdaptiveWaves, [&](int tid) { adaptiveScatterBlock(flags, pixels, b, (uint32_t)tid, wave_sums, offsets.data(), list); });
    }
    return length;
}

// mcrt_frame_noise_device's signal of a frame (the treesum of r r + g g + b b).
double emuSignal(uint64_t pixels, uint32_t spp, const double* rgb, const double* variance) {
    static double te[kFrameNoiseBlock], tg[kFrameNoiseBlock];
    std::vector<double> buf[2];
    buf[0].resize(frameNoiseBlocks(pixels) * 2);
    buf[1].resize(frameNoiseBlocks(frameNoiseBlocks(pixels)) * 2);
    FrameNoiseLevel lv{};
    lv.rgb = rgb;
    lv.variance = variance;
    lv.spp = (double)spp;
    lv.n = pixels;
    int which = 0;
    for (;;) {
        const uint64_t blocks = frameNoiseBlocks(lv.n);
        lv.out_e = buf[which].data();
        lv.out_g = buf[which].data() + blocks;
        for (uint64_t b = 0; b < blocks; b++) {
            wemu::launch().block_dim = kFrameNoiseBlock;
            wemu::runGroup(kFrameNoiseBlock / 64, [&](int tid) { frameNoiseBlock(lv, b, (uint32_t)tid, te, tg); });
        }
        if (blocks == 1) break;
        lv.rgb = lv.variance = nullptr;
        lv.in_e = lv.out_e;
        lv.in_g = lv.out_g;
        lv.n = blocks;
        which ^= 1;
    }
    return buf[which][1];
}

// The walk of one batch over `listed` entries of `list`, in chunks of chunk_rays slots (0 = one chunk): the camera rays with the pixel
// taken from the list and the seed from f_count (the counts that number a pixel's batches), the light groups' walk with one plane over
// live_paths_emu.hpp's loop (lists as they are, no depth cut), adaptiveResolvePixel into `f`.
int emuWalk(const mcrt_scene_desc* scene, const Emu& E, const AovScene& as, const mcrt_camera_desc* cam, uint32_t seed, int stage_lds, uint64_t chunk_rays,
            const uint32_t* list, uint32_t listed, const AdaptiveFrame& f, const uint32_t* f_count, uint64_t* info) {
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    const PixelChunks plan = pixelChunks(listed, spp, (uint64_t)spp * 2, chunk_rays, (uint64_t)listed * spp * 2);
    const uint64_t max_n = plan.max_rays;
    std::vector<double> state((max_n * kLgStateBytes + 7) / 8), radiance(max_n * 3);
    std::vector<uint8_t> plane(std::max<uint32_t>(scene->num_surfaces, 1u), 0);
    LgState st;
    lgPlaceState(st, state.data(), max_n);
    st.radiance = radiance.data();
    LgParams par;
    par.plane = plane.data();
    par.planes = 1u;
    par.sky_plane = 0u;
    par.max_depth = 0u;
    EmuLivePaths paths(scene, stage_lds, plan.max_slots, 0, 0u);
    for (uint64_t first = 0; first < plan.total_pixels; first += plan.chunk_pixels) {
        AdaptiveChunk c;
        static_cast<AovChunk&>(c) = chunkAt(*cam, seed, plan.spp, first, plan.chunk_pixels, plan.total_pixels);
        c.list = list;
        c.count = f_count;
        for (uint32_t p = 0; p < c.pixels; p++)  // adaptiveCameraRayKernel
            adaptiveCameraRays<true>(c, E.sh_top.scene_ior, p, E.tab.data(), st.ray.start, st.ray.direction);
        if (int rc = emu_intersect(scene, (uint64_t)c.pixels * c.spp, st.ray.start, st.ray.direction, stage_lds, st.ray.t, st.ray.surface, st.ray.uv)) return rc;
        const int rc = paths.run(
            c, [&](const AdaptiveChunk&, uint64_t s) { return lgBegin(st, s, as.sh.scene_ior, par); },  // adaptiveBeginKernel
            [&](const AdaptiveChunk& c_, const uint32_t* live, uint32_t alive, uint32_t j, uint32_t k, const AovRays& lit, RefractionHistory& rh) {
                lgRays(c_, as, st, live, alive, j, k, lit, rh, E.tab.data());  // adaptiveRayKernel
            },
            [&](const AdaptiveChunk& c_, const uint32_t* live, uint32_t alive, uint32_t j, uint32_t k, bool last, const AovRays& lit, RefractionHistory& rh, bool& too_deep) {
                return lgStep(c_, as, st, par, live, alive, j, k, last, lit, rh, too_deep, E.tab.data());  // adaptiveStepKernel
            },
            [&](const AdaptiveChunk& c_, uint32_t p) { adaptiveResolvePixel(c_, st, p, f); });  // adaptiveResolveKernel
        if (rc) return rc;
        if (info) info[1] += 1;
    }
    if (info) info[0] += paths.rays;
    return 0;
}

}  // namespace

extern "C" {

// The list of the set flags (ascending) and its length, by the three launches. list: `pixels` words.
uint32_t adaptive_emu_compact(const uint8_t* flags, uint64_t pixels, uint32_t* list) { return emuCompact(flags, pixels, list); }

// adaptiveFlagKernel on given accumulators: flags[q] for every pixel of a width x height frame. t2, f2: target and floor, squared.
void adaptive_emu_flags(const double* rgb, const double* variance, const uint32_t* count, uint32_t width, uint32_t height, double t2, double f2, uint32_t n,
                        uint32_t max_spp, uint32_t window, uint32_t force, uint8_t* flags) {
    const AdaptiveFrame f{(double*)rgb, (double*)variance, nullptr, nullptr, (uint32_t*)count};
    const AdaptiveRule rule{t2, f2, width, height, n, max_spp, window, force};
    const uint64_t pixels = (uint64_t)width * height;
    for (uint64_t q = 0; q < pixels; q++) flags[q] = adaptiveListed(f, rule, q) ? 1 : 0;
}

// What the calls refuse about the parameters: the status, and the settings they resolve to in out[0 .. 4] = target, floor (-1: derived
// from the frame), max_spp, min_batches, window.
int adaptive_emu_settings(const mcrt_adaptive_params* params, uint32_t sqrtspp, double* out) {
    AdaptiveSettings s{};
    const char* why = nullptr;
    const int rc = adaptiveSettings(params, sqrtspp, s, &why);
    if (rc == 0 && out) out[0] = s.target, out[1] = s.floor, out[2] = s.max_spp, out[3] = s.min_batches, out[4] = s.window;
    return rc;
}

// mcrt_render_adaptive_device. full_form: what a batch whose list is the whole frame does - 0 the walk into the accumulators like every
// other batch, 1 the walk into batch FRAMES (the summaries mcrt_render_pixel_stats_device delivers) and adaptiveMergeKernel from
// there. chunk_rays: the slots of a chunk of a list (0 = one chunk). Outputs [pixels]...; active: MCRT_CONVERGE_TRACE words;
// info: [0] rays handed to the search, [1] chunks walked, [2] batches, [3] the floor as bits of a double.
int adaptive_emu_render(const mcrt_scene_desc* scene, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_adaptive_params* params, int stage_lds,
                        uint64_t chunk_rays, int full_form, double* rgb, double* variance, double* half_a, double* half_b, uint32_t* count, uint32_t* active,
                        uint64_t* info) {
    if (!scene || !cam || !rgb || !variance || !half_a || !half_b || !count) return MCRT_ERR_INVALID;
    if (cam->width == 0 || cam->height == 0) return MCRT_ERR_INVALID;
    AdaptiveSettings s{};
    const char* why = nullptr;
    if (int rc = adaptiveSettings(params, cam->sqrtspp, s, &why)) return rc;
    if (cam->shard_count > 1 || filmSplats(cam->film_filter, cam->film_radius)) return MCRT_ERR_UNSUPPORTED;
    Emu E;
    if (int rc = setup(E, scene, 0)) return rc;
    const AovScene as = aovSceneOf(E);
    const uint64_t pixels = (uint64_t)cam->width * cam->height;
    const uint32_t n = cam->sqrtspp * cam->sqrtspp;
    const AdaptiveFrame acc{rgb, variance, half_a, half_b, count};
    for (uint64_t q = 0; q < pixels; q++) count[q] = 0;
    std::vector<double> batch_frames(12 * pixels);
    std::vector<uint32_t> batch_count(pixels), list(pixels);
    std::vector<uint8_t> flags(pixels);
    AdaptiveRule rule{s.target * s.target, s.floor < 0.0 ? 0.0 : s.floor * s.floor, cam->width, cam->height, n, s.max_spp, s.window, 0u};
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (active)
        for (uint32_t j = 0; j < MCRT_CONVERGE_TRACE; j++) active[j] = 0;
    bool uniform = true;
    for (uint32_t j = 0;; j++) {
        rule.force = j < s.min_batches || s.target == 0.0 ? 1u : 0u;
        for (uint64_t q = 0; q < pixels; q++) flags[q] = adaptiveListed(acc, rule, q) ? 1 : 0;  // adaptiveFlagKernel
        std::fill(list.begin(), list.end(), 0xABABABABu);
        const uint32_t listed = emuCompact(flags.data(), pixels, list.data());
        if (listed > pixels) return MCRT_ERR_HIP;
        if (listed == 0u) break;
        if (active && j < MCRT_CONVERGE_TRACE) active[j] = listed;
        const bool rendered = listed == pixels && uniform && full_form == 1;
        uniform = uniform && listed == pixels;
        if (rendered) {
            const AdaptiveFrame bat{batch_frames.data(), batch_frames.data() + 3 * pixels, batch_frames.data() + 6 * pixels, batch_frames.data() + 9 * pixels, batch_count.data()};
            std::fill(batch_count.begin(), batch_count.end(), 0u);
            if (int rc = emuWalk(scene, E, as, cam, global_seed, stage_lds, chunk_rays, list.data(), listed, bat, count, info)) return rc;
            for (uint64_t q = 0; q < pixels; q++) adaptiveMergeFramePixel(acc, bat, q, n);  // adaptiveMergeKernel
        } else if (int rc = emuWalk(scene, E, as, cam, global_seed, stage_lds, chunk_rays, list.data(), listed, acc, count, info)) {
            return rc;
        }
        if (info) info[2] = j + 1;
        if (j == 0 && s.floor < 0.0) {
            const double floor = adaptiveDefaultFloor(emuSignal(pixels, n, rgb, variance), pixels);
            rule.f2 = floor * floor;
            if (info) memcpy(&info[3], &floor, 8);
        }
    }
    if (s.floor >= 0.0 && info) memcpy(&info[3], &s.floor, 8);
    return 0;
}

}  // extern "C"
