// Launch arguments: the functions that turn a kernel selection (mcrt_select.hpp) and launch geometry (mcrt_plan.hpp) into the structs
// the kernels are launched with. Plain host C++ over values and pointers the caller owns - no HIP call, no mcrt_ctx, no allocation of
// device memory - so that mcrt_hip.hip and the emulated launches of tests/emu fill their arguments with the SAME code.
// Two sections. The first stands alone (WfFrame, FilmView, the photon pass's work split) and is included like any header. The second
// fills the structs of mcrt_kernels.hpp and is, like mcrt_photon_device.hpp, included textually after that header in the scope it was
// included in, with MCRT_LAUNCH_KERNEL_ARGS defined. It names no kernel: kernels are emitted in the order they are first named
// (instanceTable, mcrt_hip.hip).
#ifndef MCRT_LAUNCH_FRAME_SECTION
#define MCRT_LAUNCH_FRAME_SECTION

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/mcrt.h"
#include "mcrt_plan.hpp"
#include "mcrt_wavefront.hpp"

namespace mcrt {

// Film::Film(width, height, json), film.cpp:19-58: the filter's table (empty: no cache; the caller places it) ...
inline std::vector<double> filmCacheTable(const mcrt_camera_desc& cam) {
    std::vector<double> table(cam.film_cache_size);
    for (uint32_t i = 0; i < cam.film_cache_size; i++)
        table[i] = filmFilterFunction(filmViewType(cam.film_filter), (2.0 * (int)i) / (double)(cam.film_cache_size - 1));
    return table;
}
// ... and the view of a frame that splats (filmSplats) into `blob`, [height][width][4]
inline FilmView makeFilmView(const mcrt_camera_desc& cam, const double* cache, double* blob) {
    FilmView f;
    f.type = filmViewType(cam.film_filter);
    f.width = cam.width;
    f.height = cam.height;
    f.radius = cam.film_radius > 0.0 ? cam.film_radius : filmDefaultRadius(cam.film_filter);
    f.two_inv_radius = 2.0 / f.radius;
    f.cache_size = cam.film_cache_size;
    f.cache = f.cache_size ? cache : nullptr;
    f.inv_dx = f.cache_size ? (double)(f.cache_size - 1) / f.radius : 0.0;
    f.blob = blob;
    return f;
}

// The frame part of a WfFrame (film == nullptr: the box filter's per-pixel sums, through `samples`); setWfPass gives it its rows.
inline void fillWfFrame(WfFrame& fr, const mcrt_camera_desc& cam, uint32_t global_seed, const ChunkPlan& cp, double* samples, const FilmView* film,
                        double* iors_deep, uint32_t iors_depth) {
    memset(&fr, 0, sizeof(fr));
    fr.cam = cam;
    fr.global_seed = global_seed;
    fr.spp = cam.sqrtspp * cam.sqrtspp;
    fr.tiles_x = (cam.width + 7) / 8;
    fr.chunk_shift = cp.shift;
    fr.chunk = cp.chunk;
    fr.samples = samples;
    fr.film.type = MCRT_FILM_BOX;
    if (film) fr.film = *film;
    // deep refraction-history rows: [iors_depth - kMaxIors][slots] doubles (never initialised: an entry is written before it is read)
    fr.iors_deep = iors_deep;
    fr.iors_deep_rows = iors_depth - (uint32_t)kMaxIors;
}
inline void setWfPass(WfFrame& fr, uint32_t row_base, uint32_t row_end) {
    fr.row_base = row_base;
    fr.row_end = row_end;
    fr.pass_pixels = (unsigned long long)(row_end - row_base) * fr.cam.width;
    fr.work_items = ((unsigned long long)fr.tiles_x * ((row_end - row_base + 7) / 8) * 64ull) << fr.chunk_shift;
}

// [num_lights][3] emittance * area (photon-mapper.cpp:64)
inline std::vector<double> lightFlux(const mcrt_scene_desc& s) {
    std::vector<double> flux((size_t)s.num_lights * 3);
    for (uint32_t i = 0; i < s.num_lights; i++) {
        const uint32_t ls = s.light_surface[i];
        for (int c = 0; c < 3; c++) flux[(size_t)i * 3 + c] = s.materials[s.surf_material[ls]].emittance[c] * s.surf_area[ls];
    }
    return flux;
}
// The photon pass's work split over the lights, photon-mapper.cpp:31-78: light i emits the paths [first[i], first[i + 1]), each
// photon of it carrying photon_flux[i].
inline void planEmission(const std::vector<double>& flux, double emissions, double caustic_factor, std::vector<unsigned long long>& first,
                         std::vector<double>& photon_flux) {
    const size_t nl = flux.size() / 3, photon_emissions = (size_t)((double)(size_t)emissions * caustic_factor);
    double total_add_flux = 0.0;
    for (size_t i = 0; i < nl; i++) total_add_flux += 0.0 + flux[i * 3] + flux[i * 3 + 1] + flux[i * 3 + 2];  // glm::compAdd
    first.assign(nl + 1, 0ull);
    photon_flux.resize(nl * 3);
    for (size_t i = 0; i < nl; i++) {
        const double* f = &flux[i * 3];
        const double share = (0.0 + f[0] + f[1] + f[2]) / total_add_flux;
        const size_t n = (size_t)((double)photon_emissions * share);
        first[i + 1] = first[i] + n;
        for (int c = 0; c < 3; c++) photon_flux[i * 3 + c] = f[c] / (double)n;
    }
}

}  // namespace mcrt
#endif  // MCRT_LAUNCH_FRAME_SECTION

#if defined(MCRT_LAUNCH_KERNEL_ARGS) && !defined(MCRT_LAUNCH_KERNEL_SECTION)
#define MCRT_LAUNCH_KERNEL_SECTION

// ---- the scene ---------------------------------------------------------------------------------------------------------------------
// Staging plan: whole scene when its LDS image is <= 48 KiB - and the plan of the 512-lane kernels (tables, stacks, histories AND the
// image) fits max_lds: an image of 40-48 KiB did not, and its mcrt_intersect / legacy frames failed until round 4 - else the top 512
// nodes of the BVH; quadric code lives in the kAll == false kernels.
// Tiny scenes: a BVH of a few dozen primitives costs more in wavefront divergence (every lane walks its own node sequence) than it
// saves in tests. With <= flat_max primitives (MCRT_FLAT_MAX, default 64) all lanes test all primitives in one wave-uniform loop, as
// Scene::intersect does without a "bvh" key (scene.cpp:161-173); the closest hit is the same. The flat loop knows triangles and spheres.
inline void planStaging(DeviceScene& d, uint32_t max_lds, uint32_t flat_max, const HostLayout& L) {
    d.stage_all = 1;
    d.stage_nodes = 0;
    const uint32_t fixed = planLds(DeviceScene{}, kBlock).total;
    if (planLds(d, kBlock).total - fixed > 48u * 1024u || planLds(d, kBlock).total > max_lds || L.num_quadric_surfaces) {
        d.stage_all = 0;
        d.stage_nodes = std::min<uint32_t>(d.num_nodes, 512u);
    }
    d.flat = (d.stage_all && d.num_surfaces <= flat_max && !L.flat_prim.empty() && L.num_quadric_surfaces == 0) ? 1u : 0u;
}

// The photon-mapping kernel stages at most 128 nodes of a tree in memory (planMegaLds, sceneFacts).
constexpr uint32_t kPmStageNodes = 128;

// What kernel selection reads of a scene whose staging is planned (mcrt_select.hpp)
inline SceneFacts sceneFacts(const DeviceScene& d, const HostLayout& L, const mcrt_scene_desc& s) {
    SceneFacts facts;
    facts.material_flags = 0u;
    for (uint32_t i = 0; i < s.num_materials; i++) facts.material_flags |= s.materials[i].flags;
    facts.q_single = L.q_single;
    facts.flat = d.flat != 0;
    facts.cull = d.flat_pre != nullptr;
    // (the cull records travel as a kernel argument only when the host copy is what the device's counts say)
    facts.cull_floats = L.flat_pre.size() == (size_t)d.pre_tri_pairs * kTriPairFloats + (size_t)d.pre_sph_pairs * kSphPairFloats ? (uint32_t)L.flat_pre.size() : 0u;
    facts.stage_all = d.stage_all != 0;
    facts.num_nodes = d.num_nodes;
    facts.q_nodes = d.q_nodes;
    DeviceScene pm = d;
    if (!pm.stage_all) pm.stage_nodes = std::min<uint32_t>(pm.stage_nodes, kPmStageNodes);
    for (uint32_t i = 0; i < 8; i++) {
        facts.pm_lds[0][i] = alignUp(planLds(pm, kBlock, true, 2 * (i + 1), kPmLdsIors).total, 16);
        facts.pm_lds[1][i] = alignUp(planLds(pm, 1024u, true, 2 * (i + 1), kPmLdsIors).total, 16);
    }
    facts.pm_lds_full = alignUp(planLds(pm, kBlock, true, kLdsStackDepth, kMaxIors).total, 16);
    return facts;
}

// ---- megakernels -------------------------------------------------------------------------------------------------------------------
inline bool pmWide(const KernelChoice& c) { return c.instance >= kInstPMWide && c.instance <= kInstPMWide_CountAll; }
// (the 1024-lane and the wide instances keep two refraction-history entries per lane in LDS, the deeper ones in memory)
inline bool pmIorsInMemory(const KernelChoice& c) { return c.form == MCRT_KERNEL_PM_WAVE && (c.block == 1024u || pmWide(c)); }

// Dynamic LDS of the megakernel `c` names; shrinks launch_scene.stage_nodes to what that kernel stages of a tree in memory.
inline uint32_t planMegaLds(DeviceScene& launch_scene, const KernelChoice& c, uint32_t max_lds) {
    if (c.form == MCRT_KERNEL_PM_WAVE) {
        if (!launch_scene.stage_all) launch_scene.stage_nodes = std::min<uint32_t>(launch_scene.stage_nodes, kPmStageNodes);
        const uint32_t knn_bytes = waveKnnBytes(pmWide(c) ? kWaveRowsLarge : kWaveRows) + (launch_scene.stage_all ? 0u : kWaveStateBytes);
        return alignUp(planLds(launch_scene, c.block, true, c.stack_depth, pmIorsInMemory(c) ? kPmLdsIors : (uint32_t)kMaxIors).total, 16) + (c.block / 64) * knn_bytes;
    }
    if (c.form == MCRT_KERNEL_LANE_SM) {
        // the staged top of the tree shrinks to what the workgroup's stacks and refraction histories leave
        const uint32_t fixed = planSmLds(DeviceScene{}, c.block, c.stack_depth).total;
        if (!launch_scene.stage_all && fixed < max_lds) launch_scene.stage_nodes = std::min<uint32_t>(launch_scene.stage_nodes, (max_lds - fixed) / 64u);
        return planSmLds(launch_scene, c.block, c.stack_depth).total;
    }
    return planLds(launch_scene, c.block, c.form != MCRT_KERNEL_FLAT).total;  // (the flat loop has no stack in LDS)
}
// Entries of the traversal stacks' spill area: what of a lane's stack_depth entries is not in LDS
inline size_t megaSpillEntries(const DeviceScene& d, const KernelChoice& c, uint32_t total_lanes) {
    const uint32_t in_lds = c.form == MCRT_KERNEL_PM_WAVE ? std::min<uint32_t>(c.stack_depth, kLdsStackDepth) : (uint32_t)kLdsStackDepth;
    return (size_t)total_lanes * (d.stack_depth - in_lds);
}

// The state machine's scheduling thresholds (RenderParams::sm_*, mcrt_lanesm.hpp), at what the measurements left them
constexpr int kSmShadeLanes = 40, kSmRegenLanes = 16, kSmMinTrav = 20, kSmLeafLanes = 32, kSmMinInner = 8;

// The frame part of RenderParams; setRenderPass gives it its rows, setRenderMaps the photon maps.
inline void fillRenderParams(RenderParams& prm, const mcrt_camera_desc& cam, uint32_t global_seed, uint32_t owned_rows, unsigned long long* work_counter,
                             unsigned long long* stats, StackEntry* spill, double* samples, uint32_t total_lanes) {
    memset(&prm, 0, sizeof(prm));
    prm.cam = cam;
    prm.global_seed = global_seed;
    prm.spp = cam.sqrtspp * cam.sqrtspp;
    prm.owned_rows = owned_rows;
    prm.tiles_x = (cam.width + 7) / 8;
    prm.tiles_y = (owned_rows + 7) / 8;
    prm.work_items = (uint64_t)prm.tiles_x * prm.tiles_y * 64ull;
    prm.work_counter = work_counter;
    prm.stats = stats;
    prm.spill = spill;
    prm.samples = samples;
    prm.total_lanes = total_lanes;
    prm.sm_shade_lanes = kSmShadeLanes;
    prm.sm_regen_lanes = kSmRegenLanes;
    prm.sm_min_trav = kSmMinTrav;
    prm.sm_leaf_lanes = kSmLeafLanes;
    prm.sm_min_inner = kSmMinInner;
    prm.sm_lds_depth = kLdsStackDepth;
}
inline void setRenderMaps(RenderParams& prm, const PhotonMapView& global_map, const PhotonMapView& caustic_map, uint32_t k_nearest, int direct_visualization) {
    prm.global_map = global_map;
    prm.caustic_map = caustic_map;
    prm.k_nearest = k_nearest;
    prm.direct_visualization = direct_visualization ? 1u : 0u;
}
// The local rows [row, row + pass_rows) as one launch. Units per pixel: a power of two that gives every resident lane >= 128 units in
// chunks of at least 16 samples (planChunksMega, mcrt_plan.hpp: the measurements behind it); photon-mapped frames keep the short
// chunks: their paths differ far more in cost - a search per diffuse hit - and the balance is worth more than the units' fixed cost
// (C5 at 64 spp 770 ms with 64 units of 4 samples, 791 with 16 of 16). chunks: MCRT_CHUNKS, or -1.
inline void setRenderPass(RenderParams& prm, uint32_t row, uint64_t pass_rows, bool photon, long long chunks = -1) {
    prm.row_base = row;
    prm.row_end = (uint32_t)std::min<uint64_t>(prm.owned_rows, row + pass_rows);
    prm.pass_pixels = (uint64_t)(prm.row_end - prm.row_base) * prm.cam.width;
    const ChunkPlan cp = photon ? planChunks(prm.spp, unitsWanted(prm.total_lanes, 128, prm.pass_pixels, chunks))
                                : planChunksMega(prm.spp, prm.total_lanes, prm.pass_pixels, chunks);
    prm.chunk_shift = cp.shift;
    prm.chunk = cp.chunk;
    const uint64_t tiles = (uint64_t)prm.tiles_x * ((prm.row_end - prm.row_base + 7) / 8);
    prm.work_items = (tiles * 64ull) << cp.shift;
}

// renderKernelPM's own arguments and the sizes of their buffers: estimate requests, one record per resident lane; the searches'
// frontier spill lists, one per wave; refraction histories beyond the LDS part (pmIorsInMemory, else null)
inline size_t pmStageBytes(uint32_t total_lanes) { return (size_t)kStageDoubles * total_lanes * sizeof(double); }
inline size_t pmKnnSpillBytes(uint32_t total_lanes) { return (size_t)(total_lanes / 64) * kWaveSpill * 3 * sizeof(uint32_t); }
inline size_t pmIorsBytes(uint32_t total_lanes) { return (size_t)kMaxIors * total_lanes * sizeof(double); }
inline void fillPmExtra(PmExtra& pmx, const PhotonMapViewW& global_map, const PhotonMapViewW& caustic_map, const KernelChoice& c, double* stage,
                        uint32_t* knn_spill, double* iors_global) {
    pmx.global_map = global_map;
    pmx.caustic_map = caustic_map;
    pmx.stack_depth = c.stack_depth;
    pmx.stage = stage;
    pmx.knn_spill = knn_spill;
    pmx.iors_global = pmIorsInMemory(c) ? iors_global : nullptr;
}

inline void fillEmitParams(EmitParams& prm, uint32_t num_lights, const unsigned long long* light_first, const double* light_photon_flux,
                           unsigned long long first_emission, unsigned long long total_emissions, uint32_t stride, uint32_t global_seed,
                           double caustic_factor, float* const photons[2], unsigned long long* const keys[2], const unsigned long long capacity[2],
                           unsigned long long* counters, StackEntry* spill, uint32_t total_lanes) {
    memset(&prm, 0, sizeof(prm));
    prm.num_lights = num_lights;
    prm.light_first = light_first;
    prm.light_photon_flux = light_photon_flux;
    prm.total_emissions = total_emissions;
    prm.first_emission = first_emission;
    prm.stride = stride;
    prm.global_seed = global_seed;
    prm.non_caustic_reject = 1.0 / caustic_factor;
    for (int w = 0; w < 2; w++) {
        prm.photons[w] = photons[w];
        prm.keys[w] = keys[w];
        prm.capacity[w] = capacity[w];
    }
    prm.counters = counters;
    prm.spill = spill;
    prm.total_lanes = total_lanes;
}

// ---- the pipeline ------------------------------------------------------------------------------------------------------------------
// Control words of the wavefront pipeline, one allocation of kWfCtrlWords wherever it is made: the ray queue's {count[2] (one per
// iteration parity), pop, -}, then the same of the photon mapper's estimate requests. mcrt_intersect uses the first four.
enum : uint32_t { kWfCtrlCount = 0, kWfCtrlPop = 2, kWfCtrlRCount = 4, kWfCtrlRPop = 6, kWfCtrlWords = 8 };

// The trace kernel's launch values that were once A/B switches, at what the measurements left them:
constexpr uint32_t kTraceWaves = 16;       // waves per workgroup, one workgroup per CU
constexpr int kTraceRefillLanes = 16;      // (32 while the queue cursor was one global atomic)
constexpr int kTraceLeafItems = 1 << 20;
constexpr int kTraceMinInner = 8;
constexpr uint32_t kTraceDealShift = 6;
static_assert(kTraceWaves * 64u <= kTraceMaxBlock, "the trace kernel's launch bounds");

// The trace kernel's dynamic LDS: top-of-tree child blocks, the lanes' traversal stacks, the workgroup's queue cursor, the waves'
// shared-leaf maps, the root's record ...
inline uint32_t traceLdsBytes(uint32_t waves, uint32_t lds_stack, uint32_t lds_blocks) {
    return lds_blocks * 64u + lds_stack * waves * 64u * (uint32_t)sizeof(SmStackEntry) + 64u + waves * kShareMapBytes + 64u;
}
// ... with as many blocks as lds_cap leaves room for; false: the stacks alone exceed it
inline bool planTraceLds(uint32_t waves, uint32_t lds_stack, uint64_t lds_cap, uint32_t num_qblocks, uint32_t& lds_blocks) {
    const uint64_t fixed = traceLdsBytes(waves, lds_stack, 0);
    if (fixed > lds_cap) return false;
    lds_blocks = (uint32_t)std::min<uint64_t>(num_qblocks, (lds_cap - fixed) / 64u);
    return true;
}
// count / pop: the ray queue's words of `ctrl` at iteration parity 0 (bindIteration moves count). A spill region holds
// d.stack_depth entries per lane whatever part of them lives in LDS.
// leaf_lanes: MCRT_WF_LEAF, default 16 (shared step, C3 64 spp: 8 / 12 / 16 / 20 pending lanes 412.7 / 402.1 / 398.1 / 402.3 ms;
// gating on 48-56 offered primitives instead: 398.4-399.0)
inline void fillTraceArgs(WfTraceArgs& ta, const DeviceScene& d, unsigned long long* ctrl, unsigned long long* stats, SmStackEntry* spill,
                          uint32_t total_lanes, uint32_t lds_blocks, int leaf_lanes, int lds_stack = kLdsStackDepth,
                          int refill_lanes = kTraceRefillLanes, uint32_t deal_shift = kTraceDealShift) {
    memset(&ta, 0, sizeof(ta));
    ta.count = ctrl + kWfCtrlCount;
    ta.pop = ctrl + kWfCtrlPop;
    ta.stats = stats;
    ta.nodes = d.nodes64;
    ta.qblocks = d.qblocks;
    ta.num_nodes = d.q_nodes;
    ta.lds_blocks = lds_blocks;
    ta.q_root_a = d.q_root_a;
    ta.q_root_m = d.q_root_m;
    ta.prim = d.prim;
    ta.spill = spill;
    ta.total_lanes = total_lanes;
    ta.refill_lanes = refill_lanes;
    ta.leaf_lanes = leaf_lanes;
    ta.leaf_items = kTraceLeafItems;
    ta.min_inner = kTraceMinInner;
    ta.lds_stack = lds_stack;
    ta.max_stack = d.stack_depth;
    ta.deal_shift = deal_shift;
}

// Slot pool and ray queue. The queue has two entries per slot (bounce + shadow ray) and room for the last workgroups' overshoot:
// item and light words, then two sets of eight planes of doubles (WfRayQueue) - a shade launch fills one set and reads the bounce
// rays of its slots back from the other.
constexpr size_t kWfQueueEntryBytes = 2 * sizeof(uint32_t) + 2 * 8 * sizeof(double);
constexpr size_t kWfSlotBytes = (size_t)kWfWords * 8 + 2 * kWfQueueEntryBytes;
inline size_t wfPoolBytes(uint64_t slots) { return (size_t)slots * kWfWords * 8; }
inline size_t wfQueueCap(uint64_t slots) { return ((size_t)slots + 2 * kWfBlock) * 2; }
inline size_t wfQueueBytes(uint64_t slots) { return wfQueueCap(slots) * kWfQueueEntryBytes; }
inline PoolRays bindQueue(unsigned long long* pool, uint32_t* queue, uint64_t slots) {
    PoolRays pr;
    pr.pool.w = pool;
    pr.pool.n = (uint32_t)slots;
    pr.q.cap = wfQueueCap(slots);
    pr.q.item = queue;
    pr.q.light = queue + pr.q.cap;
    pr.q.ray = reinterpret_cast<double*>(queue + 2 * pr.q.cap);  // iteration parity 0 (bindIteration)
    pr.q.prev_ray = pr.q.ray + 8 * pr.q.cap;
    return pr;
}

// One pass's shade launches over the whole pool; + the materials and the light tables in LDS when they are small
inline void fillShadeArgs(WfShadeArgs& sa, const PoolRays& pr, const WfFrame& fr, const DeviceScene& d, unsigned long long* ctrl,
                          unsigned long long* work, unsigned long long* stats) {
    memset(&sa, 0, sizeof(sa));
    sa.pool = pr.pool;
    sa.slot_base = 0u;
    sa.slot_count = pr.pool.n;
    sa.fr = fr;
    sa.queue = pr.q;
    sa.pop_reset = ctrl + kWfCtrlPop;
    sa.work = work;
    sa.stats = stats;
    sa.lds_tables = wfShadeTableBytes(d.num_materials, d.num_lights);
    if (sa.lds_tables > kWfShadeTableMax) sa.lds_tables = 0;
}
inline uint32_t wfShadeLdsBytes(const WfShadeArgs& sa) { return kSobolTableWords * 4u + kMaxIors * kWfBlock * 8u + sa.lds_tables; }

// Photon mapper: the kNN launch that serves the shade launches' estimate requests, and the shade side of it. stage / est: the
// launch evaluates the estimates from staged Interactions (MCRT_WF_PM_EVAL); null: it hands the k photons back through `res`
// (photons and est of it are set here) and the shade launch sums them per lane.
inline void fillKnnArgs(WfKnnArgs& ka, WfShadeArgs& sa, unsigned long long* ctrl, const PhotonMapViewW& global_map, const PhotonMapViewW& caustic_map,
                        uint32_t k, int direct_visualization, uint32_t* requests, double* stage, double* est, uint32_t* spill, uint32_t* res_n = nullptr,
                        double* res_r2 = nullptr, uint32_t* res_idx = nullptr, double* res_d2 = nullptr) {
    memset(&ka, 0, sizeof(ka));
    ka.pool = sa.pool;
    ka.requests = sa.requests = requests;
    ka.pop = sa.rpop_reset = ctrl + kWfCtrlRPop;
    ka.stats = sa.stats;
    ka.maps[0] = global_map;
    ka.maps[1] = caustic_map;
    ka.k = sa.pm.k = k;
    ka.res_n = res_n;
    ka.res_r2 = res_r2;
    ka.res_idx = res_idx;
    ka.res_d2 = res_d2;
    ka.stage = sa.stage = stage;
    ka.est = est;
    ka.spill = spill;
    sa.pm.photons[0] = global_map.base.photons;
    sa.pm.photons[1] = caustic_map.base.photons;
    sa.pm.res_n = res_n;
    sa.pm.res_r2 = res_r2;
    sa.pm.res_idx = res_idx;
    sa.pm.res_d2 = res_d2;
    sa.pm.direct_visualization = direct_visualization != 0;
    sa.pm.est = est;
}
inline size_t wfKnnSpillBytes(uint32_t knn_grid) { return (size_t)knn_grid * (256 / 64) * kWaveSpill * 3 * sizeof(uint32_t); }

// Iteration `it` of a pass: shade(it) counts the rays (and requests) it queues in the words of its parity and clears the other
// parity's, which trace(it - 1) and knn(it - 1) consumed; the ray planes alternate the same way.
inline void bindIteration(uint64_t it, unsigned long long* ctrl, WfShadeArgs& sa, WfTraceArgs& ta, WfKnnArgs& ka, PoolRays& pr) {
    const uint32_t now = (uint32_t)(it & 1), other = now ^ 1u;
    double* const set0 = reinterpret_cast<double*>(pr.q.item + 2 * pr.q.cap);
    pr.q.ray = set0 + now * 8 * pr.q.cap;
    pr.q.prev_ray = set0 + other * 8 * pr.q.cap;
    sa.queue = pr.q;
    sa.count_out = ctrl + kWfCtrlCount + now;
    sa.count_reset = ctrl + kWfCtrlCount + other;
    ta.count = sa.count_out;
    if (sa.requests) {
        sa.rcount_out = ctrl + kWfCtrlRCount + now;
        sa.rcount_reset = ctrl + kWfCtrlRCount + other;
        ka.count = sa.rcount_out;
    }
}

// ---- mcrt_bsdf ---------------------------------------------------------------------------------------------------------------------
// bsdfKernel's constants from the ABI's consts[10] = roughness, reflectance[3], complex IOR real[3], imaginary[3]: the Oren-Nayar
// material as Material::computeProperties leaves it (material/material.cpp:99,106-108) - rough only above C::EPSILON, Lambertian below.
inline void fillBsdfKatConsts(BsdfKatConsts& c, const double* consts) {
    memset(&c, 0, sizeof(c));
    c.rough.roughness = consts[0];
    for (int k = 0; k < 3; k++) {
        c.rough.reflectance[k] = consts[1 + k];
        c.real[k] = consts[4 + k];
        c.imag[k] = consts[7 + k];
    }
    const double variance = c.rough.roughness * c.rough.roughness;
    c.rough.A = 1.0 - 0.5 * (variance / (variance + 0.33));
    c.rough.B = 0.45 * (variance / (variance + 0.09));
    c.rough.flags = c.rough.roughness > kEpsilon ? MCRT_MAT_ROUGH : 0u;
}
// bsdfKernel's workgroups of 256 lanes: past 2048 of them the lanes stride over the vectors
inline uint32_t bsdfGrid(uint64_t n) { return (uint32_t)std::min<uint64_t>(2048, (n + 255) / 256); }

#endif  // MCRT_LAUNCH_KERNEL_ARGS
