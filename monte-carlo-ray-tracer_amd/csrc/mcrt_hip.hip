// libmcrt_hip.so — host side of the gfx950 library: context, scene / photon-map upload, kernel selection and launches
// (megakernels and the wavefront frame loop), and the C ABI of include/mcrt.h. The kernels are in mcrt_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mcrt.h"
#include "mcrt_integrator.hpp"
#include "mcrt_lanesm.hpp"
#include "mcrt_qbvh.hpp"
#include "mcrt_wavefront.hpp"
#include "mcrt_waveknn.hpp"
#include "mcrt_groupknn.hpp"
#include "mcrt_widerec.hpp"
#include "mcrt_layout.hpp"
#include "mcrt_internal.hpp"
#include "mcrt_aov.hpp"
#include "mcrt_plan.hpp"
#include "mcrt_select.hpp"
#include "mcrt_stats_readout.hpp"
#include "mcrt_launch.hpp"
#include "mcrt_octree_shared.hpp"
#include "mcrt_lean.hpp"
#include "mcrt_pixel_stats_launch.hpp"
#include "mcrt_robust_launch.hpp"
#include "mcrt_summary_channels.hpp"

#include <hipcub/hipcub.hpp>

extern char** environ;

using namespace mcrt;

namespace {
#include "mcrt_kernels.hpp"
#define MCRT_LAUNCH_KERNEL_ARGS  // the builders of the kernels' arguments, in this scope
#include "mcrt_launch.hpp"

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
std::string g_create_error;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t alloc(size_t n) {
        release();
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        else p = nullptr;
        return e;
    }
    // grow-only: keeps the allocation when it is already large enough (the operator-level entry points' scratch)
    hipError_t reserve(size_t n) { return n <= bytes ? hipSuccess : alloc(n); }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// Work buffers that keep their allocation between calls: take() hands out the next buffer of the pool (the k-th take of a call
// gets the buffer the k-th take of the previous call got), rewind() starts a call.
struct DevPool {
    std::vector<std::unique_ptr<DevBuf>> bufs;
    size_t next = 0;
    void rewind() { next = 0; }
    DevBuf& take() {
        if (next == bufs.size()) bufs.emplace_back(new DevBuf());
        return *bufs[next++];
    }
};

}  // namespace

struct mcrt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string error;
    int num_cus = 0;
    size_t max_lds = 0;        // dynamic LDS a kernel that shades may ask for
    size_t max_lds_trace = 0;  // ... a kernel that only walks the tree (no static LDS)

    bool has_scene = false;
    SceneFacts facts;  // what kernel selection reads of the uploaded scene (mcrt_select.hpp)
    std::vector<float> flat_pre_host;  // the flat loop's cull records, host copy: renderKernelFlatK takes them as a kernel argument
    DeviceScene scene{};
    DevBuf node_bounds, node_meta, nodes64, qblocks, quadrics, prim, flat_prim, flat_index, flat_pre, surf_v, surf_normal, surf_rec, surf_vn, surf_area, surf_material, surf_kind, materials,
        light_surface, light_cdf, sobol_tab;

    bool has_photons = false;
    PhotonMapView maps[2]{};
    DevBuf knn_spill;  // frontier spill lists of the wave-cooperative searches (mcrt_waveknn.hpp)
    DevBuf map_bounds[2], map_start[2], map_contained[2], map_next[2], map_leaf[2], map_photons[2], map_children[2], map_pos[2];
    const WideRec* map_children_ptr[2] = {nullptr, nullptr};
    uint32_t map_root_a[2] = {0, 0}, map_root_m[2] = {0, 0};
    uint32_t k_nearest = 50;
    int direct_visualization = 0;

    DevBuf samples;  // per-sample radiance of a pass of the chunked integrator kernels (RenderParams::samples)
    DevBuf work_counter, stats, spill, knn_res_d2, knn_res_idx, knn_visit_d2, knn_visit_oct, out_tmp;
    size_t spill_bytes = 0;
    uint32_t knn_lanes = 0, knn_k = 0;
    // per-lane photon search (the kernel of k > 768 and of MCRT_KERNEL=legacy): frontier entries per lane, grown - frame rendered again,
    // operator call repeated - when a search ran out (KnnScratch::max_visit); force_pm_lane: a photon-mapped frame whose wave-cooperative
    // searches overflowed THEIR frontier (128 register entries + a 1 024-entry list per wave) is rendered again by the per-lane kernel
    uint32_t knn_visit_cap = kMaxVisit, knn_visit_alloc = 0;
    bool force_pm_lane = false;

    // scratch of the operator-level entry points (mcrt_intersect / mcrt_knn / mcrt_sampler / mcrt_bsdf): kept between calls, grown
    // on demand, so that a host that only wants traversal or k-NN does not pay five hipMalloc / hipFree pairs per call
    DevBuf op_buf[6];
    // scratch of the image passes (mcrt_pass_host.hpp: AOV, a-trous filter, sample statistics, firefly suppression), grown on demand too:
    // every (family, slot) a buffer of its own (ctxPassScratch)
    DevBuf pass_buf[mcrt::kPassFamilies][mcrt::kPassSlots];
    // the channels of the per-sample summary wanted from the renders of this context (ctxSampleTargetsBegin: set for the length of a call, so that
    // a frame mcrt_render_finish renders again fills them again): packed like the frame, rgb not used; all nullptr = none, nothing in a render changes
    mcrt_frame_summary sample_targets{};
    mcrt_lens_desc lens{};  // mcrt_set_lens ("Camera models"): model MCRT_LENS_NONE = none set
    mcrt_ray_source_desc ray_source{};  // mcrt_set_ray_source ("Ray sources"): kind MCRT_RAY_SOURCE_NONE = none set
    DevBuf ray_source_owned[2];         // mcrt_set_ray_source_host: the arrays' device copies, freed at the next set or with the context
    std::map<std::string, std::string> options;  // mcrt_set_option; seeded from the MCRT_* environment variables at mcrt_create
    DevBuf pm_iors;  // refraction histories of the 1024-lane photon-mapping kernel
    // the frame in flight, kept so that mcrt_render_finish can run it again through the wavefront pipeline (deep refraction histories)
    mcrt_camera_desc last_cam;
    uint32_t last_seed = 0;
    int last_integrator = 0;
    double* last_out = nullptr;
    double* last_film = nullptr;
    hipStream_t last_stream = nullptr;
    bool force_wf = false;
    bool lean_used = false;  // the last launch (frame, photon pass) ran a lean instance: mcrt_get_option("MCRT_LEAN_USED")
    // ... and which instances (mcrt_select.hpp: RenderInstance) it ran - the frame's (pipeline: its shade kernel; photon pass: the emission
    // kernel), the pipeline's trace and kNN kernels: mcrt_get_option("MCRT_INSTANCES_USED"), and what mcrt_render_finish reads out
    int used_instance = mcrt::kInstNone, used_trace = mcrt::kInstNone, used_knn = mcrt::kInstNone;
    std::string used_text = "-,-,-";
    uint32_t iors_depth = kMaxIorsDeep;  // RefractionHistory entries per pipeline slot (8 in LDS + deep rows); grows when a frame nests deeper
    DevBuf wf_iors_deep;
    DevPool pass_pool;  // work buffers of the device photon pass (mcrt_photon_device.hpp)
    DevBuf pm_stage; // estimate requests of the photon-mapping kernel, one record per resident lane (mcrt_waveknn.hpp)

    // photon emission pass
    std::vector<double> host_light_flux;  // [num_lights][3] emittance * area (photon-mapper.cpp:64)
    DevBuf emit_first, emit_flux, emit_counters, emit_photons[2], emit_keys[2];
    std::vector<float> host_photons[2];
    std::vector<uint64_t> host_keys[2];

    // wavefront path tracer: slot pool, ray queue, control words {count[2], pop}, pinned read-back word
    DevBuf wf_pool, wf_queue, wf_ctrl, wf_film, wf_film_cache, wf_requests, wf_res_n, wf_res_r2, wf_res_idx, wf_res_d2, wf_stage, wf_est;
    uint32_t wf_slots = 0;
    unsigned long long* wf_host = nullptr;   // pinned: one read-back word per half

    // in-flight render
    bool pending = false;
    std::chrono::steady_clock::time_point t_begin;
    uint32_t launches = 0;
    uint32_t kernel_id = MCRT_KERNEL_NONE;  // kernel form of the last render (mcrt_stats.kernel_id)
    bool dense_cell_refused = false;        // buildMapOnDevice: the 21-level cell codes could not separate a leaf's worth of photons
};

namespace {

int fail(mcrt_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->error = msg;
    else g_create_error = msg;
    return code;
}

#define HIP_TRY(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(ctx, MCRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));      \
    } while (0)

int planSampleStore(mcrt_ctx* ctx, double store_gb, uint32_t width, uint32_t owned_rows, uint32_t spp, PassPlan& pp);  // below

template <class T>
int uploadArray(mcrt_ctx* ctx, DevBuf& buf, const T* host, size_t count) {
    HIP_TRY(ctx, buf.alloc(count * sizeof(T)));
    if (count) HIP_TRY(ctx, hipMemcpy(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return MCRT_OK;
}


template <class T>
int uploadInto(mcrt_ctx* ctx, DevBuf& buf, const T* host, size_t count) {  // like uploadArray, into a grow-only buffer
    HIP_TRY(ctx, buf.reserve(std::max<size_t>(count * sizeof(T), 1)));
    if (count) HIP_TRY(ctx, hipMemcpy(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return MCRT_OK;
}

// Operator-level entry points and the emission pass share the context's stats buffer, events and scratch with a render:
// they are refused while one is in flight.
#define REJECT_IF_PENDING(ctx, what)                                                                                  \
    do {                                                                                                              \
        if ((ctx)->pending) return fail(ctx, MCRT_ERR_INVALID, what ": a render is in flight, call mcrt_render_finish first"); \
    } while (0)

struct LaunchGeom {
    uint32_t grid, lds_bytes, total_lanes, block = kBlock;
};

// Sizes `kernel`'s dynamic LDS and asks how many of its workgroups a CU holds: g.grid = that x the CUs. hipFuncSetAttribute is state of
// the kernel FUNCTION, shared by every context of the process: a frame's launches call this under the device mutex of launchRender
// (DeviceOrder's comment).
int occupancyGrid(mcrt_ctx* ctx, const void* kernel, uint32_t block, uint32_t lds_bytes, LaunchGeom& g) {
    HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    int per_cu = 0;
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)block, lds_bytes));
    if (per_cu < 1) per_cu = 1;
    g.block = block;
    g.lds_bytes = lds_bytes;
    g.grid = (uint32_t)(per_cu * ctx->num_cus);
    g.total_lanes = g.grid * block;
    return MCRT_OK;
}

// ... of a kernel with the 512-lane plan of the wave-synchronous code (the emission pass, mcrt_intersect of a staged scene)
template <class K>
int launchGeometry(mcrt_ctx* ctx, K kernel, const DeviceScene& s, LaunchGeom& g) {
    const uint32_t lds_bytes = planLds(s, kBlock).total;
    if (lds_bytes > ctx->max_lds) return fail(ctx, MCRT_ERR_INVALID, "LDS plan exceeds the device limit");
    return occupancyGrid(ctx, reinterpret_cast<const void*>(kernel), kBlock, lds_bytes, g);
}

int ensureSpill(mcrt_ctx* ctx, size_t bytes) {  // traversal-stack spill area, shared by every kernel (one render at a time)
    if (ctx->spill_bytes < bytes) {
        if (ctx->spill.alloc(bytes) != hipSuccess) {
            (void)hipGetLastError();
            ctx->spill_bytes = 0;
            return fail(ctx, MCRT_ERR_UNSUPPORTED, "the traversal stacks of this tree (" + std::to_string(ctx->scene.stack_depth) + " entries per ray: a depth-first walk may hold that many "
                                                   "pending nodes) need " + std::to_string(bytes >> 20) + " MiB of device memory, which could not be allocated");
        }
        ctx->spill_bytes = bytes;
    }
    return MCRT_OK;
}

int ensureScratch(mcrt_ctx* ctx, uint32_t total_lanes, bool photon) {
    if (!ctx->work_counter.p) HIP_TRY(ctx, ctx->work_counter.alloc(sizeof(unsigned long long)));
    if (!ctx->stats.p) HIP_TRY(ctx, ctx->stats.alloc(kStatsWords * sizeof(unsigned long long)));
    if (int rc = ensureSpill(ctx, (size_t)total_lanes * (ctx->scene.stack_depth - kLdsStackDepth) * sizeof(StackEntry))) return rc;
    if (photon && (ctx->knn_lanes < total_lanes || ctx->knn_k < ctx->k_nearest || ctx->knn_visit_alloc < ctx->knn_visit_cap)) {
        const uint32_t k = std::max<uint32_t>(ctx->k_nearest, 1);
        ctx->knn_lanes = ctx->knn_k = ctx->knn_visit_alloc = 0;
        HIP_TRY(ctx, ctx->knn_res_d2.alloc((size_t)total_lanes * k * sizeof(double)));
        HIP_TRY(ctx, ctx->knn_res_idx.alloc((size_t)total_lanes * k * sizeof(uint32_t)));
        HIP_TRY(ctx, ctx->knn_visit_d2.alloc((size_t)total_lanes * ctx->knn_visit_cap * sizeof(double)));
        HIP_TRY(ctx, ctx->knn_visit_oct.alloc((size_t)total_lanes * ctx->knn_visit_cap * sizeof(uint32_t)));
        ctx->knn_lanes = total_lanes;
        ctx->knn_k = k;
        ctx->knn_visit_alloc = ctx->knn_visit_cap;
    }
    return MCRT_OK;
}

PhotonMapViewW waveMapView(const mcrt_ctx* ctx, int which) {
    PhotonMapViewW v;
    v.base = ctx->maps[which];
    v.wide = ctx->map_children_ptr[which];
    v.root_a = ctx->map_root_a[which];
    v.root_m = ctx->map_root_m[which];
    v.pos = ctx->map_pos[which].as<PhotonPos>();
    return v;
}

// The positions of a map's photons by themselves (PhotonPos, mcrt_waveknn.hpp), from the records in map order.
__global__ void photonPosKernel(const float4* records, uint64_t n, PhotonPos* pos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = records[2 * i], b = records[2 * i + 1];  // flux rgb, x | y, z, phi, theta
    pos[i] = PhotonPos{a.w, b.x, b.y};
}
int buildMapPositions(mcrt_ctx* ctx, int which, uint64_t n) {
    if (n == 0) return MCRT_OK;
    HIP_TRY(ctx, ctx->map_pos[which].reserve(n * sizeof(PhotonPos)));
    hipLaunchKernelGGL(photonPosKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->map_photons[which].as<float4>(), n,
                       ctx->map_pos[which].as<PhotonPos>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCRT_OK;
}

int validateCamera(mcrt_ctx* ctx, const mcrt_camera_desc* cam) {
    if (!cam || cam->width == 0 || cam->height == 0 || cam->sqrtspp == 0)
        return fail(ctx, MCRT_ERR_INVALID, "camera: width, height and sqrtspp must be non-zero");
    if (cam->shard_count > 1 && cam->shard_index >= cam->shard_count)
        return fail(ctx, MCRT_ERR_INVALID, "camera: shard_index >= shard_count");
    if ((uint64_t)cam->width * cam->height > 0xFFFFFFFFull)
        return fail(ctx, MCRT_ERR_INVALID, "camera: more than 2^32 pixels");
    return MCRT_OK;
}

// Launch geometry of the trace kernel: one workgroup per CU (kTraceWaves waves), its LDS split
// between the lanes' traversal stacks and as many top-of-tree child blocks as fit.
struct TracePlan {
    uint32_t grid, block, lds_bytes;
    WfTraceArgs args;
};

}  // namespace
namespace mcrt {
const char* ctxOpt(const mcrt_ctx* ctx, const char* key) {
    if (!ctx) return nullptr;
    auto it = ctx->options.find(key);
    return it == ctx->options.end() ? nullptr : it->second.c_str();
}
long ctxOptL(const mcrt_ctx* ctx, const char* key, long dflt) {
    const char* v = ctxOpt(ctx, key);
    return v ? atol(v) : dflt;
}
bool ctxOptOn(const mcrt_ctx* ctx, const char* key) {
    const char* v = ctxOpt(ctx, key);
    return v && atoi(v) != 0;
}
}  // namespace mcrt
namespace {
using mcrt::ctxOpt;
using mcrt::ctxOptL;
using mcrt::ctxOptOn;

static_assert(kSelBlock == kBlock && kSelWfBlock == kWfBlock && kSelLdsStack == kLdsStackDepth && kSelIorsDeep == kMaxIorsDeep &&
                  kSelWaveK == waveMaxK(kWaveRows) && kSelWaveKMax == waveMaxK(kWaveRowsLarge) && kSelWaveKnnBytes == waveKnnBytes(kWaveRows) &&
                  kSelWaveKnnBytesLarge == waveKnnBytes(kWaveRowsLarge) && kSelWaveStateBytes == kWaveStateBytes &&
                  kSelFlatArgFloats == kFlatPreArgFloats && kSelVisit == kMaxVisit && kSelVisitLimit == kMaxVisitLimit &&
                  kSelKnnOverflow == kKnnOverflowFlag && kSelLeanFeaturesOff == MCRT_LEAN_FEATURES_OFF,
              "mcrt_select.hpp restates these by value");

// RenderInstance (mcrt_select.hpp) -> the kernel's address and the id of its lean twin (csrc/mcrt_hip_lean.hip), -1: it has none.
struct InstanceEntry {
    const void* full = nullptr;
    int lean_id = -1;
};
const InstanceEntry* instanceTable() {
    static InstanceEntry t[kInstCount];
    static const bool filled = [] {
        constexpr int PT = MCRT_INTEGRATOR_PATH_TRACER, PM = MCRT_INTEGRATOR_PHOTON_MAPPER;
        // (the compiler emits the kernels in the order they are first named, which is here: reordering these lines moves every kernel in the
        // code object - tests/golden/device_code_hashes.json changes and has to be validated on the GPU again)
        auto set = [](int id, auto kernel, int lean_id = -1) { t[id] = InstanceEntry{reinterpret_cast<const void*>(kernel), lean_id}; };
        set(kInstFlatK512, renderKernelFlatK<>, MCRT_LEAN_FLATK_512);
        set(kInstFlatK768, renderKernelFlatK<768>);
        set(kInstFlat512, renderKernel<PT, false, true, false, 1>, MCRT_LEAN_FLAT_512);
        set(kInstPM1024_All, renderKernelPM<false, true, 1024>, MCRT_LEAN_PM_1024_ALL);
        set(kInstPM512_All, renderKernelPM<false, true>, MCRT_LEAN_PM_512_ALL);
        set(kInstSM, renderKernelSM<false, false>, MCRT_LEAN_SM);
        set(kInstSM_All, renderKernelSM<false, true>, MCRT_LEAN_SM_ALL);
        set(kInstShadePT, wfShadeKernel<false>, MCRT_LEAN_SHADE);
        set(kInstShadePM, wfShadeKernel<true>, MCRT_LEAN_SHADE_PM);
        set(kInstEmit, emitKernel<false>, MCRT_LEAN_EMIT);
        set(kInstEmit_All, emitKernel<true>, MCRT_LEAN_EMIT_ALL);
        set(kInstKnnEval, wfKnnKernel<true>, MCRT_LEAN_KNN_EVAL);
        set(kInstTraceLeanSingle, wfTraceKernel<PoolRays, false, 3>);
        set(kInstTraceLean, wfTraceKernel<PoolRays, false, 1>);
        set(kInstTrace_Count, wfTraceKernel<PoolRays, true>);
        set(kInstTrace, wfTraceKernel<PoolRays, false>);
        set(kInstKnnEvalWide, wfKnnKernel<true, kWaveRowsLarge>);
        set(kInstKnnRawWide, wfKnnKernel<false, kWaveRowsLarge>);
        set(kInstKnnRaw, wfKnnKernel<false>);
        set(kInstPT, renderKernel<PT, false, false>);
        set(kInstPT_All, renderKernel<PT, false, true>);
        set(kInstPT_Count, renderKernel<PT, true, false>);
        set(kInstPT_CountAll, renderKernel<PT, true, true>);
        set(kInstPMLane, renderKernel<PM, false, false>);
        set(kInstPMLane_All, renderKernel<PM, false, true>);
        set(kInstPMLane_Count, renderKernel<PM, true, false>);
        set(kInstPMLane_CountAll, renderKernel<PM, true, true>);
        set(kInstPT_ProfAll, renderKernel<PT, false, true, true>);
        set(kInstPT_Prof, renderKernel<PT, false, false, true>);
        set(kInstSM_Count, renderKernelSM<true, false>);
        set(kInstSM_CountAll, renderKernelSM<true, true>);
        set(kInstSM_ProfAll, renderKernelSM<false, true, true>);
        set(kInstSM_Prof, renderKernelSM<false, false, true>);
        set(kInstPM512, renderKernelPM<false, false>);
        set(kInstPM512_Count, renderKernelPM<true, false>);
        set(kInstPM512_CountAll, renderKernelPM<true, true>);
        set(kInstPM1024, renderKernelPM<false, false, 1024>);
        set(kInstPM1024_Count, renderKernelPM<true, false, 1024>);
        set(kInstPM1024_CountAll, renderKernelPM<true, true, 1024>);
        set(kInstPMWide, renderKernelPM<false, false, (int)kBlock, kWaveRowsLarge>);
        set(kInstPMWide_All, renderKernelPM<false, true, (int)kBlock, kWaveRowsLarge>);
        set(kInstPMWide_Count, renderKernelPM<true, false, (int)kBlock, kWaveRowsLarge>);
        set(kInstPMWide_CountAll, renderKernelPM<true, true, (int)kBlock, kWaveRowsLarge>);
        return true;
    }();
    (void)filled;
    return t;
}
// The address to launch; null: the selection asked for a lean twin that does not exist.
const void* instanceAddress(int id, bool lean) {
    const InstanceEntry& e = instanceTable()[id];
    return !lean ? e.full : e.lean_id >= 0 ? mcrt_lean_kernel(e.lean_id) : nullptr;
}
template <class K>
K kernelAs(const void* address) {
    return reinterpret_cast<K>(const_cast<void*>(address));
}
using RenderKernelT = void (*)(const DeviceScene, const RenderParams);
using PmKernelT = void (*)(const DeviceScene, const RenderParams, const PmExtra);
using FlatKernelT = void (*)(const DeviceScene, const RenderParams, const FlatPreArg);
using ShadeKernelT = void (*)(const DeviceScene, const WfShadeArgs);
using KnnKernelT = void (*)(const WfKnnArgs);
using TraceKernelT = void (*)(WfTraceArgs, PoolRays);

// Launch geometry of the trace kernel over a queue of at most max_items rays whose control words are ctx->wf_ctrl (planTraceLds,
// fillTraceArgs: mcrt_launch.hpp)
template <class K>
int planTrace(mcrt_ctx* ctx, K kernel, uint64_t max_items, int leaf_lanes, TracePlan& tp) {
    tp.block = kTraceWaves * 64u;
    uint32_t lds_blocks = 0;
    if (!planTraceLds(kTraceWaves, kLdsStackDepth, ctx->max_lds_trace, ctx->scene.num_qblocks, lds_blocks))
        return fail(ctx, MCRT_ERR_INVALID, "trace kernel: traversal stacks exceed the LDS");
    tp.lds_bytes = traceLdsBytes(kTraceWaves, kLdsStackDepth, lds_blocks);
    LaunchGeom g;
    if (int rc = occupancyGrid(ctx, reinterpret_cast<const void*>(kernel), tp.block, tp.lds_bytes, g)) return rc;
    tp.grid = (uint32_t)std::min<uint64_t>(g.grid, (max_items + tp.block - 1) / tp.block);
    if (tp.grid < 1) tp.grid = 1;
    const uint32_t total_lanes = tp.grid * tp.block;
    if (!ctx->stats.p) HIP_TRY(ctx, ctx->stats.alloc(kStatsWords * sizeof(unsigned long long)));
    if (int rc = ensureSpill(ctx, (size_t)total_lanes * ctx->scene.stack_depth * sizeof(StackEntry))) return rc;
    fillTraceArgs(tp.args, ctx->scene, ctx->wf_ctrl.as<unsigned long long>(), ctx->stats.as<unsigned long long>(), ctx->spill.as<SmStackEntry>(), total_lanes,
                  lds_blocks, leaf_lanes);
    return MCRT_OK;
}

// What the launch that follows runs, for MCRT_LEAN_USED / MCRT_INSTANCES_USED and the readouts of mcrt_render_finish: "frame,trace,knn" by
// RenderInstance name, "/lean" behind a lean twin, "-" where there is none.
void noteInstances(mcrt_ctx* ctx, int instance, bool lean, int trace = kInstNone, int knn = kInstNone, bool knn_lean = false) {
    ctx->lean_used = lean || knn_lean;
    ctx->used_instance = instance;
    ctx->used_trace = trace;
    ctx->used_knn = knn;
    ctx->used_text = std::string(instanceName(instance)) + (lean ? "/lean," : ",") + instanceName(trace) + "," + instanceName(knn) + (knn_lean ? "/lean" : "");
}

// The start of every frame: the statistics cleared, the clocks started, ev0 recorded (each pass clears the work counter itself).
int beginFrame(mcrt_ctx* ctx, hipStream_t stream, uint32_t kernel_id) {
    if (!ctx->work_counter.p) HIP_TRY(ctx, ctx->work_counter.alloc(sizeof(unsigned long long)));
    if (!ctx->stats.p) HIP_TRY(ctx, ctx->stats.alloc(kStatsWords * sizeof(unsigned long long)));
    ctx->t_begin = std::chrono::steady_clock::now();
    ctx->launches = 0;
    ctx->kernel_id = kernel_id;
    HIP_TRY(ctx, hipMemsetAsync(ctx->stats.p, 0, kStatsWords * sizeof(unsigned long long), stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, stream));
    return MCRT_OK;
}
// ... and its end; a shard that owns no row ends right after it began.
int endFrame(mcrt_ctx* ctx, hipStream_t stream) {
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, stream));
    ctx->pending = true;
    return MCRT_OK;
}

// One pass of the wavefront frame loop, the rows [fr.row_base, fr.row_end): shade(0), then trace(i), [knn(i),] shade(i+1) until a shade
// launch queues nothing. The host looks at the queue length every few iterations (a launch with nothing to do costs microseconds).
int runWavefrontPass(mcrt_ctx* ctx, const WfFrame& fr, uint64_t slots, hipStream_t stream, const RenderOptions& opt, const KernelChoice& choice) {
    const bool photon = choice.form == MCRT_KERNEL_WAVEFRONT_PM;
    unsigned long long* const pool = ctx->wf_pool.as<unsigned long long>();
    unsigned long long* const ctrl = ctx->wf_ctrl.as<unsigned long long>();
    unsigned long long* const stats = ctx->stats.as<unsigned long long>();
    HIP_TRY(ctx, hipMemsetAsync(ctx->work_counter.p, 0, sizeof(unsigned long long), stream));
    HIP_TRY(ctx, hipMemsetAsync(ctrl, 0, kWfCtrlWords * sizeof(unsigned long long), stream));
    // a fresh slot is all-zero flags (no path, no pixel); nothing else is used before it is written (kWfSeq is cleared too: the
    // sampler is rebuilt from it before the flags are looked at; tests/emu runs the same code on a pool of garbage)
    HIP_TRY(ctx, hipMemsetAsync(pool + (size_t)kWfFlags * slots, 0, (size_t)slots * 8, stream));
    HIP_TRY(ctx, hipMemsetAsync(pool + (size_t)kWfSeq * slots, 0, (size_t)slots * 8, stream));

    const auto trace = kernelAs<TraceKernelT>(instanceAddress(choice.trace_instance, false));
    const auto shade = kernelAs<ShadeKernelT>(instanceAddress(choice.instance, choice.lean));
    const auto knn = photon ? kernelAs<KnnKernelT>(instanceAddress(choice.knn_instance, choice.knn_lean)) : nullptr;
    if (!shade || (photon && !knn)) return fail(ctx, MCRT_ERR_INVALID, "internal error: no such lean kernel instance");
    TracePlan tp;
    if (int rc = planTrace(ctx, trace, slots * 2, opt.wf_leaf, tp)) return rc;
    WfTraceArgs& ta = tp.args;
    PoolRays pr = bindQueue(pool, ctx->wf_queue.as<uint32_t>(), slots);
    WfShadeArgs sa;
    fillShadeArgs(sa, pr, fr, ctx->scene, ctrl, ctx->work_counter.as<unsigned long long>(), stats);
    const uint32_t shade_grid = (sa.slot_count + kWfBlock - 1) / kWfBlock, shade_lds = wfShadeLdsBytes(sa);

    WfKnnArgs ka;
    memset(&ka, 0, sizeof(ka));
    const uint32_t knn_grid = (uint32_t)ctx->num_cus * 8u;
    if (photon) {
        const uint32_t k = ctx->k_nearest;
        const bool knn_eval = opt.wf_pm_eval;  // (selectKernel: which kNN kernel)
        // Every buffer is held to the size THIS pass needs of it (grow-only). One (slots, k) record for both kinds of launch let the
        // raw buffers of an earlier k pass for those of a larger one once an evaluating frame had renewed the record in between -
        // wfKnnKernel<false> then wrote 2 k slots entries into the smaller allocation (tests/test_gpu_knn_crowds.py met it).
        HIP_TRY(ctx, ctx->wf_requests.reserve((size_t)slots * sizeof(uint32_t)));
        if (knn_eval) {
            HIP_TRY(ctx, ctx->wf_stage.reserve((size_t)slots * kStageDoubles * sizeof(double)));
            HIP_TRY(ctx, ctx->wf_est.reserve((size_t)slots * 6 * sizeof(double)));
        } else {
            HIP_TRY(ctx, ctx->wf_res_n.reserve((size_t)2 * slots * sizeof(uint32_t)));
            HIP_TRY(ctx, ctx->wf_res_r2.reserve((size_t)2 * slots * sizeof(double)));
            HIP_TRY(ctx, ctx->wf_res_idx.reserve((size_t)2 * k * slots * sizeof(uint32_t)));
            HIP_TRY(ctx, ctx->wf_res_d2.reserve((size_t)2 * k * slots * sizeof(double)));
        }
        HIP_TRY(ctx, ctx->knn_spill.reserve(wfKnnSpillBytes(knn_grid)));
        fillKnnArgs(ka, sa, ctrl, waveMapView(ctx, 0), waveMapView(ctx, 1), k, ctx->direct_visualization, ctx->wf_requests.as<uint32_t>(),
                    knn_eval ? ctx->wf_stage.as<double>() : nullptr, knn_eval ? ctx->wf_est.as<double>() : nullptr, ctx->knn_spill.as<uint32_t>(),
                    ctx->wf_res_n.as<uint32_t>(), ctx->wf_res_r2.as<double>(), ctx->wf_res_idx.as<uint32_t>(), ctx->wf_res_d2.as<double>());
    }

    const uint64_t check_every = 16;
    for (uint64_t it = 0;; it++) {
        bindIteration(it, ctrl, sa, ta, ka, pr);
        hipLaunchKernelGGL(shade, dim3(shade_grid), dim3(kWfBlock), shade_lds, stream, ctx->scene, sa);
        ctx->launches++;
        if (it % check_every == check_every - 1 || it < 2) {
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(ctx->wf_host, sa.count_out, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            if (photon)  // requests count as work too
                HIP_TRY(ctx, hipMemcpyAsync(ctx->wf_host + 1, sa.rcount_out, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            HIP_TRY(ctx, hipStreamSynchronize(stream));
            if (opt.wf_log)  // MCRT_WF_LOG: queue length over the frame
                fprintf(stderr, "[mcrt wf] iteration %llu queued %llu at %.2f ms\n", (unsigned long long)it, ctx->wf_host[0],
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->t_begin).count());
            if (ctx->wf_host[0] == 0ull && (!photon || ctx->wf_host[1] == 0ull)) break;  // nothing queued: every slot is done
        }
        hipLaunchKernelGGL(trace, dim3(tp.grid), dim3(tp.block), tp.lds_bytes, stream, ta, pr);
        ctx->launches++;
        if (photon) {
            hipLaunchKernelGGL(knn, dim3(knn_grid), dim3(256), 0, stream, ka);
            ctx->launches++;
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return MCRT_OK;
}

// The end of a pass whose samples are complete in the store, for both pass loops: the samples added up in sample order into the frame's rows
// from row_base on; then, for the sample targets that the context holds, their statistics (libmcrt_pixel_stats.so's kernel, include/mcrt.h
// "Per-pixel sample statistics") and their highlights (libmcrt_robust.so's, "Firefly suppression"), a launch each, offset to the first pixel.
int launchPassEpilogue(mcrt_ctx* ctx, hipStream_t stream, const double* samples, uint64_t pass_pixels, uint32_t spp, double* d_out, uint32_t row_base,
                       uint32_t width) {
    const mcrt_frame_summary& t = ctx->sample_targets;
    const size_t first_pixel = (size_t)row_base * width, first_word = first_pixel * 3;
    hipLaunchKernelGGL(sampleResolveKernel, dim3((uint32_t)((pass_pixels + 255) / 256)), dim3(256), 0, stream, samples, pass_pixels, spp, d_out + first_word);
    HIP_TRY(ctx, hipGetLastError());
    ctx->launches++;
    if (summaryWantsStats(t)) {
        PixelStatsPass ps;
        ps.samples = samples;
        ps.words = pass_pixels * 3;
        ps.spp = spp;
        ps.vec = pixelStatsVec(samples, ps.words);
        ps.variance = t.variance ? t.variance + first_word : nullptr;
        ps.half_a = t.half_a ? t.half_a + first_word : nullptr;
        ps.half_b = t.half_b ? t.half_b + first_word : nullptr;
        HIP_TRY(ctx, (hipError_t)launchPixelStats(stream, ps));
        ctx->launches++;
    }
    if (summaryWantsHighlights(t)) {
        HighlightsPass hp;
        hp.samples = samples;
        hp.pixels = pass_pixels;
        hp.spp = spp;
        hp.reserved = 0;
        hp.tops = t.tops ? t.tops + first_pixel * (MCRT_ROBUST_TOPS * 3) : nullptr;
        hp.level = t.level ? t.level + first_pixel : nullptr;
        HIP_TRY(ctx, (hipError_t)launchHighlights(stream, hp));
        ctx->launches++;
    }
    return MCRT_OK;
}

// The wavefront frame: the film, the pool and the passes (runWavefrontPass), so the call returns when the frame is complete;
// mcrt_render_finish() then only collects the statistics.
// film_out != NULL (mcrt_render_film_device): the splats of this shard's samples stay in the caller's full-frame RGBW buffer
// and the resolve is left to mcrt_film_resolve_device, after the caller has summed the shards' buffers.
int launchWavefront(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, double* d_out, hipStream_t stream,
                    const RenderOptions& opt, const KernelChoice& choice, double* film_out = nullptr) {
    const bool photon = choice.form == MCRT_KERNEL_WAVEFRONT_PM, splats = filmSplats(cam->film_filter, cam->film_radius);
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp, owned_rows = mcrt_shard_rows(cam, nullptr);
    if (cam->width > 0xFFFFu || owned_rows > 0xFFFFu)  // kWfUnit keeps a slot's pixel as two 16-bit numbers
        return fail(ctx, MCRT_ERR_INVALID, "camera: the wavefront integrator takes at most 65535 columns and 65535 rows per shard");
    FilmView film;
    if (splats) {  // Film::Film(width, height, json), film.cpp:19-58
        if (cam->film_filter > MCRT_FILM_LANCZOS) return fail(ctx, MCRT_ERR_INVALID, "camera: unknown film filter");
        if (cam->shard_count > 1 && !film_out)
            return fail(ctx, MCRT_ERR_UNSUPPORTED, "reconstruction filters splat across row groups: render them unsharded (shard_count <= 1) "
                                                   "or with mcrt_render_film_device + mcrt_film_resolve_device");
        if (cam->film_cache_size == 1) return fail(ctx, MCRT_ERR_INVALID, "camera: film_cache_size must be 0 or at least 2");
        if (cam->film_cache_size) {
            const std::vector<double> table = filmCacheTable(*cam);
            if (int rc = uploadArray(ctx, ctx->wf_film_cache, table.data(), table.size())) return rc;
        }
        const size_t blob_bytes = (size_t)cam->width * cam->height * 4 * sizeof(double);
        if (!film_out && ctx->wf_film.bytes < blob_bytes) HIP_TRY(ctx, ctx->wf_film.alloc(blob_bytes));
        film = makeFilmView(*cam, ctx->wf_film_cache.as<double>(), film_out ? film_out : ctx->wf_film.as<double>());
        HIP_TRY(ctx, hipMemsetAsync(film.blob, 0, blob_bytes, stream));
    }

    if (int rc = beginFrame(ctx, stream, owned_rows == 0 ? (uint32_t)MCRT_KERNEL_NONE : choice.form)) return rc;
    if (owned_rows == 0) return endFrame(ctx, stream);
    noteInstances(ctx, choice.instance, choice.lean, choice.trace_instance, choice.knn_instance, choice.knn_lean);

    // Passes: as many rows as the per-sample store holds (box filter; splat frames keep no samples and are one pass).
    uint64_t pass_rows = owned_rows;
    if (!splats) {
        PassPlan pp;
        if (int rc = planSampleStore(ctx, opt.sample_store_gb, cam->width, (uint32_t)owned_rows, spp, pp)) return rc;
        pass_rows = pp.pass_rows;
    }
    // Pool size: up to 16 M slots (5.6 GB of pool, 4.6 GB of queue) — more slots = fewer, longer trace launches (their tails amortised; metal_bunnies
    // 1447 / 1492 / 1507 Mray/s with 4 / 8 / 16 M) — but no more than the pass has work for (below); units per pixel: the power of two
    // that gives a slot up to 16 work units of at least 4 samples.
    const uint64_t pixels = (uint64_t)cam->width * std::min<uint64_t>(pass_rows, owned_rows);
    // (round 4: 16 M by default - C3 at 1024 spp 2024 / 2068 / 2072 Mray/s with 8 / 16 / 32 M; 10 GB of pool and queue - but never more
    // than an eighth of the memory that is free on this device)
    uint64_t slots = opt.wf_slots;  // MCRT_WF_SLOTS
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const uint64_t have = (uint64_t)ctx->wf_slots * kWfSlotBytes;  // what this context's pool and queue already hold
            slots = std::min<uint64_t>(slots, std::max<uint64_t>(((uint64_t)free_b + have) / 8u / kWfSlotBytes, (uint64_t)kWfBlock));
        } else {
            (void)hipGetLastError();
        }
    }
    // ... and no more than the pass has work for: paths / 48, at least 2.5 M, never fewer than 4 samples per slot (planPoolSlots,
    // mcrt_plan.hpp: the measurements)
    // (photon-mapped frames: 16 path samples per slot - their iterations carry a kNN launch whose tails a larger pool amortises: C5 at
    // full size 2 757 ms with 48, 2 725 with 24, 2 713 with 12, 2 874 with 96: profiles/r06_ab_c5_pipeline_pool.log)
    slots = planPoolSlots(pixels * spp, slots, kWfBlock, photon ? 16 : 48);
    if (ctx->wf_slots != slots) {
        HIP_TRY(ctx, ctx->wf_pool.alloc(wfPoolBytes(slots)));
        HIP_TRY(ctx, ctx->wf_queue.alloc(wfQueueBytes(slots)));
        ctx->wf_slots = (uint32_t)slots;
    }
    const size_t iors_need = (size_t)(ctx->iors_depth - kMaxIors) * slots * sizeof(double);
    if (ctx->wf_iors_deep.bytes < iors_need) HIP_TRY(ctx, ctx->wf_iors_deep.alloc(iors_need));
    if (!ctx->wf_ctrl.p) HIP_TRY(ctx, ctx->wf_ctrl.alloc(kWfCtrlWords * sizeof(unsigned long long)));
    if (!ctx->wf_host) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->wf_host), 2 * sizeof(unsigned long long)));
    WfFrame fr;
    fillWfFrame(fr, *cam, global_seed, planChunks(spp, unitsWanted(slots, 16, pixels, opt.chunks)), splats ? nullptr : ctx->samples.as<double>(),
                splats ? &film : nullptr, ctx->wf_iors_deep.as<double>(), ctx->iors_depth);
    for (uint32_t row = 0; row < owned_rows; row += (uint32_t)pass_rows) {
        setWfPass(fr, row, (uint32_t)std::min<uint64_t>(owned_rows, row + pass_rows));
        if (int rc = runWavefrontPass(ctx, fr, slots, stream, opt, choice)) return rc;
        if (!splats)
            if (int rc = launchPassEpilogue(ctx, stream, fr.samples, fr.pass_pixels, fr.spp, d_out, fr.row_base, cam->width)) return rc;
    }
    if (splats && !film_out) {
        const uint64_t all_pixels = (uint64_t)cam->width * cam->height;
        hipLaunchKernelGGL(filmResolveKernel, dim3((uint32_t)((all_pixels + 255) / 256)), dim3(256), 0, stream, fr.film.blob, all_pixels, d_out);
        HIP_TRY(ctx, hipGetLastError());
        ctx->launches++;
    }
    return endFrame(ctx, stream);
}

// Frames of DIFFERENT contexts on ONE device never overlap on the GPU: a launch waits (on the GPU, hipStreamWaitEvent) for the
// frame the device's previous launcher queued, and the host side of a launch — the whole frame for the wavefront pipeline — runs
// under the device's mutex. Two reasons. (i) The mutex makes "size this kernel's dynamic LDS, then launch it" one step:
// hipFuncSetAttribute is state of the kernel FUNCTION, shared by every context of the process - two contexts that render different
// scenes through the same kernel instance would otherwise race for it (a launch that asks for more LDS than the other context just
// set fails; loudly, but it fails). (ii) History: an experimental build of round 3 (hit records as one record per slot, never
// committed) gave wrong frames when two contexts of one process rendered on the same GPU at the same time, and was never understood.
// The committed kernels do not show it: tools/shared_gpu_stress.py with the ordering switched off - 3 processes x 2 contexts and 2 x 4,
// every kernel form, dirty memory, 1 680 concurrent frames compared bit for bit with the reference's / the oracle's - found none wrong
// (round 5, profiles/r05_shared_gpu_stress.log). So the GPU-side wait is a belt; the mutex is needed. One context per device, the
// production shape, never waits here.
struct DeviceOrder {
    std::mutex m;
    hipEvent_t last = nullptr;
    mcrt_ctx* owner = nullptr;
};
DeviceOrder g_device_order[64];

int launchRenderImpl(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_out, hipStream_t stream,
                     double* film_out, const RenderOptions& opt);
int launchRender(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_out, hipStream_t stream,
                 double* film_out = nullptr) {
    if (!ctx) return MCRT_ERR_INVALID;
    // every render call bottoms out here: the render kernels make their own camera rays, the perspective camera's
    if (ctx->lens.model != MCRT_LENS_NONE)
        return fail(ctx, MCRT_ERR_UNSUPPORTED, "a lens is set (mcrt_set_lens): the render kernels trace the camera's own rays only - the camera-ray passes render "
                                               "under a lens; mcrt_set_lens(ctx, NULL) takes it off");
    if (ctx->ray_source.kind != MCRT_RAY_SOURCE_NONE)
        return fail(ctx, MCRT_ERR_UNSUPPORTED, "a ray source is set (mcrt_set_ray_source): the render kernels trace the camera's own rays only - the camera-ray "
                                               "passes trace a source's; mcrt_set_ray_source(ctx, NULL) takes it off");
    // Option MCRT_DEVICE_ORDER=0 (per context, like every option; TEST ONLY: tools/shared_gpu_stress.py, which looks for the fault the
    // ordering was added against): this context's frames do not wait on the GPU for the device's previous launcher. The mutex stays
    // either way - "size this kernel's dynamic LDS, then launch it" must be one step (DeviceOrder's comment).
    const RenderOptions opt = parseRenderOptions(ctx->options);  // the one place a launch reads its options
    const bool gpu_wait = opt.device_order;
    DeviceOrder& o = g_device_order[(unsigned)ctx->device & 63u];
    std::lock_guard<std::mutex> guard(o.m);
    if (gpu_wait && o.owner && o.owner != ctx) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamWaitEvent(stream, o.last, 0));
    }
    const int rc = launchRenderImpl(ctx, cam, global_seed, integrator, d_out, stream, film_out, opt);
    if (rc == MCRT_OK && ctx->pending) {
        o.last = ctx->ev1;
        o.owner = ctx;
        if (cam != &ctx->last_cam) ctx->last_cam = *cam;
        ctx->last_seed = global_seed;
        ctx->last_integrator = integrator;
        ctx->last_out = d_out;
        ctx->last_film = film_out;
        ctx->last_stream = stream;
    }
    return rc;
}

// validate -> selectKernel (mcrt_select.hpp) -> the instance's address -> launch geometry and arguments (mcrt_launch.hpp) -> prologue ->
// one launch per pass
int launchRenderImpl(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_out, hipStream_t stream,
                     double* film_out, const RenderOptions& opt) {
    if (!ctx->has_scene) return fail(ctx, MCRT_ERR_NO_SCENE, "mcrt_render before mcrt_upload_scene");
    if (int rc = validateCamera(ctx, cam)) return rc;
    const bool photon = integrator == MCRT_INTEGRATOR_PHOTON_MAPPER;
    if (integrator != MCRT_INTEGRATOR_PATH_TRACER && !photon) return fail(ctx, MCRT_ERR_INVALID, "unknown integrator");
    if (photon && !ctx->has_photons) return fail(ctx, MCRT_ERR_NO_PHOTONS, "photon mapping render before mcrt_upload_photons");
    if (ctx->pending) return fail(ctx, MCRT_ERR_INVALID, "a render is already in flight: call mcrt_render_finish");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    noteInstances(ctx, kInstNone, false);

    const uint32_t owned_rows = mcrt_shard_rows(cam, nullptr);
    FrameFacts frame;
    frame.photon = photon;
    frame.paths = (uint64_t)owned_rows * cam->width * cam->sqrtspp * cam->sqrtspp;
    // Film::Film(w, h, json) with "filter": "box" and a radius other than the default 0.5 splats too (film.cpp:27-30)
    frame.filtered = filmSplats(cam->film_filter, cam->film_radius);
    frame.film_out = film_out != nullptr;
    frame.k_nearest = ctx->k_nearest;
    frame.max_lds = (uint32_t)ctx->max_lds;
    frame.force_wf = ctx->force_wf;
    frame.force_pm_lane = ctx->force_pm_lane;
    const KernelChoice choice = selectKernel(ctx->facts, frame, opt);
    if (choice.err != MCRT_OK) return fail(ctx, choice.err, choice.message);
    if (choice.form == MCRT_KERNEL_WAVEFRONT || choice.form == MCRT_KERNEL_WAVEFRONT_PM)
        return launchWavefront(ctx, cam, global_seed, d_out, stream, opt, choice, film_out);

    const void* kernel = instanceAddress(choice.instance, choice.lean);
    if (!kernel) return fail(ctx, MCRT_ERR_INVALID, "internal error: no such lean kernel instance");
    const bool pm_wave = choice.form == MCRT_KERNEL_PM_WAVE;
    const bool flat_karg = choice.instance == kInstFlatK512 || choice.instance == kInstFlatK768;
    DeviceScene launch_scene = ctx->scene;
    const uint32_t lds_bytes = planMegaLds(launch_scene, choice, (uint32_t)ctx->max_lds);
    if (lds_bytes > ctx->max_lds) return fail(ctx, MCRT_ERR_INVALID, "LDS plan exceeds the device limit");
    LaunchGeom g;
    if (int rc = occupancyGrid(ctx, kernel, choice.block, lds_bytes, g)) return rc;
    if (int rc = ensureScratch(ctx, g.total_lanes, photon && !pm_wave)) return rc;
    if (int rc = ensureSpill(ctx, megaSpillEntries(ctx->scene, choice, g.total_lanes) * sizeof(StackEntry))) return rc;
    if (int rc = beginFrame(ctx, stream, owned_rows == 0 ? (uint32_t)MCRT_KERNEL_NONE : choice.form)) return rc;
    if (owned_rows == 0) return endFrame(ctx, stream);
    noteInstances(ctx, choice.instance, choice.lean);

    // Sample-chunked work units (RenderParams): the frame goes through in passes of as many rows as the per-sample store holds
    // (MCRT_SAMPLE_STORE_GB, default 64: mcrt_plan.hpp), each pass = one integrator launch + the in-order resolve.
    PassPlan pp;
    if (int rc = planSampleStore(ctx, opt.sample_store_gb, cam->width, owned_rows, cam->sqrtspp * cam->sqrtspp, pp)) return rc;
    RenderParams prm;
    fillRenderParams(prm, *cam, global_seed, owned_rows, ctx->work_counter.as<unsigned long long>(), ctx->stats.as<unsigned long long>(),
                     ctx->spill.as<StackEntry>(), ctx->samples.as<double>(), g.total_lanes);
    if (photon) {
        setRenderMaps(prm, ctx->maps[0], ctx->maps[1], ctx->k_nearest, ctx->direct_visualization);
        prm.knn_res_d2 = ctx->knn_res_d2.as<double>();  // the per-lane searches' scratch (ensureScratch)
        prm.knn_res_idx = ctx->knn_res_idx.as<uint32_t>();
        prm.knn_visit_d2 = ctx->knn_visit_d2.as<double>();
        prm.knn_visit_oct = ctx->knn_visit_oct.as<uint32_t>();
        prm.knn_max_visit = ctx->knn_visit_alloc;
    }
    PmExtra pmx;
    if (pm_wave) {
        HIP_TRY(ctx, ctx->pm_stage.reserve(pmStageBytes(g.total_lanes)));
        HIP_TRY(ctx, ctx->knn_spill.reserve(pmKnnSpillBytes(g.total_lanes)));
        if (pmIorsInMemory(choice)) HIP_TRY(ctx, ctx->pm_iors.reserve(pmIorsBytes(g.total_lanes)));
        fillPmExtra(pmx, waveMapView(ctx, 0), waveMapView(ctx, 1), choice, ctx->pm_stage.as<double>(), ctx->knn_spill.as<uint32_t>(), ctx->pm_iors.as<double>());
    }
    FlatPreArg pre;
    if (flat_karg) {  // the cull records travel in the kernel's argument block
        memset(&pre, 0, sizeof(pre));
        memcpy(pre.v, ctx->flat_pre_host.data(), ctx->flat_pre_host.size() * sizeof(float));
    }
    for (uint32_t row = 0; row < owned_rows; row += pp.pass_rows) {
        setRenderPass(prm, row, pp.pass_rows, photon, opt.chunks);
        // never launch more lanes than there is work
        const uint32_t grid = (uint32_t)std::min<uint64_t>(g.grid, (prm.work_items + g.block - 1) / g.block);
        HIP_TRY(ctx, hipMemsetAsync(ctx->work_counter.p, 0, sizeof(unsigned long long), stream));
        if (pm_wave)
            hipLaunchKernelGGL(kernelAs<PmKernelT>(kernel), dim3(grid), dim3(g.block), g.lds_bytes, stream, launch_scene, prm, pmx);
        else if (flat_karg)
            hipLaunchKernelGGL(kernelAs<FlatKernelT>(kernel), dim3(grid), dim3(g.block), g.lds_bytes, stream, launch_scene, prm, pre);
        else
            hipLaunchKernelGGL(kernelAs<RenderKernelT>(kernel), dim3(grid), dim3(g.block), g.lds_bytes, stream, launch_scene, prm);
        ctx->launches++;
        if (int rc = launchPassEpilogue(ctx, stream, prm.samples, prm.pass_pixels, prm.spp, d_out, prm.row_base, cam->width)) return rc;
    }
    return endFrame(ctx, stream);
}


// The per-sample store of a frame (mcrt_plan.hpp): MCRT_SAMPLE_STORE_GB (default 64) is an upper bound, the device decides how much of
// it exists - at most 40 % of the memory that is free now plus what this context's store already holds (hipMemGetInfo), so that a
// 1080p @ 1024 spp frame (51 GB in one pass on a 288 GB MI355X) goes through in more passes on a smaller or shared device instead of
// failing with out-of-memory; if the allocation still fails (fragmentation, another process grew meanwhile) the store is halved
// until it fits or one 8-row pass does not. Returns the plan through `pp`.
int planSampleStore(mcrt_ctx* ctx, double store_gb, uint32_t width, uint32_t owned_rows, uint32_t spp, PassPlan& pp) {
    double gb = store_gb;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) gb = std::min(gb, 0.4 * (double)(free_b + ctx->samples.bytes) / 1e9);
    else (void)hipGetLastError();
    for (;;) {
        pp = planPasses(width, owned_rows, spp, gb);
        if (ctx->samples.bytes >= pp.store_bytes) return MCRT_OK;
        if (ctx->samples.alloc(pp.store_bytes) == hipSuccess) return MCRT_OK;
        (void)hipGetLastError();
        if (pp.pass_rows <= 8) return fail(ctx, MCRT_ERR_HIP, "out of device memory for the per-sample store of one 8-row pass");
        gb = std::min(gb, (double)pp.store_bytes / 1e9) * 0.5;
    }
}

int uploadMap(mcrt_ctx* ctx, int which, const mcrt_photon_map_desc* m) {
    PhotonMapView& v = ctx->maps[which];
    memset(&v, 0, sizeof(v));
    ctx->map_children_ptr[which] = nullptr;
    if (!m || m->num_octants == 0 || m->num_photons == 0) return MCRT_OK;
    if (m->num_photons > 0xFFFFFFFEull) return fail(ctx, MCRT_ERR_UNSUPPORTED, "photon map larger than 2^32-2 photons per GPU");
    if (!m->octant_bounds || !m->octant_start_data || !m->octant_contained_data || !m->octant_next_sibling || !m->octant_leaf || !m->photons)
        return fail(ctx, MCRT_ERR_INVALID, "photon map descriptor has null arrays");
    const size_t n = m->num_octants;
    std::vector<uint32_t> start(n), contained(n);
    for (size_t i = 0; i < n; i++) {
        if (m->octant_start_data[i] + m->octant_contained_data[i] > m->num_photons)
            return fail(ctx, MCRT_ERR_INVALID, "photon map octant range exceeds the photon array");
        start[i] = (uint32_t)m->octant_start_data[i];
        contained[i] = (uint32_t)m->octant_contained_data[i];
    }
    if (int rc = uploadArray(ctx, ctx->map_bounds[which], m->octant_bounds, n * 6)) return rc;
    if (int rc = uploadArray(ctx, ctx->map_start[which], start.data(), n)) return rc;
    if (int rc = uploadArray(ctx, ctx->map_contained[which], contained.data(), n)) return rc;
    if (int rc = uploadArray(ctx, ctx->map_next[which], m->octant_next_sibling, n)) return rc;
    if (int rc = uploadArray(ctx, ctx->map_leaf[which], m->octant_leaf, n)) return rc;
    if (int rc = uploadArray(ctx, ctx->map_photons[which], m->photons, (size_t)m->num_photons * 8)) return rc;
    {   // record lists for the wave-cooperative search (mcrt_waveknn.hpp: WideRec; built by buildWideRecords, mcrt_widerec.hpp)
        std::vector<WideRec> wide;
        uint32_t root_a = 0, root_m = 0;
        const int wrc = buildWideRecords(m, contained.data(), std::max<uint32_t>(ctx->k_nearest, 1u), wide, root_a, root_m);
        if (wrc == 1) return fail(ctx, MCRT_ERR_INVALID, "photon octant with more than 8 children");
        if (wrc == 2) return fail(ctx, MCRT_ERR_UNSUPPORTED, "photon map too large for 32-bit record indices");
        if (int rc = uploadArray(ctx, ctx->map_children[which], wide.data(), wide.size())) return rc;
        ctx->map_children_ptr[which] = ctx->map_children[which].as<WideRec>();
        ctx->map_root_a[which] = root_a;
        ctx->map_root_m[which] = root_m;
    }
    v.num_octants = m->num_octants;
    v.num_photons = m->num_photons;
    v.octant_bounds = ctx->map_bounds[which].as<double>();
    v.octant_start = ctx->map_start[which].as<uint32_t>();
    v.octant_contained = ctx->map_contained[which].as<uint32_t>();
    v.octant_next = ctx->map_next[which].as<uint32_t>();
    v.octant_leaf = ctx->map_leaf[which].as<uint8_t>();
    v.photons = ctx->map_photons[which].as<float>();
    return buildMapPositions(ctx, which, m->num_photons);
}

#include "mcrt_photon_device.hpp"

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int mcrt_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return count > 0 ? count : 0;
}

int mcrt_create(mcrt_ctx** out, int device_id) {
    if (!out) return MCRT_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, MCRT_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= count) return fail(nullptr, MCRT_ERR_NO_DEVICE, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess)
        return fail(nullptr, MCRT_ERR_NO_DEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0 && !getenv("MCRT_ALLOW_ANY_ARCH"))
        return fail(nullptr, MCRT_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    if ((e = hipSetDevice(device_id)) != hipSuccess)
        return fail(nullptr, MCRT_ERR_NO_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    mcrt_ctx* ctx = new mcrt_ctx();
    // The MCRT_* environment variables seed the context's options HERE, once; afterwards only mcrt_set_option changes them
    // (no getenv on the launch path).
    for (char** e = environ; e && *e; e++) {
        if (strncmp(*e, "MCRT_", 5) != 0) continue;
        const char* eq = strchr(*e, '=');
        if (eq) ctx->options[std::string(*e, (size_t)(eq - *e))] = std::string(eq + 1);
    }
    ctx->device = device_id;
    ctx->num_cus = prop.multiProcessorCount;
    ctx->max_lds = prop.sharedMemPerBlock > 0 ? (size_t)prop.sharedMemPerBlock : 65536;
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id) == hipSuccess && v > 0)
            ctx->max_lds = std::max(ctx->max_lds, (size_t)v);
    }
    // the kernels that shade hold the sin/cos table as static LDS (mcrt_libm.hpp): their dynamic LDS plans get the rest
    ctx->max_lds_trace = ctx->max_lds;
    ctx->max_lds -= glibc235::kShadeStaticLds;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&ctx->ev0) != hipSuccess ||
        hipEventCreate(&ctx->ev1) != hipSuccess) {
        delete ctx;
        return fail(nullptr, MCRT_ERR_HIP, "stream/event creation failed");
    }
    std::vector<uint32_t> tab(kSobolTableWords);
    buildSobolByteTables(tab.data());
    if (int rc = uploadArray(ctx, ctx->sobol_tab, tab.data(), tab.size())) {
        g_create_error = ctx->error;
        mcrt_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return MCRT_OK;
}

void mcrt_destroy(mcrt_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    {
        DeviceOrder& o = g_device_order[(unsigned)ctx->device & 63u];
        std::lock_guard<std::mutex> guard(o.m);
        if (o.owner == ctx) {  // nobody may wait on an event that is about to go
            (void)hipEventSynchronize(o.last);
            o.owner = nullptr;
            o.last = nullptr;
        }
    }
    if (ctx->stream) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamDestroy(ctx->stream);
    }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->wf_host) (void)hipHostFree(ctx->wf_host);
    delete ctx;
}

const char* mcrt_last_error(const mcrt_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int mcrt_set_option(mcrt_ctx* ctx, const char* key, const char* value) {
    if (!ctx || !key || strncmp(key, "MCRT_", 5) != 0) return ctx ? fail(ctx, MCRT_ERR_INVALID, "mcrt_set_option: keys are the MCRT_* names of include/mcrt.h") : MCRT_ERR_INVALID;
    if (value) ctx->options[key] = value;
    else ctx->options.erase(key);
    return MCRT_OK;
}

const char* mcrt_get_option(const mcrt_ctx* ctx, const char* key) {
    if (!ctx || !key) return nullptr;
    if (strcmp(key, "MCRT_LEAN_USED") == 0) return ctx->lean_used ? "1" : "0";  // (read-only: did the last frame / photon pass run a lean kernel instance)
    if (strcmp(key, "MCRT_INSTANCES_USED") == 0) return ctx->used_text.c_str();  // (read-only: ... and which instances, noteInstances)
    return mcrt::ctxOpt(ctx, key);
}

int mcrt_upload_scene(mcrt_ctx* ctx, const mcrt_scene_desc* s) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!s || s->abi_version != MCRT_ABI_VERSION) return fail(ctx, MCRT_ERR_INVALID, "scene descriptor: wrong abi_version");
    REJECT_IF_PENDING(ctx, "mcrt_upload_scene");
    if (s->num_surfaces == 0 || !s->surf_kind || !s->surf_interpolate || !s->surf_material || !s->surf_area || !s->surf_v || !s->surf_e ||
        !s->materials || s->num_materials == 0)
        return fail(ctx, MCRT_ERR_INVALID, "scene descriptor: missing surface/material arrays");
    if (s->num_nodes && (!s->node_bounds || !s->node_start_surface || !s->node_num_surfaces || !s->node_next_sibling))
        return fail(ctx, MCRT_ERR_INVALID, "scene descriptor: missing node arrays");
    if (s->num_lights && (!s->light_surface || !s->light_cdf)) return fail(ctx, MCRT_ERR_INVALID, "scene descriptor: missing light arrays");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->has_scene = false;

    const size_t ns = s->num_surfaces;
    HostLayout L;
    std::string lerr;
    if (int rc = buildLayout(s, L, lerr)) return fail(ctx, rc, lerr);
    const bool any_vn = L.any_vn;
    std::vector<double>& prim = L.prim;
    std::vector<double>& normal = L.normal;
    std::vector<double>& bounds = L.node_bounds;
    std::vector<NodeMeta>& meta = L.node_meta;

    if (int rc = uploadArray(ctx, ctx->node_bounds, bounds.data(), bounds.size())) return rc;
    if (int rc = uploadArray(ctx, ctx->node_meta, meta.data(), meta.size())) return rc;
    if (int rc = uploadArray(ctx, ctx->nodes64, L.nodes64.data(), L.nodes64.size())) return rc;
    if (int rc = uploadArray(ctx, ctx->qblocks, L.qblocks.data(), L.qblocks.size())) return rc;
    // quadric records first: the primitive records and surf_v of quadric surfaces carry their device addresses
    if (L.num_quadric_surfaces) {
        for (uint32_t i = 0; i < s->num_lights; i++)
            if (s->surf_kind[s->light_surface[i]] == MCRT_SURF_QUADRIC)
                return fail(ctx, MCRT_ERR_UNSUPPORTED, "emissive quadrics are not supported (scene/scene.cpp:125)");
        if (int rc = uploadArray(ctx, ctx->quadrics, s->quadrics, (size_t)s->num_quadrics * 22)) return rc;
        patchQuadricAddresses(s, L, ctx->quadrics.as<double>());
    } else {
        ctx->quadrics.release();
    }
    if (int rc = uploadArray(ctx, ctx->prim, prim.data(), prim.size())) return rc;
    if (int rc = uploadArray(ctx, ctx->flat_prim, L.flat_prim.data(), L.flat_prim.size())) return rc;
    if (int rc = uploadArray(ctx, ctx->flat_index, L.flat_index.data(), L.flat_index.size())) return rc;
    ctx->flat_pre_host = L.flat_pre;
    if (L.flat_pre.empty()) ctx->flat_pre.release();
    else if (int rc = uploadArray(ctx, ctx->flat_pre, L.flat_pre.data(), L.flat_pre.size())) return rc;
    if (int rc = uploadArray(ctx, ctx->surf_v, L.num_quadric_surfaces ? L.surf_v_patched.data() : s->surf_v, ns * 9)) return rc;
    if (int rc = uploadArray(ctx, ctx->surf_normal, normal.data(), normal.size())) return rc;
    if (int rc = uploadArray(ctx, ctx->surf_rec, L.shade_rec.data(), L.shade_rec.size())) return rc;
    if (any_vn) {
        if (int rc = uploadArray(ctx, ctx->surf_vn, s->surf_vn, ns * 9)) return rc;
    } else {
        ctx->surf_vn.release();
    }
    if (int rc = uploadArray(ctx, ctx->surf_area, s->surf_area, ns)) return rc;
    if (int rc = uploadArray(ctx, ctx->surf_material, s->surf_material, ns)) return rc;
    if (int rc = uploadArray(ctx, ctx->surf_kind, s->surf_kind, ns)) return rc;
    if (int rc = uploadArray(ctx, ctx->materials, s->materials, (size_t)s->num_materials)) return rc;
    if (int rc = uploadArray(ctx, ctx->light_surface, s->light_surface, (size_t)s->num_lights)) return rc;
    if (int rc = uploadArray(ctx, ctx->light_cdf, s->light_cdf, (size_t)s->num_lights)) return rc;

    DeviceScene& d = ctx->scene;
    memset(&d, 0, sizeof(d));
    d.num_nodes = s->num_nodes;
    d.num_surfaces = s->num_surfaces;
    d.num_materials = s->num_materials;
    d.num_lights = s->num_lights;
    d.node_bounds = ctx->node_bounds.as<double>();
    d.node_meta = ctx->node_meta.as<NodeMeta>();
    d.nodes64 = ctx->nodes64.as<Node64>();
    d.qblocks = ctx->qblocks.as<QBlock>();
    d.num_qblocks = (uint32_t)L.qblocks.size();
    d.q_nodes = (uint32_t)L.nodes64.size();
    // every lane's traversal stack holds what a depth-first walk of THIS tree can hold (HostLayout::stack_bound), never fewer than
    // kMaxStackDepth entries; the spill slabs behind the LDS part are sized from it at launch (ensureSpill)
    d.stack_depth = std::max<uint32_t>((uint32_t)kMaxStackDepth, L.stack_bound + 1u);
    {
        // the deepest spill slab a frame allocates: two trace launches x 256 CUs x the 2048 lanes a CU can hold (planTrace's grid is
        // occupancy x CUs) x 8 bytes per entry. A tree degenerate enough to need more than a quarter of the device's memory for it
        // (tens of thousands of stack entries: a BVH that is a list) is refused here, with its number; ensureSpill says the same
        // should an allocation below that bound fail all the same.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            total_b = (size_t)64 << 30;
        }
        const size_t slab = (size_t)d.stack_depth * sizeof(StackEntry) * 2u * (size_t)ctx->num_cus * 2048u;
        if (slab > total_b / 4)
            return fail(ctx, MCRT_ERR_UNSUPPORTED, "BVH so unbalanced that a depth-first walk may hold " + std::to_string(L.stack_bound) +
                                                       " pending nodes per ray: the traversal stacks would not fit in device memory");
    }
    d.q_root_a = L.q_root_a;
    d.q_root_m = L.q_root_m;
    d.prim = ctx->prim.as<double>();
    d.flat_prim = ctx->flat_prim.as<double>();
    d.flat_index = ctx->flat_index.as<uint32_t>();
    d.flat_tris = L.flat_tris;
    d.flat_pre = L.flat_pre.empty() ? nullptr : ctx->flat_pre.as<float>();
    d.pre_tri_pairs = L.pre_tri_pairs;
    d.pre_sph_pairs = L.pre_sph_pairs;
    for (int c = 0; c < 3; c++) d.pre_centre[c] = L.pre_centre[c];
    d.pre_bound = L.pre_bound;
    d.surf_v = ctx->surf_v.as<double>();
    d.surf_normal = ctx->surf_normal.as<double>();
    d.surf_rec = ctx->surf_rec.as<double>();
    d.surf_vn = any_vn ? ctx->surf_vn.as<double>() : nullptr;
    d.surf_area = ctx->surf_area.as<double>();
    d.surf_material = ctx->surf_material.as<uint32_t>();
    d.surf_kind = ctx->surf_kind.as<uint8_t>();
    d.materials = ctx->materials.as<mcrt_material>();
    d.light_surface = ctx->light_surface.as<uint32_t>();
    d.light_cdf = ctx->light_cdf.as<double>();
    d.sobol_tab = ctx->sobol_tab.as<uint32_t>();
    d.scene_ior = s->scene_ior;

    ctx->host_light_flux = lightFlux(*s);
    const char* fm = ctxOpt(ctx, "MCRT_FLAT_MAX");
    planStaging(d, (uint32_t)ctx->max_lds, fm ? (uint32_t)strtoul(fm, nullptr, 0) : 64u, L);
    ctx->facts = sceneFacts(d, L, *s);
    ctx->has_scene = true;
    return MCRT_OK;
}

int mcrt_upload_photons(mcrt_ctx* ctx, const mcrt_photon_map_desc* global_map, const mcrt_photon_map_desc* caustic_map,
                        uint32_t k_nearest_photons, int direct_visualization) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (k_nearest_photons == 0) return fail(ctx, MCRT_ERR_INVALID, "k_nearest_photons must be > 0");
    REJECT_IF_PENDING(ctx, "mcrt_upload_photons");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->has_photons = false;
    ctx->k_nearest = k_nearest_photons;  // before the maps: the search's record lists expand octants with more than k photons
    if (int rc = uploadMap(ctx, 0, global_map)) return rc;
    if (int rc = uploadMap(ctx, 1, caustic_map)) return rc;
    ctx->direct_visualization = direct_visualization ? 1 : 0;
    ctx->has_photons = true;
    return MCRT_OK;
}

uint32_t mcrt_shard_rows(const mcrt_camera_desc* cam, uint32_t* rows) {
    if (!cam) return 0;
    if (cam->shard_count <= 1) {
        if (rows)
            for (uint32_t y = 0; y < cam->height; y++) rows[y] = y;
        return cam->height;
    }
    const uint32_t g = cam->shard_rows ? cam->shard_rows : 1;
    uint32_t n = 0;
    for (uint32_t y = 0; y < cam->height; y++)
        if ((y / g) % cam->shard_count == cam->shard_index) {
            if (rows) rows[n] = y;
            n++;
        }
    return n;
}

int mcrt_render_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_out_rgb,
                       void* stream) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!d_out_rgb) return fail(ctx, MCRT_ERR_INVALID, "d_out_rgb is NULL");
    return launchRender(ctx, cam, global_seed, integrator, d_out_rgb, stream ? (hipStream_t)stream : ctx->stream);
}

int mcrt_render_film_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_rgbw,
                            void* stream) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!d_rgbw) return fail(ctx, MCRT_ERR_INVALID, "d_rgbw is NULL");
    return launchRender(ctx, cam, global_seed, integrator, nullptr, stream ? (hipStream_t)stream : ctx->stream, d_rgbw);
}

int mcrt_film_resolve_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* d_rgbw, double* d_out_rgb, void* stream) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!d_rgbw || !d_out_rgb || width == 0 || height == 0) return fail(ctx, MCRT_ERR_INVALID, "mcrt_film_resolve_device: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t pixels = (uint64_t)width * height;
    hipLaunchKernelGGL(filmResolveKernel, dim3((uint32_t)((pixels + 255) / 256)), dim3(256), 0, stream ? (hipStream_t)stream : ctx->stream,
                       d_rgbw, pixels, d_out_rgb);
    HIP_TRY(ctx, hipGetLastError());
    return MCRT_OK;
}

int mcrt_render_finish(mcrt_ctx* ctx, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!ctx->pending) return fail(ctx, MCRT_ERR_INVALID, "no render in flight");
    ctx->pending = false;
    // (a) wait for the frame, read its statistics words back
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    unsigned long long h[kStatsWords];
    HIP_TRY(ctx, hipMemcpy(h, ctx->stats.p, sizeof(h), hipMemcpyDeviceToHost));
    // (b) the words -> readouts, counters, outcome: pure functions of them (mcrt_stats_readout.hpp)
    fputs(statsReadout(h, ctx->used_instance, ctx->used_trace, ctx->kernel_id).c_str(), stderr);
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        statsCounters(h, *stats);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->t_begin).count();
        stats->kernel_launches = ctx->launches;
        stats->kernel_id = ctx->kernel_id;
    }
    // (test hook: MCRT_TEST_KNN_OVERFLOW=1 treats the first frame of a wave-cooperative photon-mapping kernel as if a search had overflowed;
    // no tree the tests can build in reasonable time fills 128 + 1 024 frontier entries through the render path, whose record lists
    // are made for the k it searches with)
    const bool pm_wave_frame = ctx->kernel_id == MCRT_KERNEL_PM_WAVE || ctx->kernel_id == MCRT_KERNEL_WAVEFRONT_PM;
    if (pm_wave_frame && !ctx->force_pm_lane && ctxOptOn(ctx, "MCRT_TEST_KNN_OVERFLOW")) h[kStatOverflow] |= kKnnOverflowFlag;
    // (c) Done, refused, or rendered again with a flag raised or a capacity grown: nextRender (mcrt_select.hpp) decides. The flags hold
    // until this frame is delivered or refused; the capacities a scene needed stay with the context.
    RetryState state;
    state.force_wf = ctx->force_wf;
    state.force_pm_lane = ctx->force_pm_lane;
    state.knn_visit_cap = ctx->knn_visit_cap;
    state.iors_depth = ctx->iors_depth;
    FrameOutcome frame = statsOutcome(h, ctx->kernel_id);
    frame.splats = filmSplats(ctx->last_cam.film_filter, ctx->last_cam.film_radius);
    frame.can_pipeline = ctx->scene.q_nodes > 0 && (ctx->last_integrator != MCRT_INTEGRATOR_PHOTON_MAPPER || ctx->k_nearest <= waveMaxK(kWaveRowsLarge));
    const RetryStep step = nextRender(state, frame);
    if (step.action == kRetryDone) return MCRT_OK;
    if (step.action == kRetryError) return fail(ctx, step.err, step.message);
    ctx->knn_visit_cap = step.next.knn_visit_cap;
    ctx->iors_depth = step.next.iors_depth;
    ctx->force_wf = step.next.force_wf;
    ctx->force_pm_lane = step.next.force_pm_lane;
    int rc = launchRender(ctx, &ctx->last_cam, ctx->last_seed, ctx->last_integrator, ctx->last_out, ctx->last_stream, ctx->last_film);
    if (rc == MCRT_OK) rc = mcrt_render_finish(ctx, stats);
    ctx->force_wf = state.force_wf;
    ctx->force_pm_lane = state.force_pm_lane;
    return rc;
}

int mcrt_render(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* out_rgb,
                mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!out_rgb) return fail(ctx, MCRT_ERR_INVALID, "out_rgb is NULL");
    if (int rc = validateCamera(ctx, cam)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t rows = mcrt_shard_rows(cam, nullptr);
    const size_t row_bytes = (size_t)cam->width * 3 * sizeof(double);
    if (ctx->out_tmp.bytes < rows * row_bytes) HIP_TRY(ctx, ctx->out_tmp.alloc(std::max<size_t>(rows * row_bytes, 8)));
    if (int rc = launchRender(ctx, cam, global_seed, integrator, ctx->out_tmp.as<double>(), ctx->stream)) return rc;
    mcrt_stats st;
    int rc = mcrt_render_finish(ctx, &st);
    if (rc) return rc;
    if (rows) {
        std::vector<double> packed((size_t)rows * cam->width * 3);
        HIP_TRY(ctx, hipMemcpy(packed.data(), ctx->out_tmp.p, packed.size() * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<uint32_t> idx(rows);
        mcrt_shard_rows(cam, idx.data());
        for (uint32_t r = 0; r < rows; r++) memcpy(out_rgb + (size_t)idx[r] * cam->width * 3, &packed[(size_t)r * cam->width * 3], row_bytes);
    }
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->t_begin).count();
    if (stats) *stats = st;
    return MCRT_OK;
}

int mcrt_emit_photons(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed, mcrt_photon_emission* out) {
    return mcrt_emit_photons_shard(ctx, emissions, caustic_factor, global_seed, 0, 1, out);
}

}  // extern "C"

namespace {
// The emission pass; the lists stay in ctx->emit_photons / emit_keys. h = the kernel's counters (kEmit*, mcrt_stats_words.hpp).
int emitOnDevice(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed, uint32_t shard_index, uint32_t shard_count,
                 unsigned long long h[kEmitWords], float& ms) {
    for (int i = 0; i < kEmitWords; i++) h[i] = 0ull;
    ms = 0.f;
    if (shard_count == 0 || shard_index >= shard_count) return fail(ctx, MCRT_ERR_INVALID, "shard_index >= shard_count");
    if (!ctx->has_scene) return fail(ctx, MCRT_ERR_NO_SCENE, "mcrt_emit_photons before mcrt_upload_scene");
    REJECT_IF_PENDING(ctx, "mcrt_emit_photons");
    if (!(emissions >= 0.0) || !(caustic_factor > 0.0)) return fail(ctx, MCRT_ERR_INVALID, "emissions must be >= 0 and caustic_factor > 0");
    const uint32_t nl = ctx->scene.num_lights;
    if (nl == 0 || nl > 0xFFFFu) return nl == 0 ? MCRT_OK : fail(ctx, MCRT_ERR_UNSUPPORTED, "more than 65535 lights");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    std::vector<unsigned long long> first;
    std::vector<double> pflux;
    planEmission(ctx->host_light_flux, emissions, caustic_factor, first, pflux);
    for (uint32_t i = 0; i < nl; i++)
        if (first[i + 1] - first[i] > 0xFFFFFFFFull) return fail(ctx, MCRT_ERR_UNSUPPORTED, "more than 2^32 emissions from one light");
    const unsigned long long all_paths = first[nl];
    const unsigned long long shard_begin = all_paths * shard_index / shard_count, shard_end = all_paths * (shard_index + 1ull) / shard_count;
    const unsigned long long total = shard_end - shard_begin;  // paths of this shard
    if (int rc = uploadArray(ctx, ctx->emit_first, first.data(), first.size())) return rc;
    if (int rc = uploadArray(ctx, ctx->emit_flux, pflux.data(), pflux.size())) return rc;
    if (!ctx->emit_counters.p) HIP_TRY(ctx, ctx->emit_counters.alloc(kEmitWords * sizeof(unsigned long long)));

    noteInstances(ctx, ctx->scene.stage_all ? kInstEmit_All : kInstEmit, leanScene(ctx->facts, parseRenderOptions(ctx->options)));
    auto kernel = kernelAs<void (*)(const DeviceScene, const EmitParams)>(instanceAddress(ctx->scene.stage_all ? kInstEmit_All : kInstEmit, ctx->lean_used));
    if (!kernel) return fail(ctx, MCRT_ERR_INVALID, "internal error: no such lean kernel instance");
    DeviceScene scene = ctx->scene;
    scene.flat = 0;  // the emission kernel walks the BVH
    LaunchGeom g;
    if (int rc = launchGeometry(ctx, kernel, scene, g)) return rc;
    if (int rc = ensureScratch(ctx, g.total_lanes, false)) return rc;

    // List sizes. A path leaves a photon at every diffuse bounce, so the lists can hold more photons than there are paths (C5: 1.13 per
    // path in the caustic list) or far fewer (its global list: 0.07). A launch whose lists are too small still COUNTS exactly, and the pass
    // is repeated at the exact sizes (below) - until round 4 that was the normal case for C5, whose emission so ran twice (0.37 s each).
    // Now a pilot launch over every 64th path of the range (capacity 0: counting only, ~1/64 of the time) sizes the lists first, with 5 %
    // and 64 K photons to spare; lists left by an earlier call are used at their full size.
    unsigned long long cap[2] = {std::max<unsigned long long>(1ull << 16, total), std::max<unsigned long long>(1ull << 16, total)};
    constexpr uint32_t kPilotStride = 64;
    const bool pilot = total >= (4ull << 20);
    for (int attempt = pilot ? -1 : 0; attempt < 3; attempt++) {
        const bool counting = attempt < 0;
        for (int w = 0; w < 2 && !counting; w++) {
            if (ctx->emit_photons[w].bytes < cap[w] * 32) HIP_TRY(ctx, ctx->emit_photons[w].alloc(cap[w] * 32));
            if (ctx->emit_keys[w].bytes < cap[w] * 8) HIP_TRY(ctx, ctx->emit_keys[w].alloc(cap[w] * 8));
            cap[w] = std::min<unsigned long long>(ctx->emit_photons[w].bytes / 32, ctx->emit_keys[w].bytes / 8);
        }
        float* const lists[2] = {ctx->emit_photons[0].as<float>(), ctx->emit_photons[1].as<float>()};
        unsigned long long* const keys[2] = {ctx->emit_keys[0].as<unsigned long long>(), ctx->emit_keys[1].as<unsigned long long>()};
        const unsigned long long none[2] = {0ull, 0ull};
        EmitParams prm;
        fillEmitParams(prm, nl, ctx->emit_first.as<unsigned long long>(), ctx->emit_flux.as<double>(), shard_begin, shard_end, counting ? kPilotStride : 1u,
                       global_seed, caustic_factor, lists, keys, counting ? none : cap, ctx->emit_counters.as<unsigned long long>(),
                       ctx->spill.as<StackEntry>(), g.total_lanes);
        const uint32_t grid = (uint32_t)std::min<unsigned long long>(g.grid, (total + kBlock - 1) / kBlock + 1);
        HIP_TRY(ctx, hipMemsetAsync(ctx->emit_counters.p, 0, kEmitWords * sizeof(unsigned long long), ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), g.lds_bytes, ctx->stream, scene, prm);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
        HIP_TRY(ctx, hipMemcpy(h, ctx->emit_counters.p, kEmitWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        if (h[kEmitOverflow]) return fail(ctx, MCRT_ERR_UNSUPPORTED, "traversal stack overflow in the emission pass");
        // RefractionHistory (ray.cpp:74-98) is unbounded in the reference; the emission kernel keeps kMaxIors (8) entries per lane. The eye
        // pass of such a scene retries through the 32-entry pool or fails (mcrt_render_finish); the photon pass must not be the silent one.
        if (h[kEmitIorsOverflow]) return fail(ctx, MCRT_ERR_UNSUPPORTED, "a photon path entered more than 8 nested dielectric media (RefractionHistory, ray.cpp:74-98, is kept to 8 entries per lane in the emission pass)");
        if (counting) {
            for (int w = 0; w < 2; w++) cap[w] = (unsigned long long)((double)h[kEmitGlobalCount + w] * kPilotStride * 1.05) + (1ull << 16);
            continue;
        }
        if (h[kEmitGlobalCount] <= cap[0] && h[kEmitCausticCount] <= cap[1]) break;
        cap[0] = std::max(cap[0], h[kEmitGlobalCount]);  // a list was too small: size it exactly and emit again
        cap[1] = std::max(cap[1], h[kEmitCausticCount]);
        if (attempt == 2) return fail(ctx, MCRT_ERR_HIP, "photon lists kept overflowing");
    }
    return MCRT_OK;
}
}  // namespace

extern "C" {

int mcrt_emit_photons_shard(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed, uint32_t shard_index,
                            uint32_t shard_count, mcrt_photon_emission* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!out) return fail(ctx, MCRT_ERR_INVALID, "out is NULL");
    memset(out, 0, sizeof(*out));
    unsigned long long h[kEmitWords];
    float ms = 0.f;
    if (int rc = emitOnDevice(ctx, emissions, caustic_factor, global_seed, shard_index, shard_count, h, ms)) return rc;
    for (int w = 0; w < 2; w++) {
        const size_t n = (size_t)h[kEmitGlobalCount + w];
        ctx->host_photons[w].resize(n * 8);
        ctx->host_keys[w].resize(n);
        if (n) {
            HIP_TRY(ctx, hipMemcpy(ctx->host_photons[w].data(), ctx->emit_photons[w].p, n * 32, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(ctx->host_keys[w].data(), ctx->emit_keys[w].p, n * 8, hipMemcpyDeviceToHost));
        }
    }
    out->global_count = h[kEmitGlobalCount];
    out->caustic_count = h[kEmitCausticCount];
    out->global_photons = ctx->host_photons[0].data();
    out->caustic_photons = ctx->host_photons[1].data();
    out->global_keys = ctx->host_keys[0].data();
    out->caustic_keys = ctx->host_keys[1].data();
    out->emission_paths = h[kEmitPaths];
    out->rays = h[kEmitRays];
    out->kernel_ms = ms;
    return MCRT_OK;
}

int mcrt_emit_photons_device(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed, uint32_t shard_index,
                             uint32_t shard_count, mcrt_photon_emission_device* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!out) return fail(ctx, MCRT_ERR_INVALID, "out is NULL");
    memset(out, 0, sizeof(*out));
    unsigned long long h[kEmitWords];
    float ms = 0.f;
    if (int rc = emitOnDevice(ctx, emissions, caustic_factor, global_seed, shard_index, shard_count, h, ms)) return rc;
    out->global_count = h[kEmitGlobalCount];
    out->caustic_count = h[kEmitCausticCount];
    out->d_global_photons = ctx->emit_photons[0].as<float>();
    out->d_caustic_photons = ctx->emit_photons[1].as<float>();
    out->emission_paths = h[kEmitPaths];
    out->rays = h[kEmitRays];
    out->kernel_ms = ms;
    return MCRT_OK;
}

// buildMapOnDevice, or - when more than a leaf's worth of photons share one cell of its 21-level codes (2^-21 of the map's cube: the
// focus of a sharp caustic can do that) - the same map from the recursive host builder, which splits as deep as the reference's Octree
// does (octree.cpp:35-80): the list goes to the host once, the finished map comes back (mcrt_upload_photons' path). Slower, and what the
// call used to refuse with MCRT_ERR_UNSUPPORTED until round 4.
int buildMapAnyDepth(mcrt_ctx* ctx, int which, const float* d_photons, uint64_t n, const double bb_min[3], const double bb_max[3],
                     uint32_t max_node_data, double* timing) {
    ctx->dense_cell_refused = false;
    const int rc = buildMapOnDevice(ctx, which, d_photons, n, bb_min, bb_max, max_node_data, timing);
    if (rc != MCRT_ERR_UNSUPPORTED || !ctx->dense_cell_refused) return rc;
    ctx->dense_cell_refused = false;
    std::vector<float> host;
    try {
        host.resize((size_t)n * 8);
    } catch (...) {
        return fail(ctx, MCRT_ERR_HIP, "photon map: out of host memory for the recursive builder's copy of the list");
    }
    HIP_TRY(ctx, hipMemcpy(host.data(), d_photons, (size_t)n * 32, hipMemcpyDeviceToHost));
    mcrt_photon_map* M = nullptr;
    if (int rc2 = mcrt_photon_map_build(host.data(), n, bb_min, bb_max, max_node_data, &M)) return fail(ctx, rc2, "photon map: the recursive host builder failed");
    const int rc3 = uploadMap(ctx, which, mcrt_photon_map_get(M));
    mcrt_photon_map_free(M);
    return rc3;
}

int mcrt_upload_photons_device(mcrt_ctx* ctx, const float* d_global_photons, uint64_t global_count, const float* d_caustic_photons,
                               uint64_t caustic_count, const double bb_min[3], const double bb_max[3], uint32_t max_photons_per_leaf,
                               uint32_t k_nearest_photons, int direct_visualization, mcrt_photon_pass_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (k_nearest_photons == 0 || max_photons_per_leaf == 0 || !bb_min || !bb_max) return fail(ctx, MCRT_ERR_INVALID, "mcrt_upload_photons_device: bad argument");
    if ((global_count && !d_global_photons) || (caustic_count && !d_caustic_photons)) return fail(ctx, MCRT_ERR_INVALID, "mcrt_upload_photons_device: null photon list");
    REJECT_IF_PENDING(ctx, "mcrt_upload_photons_device");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    ctx->has_photons = false;
    ctx->k_nearest = k_nearest_photons;  // before the maps: the record lists expand octants with more than k photons
    double timing[3] = {0.0, 0.0, 0.0};
    if (int rc = buildMapAnyDepth(ctx, 0, d_global_photons, global_count, bb_min, bb_max, max_photons_per_leaf, timing)) return rc;
    if (int rc = buildMapAnyDepth(ctx, 1, d_caustic_photons, caustic_count, bb_min, bb_max, max_photons_per_leaf, timing)) return rc;
    ctx->direct_visualization = direct_visualization ? 1 : 0;
    ctx->has_photons = true;
    if (stats) {
        stats->global_count = global_count;
        stats->caustic_count = caustic_count;
        stats->global_octants = ctx->maps[0].num_octants;
        stats->caustic_octants = ctx->maps[1].num_octants;
        stats->sort_ms = timing[0];
        stats->octant_ms = timing[1];
        stats->finish_ms = timing[2];
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return MCRT_OK;
}

int mcrt_photon_pass_device(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed, const double bb_min[3],
                            const double bb_max[3], uint32_t max_photons_per_leaf, uint32_t k_nearest_photons, int direct_visualization,
                            mcrt_photon_pass_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    mcrt_photon_emission_device em;
    if (int rc = mcrt_emit_photons_device(ctx, emissions, caustic_factor, global_seed, 0, 1, &em)) return rc;
    mcrt_photon_pass_stats st;
    memset(&st, 0, sizeof(st));
    if (int rc = mcrt_upload_photons_device(ctx, em.d_global_photons, em.global_count, em.d_caustic_photons, em.caustic_count, bb_min, bb_max,
                                            max_photons_per_leaf, k_nearest_photons, direct_visualization, &st))
        return rc;
    st.emission_paths = em.emission_paths;
    st.rays = em.rays;
    st.emission_ms = em.kernel_ms;
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return MCRT_OK;
}

int mcrt_photon_map_download(mcrt_ctx* ctx, int which, mcrt_photon_map** out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!out || which < 0 || which > 1) return fail(ctx, MCRT_ERR_INVALID, "mcrt_photon_map_download: bad argument");
    if (!ctx->has_photons) return fail(ctx, MCRT_ERR_NO_PHOTONS, "mcrt_photon_map_download before the maps exist");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const PhotonMapView& v = ctx->maps[which];
    mcrt_photon_map* M = nullptr;
    try {  // (host copies of up to GBs: bad_alloc must not cross the C boundary)
    M = new mcrt_photon_map();
    const size_t no = v.num_octants, np = (size_t)v.num_photons;
    if (no) {
        std::vector<uint32_t> start(no), contained(no);
        M->bounds.resize(no * 6);
        M->next.resize(no);
        M->leaf.resize(no);
        M->photons.resize(np * 8);
        hipError_t e = hipMemcpy(M->bounds.data(), v.octant_bounds, no * 48, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(start.data(), v.octant_start, no * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(contained.data(), v.octant_contained, no * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(M->next.data(), v.octant_next, no * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(M->leaf.data(), v.octant_leaf, no, hipMemcpyDeviceToHost);
        if (e == hipSuccess && np) e = hipMemcpy(M->photons.data(), v.photons, np * 32, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            delete M;
            return fail(ctx, MCRT_ERR_HIP, std::string("mcrt_photon_map_download: ") + hipGetErrorString(e));
        }
        M->start.assign(start.begin(), start.end());
        M->contained.assign(contained.begin(), contained.end());
    }
    finishMapDesc(M);
    } catch (...) {
        delete M;
        return fail(ctx, MCRT_ERR_HIP, "mcrt_photon_map_download: out of host memory");
    }
    *out = M;
    return MCRT_OK;
}

}  // extern "C"

namespace mcrt {
// (kept HERE, where mcrt_intersect's body stood: kernel instantiations are emitted in the order of their first use, and that order is part
// of the code object tests/golden/device_code_hashes.json lists)
int intersectDeviceArrays(mcrt_ctx* ctx, uint64_t n, const double* d_start, const double* d_dir, double* d_t, uint32_t* d_surf, double* d_uv) {
    if (!ctx->scene.stage_all && ctx->scene.num_nodes > 0 && n <= 0xFFF00000ull) {  // (32-bit queue cursors with room for the waves' overshoot)
        // tree in HBM: the trace kernel of the wavefront pipeline, fed from the arrays
        const RenderOptions opt = parseRenderOptions(ctx->options);
        const int lean = traceVisit(opt, ctx->facts.q_single, false);
        auto trace = lean == 3 ? wfTraceKernel<ArrayRays, false, 3> : lean == 1 ? wfTraceKernel<ArrayRays, false, 1> : wfTraceKernel<ArrayRays, false>;
        if (!ctx->wf_ctrl.p) HIP_TRY(ctx, ctx->wf_ctrl.alloc(kWfCtrlWords * sizeof(unsigned long long)));
        TracePlan tp;
        if (int rc = planTrace(ctx, trace, n, opt.wf_leaf, tp)) return rc;
        unsigned long long ctrl_init[kWfCtrlRCount] = {};  // the ray queue's words: n rays queued, none handed out
        ctrl_init[kWfCtrlCount] = n;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->wf_ctrl.p, ctrl_init, sizeof(ctrl_init), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->stats.p, 0, kStatsWords * sizeof(unsigned long long), ctx->stream));
        ArrayRays ar{d_start, d_dir, d_t, d_surf, d_uv};
        const bool op_time = ctxOptOn(ctx, "MCRT_OP_TIME");  // kernel time of the operator to stderr
        if (op_time) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(trace, dim3(tp.grid), dim3(tp.block), tp.lds_bytes, ctx->stream, tp.args, ar);
        HIP_TRY(ctx, hipGetLastError());
        if (op_time) HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (op_time) {
            float ms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            fprintf(stderr, "[mcrt op] intersect (trace kernel): %llu rays in %.3f ms = %.1f Mray/s\n", (unsigned long long)n, ms, n / (ms * 1e3));
        }
        unsigned long long h[kStatsWords];
        HIP_TRY(ctx, hipMemcpy(h, ctx->stats.p, sizeof(h), hipMemcpyDeviceToHost));
        if (h[kStatOverflow]) return fail(ctx, MCRT_ERR_UNSUPPORTED, "traversal stack overflow (internal error: the stacks are sized to the tree's own bound, HostLayout::stack_bound)");
        return MCRT_OK;
    }
    LaunchGeom g;
    auto ikernel = ctx->scene.stage_all ? intersectKernel<true> : intersectKernel<false>;
    if (int rc = launchGeometry(ctx, ikernel, ctx->scene, g)) return rc;
    if (int rc = ensureScratch(ctx, g.total_lanes, false)) return rc;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(g.grid, (n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(ikernel, dim3(grid), dim3(kBlock), g.lds_bytes, ctx->stream, ctx->scene, n, d_start, d_dir, d_t, d_surf, d_uv,
                       ctx->spill.as<StackEntry>(), g.total_lanes);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCRT_OK;
}
}  // namespace mcrt

extern "C" {

int mcrt_intersect(mcrt_ctx* ctx, uint64_t n, const double* start, const double* direction, double* out_t, uint32_t* out_surface,
                   double* out_uv) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!ctx->has_scene) return fail(ctx, MCRT_ERR_NO_SCENE, "mcrt_intersect before mcrt_upload_scene");
    REJECT_IF_PENDING(ctx, "mcrt_intersect");
    if (n == 0) return MCRT_OK;
    if (!start || !direction || !out_t || !out_surface) return fail(ctx, MCRT_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf &ds = ctx->op_buf[0], &dd = ctx->op_buf[1], &dt = ctx->op_buf[2], &dsf = ctx->op_buf[3], &duv = ctx->op_buf[4];
    if (int rc = uploadInto(ctx, ds, start, n * 3)) return rc;
    if (int rc = uploadInto(ctx, dd, direction, n * 3)) return rc;
    HIP_TRY(ctx, dt.reserve(n * 8));
    HIP_TRY(ctx, dsf.reserve(n * 4));
    HIP_TRY(ctx, duv.reserve(n * 16));
    if (int rc = intersectDeviceArrays(ctx, n, ds.as<double>(), dd.as<double>(), dt.as<double>(), dsf.as<uint32_t>(), duv.as<double>())) return rc;
    HIP_TRY(ctx, hipMemcpy(out_t, dt.p, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out_surface, dsf.p, n * 4, hipMemcpyDeviceToHost));
    if (out_uv) HIP_TRY(ctx, hipMemcpy(out_uv, duv.p, n * 16, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

int mcrt_intersect_device(mcrt_ctx* ctx, uint64_t n, const double* d_start, const double* d_direction, double* d_t, uint32_t* d_surface,
                          double* d_uv) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!ctx->has_scene) return fail(ctx, MCRT_ERR_NO_SCENE, "mcrt_intersect_device before mcrt_upload_scene");
    REJECT_IF_PENDING(ctx, "mcrt_intersect_device");
    if (n == 0) return MCRT_OK;
    if (!d_start || !d_direction || !d_t || !d_surface) return fail(ctx, MCRT_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!d_uv) {  // the kernels write every hit's uv: a caller that does not want them gets the operators' scratch behind it
        HIP_TRY(ctx, ctx->op_buf[4].reserve(n * 16));
        d_uv = ctx->op_buf[4].as<double>();
    }
    return intersectDeviceArrays(ctx, n, d_start, d_direction, d_t, d_surface, d_uv);
}

int mcrt_sampler(mcrt_ctx* ctx, uint64_t n, const uint32_t* pixel, const uint32_t* index, uint32_t shuffles, uint32_t global_seed,
                 double* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (n == 0) return MCRT_OK;
    if (!pixel || !index || !out) return fail(ctx, MCRT_ERR_INVALID, "null argument");
    REJECT_IF_PENDING(ctx, "mcrt_sampler");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf &dp = ctx->op_buf[0], &di = ctx->op_buf[1], &dout = ctx->op_buf[2];
    if (int rc = uploadInto(ctx, dp, pixel, n)) return rc;
    if (int rc = uploadInto(ctx, di, index, n)) return rc;
    HIP_TRY(ctx, dout.reserve(n * 7 * 8));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(1024, (n + 255) / 256);
    hipLaunchKernelGGL(samplerKernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->sobol_tab.as<uint32_t>(), n, dp.as<uint32_t>(),
                       di.as<uint32_t>(), shuffles, global_seed, dout.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, dout.p, n * 7 * 8, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

int mcrt_bsdf(mcrt_ctx* ctx, uint64_t n, const double* in, const double* consts, double* out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (n == 0) return MCRT_OK;
    if (!in || !consts || !out) return fail(ctx, MCRT_ERR_INVALID, "null argument");
    REJECT_IF_PENDING(ctx, "mcrt_bsdf");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BsdfKatConsts c;
    fillBsdfKatConsts(c, consts);  // (mcrt_launch.hpp)
    DevBuf &din = ctx->op_buf[0], &dout = ctx->op_buf[1];
    if (int rc = uploadInto(ctx, din, in, n * 11)) return rc;
    HIP_TRY(ctx, dout.reserve(n * 18 * 8));
    hipLaunchKernelGGL(bsdfKernel, dim3(bsdfGrid(n)), dim3(256), 0, ctx->stream, n, din.as<double>(), c, dout.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, dout.p, n * 18 * 8, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

int mcrt_libm(mcrt_ctx* ctx, int fn, uint64_t n, const double* a, const double* b, double* out0, double* out1) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (fn < MCRT_LIBM_SINCOS || fn > MCRT_LIBM_POW) return fail(ctx, MCRT_ERR_INVALID, "mcrt_libm: unknown function selector");
    if (n == 0) return MCRT_OK;
    const bool two = fn == MCRT_LIBM_SINCOS || fn == MCRT_LIBM_SINCOSF, pair = fn == MCRT_LIBM_ATAN2 || fn == MCRT_LIBM_POW;
    if (!a || !out0 || (pair && !b) || (two && !out1)) return fail(ctx, MCRT_ERR_INVALID, "null argument");
    REJECT_IF_PENDING(ctx, "mcrt_libm");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf &da = ctx->op_buf[0], &db = ctx->op_buf[1], &d0 = ctx->op_buf[2], &d1 = ctx->op_buf[3];
    if (int rc = uploadInto(ctx, da, a, n)) return rc;
    if (pair)
        if (int rc = uploadInto(ctx, db, b, n)) return rc;
    HIP_TRY(ctx, d0.reserve(n * 8));
    HIP_TRY(ctx, d1.reserve(n * 8));
    if (fn == MCRT_LIBM_POW) {  // (the output stage's function: its kernel lives with that stage, mcrt_output.hip)
        HIP_TRY(ctx, (hipError_t)launchPowKat(ctx->stream, n, da.as<double>(), db.as<double>(), d0.as<double>()));
    } else {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(4096, (n + 255) / 256);
        hipLaunchKernelGGL(libmKernel, dim3(grid), dim3(256), 0, ctx->stream, fn, n, da.as<double>(), db.as<double>(), d0.as<double>(), d1.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out0, d0.p, n * 8, hipMemcpyDeviceToHost));
    if (two) HIP_TRY(ctx, hipMemcpy(out1, d1.p, n * 8, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

int mcrt_knn(mcrt_ctx* ctx, int which, uint64_t n, const double* p, uint32_t k, uint32_t* out_count, uint32_t* out_index,
             double* out_distance2) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (!ctx->has_photons) return fail(ctx, MCRT_ERR_NO_PHOTONS, "mcrt_knn before mcrt_upload_photons");
    REJECT_IF_PENDING(ctx, "mcrt_knn");
    if (which < 0 || which > 1 || k == 0) return fail(ctx, MCRT_ERR_INVALID, "bad map selector or k");
    if (n == 0) return MCRT_OK;
    if (!p || !out_count || !out_index || !out_distance2) return fail(ctx, MCRT_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const char* kenv = ctxOpt(ctx, "MCRT_KERNEL");
    if (k <= waveMaxK(kWaveRowsLarge) && !(kenv && strcmp(kenv, "legacy") == 0)) {  // wave-cooperative search (mcrt_waveknn.hpp)
        DevBuf &dp = ctx->op_buf[0], &dc = ctx->op_buf[1], &di = ctx->op_buf[2], &dd = ctx->op_buf[3], &flags = ctx->op_buf[4];
        if (int rc = uploadInto(ctx, dp, p, n * 3)) return rc;
        HIP_TRY(ctx, dc.reserve(n * 4));
        HIP_TRY(ctx, di.reserve(n * k * 4));
        HIP_TRY(ctx, dd.reserve(n * k * 8));
        HIP_TRY(ctx, flags.reserve(8));
        HIP_TRY(ctx, hipMemsetAsync(flags.p, 0, 8, ctx->stream));
        const PhotonMapViewW mv = waveMapView(ctx, which);
        const int per_cu = 8;  // 256-lane workgroups per CU; MCRT_KNN_TIME=1: kernel time on stderr
        HIP_TRY(ctx, ctx->knn_spill.reserve((size_t)ctx->num_cus * per_cu * 4 * kWaveSpill * 12));
        const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)ctx->num_cus * per_cu, (n + 3) / 4);
        // MCRT_KNN_GROUPS=1: four queries per wave, one per row of 16 lanes (mcrt_groupknn.hpp)
        const bool groups = k <= kGrpMaxK && ctxOptOn(ctx, "MCRT_KNN_GROUPS");
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        if (groups)
            hipLaunchKernelGGL(knnGroupKernel, dim3(std::min<uint32_t>(grid, (uint32_t)((n + 15) / 16))), dim3(256), 0, ctx->stream, mv, n, dp.as<double>(), k,
                               dc.as<uint32_t>(), di.as<uint32_t>(), dd.as<double>(), flags.as<unsigned long long>());
        else
            hipLaunchKernelGGL((k > waveMaxK(kWaveRows) ? knnWaveKernel<kWaveRowsLarge> : knnWaveKernel<kWaveRows>), dim3(grid), dim3(256), 0, ctx->stream, mv, n,
                               dp.as<double>(), k, dc.as<uint32_t>(), di.as<uint32_t>(), dd.as<double>(), flags.as<unsigned long long>(),
                               ctx->knn_spill.as<uint32_t>());
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctxOptOn(ctx, "MCRT_KNN_TIME")) {
            float ms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            fprintf(stderr, "[mcrt knn] map %d: %llu searches, k = %u, %d workgroups per CU: %.3f ms = %.1f M searches/s\n", which,
                    (unsigned long long)n, k, per_cu, ms, (double)n / ms / 1e3);
        }
        unsigned long long f = 0;
        HIP_TRY(ctx, hipMemcpy(&f, flags.p, 8, hipMemcpyDeviceToHost));
        if (ctxOptOn(ctx, "MCRT_TEST_KNN_OVERFLOW")) f = 1;  // (test hook: take the branch below whatever the searches did)
        if (!f) {
            HIP_TRY(ctx, hipMemcpy(out_count, dc.p, n * 4, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(out_index, di.p, n * k * 4, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(out_distance2, dd.p, n * k * 8, hipMemcpyDeviceToHost));
            return MCRT_OK;
        }
        // a search had more octants pending at once than the wave's frontier holds (128 in registers + a 1 024-entry list in memory for the
        // wave-per-query kernel; 128 for the four-queries-per-wave kernel of small k): the call is served by the per-lane kernel below,
        // whose frontier grows (the reference's queue is unbounded, linear-octree.cpp:33; until round 6: MCRT_ERR_UNSUPPORTED)
        ctx->knn_visit_cap = std::max<uint32_t>(ctx->knn_visit_cap, 2048u);
    }
    const uint32_t block = 64;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)ctx->num_cus * 8, (n + block - 1) / block);
    const uint32_t lanes = grid * block;
    DevBuf dp, dc, di, dd, r_d2, r_idx, v_d2, v_oct, lane_flag;
    if (int rc = uploadArray(ctx, dp, p, n * 3)) return rc;
    HIP_TRY(ctx, dc.alloc(n * 4));
    HIP_TRY(ctx, di.alloc(n * k * 4));
    HIP_TRY(ctx, dd.alloc(n * k * 8));
    HIP_TRY(ctx, r_d2.alloc((size_t)lanes * k * 8));
    HIP_TRY(ctx, r_idx.alloc((size_t)lanes * k * 4));
    HIP_TRY(ctx, lane_flag.alloc(8));
    for (;;) {  // (the per-lane frontier: 160 entries per lane to begin with, eight times as many whenever a search ran out)
        const uint32_t cap = ctx->knn_visit_cap;
        HIP_TRY(ctx, v_d2.alloc((size_t)lanes * cap * 8));
        HIP_TRY(ctx, v_oct.alloc((size_t)lanes * cap * 4));
        HIP_TRY(ctx, hipMemsetAsync(lane_flag.p, 0, 8, ctx->stream));
        hipLaunchKernelGGL(knnKernel, dim3(grid), dim3(block), 0, ctx->stream, ctx->maps[which], n, dp.as<double>(), k, dc.as<uint32_t>(),
                           di.as<uint32_t>(), dd.as<double>(), r_d2.as<double>(), r_idx.as<uint32_t>(), v_d2.as<double>(),
                           v_oct.as<uint32_t>(), lanes, cap, lane_flag.as<unsigned long long>());
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        unsigned long long f = 0;
        HIP_TRY(ctx, hipMemcpy(&f, lane_flag.p, 8, hipMemcpyDeviceToHost));
        if (!f) break;
        if (cap >= kMaxVisitLimit)
            return fail(ctx, MCRT_ERR_UNSUPPORTED, "kNN frontier overflow: a search had more than " + std::to_string(kMaxVisitLimit) + " octants pending at once (per-lane kernel)");
        ctx->knn_visit_cap = std::min<uint32_t>(cap * 8u, kMaxVisitLimit);
    }
    HIP_TRY(ctx, hipMemcpy(out_count, dc.p, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out_index, di.p, n * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out_distance2, dd.p, n * k * 8, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

}  // extern "C"

namespace mcrt {
int ctxDevice(const mcrt_ctx* ctx) { return ctx->device; }
void* ctxStream(const mcrt_ctx* ctx) { return (void*)ctx->stream; }
int ctxFail(mcrt_ctx* ctx, int code, const std::string& msg) { return fail(ctx, code, msg); }

// the hooks of the image passes' host toolkit (mcrt_internal.hpp)
int ctxIdle(mcrt_ctx* ctx, const char* what) {
    if (ctx->pending) return fail(ctx, MCRT_ERR_INVALID, std::string(what) + ": a render is in flight, call mcrt_render_finish first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return MCRT_OK;
}
int ctxNeedScene(mcrt_ctx* ctx, const char* what) {
    return ctx->has_scene ? MCRT_OK : fail(ctx, MCRT_ERR_NO_SCENE, std::string(what) + " before mcrt_upload_scene");
}
void* ctxPassScratch(mcrt_ctx* ctx, PassFamily family, int which, size_t bytes) {
    if (family < 0 || family >= kPassFamilies || which < 0 || which >= kPassSlots) return nullptr;
    DevBuf& buf = ctx->pass_buf[family][which];
    if (buf.reserve(std::max<size_t>(bytes, 8)) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return buf.p;
}
void ctxAovScene(const mcrt_ctx* ctx, AovScene* out, const uint32_t** sobol_tab) {
    const DeviceScene& d = ctx->scene;
    out->sh.surf_v = d.surf_v;
    out->sh.surf_normal = d.surf_normal;
    out->sh.surf_vn = d.surf_vn;
    out->sh.surf_area = d.surf_area;
    out->sh.surf_material = d.surf_material;
    out->sh.surf_kind = d.surf_kind;
    out->sh.surf_rec = d.surf_rec;
    out->sh.materials = d.materials;
    out->sh.num_lights = d.num_lights;
    out->sh.light_surface = d.light_surface;
    out->sh.light_cdf = d.light_cdf;
    out->sh.scene_ior = d.scene_ior;
    out->prim = d.prim;
    *sobol_tab = d.sobol_tab;
}
void ctxSceneCounts(const mcrt_ctx* ctx, uint32_t* num_surfaces, uint32_t* num_materials) {
    *num_surfaces = (uint32_t)ctx->scene.num_surfaces;
    *num_materials = (uint32_t)ctx->scene.num_materials;
}
// what a render may take per-sample channels for: idle, a scene, a camera, and a film that keeps its samples when a channel is wanted
int ctxSampleTargetsBegin(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_frame_summary* targets, const char* what) {
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (int rc = ctxNeedScene(ctx, what)) return rc;
    if (!cam) return fail(ctx, MCRT_ERR_INVALID, std::string(what) + ": camera is NULL");
    const char* noun = summaryWantsHighlights(*targets) ? "highlights" : summaryWantsStats(*targets) ? "statistics" : nullptr;
    if (noun && filmSplats(cam->film_filter, cam->film_radius))
        return fail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": a frame whose film splats (a reconstruction filter, or a box of another radius) keeps no "
                                               "samples: there is nothing to take the " + noun + " of");
    ctx->sample_targets = *targets;
    ctx->sample_targets.rgb = nullptr;
    return MCRT_OK;
}
void ctxSampleTargetsEnd(mcrt_ctx* ctx) { ctx->sample_targets = mcrt_frame_summary{}; }
const mcrt_lens_desc* ctxLens(const mcrt_ctx* ctx) { return ctx->lens.model != MCRT_LENS_NONE ? &ctx->lens : nullptr; }
void ctxSetLens(mcrt_ctx* ctx, const mcrt_lens_desc& lens) { ctx->lens = lens; }
const mcrt_ray_source_desc* ctxRaySource(const mcrt_ctx* ctx) { return ctx->ray_source.kind != MCRT_RAY_SOURCE_NONE ? &ctx->ray_source : nullptr; }
void ctxSetRaySource(mcrt_ctx* ctx, const mcrt_ray_source_desc& source, void* owned_first, void* owned_second) {
    (void)hipSetDevice(ctx->device);
    ctx->ray_source = source;
    ctx->ray_source_owned[0].release();
    ctx->ray_source_owned[1].release();
    ctx->ray_source_owned[0].p = owned_first;
    ctx->ray_source_owned[1].p = owned_second;
}
}  // namespace mcrt
