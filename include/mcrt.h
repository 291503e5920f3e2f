/*
 * mcrt.h — C ABI of libmcrt_hip.so, the MI355X (gfx950) path-tracing / BVH-traversal /
 * photon-kNN engine that drops in behind linusmossberg/monte-carlo-ray-tracer's
 * Camera::sampleImage() (reference: source/camera/camera.cpp:101-145).
 *
 * The reference has no FFI; its seam is the C++ call Camera::sampleImage(), whose contract is
 * "on return camera.image(x,y) holds the filtered mean radiance of every pixel"
 * (camera/camera.cpp:138-144, camera/image.cpp:53-56). The entry points below are what a
 * maintainer binds in its place (binding stub: INTEGRATION.md). Everything is plain pointers and
 * sizes; no C++ types, no torch types, no exceptions cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success or a negative mcrt_status; mcrt_last_error() gives text
 *     (the reference's convention is exceptions caught in main, source/main.cpp:24-32,48-56);
 *   - all *_desc arrays are host memory owned by the caller and are copied during the call;
 *   - all floating point is FP64 unless the field says otherwise (the reference computes in
 *     glm::dvec3 everywhere; only stored photons are FP32, integrator/photon-mapper/photon.hpp:36-37);
 *   - the library never falls back to a CPU path: without a gfx950 device mcrt_create fails.
 */
#ifndef MCRT_H
#define MCRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCRT_ABI_VERSION 2u

typedef enum mcrt_status {
    MCRT_OK = 0,
    MCRT_ERR_INVALID = -1,      /* bad argument / inconsistent descriptor            */
    MCRT_ERR_NO_DEVICE = -2,    /* no gfx950 device / HIP runtime error at create    */
    MCRT_ERR_HIP = -3,          /* HIP runtime error (text in mcrt_last_error)       */
    MCRT_ERR_NO_SCENE = -4,     /* render called before mcrt_upload_scene            */
    MCRT_ERR_NO_PHOTONS = -5,   /* photon-mapping render without mcrt_upload_photons */
    MCRT_ERR_IO = -6,           /* scene-image file could not be read / parsed       */
    MCRT_ERR_UNSUPPORTED = -7   /* e.g. quadric surfaces, non-box film filter        */
} mcrt_status;

/* ------------------------------------------------------------------------------------------
 * Scene. Replaces the data reached through Integrator::scene (integrator/integrator.hpp:26):
 * Scene::{surfaces, emissives, cumulative_emissives_importance, bvh, ior} (scene/scene.hpp:27-40),
 * BVH::{linear_tree, ordered_surfaces} (bvh/bvh.hpp:105-108) and the per-surface / per-material
 * fields the hot path reads.
 * ---------------------------------------------------------------------------------------- */

enum { MCRT_SURF_TRIANGLE = 0, MCRT_SURF_SPHERE = 1, MCRT_SURF_QUADRIC = 2 };

/* Material flag bits = the bools of class Material (material/material.hpp:41-44) as they stand
 * AFTER scene construction (scene/scene.cpp:83-89 copies materials without recomputing them). */
enum {
    MCRT_MAT_ROUGH = 1u << 0,
    MCRT_MAT_ROUGH_SPECULAR = 1u << 1,
    MCRT_MAT_OPAQUE = 1u << 2,
    MCRT_MAT_EMISSIVE = 1u << 3,
    MCRT_MAT_DIRAC_DELTA = 1u << 4,
    MCRT_MAT_PERFECT_MIRROR = 1u << 5,
    MCRT_MAT_COMPLEX_IOR = 1u << 6
};

/* One record per Material object (material/material.hpp:9-55). emittance is the value left by
 * Scene::generateEmissives (scene/scene.cpp:202), i.e. radiosity, not flux. */
typedef struct mcrt_material {
    double reflectance[3];
    double specular_reflectance[3];
    double transmittance[3];
    double emittance[3];
    double roughness, specular_roughness, ior, transparency;
    double A, B;           /* Oren-Nayar terms, material.cpp:106-108       */
    double a[2];           /* GGX alpha, material.cpp:110                  */
    double ior_real[3];    /* ComplexIOR::real      (material/fresnel.hpp:6-11) */
    double ior_imag[3];    /* ComplexIOR::imaginary                         */
    uint32_t flags;        /* MCRT_MAT_*                                    */
    uint32_t reserved;
} mcrt_material;

typedef struct mcrt_scene_desc {
    uint32_t abi_version;              /* MCRT_ABI_VERSION */

    /* BVH::linear_tree in the reference's depth-first order (bvh/bvh.hpp:68-74).
     * num_nodes == 0 selects the brute-force loop of Scene::intersect (scene/scene.cpp:161-173). */
    uint32_t num_nodes;
    const double*   node_bounds;        /* [num_nodes][6]  BB.min xyz, BB.max xyz      */
    const uint32_t* node_start_surface; /* [num_nodes]                                  */
    const uint32_t* node_num_surfaces;  /* [num_nodes]  >0 ⇒ leaf (uint8 in reference) */
    const uint32_t* node_next_sibling;  /* [num_nodes]  0 ⇒ none                       */

    /* Surfaces in BVH::ordered_surfaces order (Scene::surfaces order when num_nodes == 0). */
    uint32_t num_surfaces;
    const uint8_t*  surf_kind;          /* MCRT_SURF_*                                          */
    const uint8_t*  surf_interpolate;   /* 1 ⇔ Triangle::N != nullptr (surface/triangle.cpp:56) */
    const uint32_t* surf_material;      /* index into materials                                 */
    const double*   surf_area;          /* Base::area_                                          */
    const double*   surf_v;             /* [n][9] triangle: v0,v1,v2 · sphere: origin,radius,0… · quadric: record index,0… */
    const double*   surf_e;             /* [n][9] triangle: E1,E2,normal_ · sphere: unused      */
    const double*   surf_vn;            /* [n][9] vertex normals N[0..2], or NULL if none       */

    uint32_t num_materials;
    const mcrt_material* materials;

    /* Scene::emissives / cumulative_emissives_importance in the order the reference produced. */
    uint32_t num_lights;
    const uint32_t* light_surface;      /* index into the surface arrays above */
    const double*   light_cdf;

    double scene_ior;                   /* Scene::ior (scene/scene.cpp:22)   */
    double bb_min[3], bb_max[3];        /* Scene::BB()                        */

    /* Surface::Quadric (surface/surface.hpp:99-116, surface/quadric.cpp). One record of 22 doubles per quadric:
     * Q as glm stores it (column-major: Q[c][r] at 4*c + r; the gradient matrix G is 2 * its upper 3 rows,
     * quadric.cpp:38-45), then BB_.min, BB_.max — the box that slices the quadric (quadric.cpp:36,72-76,92).
     * Surface i of kind MCRT_SURF_QUADRIC names its record in surf_v[9*i] (an integer stored as a double).
     * Quadrics cannot be emissive (scene/scene.cpp:125). */
    uint32_t num_quadrics;
    const double*   quadrics;           /* [num_quadrics][22] */
} mcrt_scene_desc;

/* ------------------------------------------------------------------------------------------
 * Photon maps. Replaces PhotonMapper::{caustic_map, global_map} =
 * LinearOctree<Photon>::{linear_tree, ordered_data} (octree/linear-octree.hpp:19-29).
 * ---------------------------------------------------------------------------------------- */
typedef struct mcrt_photon_map_desc {
    uint32_t num_octants;
    const double*   octant_bounds;          /* [n][6] tight BB min,max (linear-octree.cpp:220,241) */
    const uint64_t* octant_start_data;
    const uint64_t* octant_contained_data;
    const uint32_t* octant_next_sibling;    /* 0xFFFFFFFF ⇒ none (linear-octree.hpp:36) */
    const uint8_t*  octant_leaf;
    uint64_t num_photons;
    const float*    photons;                /* [n][8] flux rgb, position xyz, phi, theta (photon.hpp:36-37) */
} mcrt_photon_map_desc;

/* ------------------------------------------------------------------------------------------
 * Camera. The public fields of class Camera read by samplePixel (camera/camera.hpp:39-51,
 * camera/camera.cpp:66-99) plus the work split.
 * ---------------------------------------------------------------------------------------- */
typedef struct mcrt_camera_desc {
    double eye[3], forward[3], left[3], up[3];
    double focal_length, sensor_width, aperture_radius, focus_distance;
    uint32_t thin_lens;
    uint32_t width, height;
    uint32_t sqrtspp;
    /* Image-space sharding (multi-GPU): rows are dealt to shards in groups of shard_rows rows,
     * group g belongs to shard g % shard_count. shard_count <= 1 renders every row. Per-pixel
     * seeding stays hashCombine(global_seed, hash(y*width+x)) (camera.cpp:73, sampler.hpp:32-35)
     * so the image is independent of the split. */
    uint32_t shard_index, shard_count, shard_rows;
    /* Film reconstruction filter (camera/film.cpp:19-58, camera/filter.hpp): MCRT_FILM_BOX is the reference's default
     * Film(width, height): radius 0.5, every sample lands in its own pixel with weight 1. Any other filter makes every
     * sample a splat over the pixels within film_radius (0 = the filter's default radius, film.cpp:31-44), weights from
     * the filter function or, when film_cache_size > 0, from a table of that many samples of it (film.cpp:49-57,86-97);
     * such frames are rendered by the wavefront pipeline (either integrator; shard_count <= 1, or sharded through
     * mcrt_render_film_device; a scene without a BVH is walked through a tree over index ranges there). */
    uint32_t film_filter;
    double   film_radius;
    uint32_t film_cache_size;
    uint32_t reserved;
} mcrt_camera_desc;

enum { MCRT_FILM_BOX = 0, MCRT_FILM_MITCHELL_NETRAVALI = 1, MCRT_FILM_CATMULL_ROM = 2, MCRT_FILM_B_SPLINE = 3, MCRT_FILM_HERMITE = 4,
       MCRT_FILM_GAUSSIAN = 5, MCRT_FILM_LANCZOS = 6 };

enum { MCRT_INTEGRATOR_PATH_TRACER = 0, MCRT_INTEGRATOR_PHOTON_MAPPER = 1 };

typedef struct mcrt_stats {
    uint64_t paths;         /* pixel samples traced = Integrator::sampleRay calls             */
    uint64_t rays;          /* closest-hit queries  = Scene::intersect calls (bounce + shadow) */
    uint64_t node_tests;    /* BoundingBox::intersect calls performed by the GPU traversal     */
    uint64_t prim_tests;    /* primitive intersect calls performed by the GPU traversal        */
    uint64_t knn_searches;  /* LinearOctree::knnSearch calls                                   */
    double   kernel_ms;     /* HIP-event time of the integrator kernel(s) on their stream      */
    double   total_ms;      /* wall time of the call incl. copies                              */
    uint32_t kernel_launches;
    uint32_t kernel_id;     /* MCRT_KERNEL_*: which kernel form traced the frame (tests pin it, so a silent
                             * change of the selection rule in launchRender cannot pass unnoticed)            */
} mcrt_stats;

/* Kernel forms of the integrator; mcrt_stats.kernel_id of the last mcrt_render*. */
enum {
    MCRT_KERNEL_NONE = 0,          /* nothing launched (a shard that owns no rows)                                   */
    MCRT_KERNEL_FLAT = 1,          /* renderKernel, flat-scene instance: wave-uniform loop over all primitives, scene in LDS */
    MCRT_KERNEL_WAVESYNC = 2,      /* renderKernel<path tracer>, wave-synchronous bounce loop (MCRT_KERNEL=legacy, instrumented runs) */
    MCRT_KERNEL_LANE_SM = 3,       /* renderKernelSM: per-lane state machine megakernel                               */
    MCRT_KERNEL_WAVEFRONT = 4,     /* wfShadeKernel + wfTraceKernel over the slot pool                               */
    MCRT_KERNEL_PM_WAVE = 5,       /* renderKernelPM: photon mapper, wave-cooperative kNN estimates                  */
    MCRT_KERNEL_PM_LANE = 6,       /* renderKernel<photon mapper>: per-lane kNN (k > 768, MCRT_KERNEL=legacy)        */
    MCRT_KERNEL_WAVEFRONT_PM = 7   /* wavefront pipeline with kNN launches (MCRT_KERNEL=wf, photon-mapped frames)    */
};

typedef struct mcrt_ctx mcrt_ctx; /* opaque; owns all device memory and one HIP stream */

/* Lifecycle. device_id = HIP ordinal of the gfx950 device this context drives (one context per
 * device / per process rank). */
int  mcrt_create(mcrt_ctx** out, int device_id);
/* Number of HIP devices this process sees (0: none, or the runtime cannot start) - what a one-process host sizes its set of contexts
 * by before mcrt_render_multi; the reference's counterpart is std::thread::hardware_concurrency() (integrator/integrator.cpp:20-24).
 * mcrt_create still refuses a device that is not gfx950. */
int  mcrt_device_count(void);
void mcrt_destroy(mcrt_ctx* ctx);
const char* mcrt_last_error(const mcrt_ctx* ctx); /* ctx may be NULL: last create error */

/* Run-time options of a context: kernel selection and tuning knobs for A/B runs and parity tests (DESIGN.md "Run-time
 * options" lists them; defaults are the measured best). Keys are MCRT_* names, values decimal numbers or words. The process
 * environment SEEDS the options once, in mcrt_create (so `MCRT_KERNEL=wf ./host` still works); after that the library never
 * reads the environment: a host changes behaviour with mcrt_set_option, between frames (value NULL = back to the default).
 * Options that shape the uploaded scene (MCRT_FLAT_MAX) take effect at the next mcrt_upload_scene.
 * The reference has no counterpart (its knobs are compile-time constants); mcrt_get_option returns the value or NULL.
 * Read-only: MCRT_LEAN_USED, and MCRT_INSTANCES_USED = the kernel instances of the last launch as "frame,trace,knn" ("-": none). */
int mcrt_set_option(mcrt_ctx* ctx, const char* key, const char* value);
const char* mcrt_get_option(const mcrt_ctx* ctx, const char* key);

int mcrt_upload_scene(mcrt_ctx* ctx, const mcrt_scene_desc* scene);
int mcrt_upload_photons(mcrt_ctx* ctx, const mcrt_photon_map_desc* global_map,
                        const mcrt_photon_map_desc* caustic_map,
                        uint32_t k_nearest_photons, int direct_visualization);

/* Replaces the thread fan-out of Camera::sampleImage (camera.cpp:120-144): renders every owned
 * pixel with spp = sqrtspp^2 samples and writes image(x,y) as FP64 RGB, row-major, width*height*3
 * doubles, into caller-allocated HOST memory (rows not owned by this shard are left untouched).
 * global_seed replaces Sampler::global_seed (sampling/sampler.hpp:58).
 * PARITY: a path-traced frame (MCRT_INTEGRATOR_PATH_TRACER) of the default (exact) library is the reference's bits. A photon-mapped
 * frame of the default kernels is held to 1e-10 relative of the reference, not to its bits: the k photons of a radiance estimate are
 * added by a wave reduction instead of in the reference's heap order, and Photon::dir takes the platform's sinf / cosf (measured
 * <= 1e-12). Option MCRT_KERNEL=legacy selects the per-lane photon kernel, which keeps the reference's heap discipline and its
 * sincosf - its frames ARE the reference's bits, at a tenth of the speed. The opt-in tolerance library (libmcrt_hip_tol.so) is held
 * to BASELINE.json's 1e-4 for every frame. */
int mcrt_render(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                double* out_rgb, mcrt_stats* stats /* may be NULL */);

/* Same, but the image stays in DEVICE memory owned by the caller (e.g. the buffer RCCL gathers
 * from) and the launch is asynchronous on `stream` (a hipStream_t; NULL = the context's stream).
 * d_out_rgb holds owned rows only, packed in ascending row order: mcrt_shard_rows() rows of
 * width*3 doubles. Call mcrt_render_finish() to wait and collect stats. (Path-traced frames whose tree is walked by the
 * wavefront pipeline run as a host-driven sequence of launches on `stream`; for them the call BLOCKS until the frame is complete and
 * mcrt_render_finish() only collects the statistics. The pipeline is chosen for BVHs of 65 536 nodes or more (MCRT_WF_MIN_NODES) and,
 * for ANY tree that is not staged whole in LDS, for calls of 32 M path samples or more (MCRT_WF_MIN_PATHS) — counted over the rows THIS
 * call owns, the work the pipeline's launches are amortised over: the measured crossover. Shards of one frame that
 * straddle the threshold may therefore run different kernel forms on different ranks; every form returns the same bits, so the frame
 * does not depend on it, only mcrt_stats.kernel_id and whether this call blocks. MCRT_KERNEL=wf / sm pins the form.)
 * ORDERING: queue consumers of d_out_rgb (copies, reductions, the gather) AFTER mcrt_render_finish() has returned MCRT_OK, not right
 * after this call: a megakernel frame in which a path nests deeper than the eight dielectric media a lane keeps in LDS is rendered
 * AGAIN by mcrt_render_finish through the wavefront pipeline (32 media; mcrt_stats.kernel_id then says MCRT_KERNEL_WAVEFRONT[_PM] and
 * kernel_ms / kernel_launches describe that second run), into the same d_out_rgb on the same stream. */
int mcrt_render_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed,
                       int integrator, double* d_out_rgb, void* stream);
int mcrt_render_finish(mcrt_ctx* ctx, mcrt_stats* stats /* may be NULL */);

/* Reconstruction-filter frames across GPUs. With a filter other than the box a sample is a splat over
 * the pixels within the filter radius (Film::deposit, camera/film.cpp:61-79), so the samples of one shard's rows also
 * land in its neighbours' rows: every shard accumulates into a FULL-frame copy of Film's blob — width*height records of
 * {rgb_sum[3], weight_sum} (camera/film.hpp:22-37), 4 doubles each, overwritten by this call — the host sums the shards'
 * buffers (one RCCL all-reduce / reduce; with shard_count 1 there is nothing to sum) and mcrt_film_resolve_device applies
 * Splat::get (film.hpp:31-35, Film::scan film.cpp:81-84) to the sum: width*height*3 doubles, full frame. The reference
 * adds the same splats with std::atomic<double> in thread-timing order, so sums agree to rounding (1e-12), not bits.
 * cam->film_filter must not be MCRT_FILM_BOX. Returns when the shard's samples are complete
 * (mcrt_render_finish() then collects the statistics). */
int mcrt_render_film_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_rgbw,
                            void* stream);
int mcrt_film_resolve_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* d_rgbw, double* d_out_rgb, void* stream);

/* One host process driving several GPUs — the shape of the reference's host, whose Camera::sampleImage fans out to worker
 * threads (camera/camera.cpp:120-136). ctxs[i] is a context on device i's GPU with the scene (and photon maps) already
 * uploaded; the frame's rows are dealt over the contexts (cam->shard_rows per group, 0 = 8; cam->shard_index/count are
 * ignored), every context is driven by its own host thread and copies its rows into out_rgb (full frame, host memory). No
 * collective: shards are independent and Image::save wants the frame on the host anyway. Reconstruction-filter frames are
 * summed and resolved on the host. stats: counters summed over the contexts, times = the slowest context's. The result does
 * not depend on the number of contexts (box filter: bit for bit). */
int mcrt_render_multi(mcrt_ctx* const* ctxs, uint32_t count, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                      double* out_rgb, mcrt_stats* stats /* may be NULL */);

/* Number of rows owned by (shard_index, shard_count, shard_rows) of `cam`, and their indices. */
uint32_t mcrt_shard_rows(const mcrt_camera_desc* cam, uint32_t* rows /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * First-hit AOV pass: the geometry buffers compositing, denoising and scene debugging read next to the beauty frame. The
 * reference has no such output; every value is one it computes on the way to a pixel. The samples are the beauty frame's
 * own: for sample i in 0..sqrtspp^2-1 of pixel (x, y) the ray is Camera::samplePixel's (camera/camera.cpp:79-95, thin lens
 * included) with the sampler at initiate(y*width+x), setIndex(i) (camera.cpp:73-77) and Sampler::global_seed = global_seed,
 * so a frame made with the camera and seed of an mcrt_render lines up with it sample for sample. Per sample, with
 * hit = Scene::intersect(ray) (scene/scene.cpp:151-176) and what Interaction's constructor derives from it before any material
 * decision (ray/interaction.cpp:12-36):
 *   P  = ray(t) (ray/ray.cpp:69-72) · N = surface->normal(P) · Ns = interpolate ? interpolatedNormal(uv) : N, back to N when
 *   (dot(d,N) < 0) != (dot(d,Ns) < 0) (:23-30) · both negated when dot(d,N) > 0 (:32-36) · albedo = material->reflectance.
 * Per pixel every channel word is summed by ONE FP64 accumulator in ascending sample index - the frame does not depend on
 * chunking (option MCRT_AOV_CHUNK_RAYS: rays per launch group, default 2^24, always whole pixels), sharding or launch shape, bit
 * for bit:
 *   coverage                        hits / spp
 *   normal, shading_normal, albedo  (sum over the hit samples) / spp  - a miss adds zero
 *   position                        (sum over the hit samples) / hits - zeros at coverage 0
 *   depth                           (sum of t over the hit samples) / hits - DBL_MAX at coverage 0 (ray/intersection.hpp:14)
 *   surface, material               the hit of sample 0: index into the uploaded surface / material arrays, 0xFFFFFFFF on a miss
 * cam->shard_* is honoured exactly as in mcrt_render_device; cam->film_* is IGNORED: AOVs are per-pixel box means whatever filter
 * the beauty frame is reconstructed with. The closest hits come from the kernels behind mcrt_intersect, unchanged. Both calls are
 * synchronous on the context's stream, and refused while a render is in flight or before mcrt_upload_scene.
 * stats: paths = rays = samples traced, kernel_ms (HIP events around the pass's launches), total_ms, kernel_launches. */
typedef struct mcrt_aov_buffers {      /* every pointer may be NULL = channel not wanted; DEVICE memory, owned rows only,  */
    double*   depth;           /* [rows][width]     packed in ascending row order like mcrt_render_device's d_out_rgb      */
    double*   position;        /* [rows][width][3] */
    double*   normal;          /* [rows][width][3] */
    double*   shading_normal;  /* [rows][width][3] */
    double*   albedo;          /* [rows][width][3] */
    double*   coverage;        /* [rows][width]    */
    uint32_t* surface;         /* [rows][width]    */
    uint32_t* material;        /* [rows][width]    */
} mcrt_aov_buffers;
int mcrt_render_aov_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_aov_buffers* buffers,
                           mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers to FULL frames ([height][width]...): rows this shard does not own are left untouched. */
int mcrt_render_aov(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_aov_buffers* buffers,
                    mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Denoised output: the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010 on a beauty frame, guided by the AOV frame
 * of the same camera and seed (mcrt_render_aov*). The reference has no such output. The filter uses only FP64 + - * /, compare
 * and select, in the order written here, uncontracted: the result is a function of its inputs bit for bit, whatever the launch
 * shape, tiling or stream, and no libm routine takes part.
 *
 * Inputs are FULL frames [height][width]...: the beauty frame c (FP64 RGB) and guides->shading_normal Ns, normal N, position P,
 * coverage, albedo (depth, surface, material are not read). A frame gathered from shards is filtered after the gather: the
 * filter reads neighbouring rows, so there is no shard form.
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, |a|^2 = dot(a, a);  max0(x) = x < 0 ? 0 : x (a NaN stays a NaN).
 * Demodulate, per pixel and channel: a = albedo > albedo_floor ? albedo : 1.0, I_0 = c / a. With MCRT_DENOISE_NO_ALBEDO a = 1 and
 * guides->albedo may be NULL.
 * Iterate, for i = 0 .. iterations-1 with step s = 2^i and inv_c = 1.0 / (sc * sc), sc = sigma_color * 2^-i, sz2 = sigma_plane *
 * sigma_plane (both computed once on the host):
 *   a pixel p with coverage(p) == 0 keeps its value, I_{i+1}(p) = I_i(p). For every other p the taps q = p + s * (dx, dy) are
 *   visited with dy = -2..2 as the outer and dx = -2..2 as the inner loop; taps outside the frame are skipped;
 *   h = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *     the centre tap (dx = dy = 0) has weight w = 9/64 exactly (so the weight sum is never zero);
 *     a tap with coverage(q) == 0 is skipped (weight 0: it contributes nothing);
 *     every other tap has w = (((h[dy] * h[dx]) * w_n) * w_z) * w_c with
 *       w_n = max0(dot(Ns_p, Ns_q)), then squared normal_power_log2 times (w_n = w_n * w_n)
 *       D = P_q - P_p, dd = |D|^2, d = dot(N_p, D), x_z = dd == 0 ? 0 : (d * d) / (sz2 * dd), w_z = max0(1 - x_z), w_z = w_z * w_z
 *         (scale-free: sine^2 of the angle between the offset and p's tangent plane, against sigma_plane)
 *       e = |I_i(p) - I_i(q)|^2, den = |I_i(p)|^2 + |I_i(q)|^2, x_c = den == 0 ? 0 : (e / den) * inv_c, w_c = max0(1 - x_c),
 *         w_c = w_c * w_c  (scale-free too; e <= 2 den, so sigma_color 2 gives w_c >= 1/4 in the first iteration)
 *     sum_ch += w * I_i(q)_ch, wsum += w (both from 0.0, in tap order); I_{i+1}(p)_ch = sum_ch * (1.0 / wsum).
 * Remodulate: out = I_n * a.
 * NaN and Inf are not filtered out: a NaN or Inf in the beauty frame, in Ns, N or P reaches every pixel whose taps read it (through
 * the sums, or through a NaN weight), and spreads with every iteration; a NaN coverage counts as covered; a NaN albedo counts as
 * below the floor (a = 1).
 * d_out_rgb may be d_rgb; intermediate frames live in scratch the context owns (128 B per pixel, kept between calls). The call is
 * synchronous on the context's stream, needs no uploaded scene, and is refused (MCRT_ERR_INVALID) while a render is in flight,
 * when a pointer it needs is NULL, when width * height is 0 or >= 2^32, or with more than 16 iterations.
 * stats: kernel_ms (HIP events of the pass's own around its launches), total_ms, kernel_launches (1 + iterations).
 * Option MCRT_DENOISE_FORM: "tile" (a workgroup stages a tile of one residue class of the step plus its halo in LDS), "plain" (one
 * lane per pixel, taps from memory), unset = the measured choice per step; the forms run the same text and give the same bits. */
#define MCRT_DENOISE_NO_ALBEDO 1u
typedef struct mcrt_denoise_params {   /* NULL or a zero field = the default */
    uint32_t iterations;         /* default 5; more than 16: MCRT_ERR_INVALID */
    uint32_t normal_power_log2;  /* default 7 (exponent 128); more than 32: MCRT_ERR_INVALID */
    double   sigma_color;        /* default 2.0 */
    double   sigma_plane;        /* default 0.1 */
    double   albedo_floor;       /* default 1e-3 */
    uint32_t flags, reserved;    /* MCRT_DENOISE_NO_ALBEDO */
} mcrt_denoise_params;
int mcrt_denoise_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* d_rgb,
                        const mcrt_aov_buffers* guides /* full-frame DEVICE pointers */, const mcrt_denoise_params* params,
                        double* d_out_rgb, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers (out_rgb may be rgb). */
int mcrt_denoise(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* rgb, const mcrt_aov_buffers* guides,
                 const mcrt_denoise_params* params, double* out_rgb, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Variance-guided denoised output: the same a-trous filter with its colour weight measured in units of the pixels' estimated
 * variance instead of a fixed contrast, and that variance carried through the iterations - the filtered frame comes back with
 * an estimate of its own error in the form mcrt_frame_noise reads. The reference has no such output. Only FP64 + - * /, compare
 * and select, in the order written here, uncontracted, no libm routine: a function of its inputs bit for bit.
 *
 * Inputs are FULL frames [height][width]...: the beauty frame c, its per-pixel sample variance v (the `variance` channel of
 * mcrt_render_pixel_stats* at the same camera, seed and spp = n samples per pixel), and the guides mcrt_denoise reads (Ns, N, P,
 * coverage, albedo). dot, max0, h, the tap order, the coverage rules, w_n and w_z are exactly mcrt_denoise's (above);
 * g(V) = (V.x + V.y) + V.z.
 * Demodulate, per pixel and channel: a as in mcrt_denoise, I_0 = c / a, and the variance of the pixel's mean in the demodulated
 * frame u_ch = (v_ch / (double)n) / (a_ch * a_ch).
 * Prefilter the variance (a sample variance of 4 samples is itself noisy): a pixel with coverage(p) == 0 has V_0(p) = u(p). For
 * every other p the taps q = p + (dx, dy) are visited with dy = -1..1 as the outer and dx = -1..1 as the inner loop,
 * k = {1/4, 1/2, 1/4}, kw = k[dy] * k[dx]; taps outside the frame or with coverage(q) == 0 are skipped;
 *   s_ch += kw * u_ch(q), ks += kw (both from 0.0, in tap order); V_0(p)_ch = s_ch * (1.0 / ks) (the centre always counts).
 * Iterate, for i = 0 .. iterations-1 with step s = 2^i; sv2 = sigma_variance * sigma_variance, sf2 = sigma_floor * sigma_floor,
 * sz2 = sigma_plane * sigma_plane are computed once on the host and neither sigma shrinks with i (the variance shrinks by itself
 * as the filter averages):
 *   a pixel p with coverage(p) == 0 keeps I and V. For every other p the 25 taps q = p + s * (dx, dy) are visited as in mcrt_denoise;
 *     the centre tap has weight w = 9/64 exactly; a tap outside the frame or with coverage(q) == 0 is skipped;
 *     every other tap has w = (((h[dy] * h[dx]) * w_n) * w_z) * w_c with
 *       e = |I_i(p) - I_i(q)|^2, m = |I_i(p)|^2 + |I_i(q)|^2, den = (sv2 * (g(V_i(p)) + g(V_i(q)))) + (sf2 * m),
 *       x_c = e == 0 ? 0 : e / den (a zero den with e > 0 gives +Inf and so weight 0), w_c = max0(1 - x_c), w_c = w_c * w_c
 *         (the squared difference against sigma_variance^2 times the variance of that difference, plus a scale-free floor for
 *         pixels whose few samples happened to agree)
 *     sum_ch += w * I_i(q)_ch, vsum_ch += (w * w) * V_i(q)_ch, wsum += w (all from 0.0, in tap order);
 *     r = 1.0 / wsum, I_{i+1}(p)_ch = sum_ch * r, V_{i+1}(p)_ch = vsum_ch * (r * r).
 * Remodulate: out = I_n * a, out_variance_ch = (V_n,ch * (a_ch * a_ch)) * (double)n - a sample-variance equivalent, so
 * mcrt_frame_noise(out, out_variance, n) is the filtered frame's summary with no new call.
 * out_variance is the estimate under INDEPENDENT inputs. The prefilter already, and every iteration from the second on, combine
 * pixels that share samples, and the filter's bias is not in it, so it underestimates the filter's own part. Measured (four scenes,
 * 192 x 108, sigma_variance 3.0 and sigma_floor 0.05 - not the defaults; profiles/NOTES_denoise_variance.md): the mean of g(out_variance) / n over the covered pixels is 0.59 - 3.2 times the
 * filtered frame's mean squared error to a 1024-spp render at 4 and 16 spp - below 1 on the specular scenes, above 1 where the
 * render's stratified samples make a pixel's mean better than v / n says - and 0 at 1 spp, where v is 0: a guide, not a bound.
 * NaN, Inf and negative variances are not filtered out. A NaN or Inf in c, v, Ns, N or P reaches every pixel whose taps read it
 * (through the sums, or through a NaN weight) and spreads with every iteration; the prefilter spreads one in v over its 3 x 3
 * neighbours first. A negative variance enters den as it is: den < 0 with e > 0 gives x_c < 0 and so w_c > 1, and it is carried
 * into out_variance. A NaN coverage counts as covered; a NaN albedo counts as below the floor (a = 1).
 * d_out_rgb may be d_rgb and d_out_variance may be d_variance; d_out_variance NULL: the frame alone. Intermediate frames live in
 * scratch the context owns (176 B per pixel, kept between calls). The call is synchronous on the context's stream, needs no
 * uploaded scene, and is refused (MCRT_ERR_INVALID) while a render is in flight, when a pointer it needs is NULL (albedo only
 * without MCRT_DENOISE_NO_ALBEDO), when spp is 0, when width * height is 0 or >= 2^32, with more than 16 iterations,
 * normal_power_log2 > 32, or a sigma that is negative or not finite.
 * stats: kernel_ms, total_ms, kernel_launches (1 + iterations).
 * Option MCRT_DENOISE_VAR_FORM: "tile" / "plain" / unset = the measured choice per step, as MCRT_DENOISE_FORM; the same bits. */
typedef struct mcrt_denoise_variance_params {   /* NULL or a zero field = the default */
    uint32_t iterations;         /* default 5; more than 16: MCRT_ERR_INVALID */
    uint32_t normal_power_log2;  /* default 7 (exponent 128); more than 32: MCRT_ERR_INVALID */
    double   sigma_variance;     /* default 6.0 */
    double   sigma_floor;        /* default 0.02 */
    double   sigma_plane;        /* default 0.1 */
    double   albedo_floor;       /* default 1e-3 */
    uint32_t flags, reserved;    /* MCRT_DENOISE_NO_ALBEDO */
} mcrt_denoise_variance_params;                  /* 48 bytes */
int mcrt_denoise_variance_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* d_rgb,
                                 const double* d_variance, const mcrt_aov_buffers* guides /* full-frame DEVICE pointers */,
                                 const mcrt_denoise_variance_params* params, double* d_out_rgb,
                                 double* d_out_variance /* may be NULL */, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers (out_rgb may be rgb, out_variance may be variance or NULL). */
int mcrt_denoise_variance(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* rgb, const double* variance,
                          const mcrt_aov_buffers* guides, const mcrt_denoise_variance_params* params, double* out_rgb,
                          double* out_variance /* may be NULL */, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Dual-buffer denoised output: the non-local-means filter of Rousselle, Knaus and Zwicker 2012 on the two half-buffers of a render
 * (half_a, half_b of mcrt_render_pixel_stats*, mcrt_frame_merge* or mcrt_render_converged*: the means of the even and of the odd
 * samples). Each half is filtered with weights computed from the OTHER half, so the weights are independent of the noise they
 * average, and the squared difference of the two filtered halves estimates the filtered frame's error, the filter's bias
 * included. No AOV pass is read: it works where first-hit guides say little (glass, mirrors, depth of field, the sky). The
 * reference has no such output. Only FP64 + - * /, compare and select, in the order written here, uncontracted, no libm routine:
 * a function of its inputs bit for bit, whatever the form, tiling or stream.
 *
 * Inputs are FULL frames [height][width][3]: the halves A, B and the per-pixel sample variance v of the same render of n = spp
 * samples per pixel. max0 is mcrt_denoise's (x < 0 ? 0 : x).
 * Constants, computed once on the host: n_a = (n + 1) / 2 and n_b = n / 2 as integers (the counts the halves are means of, for a
 * render and for any merge of renders); ia = 1.0 / (double)n_a, ib = 1.0 / (double)n_b; fa = (double)n_a / (double)n,
 * fb = (double)n_b / (double)n; k2 = k * k.
 * Prefilter the variance, as mcrt_denoise_variance does but without coverage: the taps q = p + (dx, dy) are visited with
 * dy = -1..1 as the outer and dx = -1..1 as the inner loop, kk = {1/4, 1/2, 1/4}, kw = kk[dy] * kk[dx]; taps outside the frame are
 * skipped; s_ch += kw * v_ch(q), ks += kw (both from 0.0, in tap order); V0(p)_ch = s_ch * (1.0 / ks). The variance of half X's
 * pixel is VX = V0 * ix: VA = V0 * ia, VB = V0 * ib.
 * Weights from half X, applied to the other half Y, for (X, Y) = (B, A) and (A, B). For pixel p the window taps q = p + (dx, dy)
 * are visited with dy = -R..R as the outer and dx = -R..R as the inner loop; taps outside the frame are skipped; the centre tap has
 * w = 1.0 exactly (the weight sum is never below 1); every other tap:
 *   S = 0.0; cnt = 0
 *   for j = -F..F:                      (patch rows, ascending)
 *     row = 0.0
 *     for i = -F..F:                    (ascending)
 *       p' = p + (i, j); q' = q + (i, j); if p' or q' is outside the frame: skip the element
 *       cnt += 1
 *       for ch = r, g, b:
 *         vp = VX_ch(p'); vq = VX_ch(q'); delta = X_ch(p') - X_ch(q'); vm = vq < vp ? vq : vp
 *         num = delta * delta - alpha * (vp + vm); den = epsilon + k2 * (vp + vq)
 *         row = row + num / den
 *     S = S + row                       (for every j, a row without elements adds its 0.0)
 *   D = S / (double)(3 * cnt); x = max0(D); w = max0(1.0 - x); w = w * w
 * then sumY_ch += w * Y_ch(q), wsumX += w (both from 0.0, in tap order), and Y_f(p)_ch = sumY_ch * (1.0 / wsumX).
 * Outputs: rgb_ch = (fa * A_f) + (fb * B_f); with dl = A_f - B_f, variance_ch = ((dl * dl) * (fa * fb)) * (double)n;
 * half_a = A_f, half_b = B_f. For independent halves E(A - B)^2 = sigma^2 n / (n_a n_b), so (A_f - B_f)^2 fa fb estimates the
 * variance of the combined pixel; times n it is the sample-variance equivalent that mcrt_frame_noise(rgb, variance, n) reads with
 * no new call, as after mcrt_denoise_variance.
 * The row-then-column order of the patch sum is deliberate: a row sum depends only on (x, y + j, offset), so an implementation
 * that sums the rows of a tile once and then adds 2F+1 of them per pixel (the tile form does) gives these bits. A sliding or
 * running sum does not, and is not allowed. The weight is not symmetric in p and q (vm is the centre side's variance clamped by
 * the tap's), so the half-window trick that reuses w(p, q) for w(q, p) would change the result and is not used.
 * NaN, Inf and negative variances are not filtered out. A NaN in X at pixel z reaches Y_f(p) for every p within Chebyshev
 * distance R + F of z (through a patch that holds z, as p' or as q'; a frame of one pixel has no such patch) and no other pixel; a NaN in Y at z reaches Y_f(p) for those
 * within R; one in v spreads one pixel further, through the prefilter: R + F + 1. A negative variance enters num and den as it is.
 * The two halves of one Owen-scrambled Sobol pixel are NOT independent samples (the even and the odd points of one stratified
 * sequence), and one squared difference per pixel is a noisy estimate of a variance: how far the estimate is off is a measurement,
 * not a promise. Measured (four scenes, 192 x 108, the defaults; profiles/NOTES_denoise_dual.md): the mean of g(variance) / n over
 * the covered pixels is 0.10 - 1.4 times the filtered frame's mean squared error to a 1024-spp render at 4 and 16 spp on seven of
 * the eight frames - below 1 on the diffuse and the specular room, where the stratified halves agree better than independent
 * samples would and the filter's bias is shared by both halves - and 18.6 times on the eighth (coffee_maker_qsah at 16 spp, a
 * few firefly pixels): a guide, not a bound, and not a closer one than mcrt_denoise_variance's 0.59 - 3.2.
 * Every output may alias the corresponding input (rgb any input): a prep pass copies what the filter reads into scratch first,
 * one packed record {A.rgb, B.rgb, V0.rgb} per pixel - 72 B per pixel, per context, kept between calls (the host-pointer form
 * stages its frames in another 96 B per pixel). The call needs no uploaded scene, is synchronous on the context's stream, and is
 * refused (MCRT_ERR_INVALID, the cause in mcrt_last_error) while a render is in flight, with spp < 2 (half_b of one sample is not
 * a mean), width * height 0 or >= 2^32, a NULL input, out or out->rgb NULL, window_radius > 8, patch_radius > 3, or a k, alpha or
 * epsilon that is negative or not finite (epsilon must end up > 0).
 * stats: kernel_ms, total_ms, kernel_launches = 2 (prep + filter).
 * Option MCRT_DENOISE_DUAL_FORM: "tile" (a workgroup per 16 x 16 tile, records and per-offset patch terms in LDS) / "plain" (one
 * lane per pixel, the text above as written) / unset = the measured choice, the tile form; MCRT_DENOISE_DUAL_LANES: 256 / 512 /
 * 1024 lanes in the tile form's workgroup / unset = the measured choice per (R, F). The same bits all of them. */
typedef struct mcrt_denoise_dual_params {   /* NULL or a zero field = the default */
    uint32_t window_radius;   /* R, default 5; more than 8: MCRT_ERR_INVALID */
    uint32_t patch_radius;    /* F, default 2; more than 3: MCRT_ERR_INVALID */
    double   k;               /* default 0.45 (Rousselle et al.'s; profiles/NOTES_denoise_dual.md); negative or not finite: INVALID */
    double   alpha;           /* variance cancellation, default 1.0 */
    double   epsilon;         /* default 1e-10; must end up > 0 */
    uint32_t flags, reserved; /* none yet */
} mcrt_denoise_dual_params;                  /* 40 bytes */
typedef struct mcrt_denoise_dual_buffers {  /* DEVICE (or HOST) full frames [height][width][3]; NULL = not wanted */
    double* rgb;        /* required */
    double* variance;   /* filtered frame's error, sample-variance equivalent */
    double* half_a;     /* the filtered halves */
    double* half_b;
} mcrt_denoise_dual_buffers;
int mcrt_denoise_dual_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* d_half_a,
                             const double* d_half_b, const double* d_variance, const mcrt_denoise_dual_params* params,
                             const mcrt_denoise_dual_buffers* d_out, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers. */
int mcrt_denoise_dual(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* half_a, const double* half_b,
                      const double* variance, const mcrt_denoise_dual_params* params, const mcrt_denoise_dual_buffers* out,
                      mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Per-pixel sample statistics: the spread of a pixel's samples next to their mean - the sample variance and the two half-buffers
 * (the means of the even and of the odd samples) that error estimators, stopping rules and denoisers start from. The reference
 * has no such output. Every box-filter frame keeps the radiance of every sample until its pass is resolved; the statistics are
 * a second reader of that store, whatever kernel form filled it. Only FP64 + - * /, compare and select, in the order written
 * here, uncontracted, no libm routine: a function of the samples bit for bit.
 *
 * Per pixel and channel, with x_i the radiance of sample i (i = 0 .. n-1, n = sqrtspp^2):
 *   S = (((0.0 + x_0) + x_1) + ...) in ascending i, m = S / (double)n     (the frame's own sum: the frame is max(m, 0))
 *   Q = (((0.0 + (x_0 - m) * (x_0 - m)) + (x_1 - m) * (x_1 - m)) + ...) in ascending i
 *   variance = n > 1 ? Q / (double)(n - 1) : 0.0         (two passes on purpose: one-pass formulas cancel on a firefly)
 *   half_a   = (((0.0 + x_0) + x_2) + ...) / (double)((n + 1) / 2)                      (even i, ascending)
 *   half_b   = n > 1 ? (((0.0 + x_1) + x_3) + ...) / (double)(n / 2) : 0.0              (odd i, ascending)
 * None of them is clamped. NaN and Inf are not filtered: they reach the outputs of their own pixel and of no other.
 *
 * mcrt_render_pixel_stats_device renders the frame mcrt_render_device + mcrt_render_finish deliver - the same bits in d_out_rgb,
 * the same kernel_id, cam->shard_* honoured the same way - and fills the channels of d_buffers that are not NULL, packed like
 * d_out_rgb (the owned rows). The call is synchronous on the context's stream. kernel_launches counts one launch more per
 * pass (MCRT_SAMPLE_STORE_GB) when a channel is wanted; the statistics do not depend on passes, shards, the kernel form of
 * one integrator family or the launch shape. A frame that mcrt_render_finish renders again (nested media, a kNN overflow)
 * delivers the statistics of the run it delivers. d_buffers NULL or all-NULL: a plain render.
 * Refused: a camera whose film splats (a reconstruction filter, or a box of another radius) when a channel is wanted -
 * MCRT_ERR_UNSUPPORTED, such frames keep no samples; a render in flight, no scene, d_out_rgb NULL as in mcrt_render_device. */
typedef struct mcrt_pixel_stats_buffers {   /* every pointer may be NULL = not wanted; owned rows packed like d_out_rgb */
    double* variance;   /* [rows][width][3] */
    double* half_a;     /* [rows][width][3] */
    double* half_b;     /* [rows][width][3] */
} mcrt_pixel_stats_buffers;
int mcrt_render_pixel_stats_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                                   double* d_out_rgb, const mcrt_pixel_stats_buffers* d_buffers, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers to FULL frames ([height][width][3]): rows this shard does not own are left untouched. */
int mcrt_render_pixel_stats(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* out_rgb,
                            const mcrt_pixel_stats_buffers* buffers, mcrt_stats* stats /* may be NULL */);

/* The frame summary a stopping rule reads. Per pixel p of `pixels`, from the frame rgb [pixels][3] and its variance [pixels][3]:
 *   e_p = ((v_r + v_g) + v_b) / (double)spp          (the estimated variance of the pixel's mean, channels added)
 *   g_p = (r * r + g * g) + b * b
 * noise = treesum(e), signal = treesum(g), where treesum is fixed so that the result is a function of the input bit for bit:
 *   the values are taken in blocks of 256 consecutive ones (the last one may be shorter: len values); inside a block, for
 *   stride = 128, 64, ..., 1: t[k] = t[k] + t[k + stride] for every k < stride with k + stride < len; the block's value is t[0];
 *   the block values are reduced the same way again until one is left.
 * relative_error = signal > 0 ? sqrt(noise / signal) : 0, computed on the host. A NaN or Inf anywhere reaches noise or signal.
 * The call needs no scene, is synchronous on the context's stream (device inputs must be complete when it is called), moves only
 * the results across PCIe, and is refused (MCRT_ERR_INVALID) while a render is in flight, with a NULL pointer, pixels == 0 or
 * >= 2^38, or spp == 0. A sharded frame is summarised after the gather. */
typedef struct mcrt_frame_noise_result { double noise, signal, relative_error; uint64_t pixels; } mcrt_frame_noise_result;
int mcrt_frame_noise_device(mcrt_ctx* ctx, uint64_t pixels, uint32_t spp, const double* d_rgb, const double* d_variance,
                            mcrt_frame_noise_result* out);
/* Same with HOST pointers. */
int mcrt_frame_noise(mcrt_ctx* ctx, uint64_t pixels, uint32_t spp, const double* rgb, const double* variance,
                     mcrt_frame_noise_result* out);

/* ------------------------------------------------------------------------------------------
 * Firefly suppression: the brightest samples of every pixel kept aside while the per-sample store still holds them (the
 * highlights of a render), and a robust frame that clamps them against the level of the pixel's neighbourhood. The reference
 * has no such output. A pixel that sees only itself cannot tell a firefly from the edge of a directly visible light - two
 * bright samples out of sixteen look like outliers there -, so the bound comes from the largest robust level in a window.
 * Only FP64 + - * /, compare and select, in the order written here, uncontracted, no libm routine: functions of their inputs
 * bit for bit.
 *
 *   L(x) = (0.2126 * x.r + 0.7152 * x.g) + 0.0722 * x.b;   n = sqrtspp^2;   max0(x) = x < 0 ? 0 : x
 *   K = min(4, n / 4) (integer division): 0 below 4 spp, 1 at 4, 2 at 9, 4 (MCRT_ROBUST_TOPS) from 16 on.
 *
 * 1. Highlights of a render. Per pixel, with x_i the radiance of sample i (i = 0 .. n-1) and L_i = L(x_i):
 *   a list of at most K entries starts empty. For i ascending: a sample whose L_i is NaN never enters; any other sample is
 *   inserted before the first entry e with L_i > L_e, or appended when there is no such e and the list holds fewer than K
 *   entries; an entry pushed past position K-1 is dropped. (Without NaN this is the stable order: L descending, i ascending.)
 *   tops[k]  = the rgb of entry k of the final list, 0.0 for k >= the number of entries (k = 0 .. 3)
 *   rest_c   = (((0.0 + x_a,c) + x_b,c) + ...) over the samples that are not in the final list, ascending i
 *   level    = L(rest / (double)(n - K))          (the division per channel; K, not the number of entries)
 * Nothing is clamped. With K = 0 the list is empty and level = L(S / n) of the frame's own sum S.
 * mcrt_render_highlights_device renders the frame mcrt_render_device + mcrt_render_finish deliver - the same bits in d_out_rgb,
 * the same kernel_id, cam->shard_* honoured the same way - and fills the channels of d_highlights that are not NULL, packed
 * like d_out_rgb (the owned rows); d_stats_buffers, when given, is filled as by mcrt_render_pixel_stats_device in the same
 * render. The call is synchronous on the context's stream. kernel_launches counts one launch more per pass
 * (MCRT_SAMPLE_STORE_GB) when a highlight channel is wanted, and one more when a statistics channel is; the highlights do not
 * depend on passes, shards, the kernel form of one integrator family or the launch shape. A frame that mcrt_render_finish
 * renders again (nested media, a kNN overflow) delivers the highlights of the run it delivers. d_highlights NULL or all-NULL:
 * no highlights. Refused as the statistics are: a camera whose film splats when a channel is wanted - MCRT_ERR_UNSUPPORTED -;
 * a render in flight, no scene, d_out_rgb NULL as in mcrt_render_device. */
#define MCRT_ROBUST_TOPS 4
typedef struct mcrt_highlight_buffers {   /* every pointer may be NULL = not wanted; owned rows packed like d_out_rgb */
    double* tops;    /* [rows][width][MCRT_ROBUST_TOPS][3] */
    double* level;   /* [rows][width] */
} mcrt_highlight_buffers;
int mcrt_render_highlights_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* d_out_rgb,
                                  const mcrt_highlight_buffers* d_highlights, const mcrt_pixel_stats_buffers* d_stats_buffers /* may be NULL */,
                                  mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers to FULL frames ([height][width]...): rows this shard does not own are left untouched. */
int mcrt_render_highlights(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator, double* out_rgb,
                           const mcrt_highlight_buffers* highlights, const mcrt_pixel_stats_buffers* stats_buffers /* may be NULL */,
                           mcrt_stats* stats /* may be NULL */);

/* 2. Robust resolve, on FULL frames [height][width]... after the gather (it reads neighbouring rows: there is no shard form):
 * the frame rgb, its tops and its level, of a render with spp = n samples per pixel. Per pixel p, with R = radius:
 *   M = -inf; the window is visited with dy = -R..R as the outer and dx = -R..R as the inner loop, taps q outside the frame are
 *   skipped; at each tap M = M < level_q ? level_q : M   (a NaN level is never taken)
 *   t = kappa * M;  T = t > floor ? t : floor
 *   removed_c = 0.0, count = 0; for k = 0 .. K-1 with L_k = L(tops_k): if L_k > T then f = T / L_k,
 *     removed_c = removed_c + (tops_k,c - tops_k,c * f), count = count + 1
 *   removed (out) = removed_c / (double)n;   out_c = max0(rgb_c - removed_c / (double)n);   clamped = count
 * Where nothing is clamped (count == 0) out is rgb bit for bit (also a negative value of a frame that is no render's, which
 * max0 would cut: out_c = count ? max0(...) : rgb_c). NaN and Inf are not filtered: they stay in their own pixel,
 * except that an Inf level switches the clamp off in every window that holds it.
 * d_out_rgb may be d_rgb; buffers (or either of its pointers) may be NULL. The call is synchronous on the context's stream,
 * needs no uploaded scene, and is refused (MCRT_ERR_INVALID) while a render is in flight, when d_rgb, d_tops, d_level or
 * d_out_rgb is NULL, when width * height is 0 or >= 2^32, when spp is 0, or with a parameter out of range.
 * stats: kernel_ms (HIP events of the call's own around its launch), total_ms, kernel_launches (1). */
typedef struct mcrt_robust_params {   /* NULL or a zero field = the default */
    double   kappa;              /* default 8.0; must be finite and >= 1 */
    double   floor;              /* default 0.0; must be finite and >= 0 */
    uint32_t radius, reserved;   /* default 1; more than 8: MCRT_ERR_INVALID */
} mcrt_robust_params;
typedef struct mcrt_robust_buffers {  /* every pointer may be NULL = not wanted */
    double*   removed;   /* [height][width][3] */
    uint32_t* clamped;   /* [height][width]    */
} mcrt_robust_buffers;
int mcrt_robust_resolve_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* d_rgb, const double* d_tops,
                               const double* d_level, const mcrt_robust_params* params, double* d_out_rgb,
                               const mcrt_robust_buffers* d_buffers /* may be NULL */, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers (out_rgb may be rgb). */
int mcrt_robust_resolve(mcrt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, const double* rgb, const double* tops,
                        const double* level, const mcrt_robust_params* params, double* out_rgb,
                        const mcrt_robust_buffers* buffers /* may be NULL */, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Accumulated rendering: independent renders of one camera merged per pixel, and a render that stops at a target noise. The
 * reference has no such output. A render delivers the sufficient statistics of a pixel's samples - rgb, variance, half_a,
 * half_b (mcrt_render_pixel_stats*), tops, level (mcrt_render_highlights*) -, and two renders of one camera at different
 * global_seeds are independent estimates of the same pixels: the summary of their union follows from the two summaries alone.
 * No render kernel takes part. Only FP64 + - * /, compare and select, in the order written here, uncontracted, no libm routine:
 * a function of the inputs bit for bit.
 *
 * 1. mcrt_frame_merge: the summary of the sample sequence "A's n_a samples, then B's n_b samples" (sample j of B has index
 * n_a + j), n_a, n_b >= 1. With a = (double)n_a, b = (double)n_b, t = a + b, per pixel and channel:
 *   m        = (a * m_a + b * m_b) / t               (m_a, m_b: the inputs' rgb, TAKEN AS THE MEANS THEY ARE - a render's frame is
 *                                                     max(mean, 0), which is the mean wherever no sample is negative; m is not clamped)
 *   d        = m_b - m_a
 *   Q        = ((a - 1) * v_a + (b - 1) * v_b) + (d * d) * ((a * b) / t)
 *   variance = Q / (t - 1)
 * The half-buffers follow the parity of the index in the concatenation: B's even samples stay even when n_a is even and become
 * odd when n_a is odd. With the counts e_x = (n_x + 1) / 2, o_x = n_x / 2 (integer division) and
 *   wmean(c1, x1, c2, x2) = (c1 > 0 ? (c2 > 0 ? (double)c1 * x1 + (double)c2 * x2 : (double)c1 * x1) : (double)c2 * x2) / (double)(c1 + c2)
 * (a term whose count is 0 is skipped by the select, not multiplied by 0: half_b of a 1-sample input takes no part):
 *   n_a even:  half_a = wmean(e_a, half_a_A, e_b, half_a_B)    half_b = wmean(o_a, half_b_A, o_b, half_b_B)
 *   n_a odd:   half_a = wmean(e_a, half_a_A, o_b, half_b_B)    half_b = wmean(o_a, half_b_A, e_b, half_a_B)
 * so the merged halves are again the means of (n + 1) / 2 and n / 2 samples, n = n_a + n_b.
 * The highlights need full lists on both sides, n_a >= 16 and n_b >= 16 (K = MCRT_ROBUST_TOPS): below that the second-brightest
 * sample of the union may sit in an input's rest. With L as in "Firefly suppression":
 *   the list starts as A's four entries in order, with their luminances L(tops_A,k). For j = 0 .. 3, B's entry x = tops_B,j with
 *   l = L(x): it is inserted before the first entry e with l > L_e (never when l is NaN) and the entry pushed past position 3
 *   leaves; when there is no such e, x itself leaves. g_j = the luminance of what left at step j (L of the old entry 3, or l).
 *   Ties go to A and to the lower index, as in the concatenated render.
 *   tops  = the final list
 *   level = (((a - 4) * level_A + (b - 4) * level_B) + ((((0.0 + g_0) + g_1) + g_2) + g_3)) / (t - 4)
 * (from luminances, L being linear; not as a sum minus the tops, which cancels exactly when a firefly is present).
 * NaN and Inf are not filtered: they stay in their own pixel.
 *
 * The channels form three groups, each optional as a whole: {rgb, variance}, {half_a, half_b}, {tops, level}. A group is wanted
 * when out names it (both pointers; variance alone may be NULL: the mean only) and then needs the same channels of a and of b.
 * Every output may be the corresponding buffer of a (an accumulator merged into in place); it must not overlap anything else.
 * All buffers are [pixels]... packed, so the owned rows of a shard merge as they are. One launch, synchronous on the context's
 * stream, no scene needed. Refused with MCRT_ERR_INVALID: a render in flight, pixels 0 or >= 2^32, n_a or n_b 0, n_a + n_b
 * past UINT32_MAX, a, b or out NULL, no group wanted, half a group, a wanted group without its inputs; with MCRT_ERR_UNSUPPORTED:
 * {tops, level} wanted with n_a or n_b below 16.
 * stats: kernel_ms (HIP events of the call's own around its launch), total_ms, kernel_launches (1).
 *
 * Merging batches gives up the Sobol stratification across them: batch j restarts the sequence under another scramble instead of
 * continuing it. Measured on the oracle's samples (profiles/NOTES_accumulate.md; 192 x 108, summed squared error against 4096 spp
 * of another seed, 8 seed groups): 4 x 16 spp merged carries 1.27 times the squared error of 1 x 64 spp on hexagon_room_diffuse
 * and 1.21 times on coffee_maker_qsah - what a caller pays for not having to choose sqrtspp before the first ray. */
typedef struct mcrt_frame_summary {   /* a pointer may be NULL = channel not given / not wanted; [pixels]... packed */
    double* rgb;        /* [pixels][3] */
    double* variance;   /* [pixels][3] */
    double* half_a;     /* [pixels][3] */
    double* half_b;     /* [pixels][3] */
    double* tops;       /* [pixels][MCRT_ROBUST_TOPS][3] */
    double* level;      /* [pixels] */
} mcrt_frame_summary;
int mcrt_frame_merge_device(mcrt_ctx* ctx, uint64_t pixels, const mcrt_frame_summary* d_a, uint32_t n_a, const mcrt_frame_summary* d_b,
                            uint32_t n_b, const mcrt_frame_summary* d_out, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers. */
int mcrt_frame_merge(mcrt_ctx* ctx, uint64_t pixels, const mcrt_frame_summary* a, uint32_t n_a, const mcrt_frame_summary* b, uint32_t n_b,
                     const mcrt_frame_summary* out, mcrt_stats* stats /* may be NULL */);

/* 2. mcrt_render_converged: the stopping rule. Batches of cam->sqrtspp^2 samples are rendered, merged and summarised until the
 * frame is quiet enough. Batch j (j = 0, 1, ...) is one mcrt_render_highlights_device (when a highlight channel is wanted) or
 * mcrt_render_pixel_stats_device of cam as given, with the seed global_seed + j (wrapping in uint32_t). Batch 0 fills accumulators
 * kept in the context; every later batch is merged into them in place by mcrt_frame_merge_device (accumulator = A, batch = B).
 * After each batch, mcrt_frame_noise_device of the accumulated rgb and variance at the accumulated sample count gives
 * relative_error. The loop ends when at least min_batches were rendered and relative_error <= target_relative_error, or when
 * one more batch would exceed max_spp. The frame delivered is the accumulated one either way: ending above the target is not an
 * error, result->final.relative_error says where the frame stands. The frame is the merged mean (not clamped again), so with
 * one batch every output is that render's, bit for bit.
 * out_rgb / d_out_rgb and the channels of stats_buffers and highlights that are not NULL are filled with FULL frames
 * ([height][width]...). stats: paths, rays, node_tests, prim_tests, knn_searches, kernel_ms and kernel_launches summed over the
 * batches (a merge counts one launch), kernel_id of the last batch, total_ms of the call.
 * Refused with MCRT_ERR_UNSUPPORTED: what the statistics refuse (a camera whose film splats); cam->shard_count > 1 - the summary
 * needs the whole frame: a sharded host merges its owned rows per shard with mcrt_frame_merge_device and decides after its
 * gather -; a highlight channel wanted with fewer than 16 samples per batch. With MCRT_ERR_INVALID: a render in flight, cam or
 * the frame NULL, sqrtspp 0, a target that is negative or not finite, max_spp below one batch. */
#define MCRT_CONVERGE_TRACE 64
typedef struct mcrt_converge_params {   /* NULL or a zero field = the default */
    double   target_relative_error;   /* default 0.0: no target, render until max_spp; must be finite and >= 0 */
    uint32_t max_spp;                 /* default: 1024, or one batch where that is more */
    uint32_t min_batches;             /* default 1; with sqrtspp 1 it is 2 (a 1-sample batch has variance 0 and would stop at once) */
} mcrt_converge_params;
typedef struct mcrt_converge_result {
    uint32_t batches, spp;                        /* batches rendered, samples per pixel accumulated */
    mcrt_frame_noise_result final;                /* the summary of the delivered frame */
    double relative_error[MCRT_CONVERGE_TRACE];   /* after each of the first 64 batches; 0.0 past `batches` */
} mcrt_converge_result;
int mcrt_render_converged_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                                 const mcrt_converge_params* params /* may be NULL */, double* d_out_rgb,
                                 const mcrt_pixel_stats_buffers* d_stats_buffers /* may be NULL */,
                                 const mcrt_highlight_buffers* d_highlights /* may be NULL */, mcrt_converge_result* result /* may be NULL */,
                                 mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers. */
int mcrt_render_converged(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, int integrator,
                          const mcrt_converge_params* params /* may be NULL */, double* out_rgb,
                          const mcrt_pixel_stats_buffers* stats_buffers /* may be NULL */, const mcrt_highlight_buffers* highlights /* may be NULL */,
                          mcrt_converge_result* result /* may be NULL */, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * OpenEXR output: one scan-line OpenEXR 2 file that holds a frame and any number of its passes as named channels. The reference
 * has no such output. Nothing here links an OpenEXR or zlib library: the file is written from the format's public specification
 * ("OpenEXR File Layout"), and deflate is the system's libz.so.1, looked up (dlopen) at the first ZIP save. The values are
 * converted, and the bytes of every chunk laid out in file order (NONE) or in ZIP's pre-deflate order, on the device: the packed
 * buffer is the only thing that crosses to the host.
 *
 * A channel is a strided view of a frame: its value at pixel p = y * width + x is data[p * stride + offset], data being double
 * (MCRT_EXR_SRC_F64) or uint32_t (MCRT_EXR_SRC_U32) elements. An [H][W][3] frame gives R, G, B with stride 3 and offsets 0, 1, 2;
 * tops [H][W][4][3] twelve channels of stride 12; level [H][W] one of stride 1. One data pointer may serve many channels.
 *
 * Conversions, per value, all of them on the bits in integer arithmetic (no floating-point mode of the device takes part):
 *   F64 -> HALF   ONE rounding from binary64 to binary16, to nearest, ties to even, subnormal results kept; never through binary32
 *                 (1 + 2^-11 + 2^-30 becomes 0x3c01; through float it would be 0x3c00). A finite input whose rounding is infinite
 *                 becomes +-65504 (0x7bff / 0xfbff) unless MCRT_EXR_HALF_INF is set; +-Inf stays; NaN becomes 0x7e00 with the
 *                 input's sign bit; -0 stays -0.
 *   F64 -> FLOAT  one rounding to nearest, ties to even, subnormal results kept, overflow to +-Inf; NaN becomes
 *                 sign | 0x7fc00000 | (the top 22 bits below the quiet bit of the input's fraction), what (float)x gives on x86-64.
 *   U32 -> UINT   the bits.
 * Any other pair is refused.
 *
 * The file, little-endian throughout:
 *   magic 76 2f 31 01, version 02 00 00 00 (single-part scan line, short names; with MCRT_EXR_LONG_NAMES 02 04 00 00: the long-names bit 0x400)
 *   attributes, each name\0 type\0 int32 size, value, in this order:
 *     channels (chlist): per channel name\0, int32 pixelType, uint8 pLinear 0, three 0 bytes, int32 xSampling 1, int32 ySampling 1;
 *       one \0 closes the list      compression (compression): 1 byte      dataWindow, displayWindow (box2i): 0, 0, W-1, H-1
 *     lineOrder (lineOrder): 1 byte, 0      pixelAspectRatio (float): 1      screenWindowCenter (v2f): 0, 0
 *     screenWindowWidth (float): 1      the caller's attributes in the order given, type string (size = length, no terminator)
 *   one \0 ends the header
 *   the offset table: one uint64 per chunk, its absolute file position
 *   the chunks in ascending y, each int32 y, int32 size, data. NONE: a chunk is one scan line; ZIP: 16 scan lines, the last may
 *   hold fewer.
 * Channels are sorted by name as bytes, in the header and in the pixel data, whatever the caller's order. A chunk's raw bytes:
 * per scan line ascending, per channel in sorted order, W values. ZIP, with n raw bytes (always even) and h = n / 2:
 *   t[i] = raw[2i] for i < h, t[h + i] = raw[2i + 1];   u[0] = t[0], u[i] = (t[i] - t[i-1] + 128) mod 256;
 *   data = zlib-deflate(u) at zip_level, with the zlib wrapper. When the deflated size is >= n the chunk stores the untransformed
 *   raw bytes and size = n (the format's own rule; counted in raw_chunks).
 * A NONE file is therefore a function of the inputs byte for byte; a ZIP file is one up to the bytes deflate chooses, which depend
 * on the zlib version - what a reader decodes from it is a function of the inputs.
 *
 * Refused with MCRT_ERR_INVALID: a render in flight; path, the channel array or a data pointer NULL; count 0 or > 1024;
 * width * height 0 or >= 2^32; a name that is empty, longer than 31 bytes (channel names with MCRT_EXR_LONG_NAMES: 255) or not printable ASCII (0x20 .. 0x7e); duplicate
 * names; stride 0 or offset >= stride; a source / pixel type pair not listed; a compression not listed; zip_level > 9; an
 * attribute without a name or value, or whose name is one of the standard ones above. With MCRT_ERR_IO: the file cannot be
 * created or written (a partial file is removed). With MCRT_ERR_UNSUPPORTED: ZIP is asked for and libz.so.1 cannot be loaded
 * (NONE still works). The call needs no scene and is synchronous on the context's stream.
 * stats: kernel_ms (HIP events of the call's own around its launch), total_ms, kernel_launches (1). */
enum { MCRT_EXR_SRC_F64 = 0, MCRT_EXR_SRC_U32 = 1 };
enum { MCRT_EXR_UINT = 0, MCRT_EXR_HALF = 1, MCRT_EXR_FLOAT = 2 };     /* OpenEXR's pixelType numbers */
enum { MCRT_EXR_COMPRESSION_NONE = 0, MCRT_EXR_COMPRESSION_ZIP = 3 };   /* OpenEXR's compression numbers */
/* mcrt_exr_params.compression: 0 = the default (ZIP); otherwise MCRT_EXR_COMPRESSION_SET | one of the numbers above. */
#define MCRT_EXR_COMPRESSION_SET 0x100u
#define MCRT_EXR_HALF_INF 1u            /* mcrt_exr_params.flags: a finite value past the half range becomes +-Inf, not +-65504 */
#define MCRT_EXR_LONG_NAMES 2u          /* mcrt_exr_params.flags: channel names of up to 255 bytes; the file carries the long-names version bit */
#define MCRT_EXR_MAX_CHANNELS 1024u
typedef struct mcrt_exr_channel {
    const char* name;       /* 1..31 bytes (MCRT_EXR_LONG_NAMES: 255), printable ASCII, e.g. "R", "albedo.G", "denoise_dual.error.B" */
    const void* data;       /* element (pixel p) is data[p * stride + offset] of the source type; row-major, full frame */
    uint32_t source_type, pixel_type, stride, offset;
} mcrt_exr_channel;
typedef struct mcrt_exr_attribute { const char* name; const char* value; } mcrt_exr_attribute;   /* written as type "string" */
typedef struct mcrt_exr_params {    /* NULL or a zero field = the default */
    uint32_t compression;           /* default ZIP; MCRT_EXR_COMPRESSION_SET | MCRT_EXR_COMPRESSION_NONE or _ZIP */
    uint32_t zip_level;             /* default 4; 1..9 */
    uint32_t threads;               /* deflate threads, default min(16, the host's hardware threads); never more than 16 */
    uint32_t flags;                 /* MCRT_EXR_HALF_INF | MCRT_EXR_LONG_NAMES */
} mcrt_exr_params;
typedef struct mcrt_exr_result {
    uint64_t file_bytes;     /* the size of the file written */
    uint64_t packed_bytes;   /* what crossed from the device to the host: the sum over the channels of W * H * bytes per value */
    uint32_t chunks, raw_chunks;
} mcrt_exr_result;
/* channels: a HOST array of structs whose data point to DEVICE memory (complete when the call is made: the stream contract below).
 * No FP64 source leaves the device. */
int mcrt_exr_save_device(mcrt_ctx* ctx, const char* path, uint32_t width, uint32_t height, const mcrt_exr_channel* d_channels, uint32_t count,
                         const mcrt_exr_attribute* attributes /* may be NULL */, uint32_t attribute_count, const mcrt_exr_params* params /* may be NULL */,
                         mcrt_exr_result* result /* may be NULL */, mcrt_stats* stats /* may be NULL */);
/* Same with HOST data pointers: every distinct source buffer is copied to the device once, whatever the number of its channels. */
int mcrt_exr_save(mcrt_ctx* ctx, const char* path, uint32_t width, uint32_t height, const mcrt_exr_channel* channels, uint32_t count,
                  const mcrt_exr_attribute* attributes /* may be NULL */, uint32_t attribute_count, const mcrt_exr_params* params /* may be NULL */,
                  mcrt_exr_result* result /* may be NULL */, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * OpenEXR input: the mirror of the output above. A file is opened once (header and offset table, no GPU work), asked what it holds,
 * and any subset of its channels is then loaded into strided destinations. Written from the format's specification like the output:
 * no OpenEXR or zlib library is linked; inflate is the system's libz.so.1 (uncompress), looked up at the first load that needs it - a
 * lookup of its own, the save's is untouched. The host reads the chunks and inflates the deflated ones, chunk by chunk on at most 16
 * threads, into ONE pinned payload buffer (chunk k at k * chunk_bytes, still in ZIP's transformed order u) which crosses to the device
 * in one copy together with a flag per chunk (transformed or raw); payload_bytes counts the payloads. A chunk is inflated whole, so a
 * channel the caller does not ask for still rides along in it. The inverse of ZIP's transform (t[0] = u[0],
 * t[i] = (t[i-1] + u[i] - 128) mod 256: a prefix sum of bytes) and the widening to the destination's type are done on the device,
 * on the bits; no FP64 value is made on the host. What a load returns is a function of the file, bit for bit.
 *
 * Accepted: single-part scan-line OpenEXR 2 files - version 2, optionally with the long-names bit 0x400 (names up to 255 bytes);
 * compression NONE (0), ZIPS (2: one line per chunk, ZIP's transform) and ZIP (3: 16 lines); any data window with xMax >= xMin,
 * yMax >= yMin and width * height < 2^32 (the display window is reported, not used); lineOrder 0, 1 or 2 - entry k of the offset
 * table is the chunk whose first line is yMin + k * lines_per_chunk whatever the line order says, and every chunk's own y is checked
 * against its slot; channels of pixelType UINT / HALF / FLOAT with xSampling == ySampling == 1 (pLinear is ignored); attributes of
 * any type, known or not.
 * Refused with MCRT_ERR_UNSUPPORTED (the message names the cause): the tiled (0x200), deep (0x800) or multi-part (0x1000) bit; any
 * other version number; any other compression (the message gives its number); a subsampled channel; a chunk that needs inflating
 * when libz.so.1 cannot be loaded (NONE files and raw chunks still load); a load of more lanes than one launch holds.
 * Refused with MCRT_ERR_IO (the message says what and where; never a crash, never a read outside the file's bytes): the file cannot
 * be opened or read; a wrong magic number; a header, channel list or attribute cut short or not ending where its size says; a
 * negative or oversized attribute size; one of channels, compression, dataWindow, displayWindow, lineOrder missing or of the wrong
 * type or size; an unknown pixelType; no channel or more than 65 536; duplicate channel names; an empty data window or one of 2^32
 * pixels or more; an offset table cut short or an offset outside the file; a chunk whose y is not its slot's, whose size is
 * negative, larger than its raw size (or, in a NONE file, not its raw size) or runs past the end of the file, or whose inflated
 * size is not its raw size.
 * Refused with MCRT_ERR_INVALID: a render in flight; NULL arguments; count 0 or > MCRT_EXR_MAX_CHANNELS; a target name the file does
 * not hold (the message names it); two targets writing one element; stride 0 or offset >= stride; reserved or flags not 0; a type
 * pair other than HALF -> F64, FLOAT -> F64, UINT -> U32.
 *
 * Widening, per value, on the bits in integer arithmetic (no floating-point mode of the device takes part); sign = the source's sign
 * bit moved to bit 63:
 *   HALF -> F64   s = h >> 15, e = (h >> 10) & 31, f = h & 1023.  e == 0, f == 0: sign.  e == 0, f != 0 (subnormal), k the index of
 *                 f's top set bit (0..9): sign | (999 + k) << 52 | (f ^ (1 << k)) << (52 - k).  1 <= e <= 30:
 *                 sign | (e + 1008) << 52 | f << 42.  e == 31, f == 0: sign | 0x7FF0000000000000.  e == 31, f != 0:
 *                 sign | 0x7FF8000000000000 | f << 42 - the payload kept, the quiet bit set: what (double)x gives on x86-64.
 *   FLOAT -> F64  the same with 8 / 23 bits: subnormal sign | (874 + k) << 52 | (f ^ (1 << k)) << (52 - k), k = 0..22; normal
 *                 sign | (e + 896) << 52 | f << 29; NaN sign | 0x7FF8000000000000 | f << 29.
 *   UINT -> U32   the bits.
 * These are the exact left inverses of the save's roundings: saving a loaded HALF channel as HALF, or a loaded FLOAT channel as
 * FLOAT, gives back the file's bits for every pattern that is not a NaN, for 0x7e00 / 0xfe00, and for every binary32 NaN whose quiet
 * bit is set.
 *
 * A target is the mirror of mcrt_exr_channel: the value of the file's channel `name` at pixel p = y * width + x (x, y relative to
 * the data window's corner) goes to data[p * stride + offset], data being double (MCRT_EXR_SRC_F64) or uint32_t (MCRT_EXR_SRC_U32)
 * elements. Elements of a destination that no target names keep their bytes, in both forms. The calls are synchronous on the
 * context's stream and need no scene. stats: kernel_ms (HIP events of the call's own around its launches), total_ms,
 * kernel_launches (1 for a file without transformed chunks, 4 otherwise). */
enum { MCRT_EXR_COMPRESSION_ZIPS = 2 };
typedef struct mcrt_exr_file mcrt_exr_file;   /* opaque: a parsed header, the offset table, the open file */
typedef struct mcrt_exr_info {
    uint32_t width, height;                       /* of the data window */
    int32_t data_window[4], display_window[4];    /* xMin, yMin, xMax, yMax as the file gives them */
    uint32_t channels, attributes;                /* counts */
    uint32_t compression, line_order, lines_per_chunk, chunks;
    uint64_t file_bytes;
} mcrt_exr_info;
typedef struct mcrt_exr_target {
    const char* name;       /* the channel's name in the file */
    void* data;             /* element of pixel p is data[p * stride + offset] of the destination type */
    uint32_t dest_type, stride, offset, reserved;   /* dest_type: MCRT_EXR_SRC_F64 or MCRT_EXR_SRC_U32; reserved 0 */
} mcrt_exr_target;
typedef struct mcrt_exr_load_params {   /* NULL or a zero field = the default */
    uint32_t threads;       /* inflate threads, default min(16, the host's hardware threads); never more than 16 */
    uint32_t flags;         /* 0 */
} mcrt_exr_load_params;
typedef struct mcrt_exr_load_result {
    uint64_t file_bytes;
    uint64_t payload_bytes;   /* what crossed from the host to the device as pixel data: height * the bytes of a scan line */
    uint32_t chunks, raw_chunks;
} mcrt_exr_load_result;
/* Header and offset table only. *out is NULL unless MCRT_OK. ctx takes the refusal's message (mcrt_last_error). */
int mcrt_exr_open(mcrt_ctx* ctx, const char* path, mcrt_exr_file** out);
void mcrt_exr_close(mcrt_exr_file* f /* may be NULL */);
int mcrt_exr_file_info(const mcrt_exr_file* f, mcrt_exr_info* info);
/* Channel i in file (= sorted) order; the name lives as long as f. MCRT_ERR_INVALID past the last. */
int mcrt_exr_file_channel(const mcrt_exr_file* f, uint32_t i, const char** name, uint32_t* pixel_type);
/* Header attribute i in file order, standard and custom: its name, type name and raw bytes (they live as long as f). */
int mcrt_exr_file_attribute(const mcrt_exr_file* f, uint32_t i, const char** name, const char** type, const void** value, uint32_t* size);
/* targets: a HOST array of structs whose data point to DEVICE memory. */
int mcrt_exr_load_device(mcrt_ctx* ctx, mcrt_exr_file* f, const mcrt_exr_target* d_targets, uint32_t count, const mcrt_exr_load_params* params /* may be NULL */,
                         mcrt_exr_load_result* result /* may be NULL */, mcrt_stats* stats /* may be NULL */);
/* Same with HOST data pointers: every distinct destination buffer is staged on the device with its present bytes and copied back
 * once, however many channels land in it. */
int mcrt_exr_load(mcrt_ctx* ctx, mcrt_exr_file* f, const mcrt_exr_target* targets, uint32_t count, const mcrt_exr_load_params* params /* may be NULL */,
                  mcrt_exr_load_result* result /* may be NULL */, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * ID mattes: per pixel, the `ranks` keys (material, surface or a caller's object index) that cover most of it, each with its
 * coverage, in the Cryptomatte layout compositors decode from the FLOAT channels and string attributes mcrt_exr_save writes. The
 * reference has no such output. The surface / material channels of the AOV pass are "the hit of sample 0": one id per pixel,
 * aliased at every silhouette; a matte counts every sample.
 *
 * Samples and keys. The samples are the AOV pass's: sample i of pixel (x, y) is its ray (above), s_i its closest hit. With
 * n = sqrtspp^2, the key of a hit sample is key_i = map[s_i]; a miss has no key. params->key chooses map:
 *   MCRT_MATTE_MATERIAL (0, default)  map = surf_material, num_keys = num_materials
 *   MCRT_MATTE_SURFACE  (1)           the identity, num_keys = num_surfaces
 *   MCRT_MATTE_CUSTOM   (2)           params->surface_key, a HOST array [num_surfaces] (a flattener's mesh / object index);
 *                                     params->num_keys must be greater than every entry
 * 0xFFFFFFFF is never a key.
 *
 * Ranking, per pixel. For every distinct key k: c_k = #{i : key_i = k}, f_k = min{i : key_i = k}. The keys are ordered by c
 * descending, then f ascending - a total order, there are no ties. For r = 0 .. ranks-1, where a rank exists:
 *   id[r] = k_r · coverage[r] = (double)c / (double)n · layer[r] = { (double)float_with_bits(code[k_r]), coverage[r] }
 * and past the last distinct key id = 0xFFFFFFFF, coverage = 0.0, layer = {0.0, 0.0}. distinct = the number of distinct keys, NOT
 * capped by ranks: a caller sees truncation. ranks: default 6; even, 2 .. 16. Integer work and one exact FP64 division: the
 * outputs are a function of the hits bit for bit, whatever the chunking (option MCRT_AOV_CHUNK_RAYS), sharding, launch shape or
 * form of the kernel (option MCRT_MATTE_FORM: "tile" pins the form that stages a tile of pixels' keys in LDS - refused with
 * MCRT_ERR_UNSUPPORTED past 2048 samples per pixel -, "memory" the form that reads them from memory; unset: the measured choice,
 * the first up to 512 samples per pixel, the second past it).
 *
 * Codes. code[k] is the Cryptomatte code of key k's name: h = MurmurHash3_x86_32(name bytes, seed 0) - blocks of 4 little-endian
 * bytes: k *= 0xcc9e2d51, k = rotl(k, 15), k *= 0x1b873593, h ^= k, h = rotl(h, 13), h = h * 5 + 0xe6546b64; the tail bytes xor-ed in
 * at shifts 16 / 8 / 0, then the same k-mix without the h-mix; h ^= len; h ^= h >> 16, h *= 0x85ebca6b, h ^= h >> 13,
 * h *= 0xc2b2ae35, h ^= h >> 16 - then e = (h >> 23) & 255, and h ^= 1 << 23 when e is 0 or 255: as a float32 no zero, denormal,
 * Inf or NaN (a hash of 0, the empty name's, becomes 0x00800000). Names: params->names, num_keys C strings of 1 .. 255 bytes of
 * printable ASCII (anything else: MCRT_ERR_INVALID); NULL: "material%u", "surface%u" or "key%u".
 *
 * layer is double because a float32 as a double passes mcrt_exr_save's F64 -> FLOAT conversion unchanged: viewed as
 * [H][W][2 * ranks] with stride 2 * ranks, offsets 0 .. 3 are NAME00.R (id), .G (coverage), .B (id), .A (coverage), offsets 4 .. 7
 * NAME01.*, and so on. Mattes are box means like the AOVs: cam->film_* is ignored (no filter-weighted coverage). The optional preview
 * layer NAME.R/G/B and sidecar manifests are not written.
 *
 * mcrt_render_matte*: shards, chunks, refusals and stats as mcrt_render_aov*. d_aov (may be NULL): the same rays and hits also
 * fill the AOV channels - one closest-hit search for both, the bits mcrt_render_aov_device gives.
 * mcrt_matte_rank_device: the ranking on a caller's own ids, no scene needed - d_keys [spp][pixels] sample-major, 0xFFFFFFFF = none;
 * d_codes [greater than every key] or NULL = layer not wanted; the buffers hold `pixels` pixels. Synchronous on the context's
 * stream. Refused with MCRT_ERR_INVALID: a render in flight, pixels 0 or >= 2^32, spp 0, pixels * spp above 0xFFF00000, d_keys or
 * d_buffers NULL, ranks odd or outside 2 .. 16 (0 = the default), layer wanted without d_codes; with MCRT_ERR_HIP when the form that
 * reads from memory cannot allocate its 8 bytes per sample.
 * mcrt_matte_code: a name's code. mcrt_matte_manifest: the JSON object {"name":"%08x",...} of the num_keys names (params->names
 * or the defaults of params->key; params may be NULL) in key order, '"' and '\' escaped, into buf (cap bytes, NUL-terminated when
 * it fits); returns the bytes needed with the NUL, or a negative MCRT_ERR_* for a bad name - so that a C++ host and Python write
 * the same manifest. */
enum { MCRT_MATTE_MATERIAL = 0, MCRT_MATTE_SURFACE = 1, MCRT_MATTE_CUSTOM = 2 };
#define MCRT_MATTE_DEFAULT_RANKS 6u
#define MCRT_MATTE_MAX_RANKS 16u
typedef struct mcrt_matte_params {  /* NULL or a zero field = the default */
    uint32_t key;                   /* MCRT_MATTE_* */
    uint32_t ranks;                 /* default 6; even, 2 .. 16 */
    uint32_t num_keys;              /* MCRT_MATTE_CUSTOM only */
    const uint32_t* surface_key;    /* MCRT_MATTE_CUSTOM only: HOST [num_surfaces] */
    const char* const* names;       /* HOST [num_keys] or NULL = the default names */
    uint64_t reserved;
} mcrt_matte_params;
typedef struct mcrt_matte_buffers {  /* every pointer may be NULL = not wanted; owned rows only, packed like d_out_rgb */
    uint32_t* id;         /* [rows][width][ranks]    */
    double*   coverage;   /* [rows][width][ranks]    */
    double*   layer;      /* [rows][width][ranks][2] */
    uint32_t* distinct;   /* [rows][width]           */
} mcrt_matte_buffers;
int mcrt_render_matte_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_matte_params* params /* may be NULL */,
                             const mcrt_matte_buffers* d_buffers, const mcrt_aov_buffers* d_aov /* may be NULL */, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers to FULL frames: rows this shard does not own are left untouched. */
int mcrt_render_matte(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_matte_params* params /* may be NULL */,
                      const mcrt_matte_buffers* buffers, const mcrt_aov_buffers* aov /* may be NULL */, mcrt_stats* stats /* may be NULL */);
int mcrt_matte_rank_device(mcrt_ctx* ctx, uint64_t pixels, uint32_t spp, const uint32_t* d_keys, uint32_t ranks, const uint32_t* d_codes /* may be NULL */,
                           const mcrt_matte_buffers* d_buffers, mcrt_stats* stats /* may be NULL */);
uint32_t mcrt_matte_code(const char* name);
int64_t mcrt_matte_manifest(const mcrt_matte_params* params /* may be NULL */, uint32_t num_keys, char* buf /* may be NULL when cap is 0 */, uint64_t cap);

/* ------------------------------------------------------------------------------------------
 * Frame comparison: error metrics and error maps between two frames of one camera - a frame under test rgb and a reference ref,
 * both [height][width][3] FP64 - computed on the device, so that only the results cross PCIe. The reference has no such
 * output. Only FP64 + - * /, compare and select, in the order written here, uncontracted, no libm routine on the device: a
 * function of the two frames (and the mask) bit for bit. sqrt and log10 of the final scalars run on the host.
 *
 *   finite(v) = (v - v == 0.0);   eps, peak, ssim_range: mcrt_compare_params
 *
 * 1. Per pixel p (row-major, p = y * width + x), with x_c, r_c the channels of rgb and ref and d_c = x_c - r_c:
 *   p is masked when a mask [height][width] is given and !(mask_p > 0) (a NaN is not > 0); otherwise p is nonfinite when any
 *   of its six values is not finite; otherwise it is compared. A masked or nonfinite pixel is excluded: it adds 0.0 at its
 *   own position to every sum and holds 0.0 in the maps, so the reduction tree depends on width * height alone.
 *   a_c   = d_c < 0 ? 0.0 - d_c : d_c
 *   se_p  = (d_r * d_r + d_g * d_g) + d_b * d_b
 *   ae_p  = (a_r + a_g) + a_b
 *   rel_p = ((d_r * d_r) / (r_r * r_r + eps) + (d_g * d_g) / (r_g * r_g + eps)) + (d_b * d_b) / (r_b * r_b + eps)
 *   differs_p = any channel's 64-bit pattern differs between rgb and ref (+0 and -0 differ, equal NaN patterns do not); it
 *   is evaluated for every pixel that is not masked, the nonfinite ones included: the count of pixels off the reference's bits.
 * sum_se, sum_ae, sum_rel = treesum over the pixels in row-major order, treesum being the one defined for mcrt_frame_noise
 * above (blocks of 256 consecutive values, stride 128 .. 1, again on the block values): not another one.
 * compared, nonfinite, masked, differing are exact counts (compared + nonfinite + masked == pixels). max_abs is the largest a_c
 * over the compared pixels and channels, max_abs_pixel the lowest pixel that holds it and max_abs_channel the lowest channel
 * of that pixel that does; with nothing compared they are 0.0, UINT64_MAX and UINT32_MAX.
 * On the host, with n = (double)(3 * compared): mse = sum_se / n, mae = sum_ae / n, relmse = sum_rel / n, rmse = sqrt(mse),
 * psnr = 10 * log10(peak * peak / mse), +inf at mse == 0; all five are 0.0 when compared == 0.
 *
 * 2. SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) on the luminance L(x) = (0.2126 * x.r + 0.7152 * x.g) + 0.0722 * x.b - the L of
 * "Firefly suppression" - with the separable 11 x 11 Gaussian window of sigma 1.5. The mask is ignored. The eleven 1-D weights
 * g[-5 .. 5] are g[i] = MCRT_SSIM_G<|i|> below - exp(-i * i / 4.5) normalised to sum 1, computed once in float64; the
 * hexadecimal literals are the definition. With Lx = L(rgb), Lr = L(ref) and the five fields f = {Lx, Lr, Lx * Lx, Lr * Lr, Lx * Lr}:
 *   h_k(x, y) = (((0.0 + g[-5] * f_k(x - 5, y)) + g[-4] * f_k(x - 4, y)) + ... + g[5] * f_k(x + 5, y))     (ascending dx)
 *   w_k(x, y) = (((0.0 + g[-5] * h_k(x, y - 5)) + g[-4] * h_k(x, y - 4)) + ... + g[5] * h_k(x, y + 5))     (ascending dy)
 * Only the centres whose window lies inside the frame exist: 5 <= x < width - 5, 5 <= y < height - 5. At a centre:
 *   mx = w_0, mr = w_1, sxx = w_2 - mx * mx, srr = w_3 - mr * mr, sxr = w_4 - mx * mr
 *   C1 = (0.01 * ssim_range) * (0.01 * ssim_range), C2 = (0.03 * ssim_range) * (0.03 * ssim_range)
 *   ssim = ((2.0 * (mx * mr) + C1) * (2.0 * sxr + C2)) / (((mx * mx + mr * mr) + C1) * ((sxx + srr) + C2))
 * A centre whose ssim is not finite adds 0.0 and is counted in ssim_excluded. sum_ssim = treesum over the centres in row-major
 * order of the (width - 10) x (height - 10) grid, ssim_centres their number, and on the host
 * mean_ssim = sum_ssim / (double)(ssim_centres - ssim_excluded), 0.0 when that count is 0. A frame narrower or lower than 11
 * has no centre: ssim_centres == 0, mean_ssim == 0.0, no error. In this order a frame compared with itself has ssim == 1.0
 * exactly at every finite centre. The constants 0.01 and 0.03 presume display-referred values in [0, ssim_range]: for HDR
 * frames set ssim_range to the frames' white level or compare tone-mapped frames. want_ssim == 0 skips all of part 2.
 *
 * 3. Maps (mcrt_compare_maps; every pointer may be NULL, the buffers are [height][width] FP64, separate from each other and
 * from the inputs): squared_error = se_p, relative = rel_p, ssim = the centre's ssim (0.0 outside the centres and at an
 * excluded centre; not written when want_ssim == 0).
 *
 * The call needs no scene, is synchronous on the context's stream (device inputs must be complete when it is called) and, in
 * the device form, moves only the result across PCIe. Refused (MCRT_ERR_INVALID): a render in flight; rgb, ref or result NULL;
 * width * height 0 or >= 2^32; eps, peak or ssim_range not finite or negative (0 = the default). stats: kernel_ms (HIP events
 * around the call's own launches), total_ms, kernel_launches. */
#define MCRT_SSIM_G0 0x1.106560aa892c0p-2
#define MCRT_SSIM_G1 0x1.b43c3f52b19f2p-3
#define MCRT_SSIM_G2 0x1.bff0fe8e98418p-4
#define MCRT_SSIM_G3 0x1.26eb175d83f67p-5
#define MCRT_SSIM_G4 0x1.f1fe01ae5a5b8p-8
#define MCRT_SSIM_G5 0x1.0d956b52a1d70p-10
typedef struct mcrt_compare_params {   /* params NULL: every default. 0 = the default for the three doubles */
    double eps;          /* relMSE's constant; default 0.01 */
    double peak;         /* PSNR's peak value; default 1.0 */
    double ssim_range;   /* SSIM's dynamic range; default 1.0 */
    int32_t want_ssim;   /* taken as it is: 0 skips SSIM (params NULL: 1) */
    uint32_t reserved;   /* 0 */
} mcrt_compare_params;                 /* 32 bytes */
typedef struct mcrt_compare_maps {     /* DEVICE (or HOST) [height][width] FP64; NULL = not wanted */
    double* squared_error;
    double* relative;
    double* ssim;
} mcrt_compare_maps;
typedef struct mcrt_compare_result {
    double sum_se, sum_ae, sum_rel, sum_ssim;
    double max_abs;
    uint64_t max_abs_pixel;
    uint32_t max_abs_channel, reserved;
    uint64_t pixels, compared, nonfinite, masked, differing, ssim_centres, ssim_excluded;
    double mse, mae, relmse, rmse, psnr, mean_ssim;   /* computed on the host */
} mcrt_compare_result;                 /* 160 bytes */
int mcrt_frame_compare_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* d_rgb, const double* d_ref,
                              const double* d_mask /* may be NULL */, const mcrt_compare_params* params /* may be NULL */,
                              const mcrt_compare_maps* d_maps /* may be NULL */, mcrt_compare_result* result, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers. */
int mcrt_frame_compare(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* rgb, const double* ref,
                       const double* mask /* may be NULL */, const mcrt_compare_params* params /* may be NULL */,
                       const mcrt_compare_maps* maps /* may be NULL */, mcrt_compare_result* result, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Occlusion pass: how open the surface under every pixel is - ambient occlusion, sky visibility and the bent normal, the passes
 * compositors and look development read next to the AOVs, and the cheapest "clay" look at a scene: the cosine-weighted visibility
 * estimate `ao` is the irradiance under a white sky, over pi. The reference has no such output; every ray is one its path tracer
 * would draw. The camera samples are the AOV pass's: sample i in 0..sqrtspp^2-1 of pixel (x, y) is Camera::samplePixel's ray
 * (camera/camera.cpp:79-95) with the sampler at initiate(y*width+x), setIndex(i) and Sampler::global_seed = global_seed. A sample
 * that misses contributes nothing. For a sample that hits, with P, N and Ns of the first hit as the AOV pass defines them (P = ray(t),
 * N the geometric normal, Ns the shading normal with its fall-back, both on the ray's side: ray/interaction.cpp:12-36), occlusion
 * ray (i, j), j in 0..rays-1, is
 *   sampler   restore(global_seed, y*width+x, i, 1 + j): initiate, setIndex(i), then the state after 1 + j calls of shuffle()
 *             (sampling/sampler.hpp:32-52) - with j = 0 the state of the path tracer's first bounce (path-tracer.cpp:23)
 *   numbers   u0 = get<DIM_BSDF>(), u1 = get<DIM_BSDF + 1>(): the pair the diffuse bounce draws (ray/ray.cpp, the last branch)
 *   direction w = CoordinateSystem(Ns).from(cosWeightedHemi(u0, u1)) (common/coordinate-system.cpp:7-35, sampling/sampling.hpp:35-44,
 *             sin and cos of the azimuth glibc's sincos); with MCRT_OCCLUSION_GEOMETRIC the basis is CoordinateSystem(N)
 *   start     P + N * 1e-9 (C::EPSILON), whatever the sign of dot(w, N)
 * and goes through the closest-hit search behind mcrt_intersect, unchanged: (t, surface). The ray SEES THE SKY when nothing is hit,
 * and is OPEN when nothing is hit or t > max_distance; max_distance == 0 means unbounded: any hit occludes. Materials play no
 * part: glass occludes. Per pixel every word is summed by ONE FP64 accumulator in ascending (i, j) - the frame does not depend on
 * chunking (option MCRT_AOV_CHUNK_RAYS: here the OCCLUSION rays per launch group, always whole pixels, one at least), sharding or
 * launch shape, bit for bit. With hits = the camera samples that hit and n = (double)(hits * rays):
 *   ao             (number of open rays) / n                    1.0 at hits == 0
 *   sky            (number of rays that see the sky) / n        1.0 at hits == 0
 *   bent_normal    (sum of w over the open rays) / n            zeros at hits == 0; NOT normalised: + - * / only, like the AOV means
 * so ao >= sky everywhere, and a bounded ao >= the unbounded one. cam->shard_* is honoured exactly as in mcrt_render_aov_device;
 * cam->film_* is IGNORED. Both calls are synchronous on the context's stream. Refused with a message (mcrt_last_error): before
 * mcrt_upload_scene (MCRT_ERR_NO_SCENE), and with MCRT_ERR_INVALID a render in flight, rays > 64, max_distance negative or not
 * finite, flag bits other than MCRT_OCCLUSION_GEOMETRIC, and ao, sky and bent_normal all NULL.
 * stats: paths = camera samples; rays = paths * (1 + rays): the camera rays and EVERY occlusion slot traced - the slots of a camera
 * sample that missed hold its camera ray and go through the search too, their results unread (misses are not compacted) -;
 * kernel_ms (HIP events around the pass's launches), total_ms, kernel_launches (5 per chunk). */
#define MCRT_OCCLUSION_GEOMETRIC 1u     /* flags: directions around the geometric normal N instead of the shading normal Ns */
#define MCRT_OCCLUSION_MAX_RAYS 64u
typedef struct mcrt_occlusion_params {  /* NULL = the defaults */
    uint32_t rays;          /* occlusion rays per camera sample that hits: 1 .. 64; 0 = 1 */
    uint32_t flags;         /* MCRT_OCCLUSION_* */
    double max_distance;    /* hits farther than this do not occlude; 0 = unbounded; finite, >= 0 */
} mcrt_occlusion_params;                /* 16 bytes */
typedef struct mcrt_occlusion_buffers { /* every pointer may be NULL = channel not wanted (not all); DEVICE memory, owned rows only, packed like d_out_rgb */
    double* ao;            /* [rows][width]    */
    double* sky;           /* [rows][width]    */
    double* bent_normal;   /* [rows][width][3] */
} mcrt_occlusion_buffers;
int mcrt_render_occlusion_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_occlusion_params* params /* may be NULL */,
                                 const mcrt_occlusion_buffers* d_buffers, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers to FULL frames: rows this shard does not own are left untouched. */
int mcrt_render_occlusion(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_occlusion_params* params /* may be NULL */,
                          const mcrt_occlusion_buffers* buffers, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Lighting passes: the light of a path-traced frame split up per pixel - what the camera sees of emitters (`emission`) and of the sky
 * (`sky`), what the first hit receives straight from the emitters and the sky (`direct`), the sampled half of that alone (`light`) and
 * the same with nothing in its way (`unoccluded`), so that light / unoccluded is the shadow matte and beauty - emission - sky - direct
 * is what arrives after more bounces. Path tracer only. For every camera sample the pass evaluates PathTracer::sampleRay's own path
 * (path-tracer.cpp:16-50) CUT AFTER ITS SECOND VERTEX, with that function's operations in its order.
 * The sample and its interaction: sample i in 0..sqrtspp^2-1 of pixel (x, y) is the AOV pass's camera ray (Camera::samplePixel,
 * camera/camera.cpp:79-95, sampler at initiate(y*width+x), setIndex(i), Sampler::global_seed = global_seed), and goes through the
 * closest-hit search behind mcrt_intersect. The sampler is then at restore(global_seed, y*width+x, i, 1): the state after the one
 * shuffle() of the loop's first iteration (path-tracer.cpp:23). `ia` is Interaction(hit, ray, external_ior) of the first hit
 * (ray/interaction.cpp:12-54) with external_ior what RefractionHistory(camera_ray) gives (the scene's IOR), the sampler in that state
 * (selectType draws DIM_INTERACTION from it) and the ray at depth 0.
 * The camera sample misses:
 *   sky_i = Scene::skyColor(ray) (scene.cpp:219-223); everything else is 0.
 * Otherwise, with throughput (1, 1, 1) - the products with it are exact and not written out:
 *   emission_i   = Integrator::sampleEmissive(ia, ls0) (integrator.cpp:93-110), ls0 the LightSample sampleRay starts with
 *   sampled half   Integrator::sampleDirect (integrator.cpp:31-86) in two halves around its shadow ray. When the first half (:31-66)
 *                  builds a shadow ray, that ray goes through the unchanged closest-hit search and light_i is the second half (:68-86)
 *                  with that hit; otherwise light_i = 0. The first half leaves ls.light and ls.select_probability as sampleDirect does.
 *   unoccluded_i = light_i when the search returned the selected light; otherwise the second half with the hit {surface = ls.light,
 *                  t = dist}, dist = length(light point - shadow ray's start) - the light as if nothing stood before it; 0 when no
 *                  shadow ray was built. So light_i <= unoccluded_i word for word, and light / unoccluded is the shadow matte.
 *   bounce half    ia.sampleBSDF(f, ls.bsdf_pdf, ray1) (interaction.cpp:56-72), T = f / ls.bsdf_pdf. The bounce is cut when it returns
 *                  false or when compMax(T) * ray1.refraction_scale == 0 (Integrator::absorb's first test, integrator.cpp:112-116; at
 *                  depth 1 its roulette does not play): bounce_i = 0. Otherwise ray1 goes through the search; on a miss
 *                  bounce_i = skyColor(ray1) * T, on a hit bounce_i = sampleEmissive(ia1, ls) * T with ia1 what Interaction's
 *                  constructor derives for that hit at depth 1 (position, material, geometric normal, inside, t, out; dirac_delta as
 *                  ray1 carries it) and ls the light sample of vertex 1: light and select_probability from the sampled half, bsdf_pdf
 *                  from the bounce half. So a lamp the bounce finds is weighted against the sampled half exactly as the path tracer
 *                  weights it, and light + bounce is the whole direct light, once.
 *   direct_i     = light_i + bounce_i, in this order
 * Both rays of a sample go through the search in one launch of 2 rays per sample. Per pixel every channel word is
 * (sum over i, ascending, in ONE FP64 accumulator) / spp: box means like the AOVs, every sample one addend (zeros included). At
 * sqrtspp 1, in a scene whose paths all end by their second vertex, (emission + direct) + sky is the path tracer's frame bit for bit.
 * The frame does not depend on chunking (option MCRT_AOV_CHUNK_RAYS: here the shadow and bounce slots per launch group, always whole
 * pixels, one at least; default: what 2^17 pixels take, at least 2^24 and at most 2^26 slots), sharding or launch shape, bit for bit. cam->shard_* is honoured exactly as in mcrt_render_aov_device;
 * cam->film_* is IGNORED. Both calls are synchronous on the context's stream. Refused with a message (mcrt_last_error): before
 * mcrt_upload_scene (MCRT_ERR_NO_SCENE), and with MCRT_ERR_INVALID a render in flight, a bad shard, and all five channels NULL.
 * stats: paths = camera samples; rays = 3 * paths: the camera ray and BOTH slots of every sample traced - the slots of a sample without
 * a shadow or a bounce ray hold its camera ray and go through the search too, their results unread (dead slots are not compacted) -;
 * kernel_ms (HIP events around the pass's launches), total_ms, kernel_launches (5 per chunk).
 * Not done: photon-mapped frames, filter-weighted means. (Per-light frames of the whole path: "Light groups" below; the whole path
 * split by lobe, direct and indirect: "Path classes" below.) */
typedef struct mcrt_lighting_buffers { /* every pointer may be NULL = channel not wanted (not all); DEVICE memory, owned rows only, packed like d_out_rgb */
    double* emission;     /* [rows][width][3] */
    double* sky;          /* [rows][width][3] */
    double* direct;       /* [rows][width][3] */
    double* light;        /* [rows][width][3] */
    double* unoccluded;   /* [rows][width][3] */
} mcrt_lighting_buffers;
int mcrt_render_lighting_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_lighting_buffers* d_buffers,
                                mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers to FULL frames: rows this shard does not own are left untouched. */
int mcrt_render_lighting(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_lighting_buffers* buffers,
                         mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Light groups: the path-traced frame split by emitter, EVERY bounce - one frame ("plane") per group of emitters and one for the sky,
 * which add up to the beauty frame, so that dimming a lamp, recolouring another or turning the sky down is a weighted sum of planes.
 * Path tracer only. The lighting passes above are iteration 0 of what is defined here.
 * The sample: sample i in 0..sqrtspp^2-1 of pixel (x, y) is the AOV pass's camera ray (Camera::samplePixel, camera/camera.cpp:79-95,
 * sampler at initiate(y*width+x), setIndex(i), Sampler::global_seed = global_seed).
 * The path is the while (true) of PathTracer::sampleRay (path-tracer.cpp:14-51) with the same functions in the same order and the same
 * throughput: ray = the camera ray, throughput = (1, 1, 1), ls = {0, 0, none}, RefractionHistory(ray). Iteration k = 0, 1, ... begins
 * with one shuffle(), so its sampler is restore(global_seed, y*width+x, i, k + 1). Then, as :25-49 have it:
 *   the ray goes through the closest-hit search behind mcrt_intersect. On a miss c = Scene::skyColor(ray) (scene.cpp:219-223) is added
 *     and the path ends.
 *   ia = Interaction(hit, ray, history.externalIOR(ray)) (ray/interaction.cpp:12-54)
 *   c = Integrator::sampleEmissive(ia, ls) (integrator.cpp:93-110) is added
 *   c = Integrator::sampleDirect(ia, ls) (integrator.cpp:31-86) is added: its first half (:31-66) chooses the light point, leaves
 *     ls.light and ls.select_probability and builds the shadow ray or returns zeros; the shadow ray goes through the same search; the
 *     second half (:68-86) is evaluated with that hit
 *   ia.sampleBSDF(f, ls.bsdf_pdf, ray) (interaction.cpp:56-72); false ends the path
 *   throughput = throughput * (f / ls.bsdf_pdf)
 *   Integrator::absorb(ray, throughput) (integrator.cpp:112-129, its roulette drawing DIM_ABSORB of this iteration's sampler); true
 *     ends the path
 *   history.update(ray)
 * The sample keeps one radiance R_p per plane p, all starting at (0, 0, 0). Where the path tracer executes radiance = radiance +
 * c * throughput, the pass executes R_p = R_p + c * throughput for exactly ONE plane p:
 *   c = skyColor(ray):           p = sky_plane
 *   c = sampleEmissive(ia, ls):  p = plane[ia.surface]
 *   c = sampleDirect(ia, ls):    p = plane[ls.light]
 * with plane[s] = surface_group[s] for an emitter s (a surface whose material carries MCRT_MAT_EMISSIVE). The operands and their order
 * are the path tracer's: the direct light of vertex k is added with the throughput of vertex k, before anything of vertex k + 1. A term
 * that the functions return as zeros is skipped: all values are >= +0.0, so the bits are the same. Per pixel and plane every word of the
 * frame is (((0.0 + R_p(0)) + R_p(1)) + ...) / (double)spp: ascending i, one FP64 accumulator per word, not clamped - box means.
 * Parameters (params NULL, or a field zero: the default):
 *   num_groups     G, 1 .. MCRT_LIGHT_GROUPS_MAX (0 = 1)
 *   surface_group  HOST [num_surfaces of the uploaded scene]: the group of every surface. Entries of surfaces that are not emitters are
 *                  ignored; an emitter's entry must be < G. NULL: every emitter in group 0.
 *   sky_plane      read when flags carries MCRT_LIGHT_GROUPS_SKY_PLANE (0 is a plane like any other): the plane that takes the sky, any
 *                  value <= G. Otherwise G: a plane of its own after the groups. The number of planes is P = max(G, sky_plane + 1)
 *                  (mcrt_light_group_planes; at most MCRT_LIGHT_GROUPS_MAX + 1 = 16).
 *   max_depth      D; 0 = the whole path. With D > 0 iteration k == D takes only its miss or its sampleEmissive term and the path ends
 *                  there: no light sample, no bounce. D = 1 is the lighting passes' cut - planes of direct light only -, and the
 *                  indirect light per group is the full planes minus these.
 * Output: d_planes, [P][rows][width][3] doubles, the rows this shard owns packed like d_out_rgb. cam->shard_* is honoured exactly as in
 * mcrt_render_aov_device; cam->film_* is IGNORED unless flags carries MCRT_LIGHT_GROUPS_FILM ("Filtered planes" below). Both calls are synchronous on
 * the context's stream.
 * What holds, bit for bit unless said otherwise:
 *   - The planes are a function of scene, camera, seed and parameters. They do not depend on chunking (option MCRT_AOV_CHUNK_RAYS: here
 *     the shadow and bounce slots of iteration 0 per chunk - 2 per sample, whole pixels, one at least; default: what 2^17 pixels take, at least
 *     2^25 and at most 2^26 slots, cut down to what 8 GiB of path state hold), sharding, launch shape, or the order in which live samples are queued.
 *   - A group's plane does not depend on how the OTHER emitters are grouped.
 *   - With G = 1, surface_group NULL, sky_plane = 0 and D = 0, plane 0 is the box-film frame of mcrt_render (path tracer, same camera
 *     and seed), in the exact library, wherever that frame's mean is neither negative nor NaN.
 *   - With more planes their sum agrees with that frame to rounding: relative error <= 1e-12, this header's bound for sums of
 *     non-negative terms taken in another order.
 * Refused with a message (mcrt_last_error): before mcrt_upload_scene (MCRT_ERR_NO_SCENE); with MCRT_ERR_INVALID a render in flight, a bad
 * camera or shard, d_planes NULL, G > MCRT_LIGHT_GROUPS_MAX, sky_plane > G, an emitter whose surface_group entry is >= G (the surface is
 * named); with MCRT_ERR_UNSUPPORTED a path that nests more dielectric media than the history's 8 entries in registers' reach (mcrt_render
 * renders such frames again through the wavefront pipeline's deep rows; this pass says so and stops), and a frame whose paths are still
 * alive after 4096 iterations (the host loop is bounded).
 * stats: paths = camera samples; rays = the rays handed to the search: the camera rays and 2 per sample alive at every iteration that
 * traces (a sample without a shadow or a bounce ray has a finite dummy traced in that slot; a sample whose ray missed is not alive: its
 * sky was added where the miss was found); kernel_ms (HIP events around the pass's
 * launches), total_ms, kernel_launches.
 * Not done: photon-mapped frames, nesting deeper than 8 media. (A split by lobe - diffuse / glossy /
 * transmission -: "Path classes" below.) */
#define MCRT_LIGHT_GROUPS_MAX 15u
enum {
    MCRT_LIGHT_GROUPS_SKY_PLANE = 1u, /* mcrt_light_group_params.flags: sky_plane is given */
    MCRT_LIGHT_GROUPS_FILM = 2u,      /* the planes through the camera's film ("Filtered planes") */
    MCRT_LIGHT_GROUPS_FILM_CLAMP = 4u /* with FILM: max(., 0) on every word */
};
typedef struct mcrt_light_group_params {
    uint32_t num_groups;           /* G; 0 = 1 */
    uint32_t flags;                /* MCRT_LIGHT_GROUPS_* */
    uint32_t sky_plane;            /* with MCRT_LIGHT_GROUPS_SKY_PLANE: <= G; otherwise ignored (the sky's plane is G) */
    uint32_t max_depth;            /* D; 0 = the whole path */
    const uint32_t* surface_group; /* HOST [num_surfaces], or NULL = every emitter in group 0 */
} mcrt_light_group_params;         /* 24 bytes */
/* P of these parameters (NULL: 2, one group and the sky); 0 when num_groups or sky_plane is out of range. */
uint32_t mcrt_light_group_planes(const mcrt_light_group_params* params);
int mcrt_render_light_groups_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_light_group_params* params /* may be NULL */,
                                    double* d_planes, mcrt_stats* stats /* may be NULL */);
/* Same with a HOST pointer to P FULL frames, [P][height][width][3]: rows this shard does not own are left untouched. */
int mcrt_render_light_groups(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_light_group_params* params /* may be NULL */,
                             double* planes, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Path classes: the path-traced frame split by what the FIRST surface did with the light - diffuse, glossy, transmission -, each into
 * the light that arrived there directly and the light that arrived after further bounces, plus emission and background: the layers a
 * compositor grades separately and a denoiser filters separately. Path tracer only.
 * The sample, the path, the sampler positions, the closest-hit search and the order of all operations are exactly those of "Light
 * groups" above: sample i of pixel (x, y) is the AOV pass's camera ray, iteration k of the while (true) of PathTracer::sampleRay has its
 * sampler at restore(global_seed, y*width+x, i, k + 1), and every iteration runs the functions listed there in that order.
 * The class: Interaction's selectType (ray/interaction.cpp:156-183) picks ONE lobe per vertex before any light is gathered. Let L be
 * ia.type of iteration 0's interaction: DIFFUSE -> diffuse, REFLECT -> glossy (on a Dirac surface too), REFRACT -> transmission. Every
 * term of the path's radiance has one class (MCRT_PATH_CLASSES = 8, in this order):
 *   0 emission                c = sampleEmissive(ia, ls) of iteration 0
 *   1 background              c = skyColor(ray) of a camera ray that misses (iteration 0's miss)
 *   2, 4, 6 diffuse_direct, glossy_direct, transmission_direct (by L)
 *                             c = sampleDirect(ia, ls) of iteration 0; c = sampleEmissive(ia, ls) of iteration 1; c = skyColor(ray) of
 *                             iteration 1's miss: the light sample and the BSDF bounce of the first vertex, which the path tracer weights
 *                             against each other
 *   3, 5, 7 diffuse_indirect, glossy_indirect, transmission_indirect (by L)
 *                             c = sampleDirect(ia, ls) of iteration 1; every term of the iterations >= 2
 * The sample keeps one radiance R_p per plane p, all starting at (0, 0, 0). Where the path tracer executes radiance = radiance +
 * c * throughput, the pass executes R_p = R_p + c * throughput for exactly ONE plane p = class_plane[class of the term]. The operands
 * and their order are the path tracer's. A term that the functions return as zeros is skipped, as in the light groups. Per pixel,
 * plane and word the frame is (((0.0 + R_p(0)) + R_p(1)) + ...) / (double)spp: ascending i, one FP64 accumulator per word, not clamped.
 * Parameters (params NULL, or a field zero: the default):
 *   flags        MCRT_PATH_CLASSES_MAP: class_plane is given. Otherwise it is the identity: 8 planes in the order above.
 *   class_plane  the output plane of every class, each < MCRT_PATH_CLASSES. The number of planes is P = 1 + max(class_plane)
 *                (mcrt_path_class_planes). Classes may share a plane; a plane that no class maps to comes back as zeros.
 *   max_depth    D, with the light groups' meaning: 0 = the whole path; with D > 0 iteration k == D takes only its miss or its
 *                sampleEmissive term and the path ends there.
 * Output: d_planes, [P][rows][width][3] doubles, the rows this shard owns packed like d_out_rgb. cam->shard_* is honoured exactly as in
 * mcrt_render_aov_device; cam->film_* is IGNORED unless flags carries MCRT_PATH_CLASSES_FILM ("Filtered planes" below). Both calls are synchronous on
 * the context's stream.
 * What holds, bit for bit unless said otherwise:
 *   1. The planes are a function of scene, camera, seed and parameters. They do not depend on chunking (option MCRT_AOV_CHUNK_RAYS, with
 *      the light groups' meaning and default), sharding, launch shape, or the order in which live samples are queued.
 *   2. With all eight classes mapped to plane 0 and D = 0, plane 0 is the box-film frame of mcrt_render (path tracer, same camera and
 *      seed), in the exact library, wherever that frame's mean is neither negative nor NaN - and so the light groups' single plane.
 *   3. A plane does not depend on how the classes that do not map to it are mapped.
 *   4. emission, background and the three *_direct planes are the same for every D >= 1 and for D = 0: they receive terms in iterations
 *      0 and 1 only, in the same order. With D = 1 the *_indirect planes are zeros.
 *   5. The planes add up to the beauty frame to rounding: relative error <= 1e-12, this header's bound for sums of non-negative terms
 *      taken in another order.
 * Refused with a message (mcrt_last_error): before mcrt_upload_scene (MCRT_ERR_NO_SCENE); with MCRT_ERR_INVALID a render in flight, a bad
 * camera or shard, d_planes NULL, a class_plane entry >= MCRT_PATH_CLASSES (the class is named); with MCRT_ERR_UNSUPPORTED a path that
 * nests more than 8 dielectric media and a frame whose paths are still alive after 4096 iterations, as in the light groups.
 * stats: as in the light groups (rays = the camera rays and 2 per sample alive at every iteration that traces).
 * Not done: photon-mapped frames, a split of glossy into Dirac and rough, classification by any vertex other than the first, classes x
 * light groups in one call, albedo-divided planes, nesting deeper than 8 media. */
#define MCRT_PATH_CLASSES 8u
enum {
    MCRT_PATH_CLASS_EMISSION = 0,
    MCRT_PATH_CLASS_BACKGROUND = 1,
    MCRT_PATH_CLASS_DIFFUSE_DIRECT = 2,
    MCRT_PATH_CLASS_DIFFUSE_INDIRECT = 3,
    MCRT_PATH_CLASS_GLOSSY_DIRECT = 4,
    MCRT_PATH_CLASS_GLOSSY_INDIRECT = 5,
    MCRT_PATH_CLASS_TRANSMISSION_DIRECT = 6,
    MCRT_PATH_CLASS_TRANSMISSION_INDIRECT = 7
};
enum {
    MCRT_PATH_CLASSES_MAP = 1u,       /* mcrt_path_class_params.flags: class_plane is given */
    MCRT_PATH_CLASSES_FILM = 2u,      /* the planes through the camera's film ("Filtered planes") */
    MCRT_PATH_CLASSES_FILM_CLAMP = 4u /* with FILM: max(., 0) on every word */
};
typedef struct mcrt_path_class_params {
    uint32_t flags;                          /* MCRT_PATH_CLASSES_* */
    uint32_t max_depth;                      /* D; 0 = the whole path */
    uint8_t class_plane[MCRT_PATH_CLASSES];  /* with MCRT_PATH_CLASSES_MAP: the plane of every class, each < MCRT_PATH_CLASSES */
} mcrt_path_class_params;                    /* 16 bytes */
/* P of these parameters (NULL: 8); 0 when a class_plane entry is out of range. */
uint32_t mcrt_path_class_planes(const mcrt_path_class_params* params);
int mcrt_render_path_classes_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_path_class_params* params /* may be NULL */,
                                    double* d_planes, mcrt_stats* stats /* may be NULL */);
/* Same with a HOST pointer to P FULL frames, [P][height][width][3]: rows this shard does not own are left untouched. */
int mcrt_render_path_classes(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_path_class_params* params /* may be NULL */,
                             double* planes, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Filtered planes: the light groups' and the path classes' planes through the camera's reconstruction filter (film_filter, film_radius,
 * film_cache_size) instead of the box mean, so that they add up to the FILTERED beauty frame - and, with one plane, a filtered beauty
 * frame that is a function of its inputs bit for bit, with or without a lens (mcrt_render's is splatted with atomics and agrees with
 * itself to rounding only). No new call: flags on the two parameter structs, whose sizes and MCRT_ABI_VERSION stay.
 *   MCRT_LIGHT_GROUPS_FILM, MCRT_PATH_CLASSES_FILM              resolve the planes through the film
 *   MCRT_LIGHT_GROUPS_FILM_CLAMP, MCRT_PATH_CLASSES_FILM_CLAMP  with FILM: Splat::get's max(., 0) on every word (ignored without FILM).
 *       Planes are NOT clamped by default: a filter with negative lobes (Mitchell-Netravali, Catmull-Rom, Lanczos) gives signed planes,
 *       and only unclamped planes add up. Clamped, the single plane is the reference's frame.
 * Without FILM every byte of every call is what it was. With FILM and a film that does not splat (the default box: film_filter
 * MCRT_FILM_BOX with film_radius 0 or 0.5) the plain resolve runs and the bytes are the unflagged call's.
 * A film that splats, operation by operation. The walk and every sample's R_p are those of "Light groups" / "Path classes"; only the
 * resolve differs.
 *   Sample i of pixel (x, y) has the film position px = (double)x + get(kDimPixel), py = (double)y + get(kDimPixel + 1), the sampler at
 *   initiate(global_seed, y*width + x), setIndex(i): the camera ray's own pair, also under a lens.
 *   r = film_radius, or the filter's default radius when film_radius is 0 (film.cpp:31-44).
 *   The sample COVERS output pixel (qx, qy) exactly when Film::deposit (film.cpp:61-79) would write it there:
 *     max((long long)(px + 0.5 - r), 0) <= qx <= min((long long)(px - 0.5 + r), width - 1), the conversions truncating, and the same
 *     in y with height.
 *   Its weight there is w = filter(qy + 0.5 - py) * filter(qx + 0.5 - px), filter being Film::filter (film.cpp:86-97):
 *     film_cache_size == 0: filter_function(2 / r * fabs(t)) (camera/filter.hpp; the widened box: 1)
 *     otherwise:            table[(size_t)((film_cache_size - 1) / r * fabs(t) + 0.5)], table[k] = filter_function(2 k / (film_cache_size - 1))
 *   Per plane p, output pixel and channel, over the covering samples s1, s2, ... in ascending packed source pixel (y*width + x), then
 *   ascending sample index, one FP64 accumulator each, no operation contracted:
 *     S = (((0.0 + R_p(s1) * w(s1)) + R_p(s2) * w(s2)) + ...)
 *     W = ((0.0 + w(s1)) + w(s2)) + ...
 *   and the word is W == 0 ? 0 : S / W - under CLAMP max(S / W, 0), a NaN giving 0 as in Splat::get. NaN and Inf are not filtered.
 *   This is Film::deposit's own arithmetic - the same products v * weight, the same sums - in a FIXED order; the reference's order is
 *   whatever its threads' atomics make it. Clamped, the single plane therefore agrees with the reference's frame (and mcrt_render's)
 *   to rounding: 1e-12 relative in the exact library.
 * The order is global, so the planes do not depend on chunking (MCRT_AOV_CHUNK_RAYS), bit for bit: chunks are contiguous ranges of
 * packed pixels visited in ascending order on one stream, and a chunk's gather continues the running S and W where the chunk before
 * left them. S lives in d_planes (zeroed by the call), W in one frame-sized array of the family's scratch; both are normalised in place
 * after the last chunk. d_planes must therefore not be read before the call returns.
 * What holds, bit for bit: the planes are a function of scene, camera (its film included), seed and parameters - not of chunking, launch
 * shape, the live lists' order or the run; a group's plane does not depend on how the other emitters are grouped; the path classes'
 * single plane is the light groups' single plane. To rounding: the unclamped planes add up to the single unclamped plane (1e-12 relative
 * for a filter without negative lobes).
 * Refused with a message that names the reason (MCRT_ERR_UNSUPPORTED unless said otherwise), d_planes untouched:
 *   - cam->shard_count > 1: the gather needs the neighbours' rows (not done: an S, W output form like mcrt_render_film_device's)
 *   - a ray source set on the context (mcrt_set_ray_source): its pixels have no film position
 *   - the FILM flags inside mcrt_probe_params.groups (MCRT_ERR_INVALID): a probe has no film
 *   - film_filter > MCRT_FILM_LANCZOS (MCRT_ERR_INVALID)
 *   - film_cache_size == 1 (MCRT_ERR_INVALID): the table's step 2 / (film_cache_size - 1) has no value
 *   - film_radius negative, not a number, or 1e6 and more (MCRT_ERR_INVALID): the window's rows are counted in 32 bits
 * Adaptive sampling and the statistics calls stay refused for splatting films as they are.
 * Option MCRT_FILM_GATHER=force (mcrt_set_option, per context; a test's lever): a film that does not splat goes through the gather too
 * - radius 0.5, every weight 1, every window one pixel - and gives the plain resolve's bytes: S = sum of R_p, W = (double)spp.
 * Not done: the AOV, matte, occlusion and lighting passes (box means are what denoisers and id passes want); sharded cameras; adaptive
 * sampling and the statistics under a filter; a public gather over caller-supplied per-sample values. */

/* ------------------------------------------------------------------------------------------
 * Adaptive sampling: a per-pixel stopping rule. mcrt_render_converged stops when the whole FRAME is quiet enough and until then samples
 * every pixel at full price; this pass renders batch 0 over the frame and every later batch over the LIST of pixels that are still
 * noisy (or lie next to one), and delivers the accumulated summary of every pixel together with a sample-count map that shows where the
 * samples went. The reference has no such output. Path tracer only (the walk over a list is the light groups', which supports no other
 * integrator): there is no integrator argument. What decides anything - the batch summary, the merge, the criterion - is only FP64
 * + - * /, compare and select, in the order written here, uncontracted, no libm routine: a function of scene, camera, seed and
 * parameters bit for bit.
 *
 * Batches. Batch j (j = 0, 1, ...) has n = sqrtspp^2 samples per LISTED pixel. A pixel numbers its own batches: with count[p] = k n
 * samples so far, its next batch is its batch k, whichever batch of the call lists it, and the sampler of pixel (x, y) is then
 * initiate(global_seed + k (wrapping in uint32_t), y * width + x) with sample index i = 0 .. n-1: the samples a full render of cam at
 * seed global_seed + k gives that pixel, whatever else is listed. As long as no batch has left a pixel out, k = j for every pixel. The
 * batch summary of a listed pixel is what mcrt_render_pixel_stats delivers for it at that seed ("Per-pixel sample statistics"): rgb the
 * frame value max(m, 0), variance two-pass about the unclamped mean m, half_a and half_b the means of the even and of the odd samples.
 * Merge. Every pixel p has accumulators rgb, variance, half_a, half_b and a count[p], 0 before batch 0. A listed pixel takes its batch
 * summary by mcrt_frame_merge's formulas ("Accumulated rendering" 1.) with n_a = count[p], n_b = n, accumulator = A, batch = B, in place,
 * the halves' parity rule included; a pixel with count[p] = 0 takes the batch summary as it is. Then count[p] = count[p] + n. A pixel
 * that is not listed is not touched. So a pixel's outputs depend on its count alone: with count[p] = k n they are the outputs of
 * mcrt_render_converged (path tracer, same camera and seed, max_spp = k n, no target) at that pixel, bit for bit.
 * Criterion. After the merge of each batch, on the accumulated rgb (r, g, b), variance (v_r, v_g, v_b) and n_p = count[p], with
 * T2 = target * target and F2 = floor * floor computed once on the host:
 *   e_p     = ((v_r + v_g) + v_b) / (double)n_p
 *   g_p     = (r * r + g * g) + b * b
 *   noisy_p = g_p == g_p  and  e_p > T2 * (g_p > F2 ? g_p : F2)      (false when a NaN takes part: a NaN pixel retires)
 *   p is listed for the next batch when
 *     count[p] + n <= max_spp
 *     and ( batches so far < min_batches   or   target_relative_error == 0
 *           or noisy_q for some q with |x_q - x_p| <= r and |y_q - y_p| <= r inside the frame )          (r = window)
 * Before batch 0 no batch was rendered, so every pixel is listed. The list is rebuilt from scratch after every batch: a retired pixel
 * comes back when a neighbour turns noisy. It holds the packed pixels y * width + x in ascending order. The loop ends when the list is
 * empty; ending at max_spp is not an error. Nothing depends on how a list is cut into chunks (option MCRT_AOV_CHUNK_RAYS, with the
 * light groups' meaning and default) or on the order in which live samples are queued.
 * A batch whose list is the whole frame, while no batch before it has left a pixel out (every pixel is at its batch j), is one
 * mcrt_render_pixel_stats_device at seed global_seed + j followed by the merge (option MCRT_ADAPTIVE_FULL_BATCH=render, the default:
 * the render kernel is several times cheaper per sample than the walk) or a walk like every other batch (=walk); both give the same
 * bytes. The first min_batches batches are such full ones.
 * Parameters (params NULL, or a field zero: the default):
 *   target_relative_error  per PIXEL: a pixel is quiet when the estimated standard error of its mean is at most this fraction of its
 *                          radiance (sqrt(e_p) <= target * max(sqrt(g_p), floor)). 0 (the default): no pixel ever retires before max_spp.
 *   floor                  the radiance below which a pixel's signal counts as `floor`: dark pixels are not chased for a RELATIVE
 *                          error they cannot reach. Default: 0.01 * sqrt(signal / (double)pixels), signal being mcrt_frame_noise's
 *                          of the frame after batch 0 (its treesum: a function of the bits; sqrt on the host) - a hundredth of the
 *                          root mean square radiance -, or 0 when that is not finite. (For no floor pass the smallest positive double.)
 *   max_spp                per pixel; default 1024, or one batch where that is more.
 *   min_batches            default 1; with sqrtspp 1 it is at least 2 (a 1-sample batch has variance 0), as in mcrt_converge_params.
 *   window                 the Chebyshev radius r of the dilation, 1 .. 4; default 1. MCRT_ADAPTIVE_WINDOW_NONE: r = 0, a pixel
 *                          answers for itself alone.
 * Outputs: d_out_rgb and the channels of d_stats that are not NULL are FULL frames [height][width][3]; d_count, when given, is
 * [height][width] uint32_t, the samples every pixel received. result: the batches rendered, the smallest and largest count, the sum of
 * count over the frame, and the length of the list of each of the first MCRT_CONVERGE_TRACE batches (0 past `batches`). The three
 * numbers about the counts are computed on the host: both forms, the _device one too, read the count map back once at the end (4 bytes
 * a pixel), next to the one word per batch that is the list's length.
 * stats: paths, rays, node_tests, prim_tests, knn_searches, kernel_ms and kernel_launches summed over the batches (the rule and the
 * list count 4 launches a batch, a merge 1), kernel_id of the last rendered full batch (MCRT_KERNEL_NONE when every batch was a walk),
 * total_ms of the call. Both calls are synchronous on the context's stream.
 * Refused with a message (mcrt_last_error): before mcrt_upload_scene (MCRT_ERR_NO_SCENE); with MCRT_ERR_UNSUPPORTED a camera whose film
 * splats (a reconstruction filter, or a box of another radius), cam->shard_count > 1 - the window needs the neighbouring rows -, a path
 * that nests more than 8 dielectric media and a list whose paths are still alive after 4096 iterations, as in the light groups; with
 * MCRT_ERR_INVALID a render in flight, cam or the frame NULL, sqrtspp 0, a target or floor that is negative or not finite, window > 4,
 * max_spp below one batch.
 * Not done: photon-mapped frames, filtered (splatting) films, sharded cameras, highlights (tops / level) under per-pixel counts, a
 * frame-level relative_error for non-uniform counts, continuing the Sobol sequence across batches instead of reseeding, compaction of
 * the walk's tail iterations. */
#define MCRT_ADAPTIVE_WINDOW_NONE 0xFFFFFFFFu
typedef struct mcrt_adaptive_params {   /* NULL or a zero field = the default */
    double   target_relative_error;     /* per PIXEL; finite, >= 0; 0 = no pixel ever retires before max_spp */
    double   floor;                     /* radiance below which a pixel's signal counts as `floor`; finite, >= 0 */
    uint32_t max_spp;                   /* per pixel; default 1024, or one batch where that is more */
    uint32_t min_batches;               /* default 1; with sqrtspp 1 it is 2 (as in mcrt_converge_params) */
    uint32_t window;                    /* Chebyshev radius r of the dilation, 1 .. 4; MCRT_ADAPTIVE_WINDOW_NONE = 0 */
} mcrt_adaptive_params;                 /* 32 bytes */
typedef struct mcrt_adaptive_result {
    uint32_t batches, min_count, max_count;
    uint64_t samples;                         /* sum of count over the frame */
    uint32_t active[MCRT_CONVERGE_TRACE];     /* pixels listed for batch j, first 64 */
} mcrt_adaptive_result;
int mcrt_render_adaptive_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_adaptive_params* params /* may be NULL */,
                                double* d_out_rgb, const mcrt_pixel_stats_buffers* d_stats /* may be NULL */, uint32_t* d_count /* may be NULL */,
                                mcrt_adaptive_result* result /* may be NULL */, mcrt_stats* stats /* may be NULL */);
/* The list alone. DIAGNOSTIC AND UNSTABLE: it exists so that the compaction can be tested by itself on the device, is no part of the
 * interface a renderer builds on, and may change or go without a new ABI version. The pass's three list launches (count, scan, scatter) on `pixels` flags (HOST, one byte each, set =
 * not zero) -> list (HOST, room for `pixels` words): the indices of the set flags in ascending order, *length of them. Needs no scene.
 * Refused (MCRT_ERR_INVALID) while a render is in flight, with a NULL pointer, with pixels 0 or >= 2^32. */
int mcrt_adaptive_list(mcrt_ctx* ctx, uint64_t pixels, const uint8_t* flags, uint32_t* list, uint32_t* length);
/* Same with HOST pointers. */
int mcrt_render_adaptive(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_adaptive_params* params /* may be NULL */,
                         double* out_rgb, const mcrt_pixel_stats_buffers* stats_buffers /* may be NULL */, uint32_t* count /* may be NULL */,
                         mcrt_adaptive_result* result /* may be NULL */, mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Camera models: orthographic, equirectangular (panoramic) and fisheye lenses for the passes that trace camera rays. The reference has
 * one camera, the pinhole with its thin lens; a lens set on the context replaces how a pixel sample becomes a ray, and nothing else: the
 * AOV pass, the ID mattes, the occlusion pass, the lighting passes, the light groups and the path classes read their camera rays as
 * records and never look at the camera again (the walk only for `width` and the pixel's name, the sampler key). The beauty frame under a
 * lens is the light groups with everything in one plane (the binding's Context.render_lens).
 *
 * Every model starts from the film position of the existing camera, operation by operation in FP64, uncontracted:
 *   sampler at initiate(global_seed, y * width + x), setIndex(i)
 *   px = (double)x + get(kDimPixel),  py = (double)y + get(kDimPixel + 1)
 *   half_x = (double)width * 0.5,  half_y = (double)height * 0.5
 *   E, F, L, U = cam->eye, forward, left, up, read as given (not normalised, not made orthogonal)
 * and ends in makeRay(start, direction, scene_ior). normalize(v) is v * (1 / sqrt((x * x + y * y) + z * z)), the project's own (csrc/mcrt_math.hpp); sincos is glibc 2.35's, restated
 * (csrc/mcrt_libm.hpp refSinCos).
 *   MCRT_LENS_PERSPECTIVE      the camera's own ray (camera/camera.cpp:79-95), thin lens included, through the lens kernel: the model
 *                              that has an exact oracle. Reads no field of the descriptor.
 *   MCRT_LENS_ORTHOGRAPHIC     s = width_world / (double)width
 *                              lx = s * (half_x - px),  ly = s * (half_y - py)
 *                              start = (E + L * lx) + U * ly
 *                              direction = normalize(F)
 *   MCRT_LENS_EQUIRECTANGULAR  lon = ((half_x - px) / (double)width) * fov_x
 *                              lat = ((half_y - py) / (double)height) * fov_y
 *                              sincos(lon) -> sl, cl;  sincos(lat) -> st, ct
 *                              start = E
 *                              direction = normalize((F * (ct * cl) + L * (ct * sl)) + U * st)
 *                              0 < fov_x <= 2 pi (0: 2 pi), 0 < fov_y <= pi (0: pi). The frame's left edge looks along L.
 *   MCRT_LENS_FISHEYE          equidistant. R = min(half_x, half_y)
 *                              u = (half_x - px) / R,  v = (half_y - py) / R,  r = sqrt(u * u + v * v)
 *                              theta = min(r * (fov_x * 0.5), pi)
 *                              sincos(theta) -> s, c
 *                              start = E
 *                              direction = r == 0 ? normalize(F) : normalize(F * c + (L * u + U * v) * (s / r))
 *                              0 < fov_x <= 2 pi (0: pi), the full angle across the image circle; fov_y is not read.
 *                              Outside the image circle (r > 1) the mapping simply continues, up to straight backwards. The mask r <= 1
 *                              is a function of the pixel coordinates alone and is the CALLER's to compute; no pass applies it.
 * "2 pi" and "pi" are the doubles 0x1.921fb54442d18p+2 and 0x1.921fb54442d18p+1.
 *
 * mcrt_set_lens validates the descriptor and copies it into the context, where it stays until the next call; NULL or model
 * MCRT_LENS_NONE: no lens, the camera's own rays by the passes' own kernels, every byte of every call what it was. mcrt_get_lens
 * returns the descriptor as it was given (all zero with none set). Refused with MCRT_ERR_INVALID and a message: a width_world, fov_x
 * or fov_y that is not finite (whichever model reads it) or, where the model reads it, out of its range, non-zero flags or reserved, an
 * unknown model; also a render in flight. While a lens is set:
 *   - mcrt_render_aov*, _matte*, _occlusion*, _lighting*, _light_groups* and _path_classes* take their camera rays from it; the three
 *     new models refuse a camera with thin_lens != 0 (MCRT_ERR_UNSUPPORTED);
 *   - every call that makes its camera rays inside a render kernel refuses with MCRT_ERR_UNSUPPORTED and a message that names
 *     mcrt_set_lens: mcrt_render*, mcrt_render_film_device, mcrt_render_multi and what is built on them (pixel statistics, highlights,
 *     converged rendering), and mcrt_render_adaptive*, whose lists have a ray kernel of their own.
 *
 * mcrt_camera_rays_device: the rays of every sample of the shard's packed pixels under the context's lens (none set: the perspective
 * camera's), sample-major: record i * pixels + q for sample i of packed pixel q, pixels = owned rows * width, n = pixels * sqrtspp^2
 * records, d_start and d_direction [n][3] in DEVICE memory. One launch; stats: paths = rays = n, kernel_ms, kernel_launches 1. More
 * than 0xFFF00000 records (what one closest-hit search takes) are refused (MCRT_ERR_UNSUPPORTED). The arrays are what
 * mcrt_intersect_device reads. mcrt_camera_rays: the same with HOST pointers.
 * Not done: lenses inside the render kernels (mcrt_render, variance and half-buffers, highlights, adaptive and converged rendering),
 * stereo or omnidirectional-stereo cameras, a thin lens on the new models, photon-mapped frames, an inverse mapping from world point to
 * pixel. (Caller-supplied ray arrays: "Ray sources" below, a state of its own beside the lens.) */
enum { MCRT_LENS_NONE = 0, MCRT_LENS_PERSPECTIVE = 1, MCRT_LENS_ORTHOGRAPHIC = 2, MCRT_LENS_EQUIRECTANGULAR = 3, MCRT_LENS_FISHEYE = 4 };
typedef struct mcrt_lens_desc {
    uint32_t model, flags;      /* flags: 0 */
    double   width_world;       /* ORTHOGRAPHIC: world-space width of the frame, > 0 */
    double   fov_x, fov_y;      /* radians; EQUIRECTANGULAR: 0 = 2 pi / pi; FISHEYE: fov_x = full angle, 0 = pi */
    double   reserved[3];       /* 0 */
} mcrt_lens_desc;               /* 56 bytes */
int mcrt_set_lens(mcrt_ctx* ctx, const mcrt_lens_desc* lens /* NULL or model NONE: the camera's own */);
int mcrt_get_lens(mcrt_ctx* ctx, mcrt_lens_desc* out);
int mcrt_camera_rays_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, double* d_start, double* d_direction,
                            mcrt_stats* stats /* may be NULL */);
int mcrt_camera_rays(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, double* start, double* direction,
                     mcrt_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Ray sources: caller-supplied rays and surface gathers for the passes that trace camera rays. With a source set on the context the
 * first ray of every pixel sample comes from the caller's arrays instead of a camera: "what is the light along these rays" (a lens
 * computed by the caller, rays shot again from the positions of an AOV frame) and "what light arrives at these surface points"
 * (lightmap and vertex baking, irradiance probes - with the light groups per lamp). A source is a state of its own beside the lens;
 * the two exclude each other. Under a source the camera of a call gives the frame's shape (width, height, sqrtspp, shard) and the
 * sampler key of a pixel, y * width + x, and nothing else: eye, forward, left, up and the thin lens are not read, a thin-lens camera
 * is accepted.
 *
 * `pixels` is the number of packed pixels the arrays were made for: owned rows * width of the camera's shard (mcrt_shard_rows).
 * Packed pixel q is local row q / width, column q % width. Every call that uses the source checks `pixels` against its camera, and
 * `spp` against sqrtspp^2 where the source reads it; a mismatch is MCRT_ERR_INVALID with a message that names both numbers.
 * `first` and `second` are DEVICE pointers, the caller's: they must stay valid until the source is replaced or taken off, must not
 * alias an output of a pass that runs under the source, nor the output of mcrt_camera_rays_device while set.
 *
 *   MCRT_RAY_SOURCE_RAYS     first = start, second = direction, [spp][pixels][3] doubles each: record i * pixels + q is sample i of
 *                            packed pixel q - what mcrt_camera_rays_device writes and mcrt_intersect_device reads. With flag
 *                            MCRT_RAY_SOURCE_PER_PIXEL the arrays are [pixels][3], every sample of pixel q takes record q, and spp
 *                            is not read. The ray is makeRay(start, direction, scene_ior) with the six words' BITS copied: nothing
 *                            is normalised, a -0 stays -0; a unit direction is the caller's duty. A record is usable when all six
 *                            words are finite (v >= -DBL_MAX && v <= DBL_MAX) and the direction is not all zero (+0 or -0); an
 *                            unusable record becomes start (0,0,0), direction (0,0,1): nothing non-finite reaches the closest-hit
 *                            search. offset is not read.
 *   MCRT_RAY_SOURCE_SURFACE  first = position, second = normal, [pixels][3] doubles each: the AOV pass's `position` and `normal` (or
 *                            `shading_normal`) frames as they lie in device memory, or a lightmap's texels. flags must be 0, spp is
 *                            not read. Per sample i of pixel (x, y), packed pixel q, in FP64, uncontracted:
 *                              sampler at initiate(global_seed, y * width + x), setIndex(i)
 *                              u0 = get(kDimPixel),  u1 = get(kDimPixel + 1)   (the film-position pair of the camera's own ray: the
 *                                                                               sampler consumption is the camera's)
 *                              P = position[q],  N = normal[q]
 *                              nn = (N.x * N.x + N.y * N.y) + N.z * N.z
 *                              Nn = nn > 0 && nn <= DBL_MAX ? N * (1 / sqrt(nn)) : (0, 0, 1)
 *                              P = (0, 0, 0) unless its three words are finite
 *                              direction = csFrom(orthonormalBasis(Nn), cosWeightedHemi(u0, u1))   (csrc/mcrt_math.hpp, mcrt_shade.hpp:
 *                                          the occlusion pass's construction; sincos is the restated glibc routine)
 *                              start = P + Nn * offset
 *                            offset must be finite and >= 0 (the binding's default is 1e-9, the project's kEpsilon). The mean over a
 *                            pixel's samples of the radiance along these rays, times pi, is the irradiance at P (the pdf of the
 *                            direction is cos / pi); the light groups give it per lamp.
 *
 * mcrt_set_ray_source validates the descriptor and copies it into the context, where it stays until the next call; NULL or kind
 * MCRT_RAY_SOURCE_NONE takes the source off, and every byte of every call is what it was. mcrt_get_ray_source returns the descriptor
 * as it was given (all zero with none set). mcrt_set_ray_source_host is the same with HOST pointers: the arrays are copied into device
 * memory the context owns and frees at the next set (either form) or at mcrt_destroy; *sanitised (may be NULL) receives the number
 * of records the kernel will replace - RAYS: the unusable ones; SURFACE: a position that is not finite or a normal whose nn is not in
 * (0, DBL_MAX]. mcrt_get_ray_source then returns the device pointers of the copy.
 * Refused with MCRT_ERR_INVALID and a message: an unknown kind, unknown flag bits, non-zero reserved words, a NULL array,
 * pixels == 0, spp == 0 where it is read, an offset that is not finite or below 0 (SURFACE), a lens set on the context (the message
 * names mcrt_set_lens; mcrt_set_lens with a model is likewise refused while a source is set, naming mcrt_set_ray_source), a render in
 * flight. While a source is set:
 *   - mcrt_render_aov*, _matte*, _occlusion*, _lighting*, _light_groups* and _path_classes* and mcrt_camera_rays* take their rays
 *     from it (mcrt_camera_rays_device then returns the rays as the passes trace them, sanitised);
 *   - every call that makes its camera rays inside a render kernel refuses with MCRT_ERR_UNSUPPORTED and a message that names
 *     mcrt_set_ray_source: mcrt_render*, mcrt_render_film_device, mcrt_render_multi and what is built on them (pixel statistics,
 *     highlights, converged rendering), and mcrt_render_adaptive*.
 * Not done: next-event estimation at P itself (a gather, not a path vertex: P's own material is never read), photon-mapped frames, a
 * source inside the render kernels, per-ray outputs (a pixel's samples are still averaged). */
enum { MCRT_RAY_SOURCE_NONE = 0, MCRT_RAY_SOURCE_RAYS = 1, MCRT_RAY_SOURCE_SURFACE = 2 };
#define MCRT_RAY_SOURCE_PER_PIXEL 1u /* flags, RAYS: the arrays are [pixels][3] */
typedef struct mcrt_ray_source_desc {
    uint32_t      kind, flags;
    uint64_t      pixels;          /* packed pixels the arrays were made for: owned rows * width */
    uint32_t      spp, reserved0;  /* RAYS without PER_PIXEL: the samples per pixel the arrays hold; reserved0: 0 */
    const double* first;           /* RAYS: start,     SURFACE: position */
    const double* second;          /* RAYS: direction, SURFACE: normal */
    double        offset;          /* SURFACE: start = P + Nn * offset, finite and >= 0 */
    uint64_t      reserved[2];     /* 0 */
} mcrt_ray_source_desc;            /* 64 bytes */
int mcrt_set_ray_source(mcrt_ctx* ctx, const mcrt_ray_source_desc* source /* NULL or kind NONE: none */);
int mcrt_set_ray_source_host(mcrt_ctx* ctx, const mcrt_ray_source_desc* source /* first, second: HOST pointers */,
                             uint64_t* sanitised /* may be NULL */);
int mcrt_get_ray_source(mcrt_ctx* ctx, mcrt_ray_source_desc* out);

/* ------------------------------------------------------------------------------------------
 * Light probes: spherical-harmonic radiance at points, split per lamp. A probe is the mean over a pixel's samples of the radiance
 * along the sample's first ray TIMES a function of that ray's direction - here the first (L+1)^2 real spherical harmonics, L <= 2,
 * from which the irradiance for any normal follows in closed form. Split by light group it is relightable: dimming a lamp is a
 * weighted sum of coefficient sets. The walk is mcrt_render_light_groups' own - the same state, the same begin / ray / step
 * launches, the same R_p per sample and plane ("Light groups" above) -; what differs is the resolve, a projection in place of the
 * plain mean, and, with `positions`, where the first ray comes from.
 * As under a ray source the camera gives the frame's shape and the sampler keys: width * height is the number of probes,
 * sqrtspp^2 the rays per probe (spp), shard_* is honoured, `pixels` below is the shard's packed pixels (owned rows * width),
 * packed pixel q is local row q / width, column q % width.
 * The first rays. positions == NULL: whatever the context holds - the camera, a lens (mcrt_set_lens) or a ray source
 * (mcrt_set_ray_source). With positions, DEVICE [pixels][3] doubles, the probe rays: sample i of pixel (x, y), packed pixel q, in
 * FP64, uncontracted, consuming the sampler as MCRT_RAY_SOURCE_SURFACE does:
 *     sampler at initiate(global_seed, y * width + x), setIndex(i)
 *     u0 = get(kDimPixel),  u1 = get(kDimPixel + 1)
 *     z  = 1.0 - (u0 + u0)
 *     rr = 1.0 - z * z;  r = sqrt(rr > 0.0 ? rr : 0.0)
 *     (s, c) = refSinCos(u1 * kTwoPi)             (the restated glibc routine)
 *     direction = (r * c, r * s, z)               (uniform over the sphere: pdf 1 / (4 pi))
 *     start = positions[q], or (0, 0, 0) unless its three words are finite
 *     ray = makeRay(start, direction, scene_ior)
 * mcrt_probe_rays_device writes exactly these rays into d_start and d_direction, [spp][pixels][3] doubles each, sample-major
 * (record i * pixels + q), as mcrt_camera_rays_device does for a lens; fed back as a MCRT_RAY_SOURCE_RAYS source they give the
 * bytes of the call with positions. A lens or a source on the context is refused by both (positions would be ambiguous).
 * The projection. d = the direction of the sample's first ray as it was handed to the closest-hit search: the bits in the record,
 * whatever made them. w = weight[i * pixels + q] when weight, DEVICE [spp][pixels] doubles, is given: for callers whose rays are
 * not uniformly distributed (1 / pdf, up to a constant). The un-normalised basis:
 *     b0 = 1
 *     b1 = d.y            b2 = d.z                      b3 = d.x
 *     b4 = d.x * d.y      b5 = d.y * d.z
 *     b6 = 3.0 * (d.z * d.z) - 1.0
 *     b7 = d.x * d.z      b8 = (d.x * d.x) - (d.y * d.y)
 * Every word of the output - plane p, coefficient k, pixel, channel c - is (((0.0 + t(0)) + t(1)) + ...) / (double)spp, ascending
 * i, one FP64 accumulator per word, with t(i) = R_p(i).c * b_k without a weight and t(i) = (R_p(i).c * w) * b_k with one (k = 0
 * may skip the multiplication by 1: the bits are the same). Nothing is clamped: coefficients are signed.
 * Normalisation is the caller's, not the kernel's. With uniform directions the mean of L * b_k estimates (1 / 4 pi) * integral of
 * L b_k, so the coefficient of the real spherical harmonic Y_k = N_k b_k is L_k = 4 pi N_k * (output word), with the constants
 * MCRT_PROBE_SH_N* below; the irradiance at normal n is then sum_k A_l(k) L_k Y_k(n), A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4
 * (the binding's probe_sh and probe_irradiance).
 * Parameters: groups as in mcrt_render_light_groups (all zero: one group and the sky); order L = 0, 1, 2 gives K = (L + 1)^2
 * coefficients (mcrt_probe_coefficients); flags and reserved 0.
 * Output: d_coefficients, [P][K][rows][width][3] doubles, P = mcrt_light_group_planes(&groups), the rows this shard owns packed.
 * What holds, bit for bit:
 *   - coefficient 0 of every plane, with no weight, is the plane mcrt_render_light_groups returns under the same lens or source;
 *   - a weight of all 1.0 changes nothing, a weight of all 2.0 doubles every word;
 *   - positions gives the bytes of the same call with positions == NULL under a RAYS source fed with mcrt_probe_rays_device's arrays;
 *   - a coefficient does not depend on chunking (MCRT_AOV_CHUNK_RAYS), sharding, order (the nine of order 2 begin with the four
 *     of order 1) or how the OTHER emitters are grouped.
 * Refused with MCRT_ERR_INVALID and a message: params or the output NULL, order > 2, flags or reserved non-zero, everything the
 * light groups refuse, positions together with a lens or a ray source on the context (the message names mcrt_set_lens /
 * mcrt_set_ray_source).
 * stats: as the light groups'.
 * Not done: probes of the path classes, order 3 and up, non-uniform built-in direction sets (a caller's own through a RAYS source
 * and weight), any normalisation or irradiance on the device. */
#define MCRT_PROBE_ORDER_MAX 2u
#define MCRT_PROBE_SH_N0 0.28209479177387814 /* 1/2 sqrt(1/pi):  k = 0 */
#define MCRT_PROBE_SH_N1 0.4886025119029199  /* 1/2 sqrt(3/pi):  k = 1, 2, 3 */
#define MCRT_PROBE_SH_N4 1.0925484305920792  /* 1/2 sqrt(15/pi): k = 4, 5, 7 */
#define MCRT_PROBE_SH_N6 0.31539156525252005 /* 1/4 sqrt(5/pi):  k = 6 */
#define MCRT_PROBE_SH_N8 0.5462742152960396  /* 1/4 sqrt(15/pi): k = 8 */
typedef struct mcrt_probe_params {
    mcrt_light_group_params groups; /* as in mcrt_render_light_groups */
    uint32_t      order;            /* L = 0, 1, 2: K = (L + 1)^2 coefficients */
    uint32_t      flags;            /* 0 */
    const double* positions;        /* DEVICE [pixels][3] or NULL: the context's camera, lens or ray source */
    const double* weight;           /* DEVICE [spp][pixels] or NULL */
    uint64_t      reserved[2];      /* 0 */
} mcrt_probe_params;                /* 64 bytes */
/* K of an order; 0 when it is out of range. */
uint32_t mcrt_probe_coefficients(uint32_t order);
int mcrt_render_probes_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_probe_params* params,
                              double* d_coefficients, mcrt_stats* stats /* may be NULL */);
/* Same with HOST pointers: positions [pixels][3] and weight [spp][pixels] of the shard's packed pixels, coefficients P * K FULL frames,
 * [P][K][height][width][3]: rows this shard does not own are left untouched. */
int mcrt_render_probes(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_probe_params* params,
                       double* coefficients, mcrt_stats* stats /* may be NULL */);
/* The probe rays of d_positions (DEVICE [pixels][3]) into d_start and d_direction, DEVICE [spp][pixels][3] each. */
int mcrt_probe_rays_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const double* d_positions, double* d_start,
                           double* d_direction, mcrt_stats* stats /* may be NULL */);

/* Photon emission pass on the GPU. Replaces the thread fan-out of
 * PhotonMapper::PhotonMapper (integrator/photon-mapper/photon-mapper.cpp:80-115: per emission
 * Sampler::initiate(light), setIndex(offset+i), light point + cosine direction, emitPhoton :225-277) for
 * the uploaded scene. `emissions` and `caustic_factor` are the "photon_map" JSON values (:31-38); the
 * split of emissions over lights follows :43-78. The photons come back as two unordered lists in the
 * reference's 32-byte Photon layout (photon.hpp:36-37) — the host then builds its octrees from them
 * exactly as it does from the per-thread vectors (:190-207) and calls mcrt_upload_photons.
 * keys (optional diagnostics) identify a photon: light << 48 | emission index << 16 | bounce.
 * The arrays belong to the context and stay valid until the next mcrt_emit_photons / mcrt_destroy. */
typedef struct mcrt_photon_emission {
    uint64_t global_count, caustic_count;
    const float* global_photons;    /* [global_count][8]  flux rgb, position xyz, phi, theta */
    const float* caustic_photons;   /* [caustic_count][8]                                   */
    const uint64_t* global_keys;    /* [global_count]  */
    const uint64_t* caustic_keys;   /* [caustic_count] */
    uint64_t emission_paths;        /* photon paths traced = emissions * caustic_factor, split per light */
    uint64_t rays;                  /* Scene::intersect calls */
    double kernel_ms;
} mcrt_photon_emission;
int mcrt_emit_photons(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed,
                      mcrt_photon_emission* out);
/* Same, restricted to one shard of the photon paths (multi-GPU emission): the paths
 * are numbered 0..emission_paths-1 in (light, emission index) order and shard k of n takes the k-th
 * contiguous block, so the union of the n lists is exactly the unsharded result; the ranks then
 * all-gather their lists (RCCL) and every rank builds/uploads the full maps. */
int mcrt_emit_photons_shard(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed,
                            uint32_t shard_index, uint32_t shard_count, mcrt_photon_emission* out);

/* ---- The photon pass without host round trips (SURVEY.md §8(f) ranks 1 + 2; replaces PhotonMapper::PhotonMapper,
 * integrator/photon-mapper/photon-mapper.cpp:31-203, as a whole): the emission pass, then both maps built where the
 * photons are — cell codes, radix sort, gather, the octants level by level from the sorted codes, depth-first numbering,
 * leaf boxes merged upwards, the search's record lists — and installed as mcrt_upload_photons installs them. Same photons
 * as mcrt_emit_photons, same octants / boxes / photons per leaf as mcrt_photon_map_build (Octree<Photon>::insert,
 * octree/octree.cpp:35-80 + LinearOctree, octree/linear-octree.cpp:202-244) with root cell [bb_min, bb_max] = Scene::BB().
 * Only counters cross PCIe. MCRT_ERR_UNSUPPORTED when more than max_photons_per_leaf photons share one 2^-21 cell (the
 * recursive host builder's case). */
typedef struct mcrt_photon_pass_stats {
    uint64_t global_count, caustic_count;   /* photons stored */
    uint64_t global_octants, caustic_octants;
    uint64_t emission_paths, rays;
    double emission_ms;                     /* emission kernel (HIP events) */
    double sort_ms, octant_ms, finish_ms;   /* both maps: codes + sort + gather / octants + numbering / boxes + record lists (host clock) */
    double total_ms;                        /* whole call (host clock) */
} mcrt_photon_pass_stats;
int mcrt_photon_pass_device(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed, const double bb_min[3],
                            const double bb_max[3], uint32_t max_photons_per_leaf, uint32_t k_nearest_photons,
                            int direct_visualization, mcrt_photon_pass_stats* stats);
/* The same pass for the contexts of ONE host process (the reference's shape: one executable, PhotonMapper::PhotonMapper
 * fanning its emission work out to worker threads, integrator/photon-mapper/photon-mapper.cpp:40-115), sharded: context i traces
 * shard i of `count` of the emission paths, the lists cross between the GPUs on device pointers (hipMemcpyPeer: xGMI between
 * two devices), every context builds both maps from the same concatenation in shard order - the same maps everywhere, the
 * emission's time divided by `count`. ctxs[i] holds the scene already; count == 1 is mcrt_photon_pass_device.
 * stats: one record PER CONTEXT ([count]; may be NULL): emission_paths / rays / emission_ms of its own shard, the maps' counts. */
int mcrt_photon_pass_multi(mcrt_ctx* const* ctxs, uint32_t count, double emissions, double caustic_factor, uint32_t global_seed,
                           const double bb_min[3], const double bb_max[3], uint32_t max_photons_per_leaf, uint32_t k_nearest_photons,
                           int direct_visualization, mcrt_photon_pass_stats* stats);
/* The emission pass alone with the lists left in device memory (owned by the context, valid until the next emission): for
 * hosts that exchange the lists between GPUs (RCCL all-gather on the device pointers) before building the maps. */
typedef struct mcrt_photon_emission_device {
    uint64_t global_count, caustic_count;
    const float* d_global_photons;    /* DEVICE [global_count][8]  */
    const float* d_caustic_photons;   /* DEVICE [caustic_count][8] */
    uint64_t emission_paths, rays;
    double kernel_ms;
} mcrt_photon_emission_device;
int mcrt_emit_photons_device(mcrt_ctx* ctx, double emissions, double caustic_factor, uint32_t global_seed, uint32_t shard_index,
                             uint32_t shard_count, mcrt_photon_emission_device* out);
/* Both maps from photon lists in device memory (not modified), installed like mcrt_upload_photons.
 * STREAM CONTRACT for every device-pointer INPUT of this header (these lists; mcrt_film_resolve_device's blob): the library reads them
 * on the context's own non-blocking stream, which is not ordered after any stream of the caller - the data must be COMPLETE
 * (producing stream synchronised, e.g. hipStreamSynchronize / torch.cuda.synchronize) when the call is made. Device OUTPUTS
 * (mcrt_render_device's d_out) are written on the stream the caller passes and are ordered like any work on that stream. */
int mcrt_upload_photons_device(mcrt_ctx* ctx, const float* d_global_photons, uint64_t global_count, const float* d_caustic_photons,
                               uint64_t caustic_count, const double bb_min[3], const double bb_max[3], uint32_t max_photons_per_leaf,
                               uint32_t k_nearest_photons, int direct_visualization, mcrt_photon_pass_stats* stats);
/* Copy of an installed map (0 global, 1 caustic) as a host object — octants, boxes, photons — for inspection and tests. */
int mcrt_photon_map_download(mcrt_ctx* ctx, int which, struct mcrt_photon_map** out);

/* ---- operator-level entry points (each mirrors one reference function; used by parity tests
 * and by hosts that only want the traversal / kNN engine) -------------------------------- */

/* Scene::intersect (scene/scene.cpp:151-176) for n rays given as start[3], direction[3] (FP64,
 * host). Outputs: t (DBL_MAX when no hit, ray/intersection.hpp:14), surface index (0xFFFFFFFF when
 * no hit), uv[2] (meaningful when the surface interpolates normals). */
int mcrt_intersect(mcrt_ctx* ctx, uint64_t n, const double* start, const double* direction,
                   double* out_t, uint32_t* out_surface, double* out_uv);
/* The same query on DEVICE arrays (the form for hosts that only want the traversal engine and keep their rays on the GPU: nothing
 * crosses PCIe): d_start[n][3], d_direction[n][3] in, d_t[n], d_surface[n], d_uv[n][2] (may be NULL) out, same values as
 * mcrt_intersect. Inputs follow the STREAM CONTRACT above (complete when the call is made); the call is synchronous on the
 * context's stream. */
int mcrt_intersect_device(mcrt_ctx* ctx, uint64_t n, const double* d_start, const double* d_direction, double* d_t,
                          uint32_t* d_surface, double* d_uv /* may be NULL */);

/* Sampler (sampling/sampler.hpp:13-90): for each (pixel[i], index[i]) runs initiate(pixel),
 * setIndex(index), then `shuffles` times shuffle(); writes get<0,7>() after the last step
 * (shuffles == 0 gives the un-shuffled camera dimensions). out[n][7]. */
int mcrt_sampler(mcrt_ctx* ctx, uint64_t n, const uint32_t* pixel, const uint32_t* index,
                 uint32_t shuffles, uint32_t global_seed, double* out);

/* The lobe functions Interaction::BSDF is made of (ray/interaction.cpp:84-153), on n local-frame vectors (host arrays):
 * in[n][11] = wi[3], wo[3], n1, n2, alpha, u, v (wi is folded into the upper hemisphere as |z| + 1e-3, renormalised, for the
 * reflection lobes and negated for transmission); consts[10] = roughness, reflectance[3] of an Oren-Nayar material and a
 * complex IOR real[3], imaginary[3]. The material is rough as Material::computeProperties decides it (material/material.cpp:99):
 * roughness > C::EPSILON (1e-9) gives Oren-Nayar, anything else (0, 1e-160, a NaN) the Lambertian reflectance / pi. out[n][18] = Fresnel::dielectric(n1, n2, wo.z) (material/fresnel.cpp:16-27) ·
 * Fresnel::conductor rgb (:30-49) · GGX::reflection f, pdf (material/ggx.cpp:46-52) · GGX::transmission f, pdf (:54-65) ·
 * GGX::visibleMicrofacet(u, v, wo) xyz (:67-88) · GGX::D(m) (:21-24) · GGX::Lambda(wo) (:31-34) ·
 * Material::diffuseReflection rgb, pdf (material/material.cpp:17-27,82-95) · 0. No scene needed. */
int mcrt_bsdf(mcrt_ctx* ctx, uint64_t n, const double* in, const double* consts, double* out);

/* The libm calls of the path as the DEVICE computes them (csrc/mcrt_libm.hpp: glibc 2.35's algorithms restated so that the GPU returns
 * the bits the reference's std::sin / std::cos pairs (= sincos: sampling/sampling.hpp:29-44, material/ggx.cpp:77-79, surface/sphere.cpp:43),
 * std::sin alone (camera/filter.hpp:64), std::asin (scene/scene.cpp:221) and std::atan2 (integrator/photon-mapper/photon.hpp:10-11)
 * return on an x86-64 host with FMA; SINCOSF: sincosf, the sine / cosine pairs of Photon::dir's two float angles, photon.hpp:19-27 - a[n]
 * holds float values, out0 / out1 the float results widened). fn selects the function; a[n] (and b[n] for atan2: a = y, b = x, and for pow: a^b) are the
 * arguments, out0[n] (and out1[n] for sincos / sincosf: out0 = sine, out1 = cosine) the results. Known-answer tests only; no scene needed. */
enum { MCRT_LIBM_SINCOS = 0, MCRT_LIBM_SIN = 1, MCRT_LIBM_COS = 2, MCRT_LIBM_ASIN = 3, MCRT_LIBM_ATAN2 = 4, MCRT_LIBM_SINCOSF = 5,
       MCRT_LIBM_POW = 6 /* std::pow(a, b): sRGB::gammaCompress, color/srgb.hpp:54-62 - the one libm call of Image::save (csrc/mcrt_libm_pow.hpp) */ };
int mcrt_libm(mcrt_ctx* ctx, int fn, uint64_t n, const double* a, const double* b, double* out0, double* out1);

/* LinearOctree<Photon>::knnSearch (octree/linear-octree.cpp:25-117) on the uploaded map
 * (which = 0 global, 1 caustic) for n query points p[n][3]. Outputs per query: count found
 * (≤ k), photon indices and squared distances sorted by ascending distance (ties by index),
 * each [n][k]; unused slots get 0xFFFFFFFF / +inf. When more photons share the k-th distance than the answer has room for, the
 * DISTANCES are still guaranteed - the k smallest of the map, bit for bit - and so is that the indices of a query are distinct, each a
 * photon at exactly the distance reported with it, equal distances in ascending index order; WHICH of the photons tied at the k-th
 * distance are returned is not: the reference keeps them by insertion order (linear-octree.cpp:58-77), the searches here by the order of
 * their candidate buffers, and the forms of this call (wave-cooperative, four queries per wave, per lane) differ among themselves. Any k: k <= 768 is served by the wave-cooperative search,
 * larger k by the per-lane search. The search's frontier is unbounded like the reference's priority queue
 * (linear-octree.cpp:33): a wave-cooperative search that fills its 128 + 1 024 entries is repeated by the per-lane
 * search, whose frontier grows on demand (the same holds for photon-mapped frames: mcrt_render_finish). */
int mcrt_knn(mcrt_ctx* ctx, int which, uint64_t n, const double* p, uint32_t k,
             uint32_t* out_count, uint32_t* out_index, double* out_distance2);

/* ------------------------------------------------------------------------------------------
 * Scene-image files (*.mcrt): a flat dump of the three descriptors above, written by the
 * flattener that runs inside the reference host and read by stand-alone hosts.
 * Host-only helpers; they never touch the GPU.
 * ---------------------------------------------------------------------------------------- */
typedef struct mcrt_image mcrt_image; /* opaque; owns the host arrays the descs point into */

int  mcrt_image_load(const char* path, mcrt_image** out);
void mcrt_image_free(mcrt_image* img);
const mcrt_scene_desc*      mcrt_image_scene(const mcrt_image* img);
const mcrt_camera_desc*     mcrt_image_camera(const mcrt_image* img);
const mcrt_photon_map_desc* mcrt_image_photons(const mcrt_image* img, int which /*0 global,1 caustic*/);
/* key = "k_nearest_photons" | "direct_visualization" | "global_seed" | "photon_mapping"; 0 if absent */
uint64_t mcrt_image_param(const mcrt_image* img, const char* key);
int mcrt_image_save(const char* path, const mcrt_scene_desc* scene, const mcrt_camera_desc* cam,
                    const mcrt_photon_map_desc* global_map, const mcrt_photon_map_desc* caustic_map,
                    const char* const* param_keys, const uint64_t* param_values, uint32_t num_params);

/* Host-side photon-map builder: photon list (e.g. from mcrt_emit_photons) -> linear octree with the
 * semantics of Octree<Photon>::insert + LinearOctree<Photon> (octree/octree.cpp:35-80,
 * octree/linear-octree.cpp:202-244): root cell = Scene::BB(), a cell with more than
 * max_photons_per_leaf photons is split into its 8 octants, empty octants are dropped, node boxes are
 * tight. For hosts that do not carry the reference's builder; never touches the GPU. */
typedef struct mcrt_photon_map mcrt_photon_map; /* opaque; owns the arrays its descriptor points into */
int  mcrt_photon_map_build(const float* photons, uint64_t num_photons, const double bb_min[3], const double bb_max[3],
                           uint32_t max_photons_per_leaf, mcrt_photon_map** out);
/* The same tree (same octants, boxes and photons per leaf; photons of a leaf in cell-code order instead of input
 * order) built with the GPU of `ctx`: per-photon octant path codes, radix sort, gather and leaf boxes on the device,
 * octant assembly from the sorted codes on the host (replaces the serial insert loop of
 * PhotonMapper::PhotonMapper, photon-mapper.cpp:169-203, and LinearOctree's compaction, linear-octree.cpp:202-244).
 * Falls back to mcrt_photon_map_build when more than max_photons_per_leaf photons share one 2^-21 cell. */
int  mcrt_photon_map_build_gpu(mcrt_ctx* ctx, const float* photons, uint64_t num_photons, const double bb_min[3],
                               const double bb_max[3], uint32_t max_photons_per_leaf, mcrt_photon_map** out);
const mcrt_photon_map_desc* mcrt_photon_map_get(const mcrt_photon_map* map);
void mcrt_photon_map_free(mcrt_photon_map* map);

/* ------------------------------------------------------------------------------------------
 * BVH builder for hosts that do not carry the reference's: the reference's DEFAULT hierarchy ("bvh": {"type":
 * "octree"}, bvh/bvh.cpp:41-56,130-163,428-449) — an octree over the surfaces' box centroids, leaves of at most 8
 * surfaces, one node per non-empty octant with the union of its surfaces' boxes — built by sorting per-surface octant
 * path codes instead of inserting one surface at a time. The result is the reference's tree
 * bit for bit: same LinearNode arrays, same surface order (tests/test_bvh_build.py rebuilds every golden octree BVH,
 * up to the 6.9 M-triangle C5 scene; tests/test_bvh_awkward.py compares bytes, on centroids on octant mid-planes and on the
 * cube's far faces among others). A box coordinate that is zero has the reference's sign: that of the first surface, in input
 * order, of the first octant, in octant order, that attains it (BoundingBox::merge keeps the first). `scene` needs its surface arrays, quadrics, bb_min/bb_max; its node arrays are
 * ignored. ctx != NULL: boxes, codes and the radix sort run on the GPU of ctx; ctx == NULL: host only.
 * MCRT_ERR_UNSUPPORTED when more than 8 centroids share one 2^-21 cell of the root cube. */
typedef struct mcrt_bvh_desc {
    uint32_t num_nodes;
    const double*   node_bounds;        /* as mcrt_scene_desc */
    const uint32_t* node_start_surface;
    const uint32_t* node_num_surfaces;
    const uint32_t* node_next_sibling;
    uint32_t num_surfaces;
    const uint32_t* order;              /* [num_surfaces] BVH::ordered_surfaces: new position -> index in `scene` */
} mcrt_bvh_desc;
typedef struct mcrt_bvh mcrt_bvh;       /* opaque; owns the arrays its descriptor points into */
int  mcrt_bvh_build_octree(mcrt_ctx* ctx /* may be NULL */, const mcrt_scene_desc* scene, mcrt_bvh** out);
/* The reference's other two hierarchies, "binary_sah" (arity 2) and "quaternary_sah" (arity 4): its binned surface-area
 * builders (bvh/bvh.cpp:165-426) restated with the same arithmetic and tie rules — same tree — and run on `threads` host
 * threads (0 = all), one subtree per thread. bins_per_axis 0 = the reference's default (16 / 8). Host only.
 * The tree depends on the ORDER of the input surfaces where the reference's does: a node that cannot be split by position is
 * dealt round-robin (surface i of the node to part i % arity), and a box coordinate that is zero has the sign of the first
 * surface of the node, in input order, whose own box coordinate is zero (-0.0 and +0.0 are different bytes in node_bounds). */
int  mcrt_bvh_build_sah(const mcrt_scene_desc* scene, int arity, uint32_t bins_per_axis, uint32_t threads, mcrt_bvh** out);
/* The same two hierarchies built LEVEL BY LEVEL — all open nodes of a depth at once: centroid bounds, binning and the
 * order-preserving partition are passes over the surfaces on the GPU of ctx (atomics on exact minima / maxima / counts, one
 * prefix sum per level), the split of every open node is decided by one thread with the reference's cost loop, the host
 * only strings the nodes together (csrc/mcrt_sah_shared.hpp, mcrt_sah_gpu.hip). Same tree as mcrt_bvh_build_sah and the
 * reference, bit for bit - the signs of zero box coordinates included, which the atomic reductions do not give and a host
 * step over the zero coordinates alone restores. ctx == NULL runs the same level loop on the host (one thread). More than
 * 16 bins per axis: built by mcrt_bvh_build_sah on all host threads, same tree. */
int  mcrt_bvh_build_sah_gpu(mcrt_ctx* ctx /* may be NULL */, const mcrt_scene_desc* scene, int arity, uint32_t bins_per_axis, mcrt_bvh** out);
const mcrt_bvh_desc* mcrt_bvh_get(const mcrt_bvh* bvh);
void mcrt_bvh_free(mcrt_bvh* bvh);
/* `scene` with its surfaces put in bvh->order, its lights re-indexed and the node arrays of `bvh`: an owning copy whose
 * descriptor can go to mcrt_upload_scene / mcrt_image_save. */
typedef struct mcrt_scene mcrt_scene;
int  mcrt_scene_with_bvh(const mcrt_scene_desc* scene, const mcrt_bvh_desc* bvh, mcrt_scene** out);
const mcrt_scene_desc* mcrt_scene_get(const mcrt_scene* scene);
void mcrt_scene_free(mcrt_scene* scene);

/* ------------------------------------------------------------------------------------------
 * Image::save on the GPU (camera/image.cpp:37-88; SURVEY.md §8(f) rank 4, "tonemap/exposure"): what the reference does with
 * the frame after Camera::sampleImage — auto exposure from the median of a 65 536-bin brightness histogram (getExposure
 * :62-72, common/histogram.cpp:6-41), auto gain from the 99th percentile of the tone-mapped brightness (getGain :77-87),
 * the tone map (camera/pixel-operators.cpp:7-44), sRGB gamma (color/srgb.hpp:55-63) and truncation to bytes in B,G,R
 * order (pixel-operators.cpp:51-55) — as five kernels on the frame where mcrt_render_device left it, so that 3 bytes per
 * pixel cross PCIe instead of 24. Every step but pow() is IEEE-exact and in the reference's order; a byte can differ from
 * the reference's only where pow's last bit moves a value across an integer (tests allow 1 step on < 1e-4 of the bytes).
 * The fields are the scene file's camera "image" object (image.cpp:10-35). */
enum { MCRT_TONEMAP_HABLE = 0, MCRT_TONEMAP_ACES = 1 };
typedef struct mcrt_image_desc {
    uint32_t width, height;          /* of the buffer handed in (the full frame: exposure is a whole-image statistic) */
    uint32_t tonemapper;             /* MCRT_TONEMAP_*; "tonemapper" (default Hable)                                  */
    uint32_t plain;                  /* "plain": no tone map, exposure and gain 1                                      */
    double exposure_compensation;    /* EV: exposure = 0.5 / median * 2^EV                                             */
    double gain_compensation;        /* EV                                                                             */
} mcrt_image_desc;
/* d_rgb: width*height*3 doubles in device memory; d_bgr: width*height*3 bytes in device memory (rows top to bottom, the
 * TGA payload). factors (host, may be NULL) receives {exposure_factor, gain_factor}. Synchronous on `stream`. */
int mcrt_tonemap_device(mcrt_ctx* ctx, const double* d_rgb, const mcrt_image_desc* image, uint8_t* d_bgr, double* factors,
                        void* stream);
/* Same from/to host memory (copies in, runs the kernels, copies the bytes out). */
int mcrt_tonemap(mcrt_ctx* ctx, const double* rgb, const mcrt_image_desc* image, uint8_t* bgr, double* factors);
/* HeaderTGA + payload (camera/image.hpp:39-50, image.cpp:42-51): uncompressed 24 bpp, top-left origin. Host only. */
int mcrt_tga_save(const char* path, uint32_t width, uint32_t height, const uint8_t* bgr);

uint32_t mcrt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MCRT_H */
