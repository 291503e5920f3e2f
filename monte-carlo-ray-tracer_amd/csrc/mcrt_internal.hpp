// Internal links between the translation units of libmcrt_hip.so (not part of the C ABI).
#pragma once

#include <string>

#include "../../include/mcrt.h"

struct mcrt_bvh;

namespace mcrt {
int ctxDevice(const mcrt_ctx* ctx);
void* ctxStream(const mcrt_ctx* ctx);  // the context's hipStream_t
int ctxFail(mcrt_ctx* ctx, int code, const std::string& msg);  // records the message for mcrt_last_error, returns code
// Run-time options of a context (mcrt_set_option; the MCRT_* environment variables only seed them at mcrt_create).
const char* ctxOpt(const mcrt_ctx* ctx, const char* key);       // value or nullptr when unset
long ctxOptL(const mcrt_ctx* ctx, const char* key, long dflt);  // integer value or dflt
bool ctxOptOn(const mcrt_ctx* ctx, const char* key);            // set and not 0
// mcrt_octree_gpu.hip: the octree BVH of `scene` with the per-surface work on the GPU of ctx (mcrt_bvh_shared.hpp)
int bvhOctreeGpu(mcrt_ctx* ctx, const mcrt_scene_desc* scene, struct ::mcrt_bvh* out);
// mcrt_sah_gpu.hip: the binned-SAH hierarchies level by level with the per-surface passes on the GPU of ctx (mcrt_sah_shared.hpp)
int bvhSahGpu(mcrt_ctx* ctx, const mcrt_scene_desc* scene, int arity, int bins, struct ::mcrt_bvh* out);
// mcrt_output.hip: refPow (mcrt_libm_pow.hpp, the output stage's one libm call) on device arrays, launched on `stream`: out[i] =
// pow(a[i], b[i]). The known-answer kernel behind mcrt_libm's MCRT_LIBM_POW; returns the hipError_t of the launch as an int.
int launchPowKat(void* stream, uint64_t n, const double* a, const double* b, double* out);
// mcrt_hip.hip: Scene::intersect on n rays in DEVICE arrays - the body of mcrt_intersect behind its uploads (trees in memory: the trace
// kernel fed from the arrays, otherwise the intersect kernel). d_uv must not be null. Synchronous on the context's stream.
int intersectDeviceArrays(mcrt_ctx* ctx, uint64_t n, const double* d_start, const double* d_dir, double* d_t, uint32_t* d_surf, double* d_uv);
// The hooks of the image passes' host toolkit (mcrt_pass_host.hpp, mcrt_camera_pass.hpp; DESIGN.md "Image passes"), which every
// mcrt_*_host.hip reaches the context through - one PassFamily below each, but the OpenEXR output and input, which share kPassExr.
// ctxIdle: no render in flight (MCRT_ERR_INVALID recorded under `what`), device selected. ctxNeedScene: MCRT_ERR_NO_SCENE under `what`.
// ctxPassScratch: buffer `which` (0..kPassSlots-1) of a family's scratch - every (family, slot) a buffer of its own, kept in the context
// and grown on demand like the operators'; at least 8 bytes; nullptr, the HIP error cleared, when the allocation fails.
// ctxAovScene: the uploaded scene's arrays in device memory. ctxSceneCounts: its numbers of surfaces and materials.
// ctxSampleTargetsBegin: ctxIdle, ctxNeedScene, MCRT_ERR_INVALID for no camera, MCRT_ERR_UNSUPPORTED for a camera whose film splats when
// a channel is wanted - then the channels of `targets` other than rgb (mcrt_summary_channels.hpp; nullptr: not wanted) are what the pass
// loops of the next renders of this context fill (their epilogue's launches), until ctxSampleTargetsEnd clears them (SampleTargetsScope does).
struct AovScene;
enum PassFamily { kPassAov, kPassDenoise, kPassPixelStats, kPassRobust, kPassDenoiseVar, kPassAccumulate, kPassDenoiseDual, kPassExr, kPassMatte, kPassCompare, kPassOcclusion, kPassLighting, kPassLightGroups, kPassPathClasses, kPassAdaptive, kPassProbes, kPassFamilies };
constexpr int kPassSlots = 6;
int ctxIdle(mcrt_ctx* ctx, const char* what);
int ctxNeedScene(mcrt_ctx* ctx, const char* what);
void* ctxPassScratch(mcrt_ctx* ctx, PassFamily family, int which, size_t bytes);
void ctxAovScene(const mcrt_ctx* ctx, AovScene* out, const uint32_t** sobol_tab);
void ctxSceneCounts(const mcrt_ctx* ctx, uint32_t* num_surfaces, uint32_t* num_materials);
int ctxSampleTargetsBegin(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_frame_summary* targets, const char* what);
void ctxSampleTargetsEnd(mcrt_ctx* ctx);
// The context's lens ("Camera models" in mcrt.h; mcrt_lens_host.hip validates and writes it): nullptr while none is set - then the
// camera-ray passes run their own ray kernels and the render calls are not guarded.
const mcrt_lens_desc* ctxLens(const mcrt_ctx* ctx);
void ctxSetLens(mcrt_ctx* ctx, const mcrt_lens_desc& lens);  // model MCRT_LENS_NONE: none
// The context's ray source ("Ray sources" in mcrt.h; mcrt_ray_source_host.hip validates and writes it): nullptr while none is set.
// ctxSetRaySource frees the device copies the context owned and adopts owned_first / owned_second (hipMalloc'ed, or nullptr: the
// arrays are the caller's); kind MCRT_RAY_SOURCE_NONE: none.
const mcrt_ray_source_desc* ctxRaySource(const mcrt_ctx* ctx);
void ctxSetRaySource(mcrt_ctx* ctx, const mcrt_ray_source_desc& source, void* owned_first, void* owned_second);
}  // namespace mcrt
