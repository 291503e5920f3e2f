// The four launches of the light groups: defined in csrc/mcrt_light_groups.hip (libmcrt_light_groups.so, the pass's own code object),
// called by csrc/mcrt_light_groups_host.hip (libmcrt_hip.so). All queue one kernel on `stream` (a hipStream_t) and return the launch's
// hipError_t as an int.
#pragma once

#include "mcrt_film_gather.hpp"
#include "mcrt_light_groups.hpp"
#include "mcrt_probes.hpp"

namespace mcrt {

// pathBegin for the chunk's n samples (their camera rays and hits are in st.ray) and the first live list - the samples that hit -,
// counted in counters->live[0], which the caller has set to zero.
int launchLightGroupsBegin(void* stream, const LgState& st, uint64_t n, double scene_ior, const LgParams& par, uint32_t* list, LgCounters* counters);
// lit: start and direction of the 2 * n_live shadow and bounce rays of iteration k are written; counters->live[next] is set to zero for
// the step kernel of the same iteration.
int launchLightGroupsRays(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const LgState& st, const uint32_t* list, uint32_t n_live,
                          uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next);
// lit: those rays with their closest hits (not read when `last`). The survivors go to next_list, counted in counters->live[next], which
// is zero when the kernel starts (the ray kernel of the iteration set it; `last` has no ray kernel: the caller did).
int launchLightGroupsStep(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const LgState& st, const LgParams& par, const uint32_t* list,
                          uint32_t n_live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next);
// out: `planes` frames of frame_pixels pixels each.
int launchLightGroupsResolve(void* stream, const AovChunk& c, const LgState& st, uint32_t planes, double* out, uint64_t frame_pixels);
// The same kernel's projection (include/mcrt.h "Light probes", mcrt_probes.hpp): out is planes * proj.coefficients frames of frame_pixels
// pixels each; proj.direction holds the first-ray directions of the chunk's samples. What would read or write past the chunk's arrays
// is hipErrorInvalidValue and nothing is queued.
int launchProbeResolve(void* stream, const AovChunk& c, const LgState& st, uint32_t planes, const ProbeProjection& proj, double* out, uint64_t frame_pixels);
// The same kernel's branches for the filtered planes (include/mcrt.h "Filtered planes", mcrt_film_gather.hpp), film.mode one of the
// three: the chunk's film positions into film.offset; S in `out` and W in film.weight continued over the pixels the chunk reaches;
// after the last chunk the division in place. What would read or write past an array is hipErrorInvalidValue and nothing is queued.
int launchLightGroupsFilm(void* stream, const AovChunk& c, const LgState& st, uint32_t planes, const FilmGather& film, double* out, uint64_t frame_pixels);

}  // namespace mcrt
