// The four launches of the path classes: defined in csrc/mcrt_path_classes.hip (libmcrt_path_classes.so, the pass's own code object),
// called by csrc/mcrt_path_classes_host.hip (libmcrt_hip.so). All queue one kernel on `stream` (a hipStream_t) and return the launch's
// hipError_t as an int. They are the light groups' four (mcrt_light_groups_launch.hpp says what each reads and leaves), on PcState.
#pragma once

#include "mcrt_film_gather.hpp"
#include "mcrt_path_classes.hpp"

namespace mcrt {

int launchPathClassesBegin(void* stream, const PcState& st, uint64_t n, double scene_ior, const PcParams& par, uint32_t* list, LgCounters* counters);
int launchPathClassesRays(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const PcState& st, const uint32_t* list, uint32_t n_live,
                          uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next);
int launchPathClassesStep(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const PcState& st, const PcParams& par, const uint32_t* list,
                          uint32_t n_live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next);
int launchPathClassesResolve(void* stream, const AovChunk& c, const PcState& st, uint32_t planes, double* out, uint64_t frame_pixels);
// pathClassesResolveKernel's branches for the filtered planes: launchLightGroupsFilm's (mcrt_light_groups_launch.hpp), on PcState.
int launchPathClassesFilm(void* stream, const AovChunk& c, const PcState& st, uint32_t planes, const FilmGather& film, double* out, uint64_t frame_pixels);

}  // namespace mcrt
