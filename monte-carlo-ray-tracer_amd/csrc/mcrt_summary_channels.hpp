// The per-sample summary of a render (include/mcrt.h mcrt_frame_summary), the one statement of its channels for the host code: which
// they are, their bytes per pixel, and how the two structs that the render entry points take lie inside it. The sample targets of the
// context, the host-pointer forms and the accumulated renders work on this form. No HIP here, like mcrt_rows.hpp.
#pragma once

#include <cstddef>

#include "../../include/mcrt.h"

namespace mcrt {

struct SummaryChannel { double* mcrt_frame_summary::*member; size_t pixel_bytes; };
constexpr int kSummaryChannels = 6;
constexpr SummaryChannel kSummaryChannel[kSummaryChannels] = {
    {&mcrt_frame_summary::rgb, 24},    {&mcrt_frame_summary::variance, 24},
    {&mcrt_frame_summary::half_a, 24}, {&mcrt_frame_summary::half_b, 24},
    {&mcrt_frame_summary::tops, MCRT_ROBUST_TOPS * 24}, {&mcrt_frame_summary::level, 8}};
inline double*& summaryChannel(mcrt_frame_summary& s, int i) { return s.*kSummaryChannel[i].member; }
inline double* summaryChannel(const mcrt_frame_summary& s, int i) { return s.*kSummaryChannel[i].member; }

// mcrt_frame_summary is six double* in the table's order; mcrt_pixel_stats_buffers is its members 1..3, mcrt_highlight_buffers 4..5
constexpr size_t kSummaryPointer = sizeof(double*);
static_assert(sizeof(mcrt_frame_summary) == 6 * kSummaryPointer && offsetof(mcrt_frame_summary, rgb) == 0 && offsetof(mcrt_frame_summary, variance) == kSummaryPointer &&
                  offsetof(mcrt_frame_summary, half_a) == 2 * kSummaryPointer && offsetof(mcrt_frame_summary, half_b) == 3 * kSummaryPointer &&
                  offsetof(mcrt_frame_summary, tops) == 4 * kSummaryPointer && offsetof(mcrt_frame_summary, level) == 5 * kSummaryPointer,
              "mcrt_frame_summary");
static_assert(sizeof(mcrt_pixel_stats_buffers) == 3 * kSummaryPointer && offsetof(mcrt_pixel_stats_buffers, variance) == 0 &&
                  offsetof(mcrt_pixel_stats_buffers, half_a) == kSummaryPointer && offsetof(mcrt_pixel_stats_buffers, half_b) == 2 * kSummaryPointer,
              "mcrt_pixel_stats_buffers");
static_assert(sizeof(mcrt_highlight_buffers) == 2 * kSummaryPointer && offsetof(mcrt_highlight_buffers, tops) == 0 && offsetof(mcrt_highlight_buffers, level) == kSummaryPointer,
              "mcrt_highlight_buffers");

// A NULL struct: none of its channels.
inline mcrt_frame_summary summaryOf(double* rgb, const mcrt_pixel_stats_buffers* st, const mcrt_highlight_buffers* hl) {
    return mcrt_frame_summary{rgb, st ? st->variance : nullptr, st ? st->half_a : nullptr, st ? st->half_b : nullptr, hl ? hl->tops : nullptr, hl ? hl->level : nullptr};
}
inline mcrt_pixel_stats_buffers summaryStats(const mcrt_frame_summary& s) { return mcrt_pixel_stats_buffers{s.variance, s.half_a, s.half_b}; }
inline mcrt_highlight_buffers summaryHighlights(const mcrt_frame_summary& s) { return mcrt_highlight_buffers{s.tops, s.level}; }
inline bool summaryWantsStats(const mcrt_frame_summary& s) { return s.variance || s.half_a || s.half_b; }
inline bool summaryWantsHighlights(const mcrt_frame_summary& s) { return s.tops || s.level; }

// The table of a host-pointer form (mcrt_pass_host.hpp FrameChannel; templates so that this header needs no HIP): channel i of `host`,
// nullptr = not wanted, as the output of frame i - and the summary of the device copies that place() then gave the frames.
template <class Channel>
inline void summaryFrameChannels(const mcrt_frame_summary& host, Channel (&ch)[kSummaryChannels]) {
    for (int i = 0; i < kSummaryChannels; i++) ch[i] = Channel{nullptr, summaryChannel(host, i), kSummaryChannel[i].pixel_bytes};
}
template <class Channel>
inline mcrt_frame_summary summaryOfDevice(const Channel* ch) {
    mcrt_frame_summary d{};
    for (int i = 0; i < kSummaryChannels; i++) summaryChannel(d, i) = (double*)ch[i].dev;
    return d;
}

}  // namespace mcrt
