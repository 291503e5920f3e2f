// The image passes' host toolkit (DESIGN.md "Image passes"): what the host sides of every image pass (mcrt_*_host.hip: the first-hit AOV
// pass, the three filters, the sample statistics, the firefly suppression, accumulated rendering, the OpenEXR output and input, the ID
// mattes, the frame comparison, the occlusion pass, the lighting passes, the light groups) share - the HIP-error macro, a call's event pair
// and statistics, the guard of a render's sample targets, and the device copies of the host-pointer forms' frames. The context's side of
// it is in mcrt_internal.hpp; what the passes that trace camera rays share beyond it is mcrt_camera_pass.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "mcrt_internal.hpp"
#include "mcrt_rows.hpp"

#define MCRT_HIP_TRY(ctx, call)                                                                              \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return mcrt::ctxFail(ctx, MCRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace mcrt {

// A call's clock and its own event pair (the context's belong to renders and to the operators' timing option): construct it where the
// call's time starts; begin / end go around the launches, end waits for them; finish writes the statistics of a pass that ran no integrator.
struct PassTimer {
    mcrt_ctx* ctx;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit PassTimer(mcrt_ctx* c) : ctx(c) {}
    ~PassTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    double hostMs() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    int begin(hipStream_t stream) {
        MCRT_HIP_TRY(ctx, hipEventCreate(&e0));
        MCRT_HIP_TRY(ctx, hipEventCreate(&e1));
        MCRT_HIP_TRY(ctx, hipEventRecord(e0, stream));
        return MCRT_OK;
    }
    int end(hipStream_t stream) {
        MCRT_HIP_TRY(ctx, hipEventRecord(e1, stream));
        MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
        return MCRT_OK;
    }
    int finish(mcrt_stats* stats, uint32_t launches) {
        if (!stats) return MCRT_OK;
        float ms = 0.f;
        MCRT_HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
        memset(stats, 0, sizeof(*stats));
        stats->kernel_ms = ms;
        stats->total_ms = hostMs();
        stats->kernel_launches = launches;
        stats->kernel_id = MCRT_KERNEL_NONE;  // (names the integrator's kernel form: none ran)
        return MCRT_OK;
    }
};

// Clears the sample targets of ctxSampleTargetsBegin when the call that set them returns, whichever way.
struct SampleTargetsScope {
    mcrt_ctx* ctx;
    ~SampleTargetsScope() { ctxSampleTargetsEnd(ctx); }
};

// One frame of a host-pointer form and its device copy. A frame with neither host pointer is not wanted: it gets no device copy.
struct FrameChannel {
    const void* in;       // host frame copied up before the _device call, or nullptr
    void* out;            // host frame filled after it, or nullptr
    size_t pixel_bytes;   // element bytes x elements per pixel
    void* dev = nullptr;  // set by place()
};
// kSlotEach: frame i in scratch slot `slot + i`. kPackedWanted / kPackedAll: one allocation in `slot`, the wanted frames / every frame
// of the table at offsets rounded up to 8 bytes.
enum FrameLayout { kSlotEach, kPackedWanted, kPackedAll };

struct HostFrames {
    mcrt_ctx* ctx;
    const char* what;
    PassFamily family;
    int slot;
    FrameLayout layout;
    FrameChannel* ch;
    int n;
    int place(size_t pixels, const char* noun = "frames'") {
        const std::string failed = std::string(what) + ": the " + noun + " device copy could not be allocated";
        std::vector<size_t> at(n);
        size_t total = 0;
        for (int i = 0; i < n; i++) {
            at[i] = total;
            if (ch[i].in || ch[i].out || layout == kPackedAll) total += (pixels * ch[i].pixel_bytes + 7) / 8 * 8;
        }
        unsigned char* base = layout == kSlotEach ? nullptr : (unsigned char*)ctxPassScratch(ctx, family, slot, total);
        if (layout != kSlotEach && !base) return ctxFail(ctx, MCRT_ERR_HIP, failed);
        for (int i = 0; i < n; i++) {
            if (!ch[i].in && !ch[i].out) continue;
            ch[i].dev = base ? base + at[i] : ctxPassScratch(ctx, family, slot + i, pixels * ch[i].pixel_bytes);
            if (!ch[i].dev) return ctxFail(ctx, MCRT_ERR_HIP, failed);
        }
        return MCRT_OK;
    }
};

// The whole-frame forms: up() before the _device call (device copies placed, the inputs copied to them), down() after it.
struct StagedFrames : HostFrames {
    int up(size_t pixels) {
        if (int rc = place(pixels)) return rc;
        for (int i = 0; i < n; i++)
            if (ch[i].in) MCRT_HIP_TRY(ctx, hipMemcpy(ch[i].dev, ch[i].in, pixels * ch[i].pixel_bytes, hipMemcpyHostToDevice));
        return MCRT_OK;
    }
    int down(size_t pixels) {
        for (int i = 0; i < n; i++)
            if (ch[i].out) MCRT_HIP_TRY(ctx, hipMemcpy(ch[i].out, ch[i].dev, pixels * ch[i].pixel_bytes, hipMemcpyDeviceToHost));
        return MCRT_OK;
    }
};

// The sharded forms: the device holds the rows that cam's shard owns, packed; the host frames are whole and only those rows are written.
struct ShardFrames : HostFrames {
    int place(const mcrt_camera_desc* cam, const char* noun = "frames'") {
        if (!cam || cam->width == 0) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": camera is NULL or has no columns");
        if (cam->shard_count > 1 && cam->shard_index >= cam->shard_count) return ctxFail(ctx, MCRT_ERR_INVALID, "shard_index >= shard_count");
        return HostFrames::place((size_t)mcrt_shard_rows(cam, nullptr) * cam->width, noun);
    }
    int down(const mcrt_camera_desc* cam) {
        const uint32_t rows = mcrt_shard_rows(cam, nullptr);
        if (!rows) return MCRT_OK;
        std::vector<uint32_t> idx(rows);
        mcrt_shard_rows(cam, idx.data());
        std::vector<unsigned char> packed;
        for (int i = 0; i < n; i++) {
            if (!ch[i].out) continue;
            const size_t row_bytes = (size_t)cam->width * ch[i].pixel_bytes;
            packed.resize(rows * row_bytes);
            MCRT_HIP_TRY(ctx, hipMemcpy(packed.data(), ch[i].dev, packed.size(), hipMemcpyDeviceToHost));
            scatterRows(ch[i].out, packed.data(), idx.data(), rows, row_bytes);
        }
        return MCRT_OK;
    }
};

}  // namespace mcrt
