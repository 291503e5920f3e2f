// Frame comparison (include/mcrt.h mcrt_frame_compare*), host side: the entry points, validation, defaults, the host-pointer form,
// scratch and the loop over the tree sums' levels. No kernel here: they are libmcrt_compare.so (csrc/mcrt_compare.hip; DESIGN.md "Image
// passes" says why, and what mcrt_pass_host.hpp shares). Scratch slots of the family: 0 the host form's frames and maps, 1 level 0's
// block values (se, ae, rel, the maximum's values and indices, the three counts), 2 and 3 the upper levels' ping and pong, 4 the per-centre ssim,
// 5 the count of excluded centres.
#include <algorithm>
#include <cmath>

#include "mcrt_compare.hpp"
#include "mcrt_compare_launch.hpp"
#include "mcrt_pass_host.hpp"

using namespace mcrt;

namespace {

int compareCheck(mcrt_ctx* ctx, const char* what, uint32_t width, uint32_t height, const void* rgb, const void* ref, const mcrt_compare_params* params,
                 const mcrt_compare_result* result, CompareSettings* s) {
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (!rgb || !ref || !result) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": the frame, the reference or the result is NULL");
    const uint64_t pixels = (uint64_t)width * height;
    if (pixels == 0 || pixels > 0xFFFFFFFFull) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": width * height must be non-zero and below 2^32");
    const char* why = nullptr;
    if (int rc = compareSettings(params, s, &why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);
    return MCRT_OK;
}

}  // namespace

extern "C" int mcrt_frame_compare_device(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* d_rgb, const double* d_ref, const double* d_mask,
                                         const mcrt_compare_params* params, const mcrt_compare_maps* d_maps, mcrt_compare_result* result, mcrt_stats* stats) {
    const char* what = "mcrt_frame_compare_device";
    if (!ctx) return MCRT_ERR_INVALID;
    CompareSettings s;
    if (int rc = compareCheck(ctx, what, width, height, d_rgb, d_ref, params, result, &s)) return rc;
    PassTimer timer(ctx);
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const uint64_t pixels = (uint64_t)width * height;
    const uint64_t centres = s.ssim ? ssimCentres(width, height) : 0;
    const uint64_t blocks0 = compareBlocks(pixels);
    const uint64_t stride1 = std::max(compareBlocks(blocks0), compareBlocks(centres));  // the widest column the first upper level writes
    double* level0 = (double*)ctxPassScratch(ctx, kPassCompare, 1, blocks0 * (5 + kCompareCounts) * sizeof(double));
    double* buf[2] = {(double*)ctxPassScratch(ctx, kPassCompare, 2, stride1 * kCompareRecordWords * sizeof(double)),
                      (double*)ctxPassScratch(ctx, kPassCompare, 3, compareBlocks(stride1) * kCompareRecordWords * sizeof(double))};
    double* values = centres ? (double*)ctxPassScratch(ctx, kPassCompare, 4, centres * sizeof(double)) : nullptr;
    unsigned long long* excluded = (unsigned long long*)ctxPassScratch(ctx, kPassCompare, 5, sizeof(unsigned long long));
    if (!level0 || !buf[0] || !buf[1] || (centres && !values) || !excluded) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": scratch could not be allocated");

    MCRT_HIP_TRY(ctx, hipMemsetAsync(excluded, 0, sizeof(unsigned long long), stream));
    if (int rc = timer.begin(stream)) return rc;
    uint32_t launches = 0;
    ComparePixels cp{};
    cp.rgb = d_rgb;
    cp.ref = d_ref;
    cp.mask = d_mask;
    cp.map_se = d_maps ? d_maps->squared_error : nullptr;
    cp.map_rel = d_maps ? d_maps->relative : nullptr;
    cp.map_zero = d_maps && s.ssim ? d_maps->ssim : nullptr;
    for (int c = 0; c < 3; c++) cp.out_sum[c] = level0 + c * blocks0;
    cp.out_max = level0 + 3 * blocks0;
    cp.out_idx = (uint64_t*)(level0 + 4 * blocks0);
    for (uint32_t k = 0; k < kCompareCounts; k++) cp.out_cnt[k] = (uint64_t*)(level0 + (5 + k) * blocks0);
    cp.pixels = pixels;
    cp.width = width;
    cp.height = height;
    cp.vec = compareVec(d_rgb, d_ref);
    cp.eps = s.eps;
    MCRT_HIP_TRY(ctx, (hipError_t)launchComparePixels(stream, cp));
    launches++;
    if (centres) {
        CompareSsim cs{};
        cs.rgb = d_rgb;
        cs.ref = d_ref;
        cs.values = values;
        cs.map = d_maps ? d_maps->ssim : nullptr;
        cs.excluded = excluded;
        cs.width = width;
        cs.height = height;
        cs.c1 = (0.01 * s.range) * (0.01 * s.range);
        cs.c2 = (0.03 * s.range) * (0.03 * s.range);
        MCRT_HIP_TRY(ctx, (hipError_t)launchCompareSsim(stream, cs));
        launches++;
    }
    // the upper levels, at least one: the last one leaves the columns side by side (se, ae, rel, ssim, the maximum, its index)
    CompareLevel lv{};
    for (int c = 0; c < 3; c++) lv.in[c] = cp.out_sum[c], lv.n[c] = blocks0;
    lv.in[3] = values;
    lv.n[3] = centres;
    lv.in_max = cp.out_max;
    lv.in_idx = cp.out_idx;
    for (uint32_t k = 0; k < kCompareCounts; k++) lv.in_cnt[k] = cp.out_cnt[k];
    int which = 0;
    for (;;) {
        const uint64_t stride = compareLevelBlocks(lv);
        for (uint32_t c = 0; c < kCompareColumns; c++) lv.out[c] = buf[which] + c * stride;
        lv.out_max = buf[which] + kCompareColumns * stride;
        lv.out_idx = (uint64_t*)(buf[which] + (kCompareColumns + 1) * stride);
        for (uint32_t k = 0; k < kCompareCounts; k++) lv.out_cnt[k] = (uint64_t*)(buf[which] + (kCompareColumns + 2 + k) * stride);
        MCRT_HIP_TRY(ctx, (hipError_t)launchCompareLevel(stream, lv));
        launches++;
        if (stride == 1) break;
        for (uint32_t c = 0; c < kCompareColumns; c++) lv.in[c] = lv.out[c], lv.n[c] = compareBlocks(lv.n[c]);
        lv.in_max = lv.out_max;
        lv.in_idx = lv.out_idx;
        for (uint32_t k = 0; k < kCompareCounts; k++) lv.in_cnt[k] = lv.out_cnt[k];
        which ^= 1;
    }
    if (int rc = timer.end(stream)) return rc;
    struct {
        double sum[kCompareColumns], max_abs;
        uint64_t max_index, n[kCompareCounts];
    } top;
    static_assert(sizeof(top) == kCompareRecordWords * 8, "the last level's record");
    unsigned long long bad = 0;
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(&top, buf[which], sizeof(top), hipMemcpyDeviceToHost, stream));
    if (centres) MCRT_HIP_TRY(ctx, hipMemcpyAsync(&bad, excluded, sizeof(bad), hipMemcpyDeviceToHost, stream));
    MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
    mcrt_compare_result r{};
    r.sum_se = top.sum[0];
    r.sum_ae = top.sum[1];
    r.sum_rel = top.sum[2];
    r.sum_ssim = centres ? top.sum[3] : 0.0;
    r.max_abs = top.max_abs;
    r.pixels = pixels;
    r.nonfinite = top.n[kCompareNonfinite];
    r.masked = top.n[kCompareMasked];
    r.differing = top.n[kCompareDiffering];
    r.ssim_centres = centres;
    r.ssim_excluded = bad;
    compareFinish(&r, s, top.max_index);
    *result = r;
    return timer.finish(stats, launches);
}

extern "C" int mcrt_frame_compare(mcrt_ctx* ctx, uint32_t width, uint32_t height, const double* rgb, const double* ref, const double* mask,
                                  const mcrt_compare_params* params, const mcrt_compare_maps* maps, mcrt_compare_result* result, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    CompareSettings s;
    if (int rc = compareCheck(ctx, "mcrt_frame_compare", width, height, rgb, ref, params, result, &s)) return rc;
    PassTimer whole(ctx);
    const size_t pixels = (size_t)width * height;
    FrameChannel ch[6] = {{rgb, nullptr, 24}, {ref, nullptr, 24}, {mask, nullptr, 8}, {nullptr, maps ? maps->squared_error : nullptr, 8},
                          {nullptr, maps ? maps->relative : nullptr, 8}, {nullptr, maps && s.ssim ? maps->ssim : nullptr, 8}};
    StagedFrames frames{{ctx, "mcrt_frame_compare", kPassCompare, 0, kPackedWanted, ch, 6}};
    if (int rc = frames.up(pixels)) return rc;
    const mcrt_compare_maps d_maps{(double*)ch[3].dev, (double*)ch[4].dev, (double*)ch[5].dev};
    mcrt_stats st;
    if (int rc = mcrt_frame_compare_device(ctx, width, height, (const double*)ch[0].dev, (const double*)ch[1].dev, (const double*)ch[2].dev, params, &d_maps, result, &st)) return rc;
    if (int rc = frames.down(pixels)) return rc;
    st.total_ms = whole.hostMs();
    if (stats) *stats = st;
    return MCRT_OK;
}
