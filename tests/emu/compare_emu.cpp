// tests/emu/compare_emu.cpp — TEST HARNESS ONLY (built by tests/test_compare_emulation.py into tests/emu/_build/).
//
// The frame comparison on the host: csrc/mcrt_compare.hpp unchanged - the text the three kernels of csrc/mcrt_compare.hip run - on
// wave_emu.hpp's emulated workgroup (4 wavefronts of 64 fibers, __syncthreads a rendezvous of all of them, ballots served from the
// lanes' operands), driven launch by launch the way mcrt_frame_compare_device drives it. A kernel's LDS is an array here of exactly the
// words its launch has, filled with NaN before every workgroup (a word read before it is written shows) and fenced behind. Not a CPU
// fallback: nothing in the product links or loads it. With -DCOMPARE_EMU_MAIN it is a program of its own (the sanitizer run).
#define MCRT_WAVE_EMU 1
#include "wave_emu.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_compare.hpp"

using namespace mcrt;

namespace {

constexpr uint32_t kFence = 64;
struct Lds {
    std::vector<double> w;
    uint32_t words;
    explicit Lds(uint32_t n) : w(n + kFence + 2), words(n) {}
    double* data() { return (double*)(((uintptr_t)w.data() + 15) & ~(uintptr_t)15); }  // 16-byte aligned like the kernel's
    void arm() {
        double* d = data();
        for (uint32_t i = 0; i < words; i++) d[i] = __builtin_nan("");
        for (uint32_t i = 0; i < kFence; i++) d[words + i] = 1234.5 + i;
    }
    bool intact() {
        const double* d = data();
        for (uint32_t i = 0; i < kFence; i++)
            if (d[words + i] != 1234.5 + i) return false;
        return true;
    }
};

template <uint32_t kTileW, uint32_t kTileH>
bool runSsim(const CompareSsim& cs) {
    Lds lds(ssimLdsWords(kTileW, kTileH));
    const uint64_t blocks = ssimTiles(cs.width, cs.height, kTileW, kTileH);
    for (uint64_t b = 0; b < blocks; b++) {
        lds.arm();
        wemu::launch().block_dim = kSsimBlock;
        wemu::launch().block_idx = (uint32_t)b;
        wemu::launch().grid_dim = (uint32_t)blocks;
        wemu::runGroup(kSsimBlock / 64, [&](int tid) { compareSsimBlock<kTileW, kTileH>(cs, b, (uint32_t)tid, lds.data()); });
        if (!lds.intact()) return false;
    }
    return true;
}

}  // namespace

extern "C" {

// Frames [height][width][3], mask [height][width] or null, maps' pointers [height][width] or null. tile: 0 = the library's 32 x 16,
// 1 = 8 x 8, 2 = 64 x 4. vec: -1 = what the launch decides from the frames' alignment, 0 = the 8-byte loads. Returns the number of
// launches, -1 for what the entry points refuse, -2 when a kernel wrote past its LDS.
int compare_emu(uint32_t width, uint32_t height, const double* rgb, const double* ref, const double* mask, const mcrt_compare_params* params,
                const mcrt_compare_maps* maps, mcrt_compare_result* result, int tile, int vec) {
    CompareSettings s;
    const char* why = nullptr;
    const uint64_t pixels = (uint64_t)width * height;
    if (!rgb || !ref || !result || pixels == 0 || pixels > 0xFFFFFFFFull || compareSettings(params, &s, &why)) return -1;
    const uint64_t centres = s.ssim ? ssimCentres(width, height) : 0;
    const uint64_t blocks0 = compareBlocks(pixels);
    const uint64_t stride1 = std::max(compareBlocks(blocks0), compareBlocks(centres));
    std::vector<double> level0(blocks0 * (5 + kCompareCounts), -3.0), values(centres, -3.0), buf[2];
    buf[0].assign(stride1 * kCompareRecordWords, -3.0);
    buf[1].assign(compareBlocks(stride1) * kCompareRecordWords, -3.0);
    unsigned long long excluded = 0;
    int launches = 0;

    ComparePixels cp{};
    cp.rgb = rgb;
    cp.ref = ref;
    cp.mask = mask;
    cp.map_se = maps ? maps->squared_error : nullptr;
    cp.map_rel = maps ? maps->relative : nullptr;
    cp.map_zero = maps && s.ssim ? maps->ssim : nullptr;
    for (int c = 0; c < 3; c++) cp.out_sum[c] = level0.data() + c * blocks0;
    cp.out_max = level0.data() + 3 * blocks0;
    cp.out_idx = (uint64_t*)(level0.data() + 4 * blocks0);
    for (uint32_t k = 0; k < kCompareCounts; k++) cp.out_cnt[k] = (uint64_t*)(level0.data() + (5 + k) * blocks0);
    cp.pixels = pixels;
    cp.width = width;
    cp.height = height;
    cp.vec = vec == 0 ? 0u : compareVec(rgb, ref);
    cp.eps = s.eps;
    {
        Lds lds(kCompareStageWords);
        for (uint64_t b = 0; b < blocks0; b++) {
            lds.arm();
            wemu::launch().block_dim = kCompareBlock;
            wemu::launch().block_idx = (uint32_t)b;
            wemu::launch().grid_dim = (uint32_t)blocks0;
            wemu::runGroup(kCompareBlock / 64, [&](int tid) { comparePixelsBlock(cp, b, (uint32_t)tid, lds.data()); });
            if (!lds.intact()) return -2;
        }
        launches++;
    }
    if (centres) {
        CompareSsim cs{};
        cs.rgb = rgb;
        cs.ref = ref;
        cs.values = values.data();
        cs.map = maps ? maps->ssim : nullptr;
        cs.excluded = &excluded;
        cs.width = width;
        cs.height = height;
        cs.c1 = (0.01 * s.range) * (0.01 * s.range);
        cs.c2 = (0.03 * s.range) * (0.03 * s.range);
        const bool ok = tile == 1 ? runSsim<8, 8>(cs) : tile == 2 ? runSsim<64, 4>(cs) : runSsim<kSsimTileW, kSsimTileH>(cs);
        if (!ok) return -2;
        launches++;
    }
    CompareLevel lv{};
    for (int c = 0; c < 3; c++) lv.in[c] = cp.out_sum[c], lv.n[c] = blocks0;
    lv.in[3] = centres ? values.data() : nullptr;
    lv.n[3] = centres;
    lv.in_max = cp.out_max;
    lv.in_idx = cp.out_idx;
    for (uint32_t k = 0; k < kCompareCounts; k++) lv.in_cnt[k] = cp.out_cnt[k];
    int which = 0;
    Lds lds(kCompareLevelWords);
    for (;;) {
        const uint64_t stride = compareLevelBlocks(lv);
        for (uint32_t c = 0; c < kCompareColumns; c++) lv.out[c] = buf[which].data() + c * stride;
        lv.out_max = buf[which].data() + kCompareColumns * stride;
        lv.out_idx = (uint64_t*)(buf[which].data() + (kCompareColumns + 1) * stride);
        for (uint32_t k = 0; k < kCompareCounts; k++) lv.out_cnt[k] = (uint64_t*)(buf[which].data() + (kCompareColumns + 2 + k) * stride);
        for (uint64_t b = 0; b < stride; b++) {
            lds.arm();
            wemu::launch().block_dim = kCompareBlock;
            wemu::launch().block_idx = (uint32_t)b;
            wemu::launch().grid_dim = (uint32_t)stride;
            wemu::runGroup(kCompareBlock / 64, [&](int tid) { compareLevelBlock(lv, b, (uint32_t)tid, lds.data()); });
            if (!lds.intact()) return -2;
        }
        launches++;
        if (stride == 1) break;
        for (uint32_t c = 0; c < kCompareColumns; c++) lv.in[c] = lv.out[c], lv.n[c] = compareBlocks(lv.n[c]);
        lv.in_max = lv.out_max;
        lv.in_idx = lv.out_idx;
        for (uint32_t k = 0; k < kCompareCounts; k++) lv.in_cnt[k] = lv.out_cnt[k];
        which ^= 1;
    }
    const double* top = buf[which].data();
    mcrt_compare_result r{};
    r.sum_se = top[0];
    r.sum_ae = top[1];
    r.sum_rel = top[2];
    r.sum_ssim = centres ? top[3] : 0.0;
    r.max_abs = top[4];
    uint64_t max_index, n[kCompareCounts];
    memcpy(&max_index, top + 5, 8);
    memcpy(n, top + 6, sizeof n);
    r.pixels = pixels;
    r.nonfinite = n[kCompareNonfinite];
    r.masked = n[kCompareMasked];
    r.differing = n[kCompareDiffering];
    r.ssim_centres = centres;
    r.ssim_excluded = excluded;
    compareFinish(&r, s, max_index);
    *result = r;
    return launches;
}

// g[i - 5], i = 0 .. 10, as the kernels take them
double compare_emu_weight(uint32_t i) { return ssimWeight(i); }
uint32_t compare_emu_ssim_lds_bytes(void) { return ssimLdsWords(kSsimTileW, kSsimTileH) * 8; }

}  // extern "C"

#if defined(COMPARE_EMU_MAIN)
// The 70 x 13 case as a program of its own: seeded frames, a mask, planted non-finite values, every map, two tile shapes and both
// load forms, which must agree. Exit status 0 when they do.
int main() {
    const uint32_t w = 70, h = 13;
    std::vector<double> rgb(w * h * 3), ref(w * h * 3), mask(w * h);
    uint64_t state = 0x5EED0A0Full;
    auto next = [&] {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(state >> 11) / 9007199254740992.0;
    };
    for (size_t i = 0; i < rgb.size(); i++) ref[i] = next(), rgb[i] = ref[i] + (next() - 0.5) * 0.1;
    for (size_t i = 0; i < mask.size(); i++) mask[i] = next() < 0.1 ? 0.0 : 1.0;
    rgb[3 * 100 + 1] = __builtin_nan("");
    ref[3 * 500] = __builtin_inf();
    mcrt_compare_result first{};
    for (int run = 0; run < 4; run++) {
        std::vector<double> m0(w * h, -1.0), m1(w * h, -1.0), m2(w * h, -1.0);
        const mcrt_compare_maps maps{m0.data(), m1.data(), m2.data()};
        mcrt_compare_result r{};
        const int rc = compare_emu(w, h, rgb.data(), ref.data(), mask.data(), nullptr, &maps, &r, run & 1 ? 1 : 0, run & 2 ? 0 : -1);
        if (rc < 0) return std::printf("compare_emu: %d\n", rc), 1;
        if (run == 0) first = r;
        if (memcmp(&first, &r, sizeof r) != 0) return std::printf("run %d differs\n", run), 1;
    }
    std::printf("compared %llu nonfinite %llu masked %llu sum_se %a mean_ssim %a\n", (unsigned long long)first.compared,
                (unsigned long long)first.nonfinite, (unsigned long long)first.masked, first.sum_se, first.mean_ssim);
    return first.compared + first.nonfinite + first.masked == w * h && first.nonfinite >= 1 ? 0 : 1;
}
#endif
