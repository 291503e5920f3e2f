// tests/emu/denoise_dual_emu.cpp — TEST HARNESS ONLY (built by tests/test_denoise_dual_emulation.py into tests/emu/_build/).
//
// The dual-buffer filter on the host: csrc/mcrt_denoise_dual.hpp unchanged - the text the three kernels of csrc/mcrt_denoise_dual.hip
// run - driven the way mcrt_denoise_dual_device drives them: the prep pass into a scratch of records, then the filter. The plain form
// is a loop over the pixels; the tile form runs workgroup by workgroup on wave_emu.hpp's emulated workgroup (4 wavefronts of 64 fibers,
// __syncthreads a rendezvous of all of them), its LDS an array here of exactly denoiseDualTileLdsWords(R, F) doubles, filled with NaN
// before every workgroup and fenced behind. Not a CPU fallback: nothing in the product links or loads it.
#define MCRT_WAVE_EMU 1
#include "wave_emu.hpp"

#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_denoise_dual.hpp"

using namespace mcrt;

extern "C" {

// form: 0 plain, 1 tile with the workgroup the launch uses, 256 / 512 / 1024 tile with that many lanes. Host pointers to full frames; every output may alias the corresponding input (rgb any input); variance, half_a,
// half_b of `out` may be null. Returns 0, -1 for what mcrt_denoise_dual_device refuses, -2 when the tile form wrote past its LDS.
int denoise_dual_emu(uint32_t width, uint32_t height, uint32_t spp, const double* half_a, const double* half_b, const double* variance,
                     const mcrt_denoise_dual_params* params, int form, const mcrt_denoise_dual_buffers* out) {
    const DenoiseDualSettings s = denoiseDualSettings(params);
    const uint64_t pixels = (uint64_t)width * height;
    if (pixels == 0 || pixels > 0xFFFFFFFFull || spp < 2 || !half_a || !half_b || !variance || !out || !out->rgb || denoiseDualSettingsError(s)) return -1;
    std::vector<double> rec(pixels * kDenoiseDualRecWords);
    DenoiseDualFrame f;
    f.width = width;
    f.height = height;
    f.half_a = half_a;
    f.half_b = half_b;
    f.variance = variance;
    f.rec = rec.data();
    for (uint64_t p = 0; p < pixels; p++) denoiseDualPrepPixel(f, p);  // denoiseDualPrepKernel
    DenoiseDualStep st;
    st.width = width;
    st.height = height;
    denoiseDualStepConstants(s, spp, st);
    st.rec = rec.data();
    st.out_rgb = out->rgb;
    st.out_variance = out->variance;
    st.out_half_a = out->half_a;
    st.out_half_b = out->half_b;
    if (form == 0) {
        for (uint64_t p = 0; p < pixels; p++) denoiseDualPlainPixel(st, p);  // denoiseDualPlainKernel
        return 0;
    }
    const uint32_t lanes = form == 1 ? denoiseDualTileLanes(s.window_radius, s.patch_radius) : (uint32_t)form;
    if (lanes != 256 && lanes != 512 && lanes != 1024) return -1;
    const uint32_t words = denoiseDualTileLdsWords(s.window_radius, s.patch_radius);
    const double fence = -12345.0;
    std::vector<double> lds(words + 64);
    const uint64_t blocks = denoiseDualTileBlocks(width, height);
    for (uint64_t blk = 0; blk < blocks; blk++) {  // denoiseDualTileKernel, one workgroup after the other
        for (uint32_t i = 0; i < words; i++) lds[i] = __builtin_nan("");  // (a record or a term the cooperative steps forgot shows)
        for (uint32_t i = words; i < words + 64; i++) lds[i] = fence;
        wemu::launch().block_dim = lanes;
        wemu::runGroup((int)(lanes / 64), [&](int tid) { denoiseDualTileBlock(st, (uint32_t)blk, (uint32_t)tid, lanes, lds.data()); });
        for (uint32_t i = words; i < words + 64; i++)
            if (!(lds[i] == fence)) return -2;
    }
    return 0;
}

// The bytes of dynamic LDS the tile form's launch asks for (what tests/test_denoise_dual_library.py holds to its own restatement).
uint32_t denoise_dual_emu_tile_lds_bytes(uint32_t window_radius, uint32_t patch_radius) { return denoiseDualTileLdsBytes(window_radius, patch_radius); }
uint32_t denoise_dual_emu_tile_lds_max_bytes() { return kDenoiseDualTileLdsMaxBytes; }

}  // extern "C"
