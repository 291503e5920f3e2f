// tests/emu/denoise_var_emu.cpp — TEST HARNESS ONLY (built by tests/test_denoise_var_emulation.py into tests/emu/_build/).
//
// The variance-guided a-trous filter on the host: csrc/mcrt_denoise_var.hpp unchanged - the text the three kernels of
// csrc/mcrt_denoise_var.hip run - driven pass by pass the way mcrt_denoise_variance_device drives them. The plain form is a loop over the
// pixels; the tile form runs workgroup by workgroup on wave_emu.hpp's emulated workgroup (4 wavefronts of 64 fibers, __syncthreads a
// rendezvous of all of them), its LDS an array here. Not a CPU fallback: nothing in the product links or loads it.
#define MCRT_WAVE_EMU 1
#include "wave_emu.hpp"

#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_denoise_var.hpp"

using namespace mcrt;

extern "C" {

// form: 0 plain, 1 tile. Host pointers to full frames; guides->albedo may be null with MCRT_DENOISE_NO_ALBEDO; out may be rgb, out_variance
// may be variance or null. Returns 0, or -1 for what mcrt_denoise_variance_device refuses.
int denoise_var_emu(uint32_t width, uint32_t height, uint32_t spp, const double* rgb, const double* variance, const mcrt_aov_buffers* guides,
                    const mcrt_denoise_variance_params* params, int form, double* out, double* out_variance) {
    const DenoiseVarSettings s = denoiseVarSettings(params);
    const uint64_t pixels = (uint64_t)width * height;
    const bool with_albedo = !(s.flags & MCRT_DENOISE_NO_ALBEDO);
    if (pixels == 0 || pixels > 0xFFFFFFFFull || spp == 0 || !rgb || !variance || !out || !guides || !guides->shading_normal || !guides->normal ||
        !guides->position || !guides->coverage || (with_albedo && !guides->albedo) || denoiseVarSettingsError(s))
        return -1;
    std::vector<double> guide(pixels * kDenoiseGuideWords), a(pixels * kDenoiseVarIvWords), b(pixels * kDenoiseVarIvWords);
    DenoiseVarFrame f;
    f.width = width;
    f.height = height;
    f.spp = (double)spp;
    f.rgb = rgb;
    f.variance = variance;
    f.shading_normal = guides->shading_normal;
    f.normal = guides->normal;
    f.position = guides->position;
    f.coverage = guides->coverage;
    f.albedo = with_albedo ? guides->albedo : nullptr;
    f.albedo_floor = s.albedo_floor;
    f.guide = guide.data();
    f.iv = a.data();
    for (uint64_t p = 0; p < pixels; p++) denoiseVarPrepPixel(f, p);  // denoiseVarPrepKernel
    static double lds[kDenoiseVarTileWords];
    DenoiseVarStep st;
    st.width = width;
    st.height = height;
    st.guide = guide.data();
    denoiseVarStepConstants(s, spp, st);
    const double* in = a.data();
    for (uint32_t i = 0; i < s.iterations; i++) {
        const bool last = i + 1 == s.iterations;
        st.step = 1u << i;
        st.in = in;
        st.out = last ? nullptr : (in == a.data() ? b.data() : a.data());
        st.out_rgb = last ? out : nullptr;
        st.out_variance = last ? out_variance : nullptr;
        st.albedo = last ? f.albedo : nullptr;
        if (form == 0) {
            for (uint64_t p = 0; p < pixels; p++) denoiseVarPlainPixel(st, p);  // denoiseVarPlainKernel
        } else {
            const uint64_t blocks = denoiseTileBlocks(denoiseTiling(width, height, st.step));
            for (uint64_t blk = 0; blk < blocks; blk++) {  // denoiseVarTileKernel, one workgroup after the other
                for (double& w : lds) w = __builtin_nan("");  // (a record the staging loop forgot shows)
                wemu::launch().block_dim = kDenoiseBlock;
                wemu::runGroup(kDenoiseBlock / 64, [&](int tid) { denoiseVarTileBlock(st, (uint32_t)blk, (uint32_t)tid, lds); });
            }
        }
        in = st.out;
    }
    return 0;
}

// The bytes of LDS the tile form's workgroup declares (what tests/test_denoise_var_library.py holds the kernel to).
uint32_t denoise_var_emu_tile_lds_bytes() { return kDenoiseVarTileLdsBytes; }

}  // extern "C"
