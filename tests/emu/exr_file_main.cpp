// tests/emu/exr_file_main.cpp — TEST HARNESS ONLY: a stand-alone program (its own main) that tests/test_exr_emulation.py compiles with
// -fsanitize=address,undefined and runs once. It writes small files through the emulation of tests/emu/exr_emu.cpp - csrc/mcrt_exr.hpp
// and csrc/mcrt_exr_file.hpp unchanged - into the directory given: mixed channels at a ragged size without and with ZIP, a frame of random
// integers (every chunk a raw chunk) and a smooth ramp, with several deflate threads. Each line printed: file, status, file_bytes,
// packed_bytes, chunks, raw_chunks. The exit status is the number of saves that failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "exr_emu.cpp"

namespace {
uint64_t state = 0x9E3779B97F4A7C15ull;
uint64_t next() {  // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return state * 0x2545F4914F6CDD1Dull;
}

int save(const std::string& path, uint32_t w, uint32_t h, const std::vector<mcrt_exr_channel>& ch, uint32_t compression, uint32_t threads) {
    mcrt_exr_params params{};
    params.compression = MCRT_EXR_COMPRESSION_SET | compression;
    params.threads = threads;
    const mcrt_exr_attribute attr[2] = {{"mcrt:spp", "16"}, {"mcrt:kernel", "none"}};
    mcrt_exr_result r{};
    char message[256];
    const int rc = exr_save_emu(path.c_str(), w, h, ch.data(), (uint32_t)ch.size(), attr, 2, &params, &r, message);
    printf("%s %d %llu %llu %u %u %s\n", path.c_str(), rc, (unsigned long long)r.file_bytes, (unsigned long long)r.packed_bytes, r.chunks, r.raw_chunks, message);
    return rc != 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 99;
    const std::string dir = argv[1];
    int failed = 0;
    {
        const uint32_t w = 65, h = 33;
        std::vector<double> rgb((size_t)w * h * 3), tops((size_t)w * h * 12);
        std::vector<uint32_t> ids((size_t)w * h);
        for (double& v : rgb) v = std::ldexp((double)(next() >> 11), -53 + (int)(next() % 40) - 20);
        for (double& v : tops) v = -(double)(next() % 1000) / 7.0;
        for (uint32_t& v : ids) v = (uint32_t)next();
        rgb[5] = HUGE_VAL, rgb[6] = -std::nan(""), rgb[7] = 1e300, rgb[8] = -0.0;
        std::vector<mcrt_exr_channel> ch = {{"R", rgb.data(), MCRT_EXR_SRC_F64, MCRT_EXR_HALF, 3, 0},
                                            {"surface.id", ids.data(), MCRT_EXR_SRC_U32, MCRT_EXR_UINT, 1, 0},
                                            {"G", rgb.data(), MCRT_EXR_SRC_F64, MCRT_EXR_FLOAT, 3, 1},
                                            {"B", rgb.data(), MCRT_EXR_SRC_F64, MCRT_EXR_HALF, 3, 2}};
        static const char* names[12] = {"tops0.R", "tops0.G", "tops0.B", "tops1.R", "tops1.G", "tops1.B", "tops2.R", "tops2.G", "tops2.B", "tops3.R", "tops3.G", "tops3.B"};
        for (uint32_t i = 0; i < 12; i++) ch.push_back({names[i], tops.data(), MCRT_EXR_SRC_F64, i % 2 ? MCRT_EXR_FLOAT : MCRT_EXR_HALF, 12, i});
        failed += save(dir + "/mixed_none.exr", w, h, ch, MCRT_EXR_COMPRESSION_NONE, 1);
        failed += save(dir + "/mixed_zip.exr", w, h, ch, MCRT_EXR_COMPRESSION_ZIP, 3);
        failed += save(dir + "/one_pixel.exr", 1, 1, ch, MCRT_EXR_COMPRESSION_ZIP, 16);
    }
    {
        const uint32_t w = 64, h = 16;
        std::vector<uint32_t> noise((size_t)w * h);
        for (uint32_t& v : noise) v = (uint32_t)(next() >> 16);
        failed += save(dir + "/noise_zip.exr", w, h, {{"noise", noise.data(), MCRT_EXR_SRC_U32, MCRT_EXR_UINT, 1, 0}}, MCRT_EXR_COMPRESSION_ZIP, 2);
        std::vector<double> ramp((size_t)w * h);
        for (size_t i = 0; i < ramp.size(); i++) ramp[i] = (double)(i % w) / 64.0;
        failed += save(dir + "/ramp_zip.exr", w, h, {{"Y", ramp.data(), MCRT_EXR_SRC_F64, MCRT_EXR_HALF, 1, 0}}, MCRT_EXR_COMPRESSION_ZIP, 2);
    }
    return failed;
}
