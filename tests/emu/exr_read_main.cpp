// tests/emu/exr_read_main.cpp — TEST HARNESS ONLY: a stand-alone program (its own main) that tests/test_exr_read_emulation.py compiles
// with -fsanitize=address,undefined and runs once. It writes a 9 x 18 file of mixed channels with ZIP and without compression through the
// save emulation (tests/emu/exr_emu.cpp) into the directory given, and loads each through the load emulation (tests/emu/exr_read_emu.cpp -
// csrc/mcrt_exr_read.hpp and csrc/mcrt_exr_read_file.hpp unchanged) whole; cut at every byte length from 0 to its size - 1; with every
// byte of the header and the offset table replaced by 0x00, 0xff and byte ^ 0x80; and with 2 000 bytes of the chunk area flipped one at a
// time (xorshift, fixed seed). Every load must come back with MCRT_OK, MCRT_ERR_IO or MCRT_ERR_UNSUPPORTED, and a truncated file never
// with MCRT_OK. Each line printed: the file and its counts. The exit status is the number of violations.
#include <cstdio>
#include <cstdlib>

#include "exr_read_emu.cpp"

#include "exr_emu.cpp"

namespace {

uint64_t state = 0x2545F4914F6CDD1Dull;
uint64_t next() {  // xorshift64
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
}

bool writeFile(const std::string& path, const std::vector<unsigned char>& bytes, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(bytes.data(), 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

// Opens the file and loads every channel of it into frames of its own -> the status. table_end: where the offset table ends.
int loadAll(const std::string& path, uint64_t* table_end) {
    void* handle = nullptr;
    char message[512];
    if (int rc = exr_read_open_emu(path.c_str(), &handle, message)) return rc;
    const ExrFile& file = ((exr_read_emu::Handle*)handle)->file;
    if (table_end) *table_end = file.table_at + 8ull * file.chunks;
    int rc;
    {
        // (the frames are sized by the header: the chunks' checks first, so that a header that lies about its window is refused before)
        std::vector<ExrChunkPlace> places;
        std::string why;
        rc = exrReadChunkPlaces(file, places, nullptr, why);
    }
    if (rc == MCRT_OK) {
        const size_t pixels = (size_t)file.width * file.height, count = std::min<size_t>(file.channels.size(), MCRT_EXR_MAX_CHANNELS);
        std::vector<std::vector<uint64_t>> frames(count);
        std::vector<mcrt_exr_target> targets(count);
        for (size_t i = 0; i < count; i++) {
            const bool uint = file.channels[i].pixel_type == MCRT_EXR_UINT;
            frames[i].assign(uint ? (pixels + 1) / 2 : pixels, 0);
            targets[i] = mcrt_exr_target{file.channels[i].name.c_str(), frames[i].data(), uint ? (uint32_t)MCRT_EXR_SRC_U32 : (uint32_t)MCRT_EXR_SRC_F64, 1, 0, 0};
        }
        mcrt_exr_load_params params{2, 0};
        mcrt_exr_load_result result{};
        rc = exr_read_load_emu(handle, targets.data(), (uint32_t)count, &params, &result, message);
    }
    exr_read_close_emu(handle);
    return rc;
}

struct Counts {
    unsigned long long violations = 0, whole = 0, ok = 0, io = 0, unsupported = 0;
    void take(int rc, bool truncated) {
        if (rc == MCRT_OK) ok++;
        else if (rc == MCRT_ERR_IO) io++;
        else if (rc == MCRT_ERR_UNSUPPORTED) unsupported++;
        else violations++;
        if (rc == MCRT_OK && truncated) whole++, violations++;
    }
};

int torture(const char* label, const std::string& path, const std::string& work) {
    std::vector<unsigned char> bytes;
    {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) return 1000;
        unsigned char buf[4096];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
        fclose(f);
    }
    Counts c;
    uint64_t table_end = 0;
    if (loadAll(path, &table_end) != MCRT_OK || table_end == 0 || table_end >= bytes.size()) return 1000;
    unsigned long long truncations = 0, header_loads = 0, flips = 0;
    for (size_t n = 0; n < bytes.size(); n++, truncations++) {
        if (!writeFile(work, bytes, n)) return 1000;
        c.take(loadAll(work, nullptr), true);
    }
    for (size_t at = 0; at < table_end; at++) {
        const unsigned char was = bytes[at];
        for (const unsigned char now : {(unsigned char)0x00, (unsigned char)0xff, (unsigned char)(was ^ 0x80)}) {
            bytes[at] = now;
            if (!writeFile(work, bytes, bytes.size())) return 1000;
            c.take(loadAll(work, nullptr), false);
            header_loads++;
        }
        bytes[at] = was;
    }
    for (; flips < 2000; flips++) {
        const size_t at = (size_t)table_end + (size_t)(next() % (bytes.size() - table_end));
        const unsigned char was = bytes[at];
        bytes[at] = (unsigned char)(was ^ (unsigned char)(1u + next() % 255u));
        if (!writeFile(work, bytes, bytes.size())) return 1000;
        c.take(loadAll(work, nullptr), false);
        bytes[at] = was;
    }
    printf("%s bytes %zu header_bytes %llu truncations %llu header_loads %llu flips %llu violations %llu whole %llu ok %llu io %llu unsupported %llu\n", label,
           bytes.size(), (unsigned long long)table_end, truncations, header_loads, flips, c.violations, c.whole, c.ok, c.io, c.unsupported);
    return (int)std::min<unsigned long long>(c.violations, 100);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 99;
    const std::string dir = argv[1];
    const uint32_t w = 9, h = 18;
    std::vector<double> rgb((size_t)w * h * 3), depth((size_t)w * h);
    std::vector<uint32_t> ids((size_t)w * h);
    for (size_t i = 0; i < rgb.size(); i++) rgb[i] = (double)(i / 3) / 64.0 + (double)(i % 3);
    for (size_t i = 0; i < depth.size(); i++) depth[i] = 3.0 + (double)i / 8.0, ids[i] = (uint32_t)(i / 7);
    rgb[5] = __builtin_inf(), rgb[6] = -__builtin_nan(""), rgb[7] = 1e300, rgb[8] = -0.0;
    const std::vector<mcrt_exr_channel> ch = {{"R", rgb.data(), MCRT_EXR_SRC_F64, MCRT_EXR_HALF, 3, 0},       {"surface.id", ids.data(), MCRT_EXR_SRC_U32, MCRT_EXR_UINT, 1, 0},
                                              {"G", rgb.data(), MCRT_EXR_SRC_F64, MCRT_EXR_FLOAT, 3, 1},      {"B", rgb.data(), MCRT_EXR_SRC_F64, MCRT_EXR_HALF, 3, 2},
                                              {"depth.Z", depth.data(), MCRT_EXR_SRC_F64, MCRT_EXR_FLOAT, 1, 0}};
    const mcrt_exr_attribute attr[1] = {{"mcrt:spp", "16"}};
    int failed = 0;
    for (const uint32_t compression : {(uint32_t)MCRT_EXR_COMPRESSION_ZIP, (uint32_t)MCRT_EXR_COMPRESSION_NONE}) {
        const char* label = compression == MCRT_EXR_COMPRESSION_ZIP ? "zip" : "none";
        const std::string path = dir + "/" + label + ".exr";
        mcrt_exr_params params{};
        params.compression = MCRT_EXR_COMPRESSION_SET | compression;
        mcrt_exr_result r{};
        char message[256];
        if (exr_save_emu(path.c_str(), w, h, ch.data(), (uint32_t)ch.size(), attr, 1, &params, &r, message) != 0) return 98;
        if (compression == MCRT_EXR_COMPRESSION_ZIP && r.raw_chunks != 0) return 97;  // (the deflated path is what is tortured)
        failed += torture(label, path, dir + "/work.exr");
    }
    return std::min(failed, 100);
}
