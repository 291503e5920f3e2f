// tests/emu/exr_emu.cpp — TEST HARNESS ONLY (built by tests/test_exr_emulation.py into tests/emu/_build/; tests/emu/exr_file_main.cpp
// includes it for its stand-alone sanitizer run).
//
// The OpenEXR output on the host: csrc/mcrt_exr.hpp unchanged - the text the kernel of csrc/mcrt_exr.hip runs - driven as a loop over its
// lanes in the launch's own geometry (csrc/mcrt_exr_launch.hpp: the ragged last workgroup is walked lane by lane past the end like the
// launch does), and csrc/mcrt_exr_file.hpp as it is. Not a CPU fallback: nothing in the product links or loads it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_exr_file.hpp"
#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_exr_launch.hpp"

using namespace mcrt;

namespace {
void packOnHost(const ExrPlan& plan, std::vector<unsigned char>& out) {
    const ExrPack shape = exrPackOf(plan, nullptr, nullptr);
    out.assign((size_t)exrPackedWords(shape) * 4, 0xEE);
    const ExrPack pk = exrPackOf(plan, plan.table.data(), out.data());
    const uint64_t blocks = exrPackBlocks(pk);
    for (uint64_t blk = 0; blk < blocks; blk++)
        for (uint32_t t = 0; t < kExrPackBlock; t++) exrPackLane(pk, pk.table, blk, t);
}
}  // namespace

extern "C" {

// bits -> the file's bits, per value
void exr_half_emu(const uint64_t* in, uint64_t n, int keep_inf, uint16_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = (uint16_t)exrHalfBits(in[i], keep_inf != 0);
}
void exr_float_emu(const uint64_t* in, uint64_t n, uint32_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = exrFloatBits(in[i]);
}

// The packed buffer of a save (packed: at least width * height * the channels' bytes, rounded up to 4) and, per byte of it, the byte by
// the per-byte map exrPayloadByte (by_byte: as long; may be NULL). Returns the library's status for these arguments.
int exr_pack_emu(uint32_t width, uint32_t height, const mcrt_exr_channel* channels, uint32_t count, const mcrt_exr_params* params, unsigned char* packed,
                 unsigned char* by_byte, uint64_t* packed_bytes) {
    ExrPlan plan;
    std::string why;
    if (int rc = exrPlan("", width, height, channels, count, nullptr, 0, params, plan, why)) return rc;
    std::vector<unsigned char> out;
    packOnHost(plan, out);
    memcpy(packed, out.data(), out.size());
    *packed_bytes = plan.total_bytes;
    if (by_byte) {
        const ExrPack pk = exrPackOf(plan, plan.table.data(), nullptr);
        for (uint64_t g = 0; g < plan.total_bytes; g++) by_byte[g] = (unsigned char)exrPayloadByte(pk, pk.table, g / pk.chunk_bytes, g % pk.chunk_bytes);
    }
    return 0;
}

// A whole save with HOST data pointers: the plain-C++ path of mcrt_exr_save. message (may be NULL): the refusal's text, 256 bytes.
int exr_save_emu(const char* path, uint32_t width, uint32_t height, const mcrt_exr_channel* channels, uint32_t count, const mcrt_exr_attribute* attributes,
                 uint32_t attribute_count, const mcrt_exr_params* params, mcrt_exr_result* result, char* message) {
    std::string why;
    std::vector<unsigned char> out;
    const int rc = exrSave(path, width, height, channels, count, attributes, attribute_count, params, result, why, [&out](const ExrPlan& plan, const unsigned char** packed) {
        packOnHost(plan, out);
        *packed = out.data();
        return 0;
    });
    if (message) {
        strncpy(message, why.c_str(), 255);
        message[255] = 0;
    }
    return rc;
}

}  // extern "C"
