// OpenEXR output (include/mcrt.h "OpenEXR output"), the host's part in plain C++ (no HIP: tests/emu/exr_emu.cpp and
// tests/emu/exr_file_main.cpp compile it as it is): validation, the name sort, the header's bytes, the chunk table, the deflate fan-out
// over host threads, the raw-chunk rule and the file write. What comes in is the packed buffer of csrc/mcrt_exr.hpp - the chunks' payloads
// in file order (NONE) or in ZIP's pre-deflate order - from the kernel (csrc/mcrt_exr_host.hip) or from the emulation.
// zlib is not linked: compress2 and compressBound are looked up in MCRT_EXR_LIBZ at the first ZIP save.
#pragma once

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "mcrt_exr.hpp"

#ifndef MCRT_EXR_LIBZ
#define MCRT_EXR_LIBZ "libz.so.1"
#endif

namespace mcrt {

constexpr uint32_t kExrZipLines = 16;      // scan lines of a ZIP chunk
constexpr uint32_t kExrMaxThreads = 16;    // deflate threads, whatever the host has
constexpr uint32_t kExrDefaultZipLevel = 4;

struct ExrZlib {
    int (*compress2)(unsigned char*, unsigned long*, const unsigned char*, unsigned long, int) = nullptr;
    unsigned long (*compressBound)(unsigned long) = nullptr;
};
// The system's zlib, loaded once; nullptr when it is not there
inline const ExrZlib* exrZlib() {
    static const ExrZlib z = [] {
        ExrZlib f;
        if (void* h = dlopen(MCRT_EXR_LIBZ, RTLD_NOW | RTLD_LOCAL)) {
            f.compress2 = (decltype(f.compress2))dlsym(h, "compress2");
            f.compressBound = (decltype(f.compressBound))dlsym(h, "compressBound");
        }
        return f;
    }();
    return z.compress2 && z.compressBound ? &z : nullptr;
}

// A save, validated and laid out: the sorted channels (data: the caller's pointers), the settings, the geometry of the packed buffer and
// the header's bytes.
struct ExrPlan {
    std::vector<ExrChannelRec> table;
    std::vector<uint32_t> order;   // table[i] is the caller's channel order[i]
    uint32_t compression = MCRT_EXR_COMPRESSION_ZIP, zip_level = kExrDefaultZipLevel, threads = 1, flags = 0;
    uint32_t width = 0, height = 0, lines_per_chunk = 1, chunks = 0;
    uint64_t line_bytes = 0, chunk_bytes = 0, total_bytes = 0;
    std::vector<unsigned char> header;  // magic .. the \0 that ends the attributes
};

namespace exr_detail {
inline void put32(std::vector<unsigned char>& b, uint32_t v) {
    for (int i = 0; i < 4; i++) b.push_back((unsigned char)(v >> (8 * i)));
}
inline void putStr(std::vector<unsigned char>& b, const char* s) { b.insert(b.end(), (const unsigned char*)s, (const unsigned char*)s + strlen(s) + 1); }
inline void putAttr(std::vector<unsigned char>& b, const char* name, const char* type, uint32_t size) {
    putStr(b, name);
    putStr(b, type);
    put32(b, size);
}
inline bool shortName(const char* s, size_t most = 31) {
    if (!s) return false;
    size_t n = 0;
    for (; s[n]; n++)
        if (n >= most || (unsigned char)s[n] < 0x20 || (unsigned char)s[n] > 0x7e) return false;
    return n >= 1;
}
inline const char* const kStandardAttributes[] = {"channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter", "screenWindowWidth"};
}  // namespace exr_detail

inline int exrPlan(const char* path, uint32_t width, uint32_t height, const mcrt_exr_channel* channels, uint32_t count, const mcrt_exr_attribute* attributes,
                   uint32_t attribute_count, const mcrt_exr_params* params, ExrPlan& plan, std::string& why) {
    using namespace exr_detail;
    const auto refuse = [&why](int code, const std::string& w) { why = w; return code; };
    if (!path) return refuse(MCRT_ERR_INVALID, "path is NULL");
    if (!channels) return refuse(MCRT_ERR_INVALID, "the channel array is NULL");
    if (count == 0 || count > MCRT_EXR_MAX_CHANNELS) return refuse(MCRT_ERR_INVALID, "1 .. 1024 channels");
    const uint64_t pixels = (uint64_t)width * height;
    if (pixels == 0 || pixels > 0xFFFFFFFFull) return refuse(MCRT_ERR_INVALID, "width * height must be non-zero and below 2^32");
    // (the flags are read before the names they bound; they are checked with the other parameters below)
    const bool long_names = params && (params->flags & MCRT_EXR_LONG_NAMES);
    for (uint32_t i = 0; i < count; i++) {
        const mcrt_exr_channel& c = channels[i];
        const std::string at = "channel " + std::to_string(i);
        if (!shortName(c.name, long_names ? 255 : 31))
            return refuse(MCRT_ERR_INVALID, at + (long_names ? ": a name is 1 .. 255 bytes of printable ASCII" : ": a name is 1 .. 31 bytes of printable ASCII"));
        if (!c.data) return refuse(MCRT_ERR_INVALID, at + " (" + c.name + "): data is NULL");
        if (c.stride == 0 || c.offset >= c.stride) return refuse(MCRT_ERR_INVALID, at + " (" + c.name + "): stride 0 or offset >= stride");
        const bool pair = (c.source_type == MCRT_EXR_SRC_F64 && (c.pixel_type == MCRT_EXR_HALF || c.pixel_type == MCRT_EXR_FLOAT)) ||
                          (c.source_type == MCRT_EXR_SRC_U32 && c.pixel_type == MCRT_EXR_UINT);
        if (!pair) return refuse(MCRT_ERR_INVALID, at + " (" + c.name + "): F64 goes to HALF or FLOAT, U32 to UINT");
    }
    plan.order.resize(count);
    for (uint32_t i = 0; i < count; i++) plan.order[i] = i;
    std::sort(plan.order.begin(), plan.order.end(), [channels](uint32_t a, uint32_t b) { return strcmp(channels[a].name, channels[b].name) < 0; });
    for (uint32_t i = 1; i < count; i++)
        if (!strcmp(channels[plan.order[i - 1]].name, channels[plan.order[i]].name))
            return refuse(MCRT_ERR_INVALID, std::string("two channels are named ") + channels[plan.order[i]].name);
    if (params) {
        if (params->compression) {
            const uint32_t c = params->compression & ~MCRT_EXR_COMPRESSION_SET;
            if (!(params->compression & MCRT_EXR_COMPRESSION_SET) || (c != MCRT_EXR_COMPRESSION_NONE && c != MCRT_EXR_COMPRESSION_ZIP))
                return refuse(MCRT_ERR_INVALID, "compression is 0 or MCRT_EXR_COMPRESSION_SET | NONE or ZIP");
            plan.compression = c;
        }
        if (params->zip_level > 9) return refuse(MCRT_ERR_INVALID, "zip_level is 1 .. 9");
        if (params->zip_level) plan.zip_level = params->zip_level;
        if (params->flags & ~(MCRT_EXR_HALF_INF | MCRT_EXR_LONG_NAMES)) return refuse(MCRT_ERR_INVALID, "unknown flags");
        plan.flags = params->flags;
    }
    if (attribute_count && !attributes) return refuse(MCRT_ERR_INVALID, "the attribute array is NULL");
    for (uint32_t i = 0; i < attribute_count; i++) {
        const std::string at = "attribute " + std::to_string(i);
        if (!shortName(attributes[i].name) || !attributes[i].value) return refuse(MCRT_ERR_INVALID, at + ": a name of 1 .. 31 bytes of printable ASCII and a value");
        for (const char* s : kStandardAttributes)
            if (!strcmp(s, attributes[i].name)) return refuse(MCRT_ERR_INVALID, at + ": " + s + " is a standard attribute");
        for (uint32_t j = 0; j < i; j++)
            if (!strcmp(attributes[j].name, attributes[i].name)) return refuse(MCRT_ERR_INVALID, at + ": " + attributes[i].name + " is given twice");
    }
    if (plan.compression == MCRT_EXR_COMPRESSION_ZIP && !exrZlib())
        return refuse(MCRT_ERR_UNSUPPORTED, "ZIP compression needs " MCRT_EXR_LIBZ " (compress2, compressBound), which could not be loaded; MCRT_EXR_COMPRESSION_NONE works without it");

    plan.width = width;
    plan.height = height;
    plan.table.resize(count);
    uint64_t at = 0;
    for (uint32_t i = 0; i < count; i++) {
        const mcrt_exr_channel& c = channels[plan.order[i]];
        const uint32_t bytes = c.pixel_type == MCRT_EXR_HALF ? 2u : 4u;
        plan.table[i] = ExrChannelRec{c.data, at, c.stride, c.offset, c.pixel_type, bytes};
        at += (uint64_t)width * bytes;
    }
    plan.line_bytes = at;
    plan.lines_per_chunk = plan.compression == MCRT_EXR_COMPRESSION_ZIP ? kExrZipLines : 1u;
    plan.chunk_bytes = plan.line_bytes * plan.lines_per_chunk;
    plan.total_bytes = plan.line_bytes * height;
    plan.chunks = (height + plan.lines_per_chunk - 1) / plan.lines_per_chunk;
    uint32_t threads = params && params->threads ? params->threads : std::max(1u, std::thread::hardware_concurrency());
    plan.threads = std::max(1u, std::min(std::min(threads, kExrMaxThreads), plan.chunks));

    std::vector<unsigned char>& h = plan.header;
    const unsigned char magic[8] = {0x76, 0x2f, 0x31, 0x01, 0x02, 0x00, 0x00, 0x00};
    h.assign(magic, magic + 8);
    if (long_names) h[5] = 0x04;  // version bit 0x400: names of up to 255 bytes
    uint32_t chlist = 1;
    for (uint32_t i = 0; i < count; i++) chlist += (uint32_t)strlen(channels[plan.order[i]].name) + 1 + 16;
    putAttr(h, "channels", "chlist", chlist);
    for (uint32_t i = 0; i < count; i++) {
        putStr(h, channels[plan.order[i]].name);
        put32(h, plan.table[i].pixel_type);
        put32(h, 0);  // pLinear 0 and three reserved bytes
        put32(h, 1);
        put32(h, 1);
    }
    h.push_back(0);
    putAttr(h, "compression", "compression", 1);
    h.push_back((unsigned char)plan.compression);
    for (const char* name : {"dataWindow", "displayWindow"}) {
        putAttr(h, name, "box2i", 16);
        put32(h, 0);
        put32(h, 0);
        put32(h, width - 1);
        put32(h, height - 1);
    }
    putAttr(h, "lineOrder", "lineOrder", 1);
    h.push_back(0);
    putAttr(h, "pixelAspectRatio", "float", 4);
    put32(h, 0x3f800000u);
    putAttr(h, "screenWindowCenter", "v2f", 8);
    put32(h, 0);
    put32(h, 0);
    putAttr(h, "screenWindowWidth", "float", 4);
    put32(h, 0x3f800000u);
    for (uint32_t i = 0; i < attribute_count; i++) {
        const size_t n = strlen(attributes[i].value);
        putAttr(h, attributes[i].name, "string", (uint32_t)n);
        h.insert(h.end(), (const unsigned char*)attributes[i].value, (const unsigned char*)attributes[i].value + n);
    }
    h.push_back(0);
    return MCRT_OK;
}

// The kernel's (or the emulation's) arguments of a plan: `table` the plan's table where the lanes can read it, its data pointers where
// the lanes can read the frames; `out` the packed buffer, exrPackedWords(...) * 4 bytes.
inline ExrPack exrPackOf(const ExrPlan& plan, const ExrChannelRec* table, unsigned char* out) {
    ExrPack pk;
    pk.table = table;
    pk.out = out;
    pk.line_bytes = plan.line_bytes;
    pk.chunk_bytes = plan.chunk_bytes;
    pk.total_bytes = plan.total_bytes;
    pk.width = plan.width;
    pk.height = plan.height;
    pk.count = (uint32_t)plan.table.size();
    pk.lines_per_chunk = plan.lines_per_chunk;
    pk.zip = plan.compression == MCRT_EXR_COMPRESSION_ZIP ? 1u : 0u;
    pk.flags = plan.flags;
    return pk;
}

// The raw bytes of a chunk back from its transformed ones (for the format's raw-chunk rule: rare)
inline void exrZipUndo(const unsigned char* u, size_t n, unsigned char* raw) {
    const size_t h = n / 2;
    unsigned char t = 0;
    for (size_t i = 0; i < n; i++) {
        t = i == 0 ? u[0] : (unsigned char)(t + u[i] - 128);
        raw[i < h ? 2 * i : 2 * (i - h) + 1] = t;
    }
}

// The file of a plan and its packed buffer. A partial file is removed.
inline int exrWriteFile(const char* path, const ExrPlan& plan, const unsigned char* packed, mcrt_exr_result* result, std::string& why) {
    const uint32_t chunks = plan.chunks;
    const bool zip = plan.compression == MCRT_EXR_COMPRESSION_ZIP;
    const auto chunkBytes = [&plan](uint32_t k) { return (size_t)std::min<uint64_t>(plan.chunk_bytes, plan.total_bytes - (uint64_t)k * plan.chunk_bytes); };
    std::vector<std::vector<unsigned char>> data(zip ? chunks : 0);
    std::atomic<uint32_t> next{0}, raw_chunks{0};
    if (zip) {
        const ExrZlib* z = exrZlib();
        if (!z) {
            why = "ZIP compression needs " MCRT_EXR_LIBZ;
            return MCRT_ERR_UNSUPPORTED;
        }
        const auto work = [&]() {  // chunks are independent: each thread takes the next one
            for (uint32_t k; (k = next.fetch_add(1)) < chunks;) {
                const size_t n = chunkBytes(k);
                const unsigned char* u = packed + (size_t)k * plan.chunk_bytes;
                std::vector<unsigned char>& d = data[k];
                d.resize(z->compressBound((unsigned long)n));
                unsigned long got = (unsigned long)d.size();
                if (z->compress2(d.data(), &got, u, (unsigned long)n, (int)plan.zip_level) == 0 && got < n) {
                    d.resize(got);
                } else {
                    d.resize(n);
                    exrZipUndo(u, n, d.data());
                    raw_chunks.fetch_add(1);
                }
            }
        };
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < plan.threads; t++) pool.emplace_back(work);
        work();
        for (std::thread& t : pool) t.join();
    }

    std::vector<unsigned char> head = plan.header;
    uint64_t at = head.size() + 8ull * chunks;
    for (uint32_t k = 0; k < chunks; k++) {
        for (int i = 0; i < 8; i++) head.push_back((unsigned char)(at >> (8 * i)));
        at += 8 + (zip ? data[k].size() : chunkBytes(k));
    }
    FILE* f = fopen(path, "wb");
    if (!f) {
        why = std::string(path) + " could not be created";
        return MCRT_ERR_IO;
    }
    bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
    for (uint32_t k = 0; ok && k < chunks; k++) {
        const unsigned char* d = zip ? data[k].data() : packed + (size_t)k * plan.chunk_bytes;
        const size_t n = zip ? data[k].size() : chunkBytes(k);
        std::vector<unsigned char> lead;
        exr_detail::put32(lead, k * plan.lines_per_chunk);
        exr_detail::put32(lead, (uint32_t)n);
        ok = fwrite(lead.data(), 1, 8, f) == 8 && fwrite(d, 1, n, f) == n;
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        remove(path);
        why = std::string(path) + " could not be written";
        return MCRT_ERR_IO;
    }
    if (result) {
        result->file_bytes = at;
        result->packed_bytes = plan.total_bytes;
        result->chunks = chunks;
        result->raw_chunks = raw_chunks.load();
    }
    return MCRT_OK;
}

// A whole save: plan, pack (pack(plan, &packed) leaves the packed buffer where the host reads it and returns a status), file.
template <class PackFn>
int exrSave(const char* path, uint32_t width, uint32_t height, const mcrt_exr_channel* channels, uint32_t count, const mcrt_exr_attribute* attributes,
            uint32_t attribute_count, const mcrt_exr_params* params, mcrt_exr_result* result, std::string& why, PackFn&& pack) {
    ExrPlan plan;
    if (int rc = exrPlan(path, width, height, channels, count, attributes, attribute_count, params, plan, why)) return rc;
    const unsigned char* packed = nullptr;
    if (int rc = pack(plan, &packed)) return rc;
    return exrWriteFile(path, plan, packed, result, why);
}

}  // namespace mcrt
