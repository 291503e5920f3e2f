// OpenEXR input (include/mcrt.h "OpenEXR input"), the host's part in plain C++ (no HIP: tests/emu/exr_read_emu.cpp and
// tests/emu/exr_read_main.cpp compile it as it is): the header's parse and validation, the offset table, the chunks' checks, the inflate
// fan-out over host threads into the payload buffer of csrc/mcrt_exr_read.hpp, the per-chunk flags, and the validation of a load's
// targets. Every byte of the file is read through ExrFile::bytes(), which refuses a range outside the file's size: nothing here indexes
// by a number the file gave without that check. No FP64 value is made here.
// zlib is not linked: uncompress is looked up in MCRT_EXR_LIBZ at the first load that has a chunk to inflate - a lookup of its own,
// the save's (csrc/mcrt_exr_file.hpp) is untouched.
#pragma once

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mcrt_exr_read.hpp"
#include "mcrt_exr_read_launch.hpp"

#ifndef MCRT_EXR_LIBZ
#define MCRT_EXR_LIBZ "libz.so.1"
#endif

namespace mcrt {

constexpr uint32_t kExrReadZipLines = 16;       // scan lines of a ZIP chunk
constexpr uint32_t kExrReadMaxThreads = 16;     // inflate threads, whatever the host has
constexpr uint32_t kExrReadMaxFileChannels = 65536;
constexpr uint32_t kExrReadMaxName = 255;
constexpr uint64_t kExrReadMaxInflate = 1032;   // deflate cannot shrink its input further: a stored size below raw / 1032 is no deflate stream's
constexpr uint64_t kExrReadPayloadPad = 32;     // readable bytes behind the payloads (the kernels' whole-word loads)

using ExrUncompress = int (*)(unsigned char*, unsigned long*, const unsigned char*, unsigned long);
// The system's zlib, loaded once; nullptr when it is not there
inline ExrUncompress exrReadZlib() {
    static const ExrUncompress f = [] {
        void* h = dlopen(MCRT_EXR_LIBZ, RTLD_NOW | RTLD_LOCAL);
        return h ? (ExrUncompress)dlsym(h, "uncompress") : (ExrUncompress) nullptr;
    }();
    return f;
}

struct ExrFileChannel {
    std::string name;
    uint32_t pixel_type, bytes;
    uint64_t line_at;   // where its W values start within a scan line's bytes
};
struct ExrFileAttribute {
    std::string name, type;
    std::vector<unsigned char> value;
};

// An open file: the parsed header and the offset table
struct ExrFile {
    int fd = -1;
    std::string path;
    uint64_t file_bytes = 0;
    std::vector<ExrFileChannel> channels;
    std::vector<ExrFileAttribute> attributes;
    int32_t data_window[4] = {0, 0, 0, 0}, display_window[4] = {0, 0, 0, 0};
    uint32_t width = 0, height = 0, compression = 0, line_order = 0, lines_per_chunk = 1, chunks = 0;
    uint64_t line_bytes = 0, chunk_bytes = 0, total_bytes = 0;
    uint64_t table_at = 0;   // where the offset table starts: the header's bytes
    std::vector<uint64_t> offsets;
    ExrFile() = default;
    ExrFile(const ExrFile&) = delete;
    ExrFile& operator=(const ExrFile&) = delete;
    ~ExrFile() {
        if (fd >= 0) close(fd);
    }
    // n bytes from position `at` of the file; false when the range is not inside the file or cannot be read
    bool bytes(uint64_t at, void* dst, uint64_t n) const {
        if (at > file_bytes || n > file_bytes - at) return false;
        unsigned char* d = (unsigned char*)dst;
        while (n) {
            const ssize_t got = pread(fd, d, (size_t)std::min<uint64_t>(n, 1u << 30), (off_t)at);
            if (got <= 0) return false;
            d += got, at += (uint64_t)got, n -= (uint64_t)got;
        }
        return true;
    }
    uint64_t chunkBytes(uint64_t k) const { return std::min(chunk_bytes, total_bytes - k * chunk_bytes); }
};

namespace exr_read_detail {
inline uint32_t get32(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t get64(const unsigned char* p) { return (uint64_t)get32(p) | (uint64_t)get32(p + 4) << 32; }

// The file's first bytes, fetched as the parse asks for them
struct Head {
    const ExrFile& file;
    std::vector<unsigned char> buf;
    explicit Head(const ExrFile& f) : file(f) {}
    bool need(uint64_t end) {  // bytes [0, end) are in buf
        if (end <= buf.size()) return true;
        if (end > file.file_bytes) return false;
        const uint64_t have = buf.size(), want = std::min<uint64_t>(file.file_bytes, std::max<uint64_t>(end, have + 65536));
        buf.resize((size_t)want);
        if (!file.bytes(have, buf.data() + have, want - have)) {
            buf.resize((size_t)have);
            return false;
        }
        return true;
    }
    // A \0-terminated name of 1 .. kExrReadMaxName bytes at `at`; 0: fine, 1: the file ends first, 2: empty or too long
    int name(uint64_t& at, std::string& out) {
        out.clear();
        for (;;) {
            if (!need(at + 1)) return 1;
            const unsigned char c = buf[(size_t)at++];
            if (!c) return out.empty() ? 2 : 0;
            if (out.size() >= kExrReadMaxName) return 2;
            out.push_back((char)c);
        }
    }
};
}  // namespace exr_read_detail

// Opens path, parses and validates the header, reads the offset table
inline int exrReadOpen(const char* path, ExrFile& file, std::string& why) {
    using namespace exr_read_detail;
    const auto refuse = [&why](int code, const std::string& w) { why = w; return code; };
    if (!path) return refuse(MCRT_ERR_INVALID, "path is NULL");
    file.path = path;
    file.fd = open(path, O_RDONLY | O_CLOEXEC);
    struct stat st;
    if (file.fd < 0 || fstat(file.fd, &st) != 0 || !S_ISREG(st.st_mode)) return refuse(MCRT_ERR_IO, file.path + " could not be opened as a file");
    file.file_bytes = (uint64_t)st.st_size;
    Head head(file);
    if (!head.need(8)) return refuse(MCRT_ERR_IO, file.path + ": the file ends within the magic number and version");
    if (get32(head.buf.data()) != 0x01312f76u) return refuse(MCRT_ERR_IO, file.path + ": not an OpenEXR file (wrong magic number)");
    const uint32_t version = get32(head.buf.data() + 4);
    if (version & 0x200u) return refuse(MCRT_ERR_UNSUPPORTED, file.path + ": a tiled file (version bit 0x200)");
    if (version & 0x800u) return refuse(MCRT_ERR_UNSUPPORTED, file.path + ": a deep-data file (version bit 0x800)");
    if (version & 0x1000u) return refuse(MCRT_ERR_UNSUPPORTED, file.path + ": a multi-part file (version bit 0x1000)");
    if ((version & ~0x400u) != 2u) return refuse(MCRT_ERR_UNSUPPORTED, file.path + ": version field " + std::to_string(version) + ", not 2 (or 2 with the long-names bit 0x400)");

    bool have_channels = false, have_compression = false, have_data = false, have_display = false, have_order = false;
    uint64_t at = 8;
    for (;;) {
        const std::string where = file.path + ": attribute " + std::to_string(file.attributes.size());
        if (!head.need(at + 1)) return refuse(MCRT_ERR_IO, where + ": the file ends within the header");
        if (head.buf[(size_t)at] == 0) {
            at++;
            break;
        }
        ExrFileAttribute a;
        if (int bad = head.name(at, a.name)) return refuse(MCRT_ERR_IO, where + (bad == 1 ? ": the file ends within its name" : ": a name is 1 .. 255 bytes"));
        if (int bad = head.name(at, a.type)) return refuse(MCRT_ERR_IO, where + " (" + a.name + ")" + (bad == 1 ? ": the file ends within its type" : ": a type name is 1 .. 255 bytes"));
        if (!head.need(at + 4)) return refuse(MCRT_ERR_IO, where + " (" + a.name + "): the file ends within its size");
        const int32_t size = (int32_t)get32(head.buf.data() + at);
        at += 4;
        if (size < 0) return refuse(MCRT_ERR_IO, where + " (" + a.name + "): size " + std::to_string(size) + " is negative");
        if (!head.need(at + (uint64_t)size)) return refuse(MCRT_ERR_IO, where + " (" + a.name + "): its " + std::to_string(size) + " bytes run past the end of the file");
        a.value.assign(head.buf.begin() + (size_t)at, head.buf.begin() + (size_t)(at + (uint64_t)size));
        at += (uint64_t)size;
        const unsigned char* v = a.value.data();
        const auto typed = [&](const char* type, int32_t want) { return a.type == type && (want < 0 || size == want); };
        if (a.name == "channels") {
            if (have_channels || !typed("chlist", -1)) return refuse(MCRT_ERR_IO, where + ": channels is given twice or is not a chlist");
            have_channels = true;
            size_t q = 0;
            const size_t n = a.value.size();
            for (;;) {
                const std::string ch = file.path + ": channel " + std::to_string(file.channels.size());
                if (q >= n) return refuse(MCRT_ERR_IO, ch + ": the channel list is cut short");
                if (v[q] == 0) {
                    if (q + 1 != n) return refuse(MCRT_ERR_IO, ch + ": the channel list does not end where its size says");
                    break;
                }
                ExrFileChannel c;
                while (q < n && v[q]) c.name.push_back((char)v[q++]);
                if (q >= n) return refuse(MCRT_ERR_IO, ch + ": the channel list ends within a name");
                if (c.name.size() > kExrReadMaxName) return refuse(MCRT_ERR_IO, ch + ": a name is 1 .. 255 bytes");
                q++;
                if (n - q < 16) return refuse(MCRT_ERR_IO, ch + " (" + c.name + "): the channel list is cut short");
                c.pixel_type = get32(v + q);
                const int32_t xs = (int32_t)get32(v + q + 8), ys = (int32_t)get32(v + q + 12);  // (pLinear and the reserved bytes are ignored)
                q += 16;
                if (c.pixel_type > MCRT_EXR_FLOAT) return refuse(MCRT_ERR_IO, ch + " (" + c.name + "): pixelType " + std::to_string(c.pixel_type) + " is none of UINT, HALF, FLOAT");
                if (xs != 1 || ys != 1)
                    return refuse(MCRT_ERR_UNSUPPORTED, ch + " (" + c.name + "): a subsampled channel (xSampling " + std::to_string(xs) + ", ySampling " + std::to_string(ys) + ")");
                c.bytes = c.pixel_type == MCRT_EXR_HALF ? 2u : 4u;
                c.line_at = 0;
                if (file.channels.size() >= kExrReadMaxFileChannels) return refuse(MCRT_ERR_IO, file.path + ": more than 65536 channels");
                file.channels.push_back(std::move(c));
            }
            if (file.channels.empty()) return refuse(MCRT_ERR_IO, file.path + ": the channel list is empty");
        } else if (a.name == "compression") {
            if (have_compression || !typed("compression", 1)) return refuse(MCRT_ERR_IO, where + ": compression is given twice or is not one byte of type compression");
            have_compression = true;
            file.compression = v[0];
        } else if (a.name == "dataWindow" || a.name == "displayWindow") {
            bool& have = a.name == "dataWindow" ? have_data : have_display;
            if (have || !typed("box2i", 16)) return refuse(MCRT_ERR_IO, where + ": " + a.name + " is given twice or is not a box2i of 16 bytes");
            have = true;
            int32_t* w = a.name == "dataWindow" ? file.data_window : file.display_window;
            for (int i = 0; i < 4; i++) w[i] = (int32_t)get32(v + 4 * i);
        } else if (a.name == "lineOrder") {
            if (have_order || !typed("lineOrder", 1) || v[0] > 2) return refuse(MCRT_ERR_IO, where + ": lineOrder is given twice or is not one byte 0, 1 or 2 of type lineOrder");
            have_order = true;
            file.line_order = v[0];
        }
        file.attributes.push_back(std::move(a));
    }
    for (const auto& need : {std::make_pair("channels", have_channels), std::make_pair("compression", have_compression), std::make_pair("dataWindow", have_data),
                             std::make_pair("displayWindow", have_display), std::make_pair("lineOrder", have_order)})
        if (!need.second) return refuse(MCRT_ERR_IO, file.path + ": the header has no " + need.first);
    if (file.compression != MCRT_EXR_COMPRESSION_NONE && file.compression != MCRT_EXR_COMPRESSION_ZIPS && file.compression != MCRT_EXR_COMPRESSION_ZIP)
        return refuse(MCRT_ERR_UNSUPPORTED, file.path + ": compression " + std::to_string(file.compression) + " (NONE 0, ZIPS 2 and ZIP 3 are read)");
    {
        std::vector<const std::string*> names;
        for (const ExrFileChannel& c : file.channels) names.push_back(&c.name);
        std::sort(names.begin(), names.end(), [](const std::string* a, const std::string* b) { return *a < *b; });
        for (size_t i = 1; i < names.size(); i++)
            if (*names[i - 1] == *names[i]) return refuse(MCRT_ERR_IO, file.path + ": two channels are named " + *names[i]);
    }
    const int64_t w = (int64_t)file.data_window[2] - file.data_window[0] + 1, h = (int64_t)file.data_window[3] - file.data_window[1] + 1;
    if (w < 1 || h < 1) return refuse(MCRT_ERR_IO, file.path + ": the data window is empty (xMax < xMin or yMax < yMin)");
    if ((uint64_t)w * (uint64_t)h > 0xFFFFFFFFull) return refuse(MCRT_ERR_IO, file.path + ": a data window of 2^32 pixels or more");
    file.width = (uint32_t)w;
    file.height = (uint32_t)h;
    uint64_t line = 0;
    for (ExrFileChannel& c : file.channels) {
        c.line_at = line;
        line += (uint64_t)file.width * c.bytes;
    }
    file.line_bytes = line;
    file.lines_per_chunk = file.compression == MCRT_EXR_COMPRESSION_ZIP ? kExrReadZipLines : 1u;
    file.chunk_bytes = file.line_bytes * file.lines_per_chunk;
    file.total_bytes = file.line_bytes * file.height;
    file.chunks = (file.height + file.lines_per_chunk - 1) / file.lines_per_chunk;
    if (!head.need(at + 8ull * file.chunks)) return refuse(MCRT_ERR_IO, file.path + ": the offset table of " + std::to_string(file.chunks) + " chunks is cut short");
    file.table_at = at;
    file.offsets.resize(file.chunks);
    for (uint32_t k = 0; k < file.chunks; k++) {
        const uint64_t o = get64(head.buf.data() + at + 8ull * k);
        if (o < at + 8ull * file.chunks || o > file.file_bytes || file.file_bytes - o < 8)
            return refuse(MCRT_ERR_IO, file.path + ": offset " + std::to_string(o) + " of chunk " + std::to_string(k) + " is outside the file's chunk area");
        file.offsets[k] = o;
    }
    return MCRT_OK;
}

// A chunk as its eight leading bytes and the header give it
struct ExrChunkPlace {
    uint64_t data_at;      // file position of its data
    uint32_t stored;       // bytes of data in the file
    uint32_t transformed;  // 1: deflated (inflate gives ZIP's transformed order u), 0: raw bytes
};

// Every chunk's leading bytes against the header: y, size, the end of the file. raw_chunks: the chunks stored as raw bytes.
inline int exrReadChunkPlaces(const ExrFile& file, std::vector<ExrChunkPlace>& places, uint32_t* raw_chunks, std::string& why) {
    using namespace exr_read_detail;
    const auto refuse = [&why](int code, const std::string& w) { why = w; return code; };
    places.resize(file.chunks);
    uint32_t raws = 0;
    bool inflate = false;
    for (uint32_t k = 0; k < file.chunks; k++) {
        const std::string where = file.path + ": chunk " + std::to_string(k) + " at " + std::to_string(file.offsets[k]);
        unsigned char lead[8];
        if (!file.bytes(file.offsets[k], lead, 8)) return refuse(MCRT_ERR_IO, where + ": its leading bytes could not be read");
        const int64_t y = (int32_t)get32(lead), want_y = (int64_t)file.data_window[1] + (int64_t)k * file.lines_per_chunk;
        const int64_t size = (int32_t)get32(lead + 4);
        const uint64_t n = file.chunkBytes(k);
        if (y != want_y) return refuse(MCRT_ERR_IO, where + ": its y is " + std::to_string(y) + ", its slot's " + std::to_string(want_y));
        if (size < 0) return refuse(MCRT_ERR_IO, where + ": size " + std::to_string(size) + " is negative");
        if ((uint64_t)size > n) return refuse(MCRT_ERR_IO, where + ": size " + std::to_string(size) + " is larger than its raw size " + std::to_string(n));
        if (file.compression == MCRT_EXR_COMPRESSION_NONE && (uint64_t)size != n)
            return refuse(MCRT_ERR_IO, where + ": size " + std::to_string(size) + " of an uncompressed chunk is not its raw size " + std::to_string(n));
        const uint64_t data_at = file.offsets[k] + 8;
        if ((uint64_t)size > file.file_bytes - data_at) return refuse(MCRT_ERR_IO, where + ": its " + std::to_string(size) + " bytes run past the end of the file");
        const bool deflated = (uint64_t)size < n;
        if (deflated && n > (uint64_t)size * kExrReadMaxInflate)
            return refuse(MCRT_ERR_IO, where + ": " + std::to_string(size) + " stored bytes cannot inflate to its raw size " + std::to_string(n));
        places[k] = ExrChunkPlace{data_at, (uint32_t)size, deflated ? 1u : 0u};
        raws += deflated ? 0u : 1u;
        inflate = inflate || deflated;
    }
    if (inflate && !exrReadZlib())
        return refuse(MCRT_ERR_UNSUPPORTED, file.path + ": its deflated chunks need " MCRT_EXR_LIBZ " (uncompress), which could not be loaded; uncompressed files and raw chunks load without it");
    if (raw_chunks) *raw_chunks = raws;
    return MCRT_OK;
}

inline uint32_t exrReadThreads(const mcrt_exr_load_params* params, uint32_t chunks) {
    const uint32_t asked = params && params->threads ? params->threads : std::max(1u, std::thread::hardware_concurrency());
    return std::max(1u, std::min(std::min(asked, kExrReadMaxThreads), chunks));
}

// The bytes of the buffer that crosses to the device: the payloads, the pad, a flag per chunk
inline uint64_t exrReadFlagsAt(const ExrFile& file) { return (file.total_bytes + kExrReadPayloadPad + 15) / 16 * 16; }
inline uint64_t exrReadUploadBytes(const ExrFile& file) { return exrReadFlagsAt(file) + 4ull * file.chunks; }

// The chunks into `upload` (exrReadUploadBytes(file) bytes): chunk k's payload at k * chunk_bytes - a raw chunk's bytes as they are, a
// deflated one's inflated in place, still in ZIP's transformed order -, the flags at exrReadFlagsAt(file). Chunks are independent: each
// thread takes the next one.
inline int exrReadPayloads(const ExrFile& file, const std::vector<ExrChunkPlace>& places, uint32_t threads, unsigned char* upload, std::string& why) {
    memset(upload + file.total_bytes, 0, (size_t)(exrReadFlagsAt(file) - file.total_bytes));
    uint32_t* flags = (uint32_t*)(upload + exrReadFlagsAt(file));
    const ExrUncompress uncompress = exrReadZlib();
    std::atomic<uint32_t> next{0};
    std::atomic<bool> failed{false};
    std::mutex first;
    const auto fail = [&](const std::string& w) {
        std::lock_guard<std::mutex> lock(first);
        if (!failed.exchange(true)) why = w;
    };
    const auto work = [&]() {
        std::vector<unsigned char> stored;
        for (uint32_t k; !failed.load() && (k = next.fetch_add(1)) < file.chunks;) {
            const ExrChunkPlace& c = places[k];
            const uint64_t n = file.chunkBytes(k);
            unsigned char* dst = upload + (uint64_t)k * file.chunk_bytes;
            const std::string where = file.path + ": chunk " + std::to_string(k);
            flags[k] = c.transformed;
            if (!c.transformed) {
                if (!file.bytes(c.data_at, dst, n)) fail(where + ": its bytes could not be read");
                continue;
            }
            stored.resize(c.stored);
            if (!file.bytes(c.data_at, stored.data(), c.stored)) {
                fail(where + ": its bytes could not be read");
                continue;
            }
            unsigned long got = (unsigned long)n;
            if (!uncompress || uncompress(dst, &got, stored.data(), (unsigned long)c.stored) != 0 || got != n)
                fail(where + ": its " + std::to_string(c.stored) + " bytes do not inflate to its raw size " + std::to_string(n));
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < threads; t++) pool.emplace_back(work);
    work();
    for (std::thread& t : pool) t.join();
    return failed.load() ? MCRT_ERR_IO : MCRT_OK;
}

// A load's targets, validated: the table the kernels read, data as the caller gave it
inline int exrReadPlan(const ExrFile& file, const mcrt_exr_target* targets, uint32_t count, const mcrt_exr_load_params* params, std::vector<ExrReadTarget>& table,
                       std::string& why) {
    const auto refuse = [&why](int code, const std::string& w) { why = w; return code; };
    if (!targets) return refuse(MCRT_ERR_INVALID, "the target array is NULL");
    if (count == 0 || count > MCRT_EXR_MAX_CHANNELS) return refuse(MCRT_ERR_INVALID, "1 .. 1024 targets");
    if (params && params->flags) return refuse(MCRT_ERR_INVALID, "unknown flags");
    const uint64_t pixels = (uint64_t)file.width * file.height;
    table.resize(count);
    struct Span {
        uintptr_t first, pitch;  // address of pixel 0's element, bytes from pixel to pixel
        uint32_t element;
    };
    std::vector<Span> spans(count);
    for (uint32_t i = 0; i < count; i++) {
        const mcrt_exr_target& t = targets[i];
        const std::string at = "target " + std::to_string(i);
        if (!t.name) return refuse(MCRT_ERR_INVALID, at + ": name is NULL");
        const ExrFileChannel* c = nullptr;
        for (const ExrFileChannel& fc : file.channels)
            if (fc.name == t.name) c = &fc;
        if (!c) return refuse(MCRT_ERR_INVALID, at + ": the file holds no channel named " + t.name);
        if (!t.data) return refuse(MCRT_ERR_INVALID, at + " (" + t.name + "): data is NULL");
        if (t.stride == 0 || t.offset >= t.stride) return refuse(MCRT_ERR_INVALID, at + " (" + t.name + "): stride 0 or offset >= stride");
        if (t.reserved) return refuse(MCRT_ERR_INVALID, at + " (" + t.name + "): reserved is not 0");
        const bool pair = (t.dest_type == MCRT_EXR_SRC_F64 && (c->pixel_type == MCRT_EXR_HALF || c->pixel_type == MCRT_EXR_FLOAT)) ||
                          (t.dest_type == MCRT_EXR_SRC_U32 && c->pixel_type == MCRT_EXR_UINT);
        if (!pair) return refuse(MCRT_ERR_INVALID, at + " (" + t.name + "): HALF and FLOAT go to F64, UINT to U32");
        table[i] = ExrReadTarget{t.data, c->line_at, t.stride, t.offset, c->pixel_type, c->bytes};
        const uint32_t element = t.dest_type == MCRT_EXR_SRC_U32 ? 4u : 8u;
        spans[i] = Span{(uintptr_t)t.data + (uintptr_t)t.offset * element, (uintptr_t)t.stride * element, element};
    }
    // Two targets writing one element. Targets of one pitch interleave (R, G, B of one frame): their elements meet when the distance of
    // their first ones, modulo the pitch, is less than an element, within the frame's length. Targets of different pitch may not share bytes.
    for (uint32_t i = 0; i < count; i++)
        for (uint32_t j = 0; j < i; j++) {
            const Span &a = spans[i], &b = spans[j];
            const uintptr_t a_end = a.first + (uintptr_t)(pixels - 1) * a.pitch + a.element, b_end = b.first + (uintptr_t)(pixels - 1) * b.pitch + b.element;
            if (a.first >= b_end || b.first >= a_end) continue;
            bool meet = true;
            if (a.pitch == b.pitch) {
                const uintptr_t m = (a.first >= b.first ? a.first - b.first : b.first - a.first) % a.pitch;
                const uint32_t lo = a.first >= b.first ? b.element : a.element, hi = a.first >= b.first ? a.element : b.element;
                meet = m < lo || a.pitch - m < hi;
            }
            if (meet)
                return refuse(MCRT_ERR_INVALID, "targets " + std::to_string(j) + " (" + targets[j].name + ") and " + std::to_string(i) + " (" + targets[i].name +
                                                    ") write the same elements, or share memory at different strides");
        }
    return MCRT_OK;
}

// The kernels' (or the emulation's) arguments of a file: `table` the targets where the lanes can read them, `upload` the buffer of
// exrReadPayloads, `plane` exrReadPlaneBytes(file) bytes, `tile_sums` exrReadTileSumWords(file) words.
inline uint64_t exrReadPlaneBytes(const ExrFile& file) { return (uint64_t)file.chunks * exrReadTilesPerChunk(file.chunk_bytes) * kExrReadTileBytes; }
inline uint64_t exrReadTileSumWords(const ExrFile& file) { return (uint64_t)file.chunks * exrReadTilesPerChunk(file.chunk_bytes); }
inline ExrRead exrReadOf(const ExrFile& file, const ExrReadTarget* table, uint32_t count, const unsigned char* upload, unsigned char* plane, uint32_t* tile_sums) {
    ExrRead rd;
    rd.table = table;
    rd.payload = upload;
    rd.flags = (const uint32_t*)(upload + exrReadFlagsAt(file));
    rd.plane = plane;
    rd.tile_sums = tile_sums;
    rd.line_bytes = file.line_bytes;
    rd.chunk_bytes = file.chunk_bytes;
    rd.total_bytes = file.total_bytes;
    rd.tiles_per_chunk = (uint32_t)std::min<uint64_t>(exrReadTilesPerChunk(file.chunk_bytes), 0xFFFFFFFFull);
    rd.plane_pitch = (uint64_t)rd.tiles_per_chunk * kExrReadTileBytes;
    rd.pixels = (uint64_t)file.width * file.height;
    rd.width = file.width;
    rd.height = file.height;
    rd.count = count;
    rd.lines_per_chunk = file.lines_per_chunk;
    rd.chunks = file.chunks;
    rd.blocks_per_target = (uint32_t)exrReadBlocksPerTarget(rd.pixels);
    rd.reserved = 0;
    return rd;
}

}  // namespace mcrt
