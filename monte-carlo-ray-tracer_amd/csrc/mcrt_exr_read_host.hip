// OpenEXR input (include/mcrt.h mcrt_exr_open .. mcrt_exr_load*), host side: the entry points. No kernel here: they are
// libmcrt_exr_read.so (csrc/mcrt_exr_read.hip; DESIGN.md "Image passes" says why); the parse, the chunks' checks, inflate and the
// targets' validation are csrc/mcrt_exr_read_file.hpp. A load reads and inflates the chunks into pinned memory, moves payloads and
// flags to the device in one copy, undoes the predictor of the transformed chunks (three launches, skipped when there is none) and
// gathers, widens and scatters (one launch). The host form first stages every distinct destination region on the device with its
// present bytes - an element no target names keeps them - and copies each back once.
// Scratch slots of the family (0 .. 2 are the save's): 3 the upload and the target table, 4 the plane and the tile sums, 5 the host
// form's staged destinations.
#include <algorithm>

#include "mcrt_pass_host.hpp"  // (the HIP runtime before the kernels' text)

#include "mcrt_exr_read_file.hpp"
#include "mcrt_exr_read_launch.hpp"

using namespace mcrt;

struct mcrt_exr_file {
    ExrFile file;
};

namespace {

struct PinnedBuffer {
    void* p = nullptr;
    ~PinnedBuffer() {
        if (p) (void)hipHostFree(p);
    }
};

// A region of host memory that targets write into, and its device copy
struct Region {
    uintptr_t first, end;
    unsigned char* dev;
};

int load(mcrt_ctx* ctx, const char* what, bool host_data, mcrt_exr_file* f, const mcrt_exr_target* targets, uint32_t count, const mcrt_exr_load_params* params,
         mcrt_exr_load_result* result, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, what)) return rc;
    if (!f) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": the file is NULL");
    PassTimer timer(ctx);
    const ExrFile& file = f->file;
    std::string why;
    std::vector<ExrReadTarget> table;
    if (int rc = exrReadPlan(file, targets, count, params, table, why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);
    std::vector<ExrChunkPlace> places;
    uint32_t raw_chunks = 0;
    if (int rc = exrReadChunkPlaces(file, places, &raw_chunks, why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);
    const bool transformed = raw_chunks < file.chunks;

    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const size_t upload_bytes = (size_t)exrReadUploadBytes(file), table_at = (upload_bytes + 15) / 16 * 16, table_bytes = table.size() * sizeof(ExrReadTarget);
    const size_t plane_bytes = transformed ? (size_t)exrReadPlaneBytes(file) : 0, sums_bytes = transformed ? (size_t)exrReadTileSumWords(file) * 4 : 0;
    const ExrRead shape = exrReadOf(file, nullptr, count, nullptr, nullptr, nullptr);
    if (exrReadGatherBlocks(shape) == 0 || (transformed && (exrReadTileBlocks(shape) == 0 || shape.tiles_per_chunk != exrReadTilesPerChunk(file.chunk_bytes))))
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": the load is past what one launch holds");
    unsigned char* d_upload = (unsigned char*)ctxPassScratch(ctx, kPassExr, 3, table_at + table_bytes);
    unsigned char* d_plane = (unsigned char*)ctxPassScratch(ctx, kPassExr, 4, plane_bytes + sums_bytes);
    PinnedBuffer host;
    if (!d_upload || !d_plane || hipHostMalloc(&host.p, upload_bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        host.p = nullptr;
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the payload buffers could not be allocated");
    }
    if (int rc = exrReadPayloads(file, places, exrReadThreads(params, file.chunks), (unsigned char*)host.p, why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);

    std::vector<Region> regions;
    if (host_data) {
        // the destinations' byte ranges, merged where they meet: each region is staged, and copied back, once
        const uint64_t pixels = shape.pixels;
        for (const ExrReadTarget& t : table) {
            const uintptr_t element = t.pixel_type == MCRT_EXR_UINT ? 4 : 8;
            const uintptr_t first = (uintptr_t)t.data + t.offset * element;
            regions.push_back(Region{first, first + (uintptr_t)((pixels - 1) * t.stride * element + element), nullptr});
        }
        std::sort(regions.begin(), regions.end(), [](const Region& a, const Region& b) { return a.first < b.first; });
        size_t kept = 0;
        for (size_t i = 1; i < regions.size(); i++) {
            if (regions[i].first <= regions[kept].end) regions[kept].end = std::max(regions[kept].end, regions[i].end);
            else regions[++kept] = regions[i];
        }
        regions.resize(kept + 1);
        size_t total = 0;
        std::vector<size_t> at(regions.size());
        for (size_t i = 0; i < regions.size(); i++) {  // (a region keeps its address modulo 8)
            at[i] = (total + 7) / 8 * 8 + (regions[i].first & 7u);
            total = at[i] + (regions[i].end - regions[i].first);
        }
        unsigned char* base = (unsigned char*)ctxPassScratch(ctx, kPassExr, 5, total);
        if (!base) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the destinations' device copy could not be allocated");
        for (size_t i = 0; i < regions.size(); i++) {
            regions[i].dev = base + at[i];
            MCRT_HIP_TRY(ctx, hipMemcpy(regions[i].dev, (const void*)regions[i].first, regions[i].end - regions[i].first, hipMemcpyHostToDevice));
        }
        for (ExrReadTarget& t : table) {
            const uintptr_t a = (uintptr_t)t.data;
            const Region* r = &regions[0];
            for (const Region& c : regions)
                if (c.first <= a + t.offset * (t.pixel_type == MCRT_EXR_UINT ? 4u : 8u)) r = &c;
            t.data = r->dev + (ptrdiff_t)(a - r->first);  // (data itself may lie before the region: only data + offset is in it)
        }
    }

    ExrReadTarget* d_table = (ExrReadTarget*)(d_upload + table_at);
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_upload, host.p, upload_bytes, hipMemcpyHostToDevice, stream));
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_table, table.data(), table_bytes, hipMemcpyHostToDevice, stream));
    MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));  // (the table is pageable host memory of this frame)
    const ExrRead rd = exrReadOf(file, d_table, count, d_upload, d_plane, (uint32_t*)(d_plane + plane_bytes));
    if (int rc = timer.begin(stream)) return rc;
    if (transformed) {
        MCRT_HIP_TRY(ctx, (hipError_t)launchExrReadSum(stream, rd));
        MCRT_HIP_TRY(ctx, (hipError_t)launchExrReadScan(stream, rd));
        MCRT_HIP_TRY(ctx, (hipError_t)launchExrReadUndo(stream, rd));
    }
    MCRT_HIP_TRY(ctx, (hipError_t)launchExrReadGather(stream, rd));
    if (int rc = timer.end(stream)) return rc;
    for (const Region& r : regions) MCRT_HIP_TRY(ctx, hipMemcpy((void*)r.first, r.dev, r.end - r.first, hipMemcpyDeviceToHost));
    if (result) {
        result->file_bytes = file.file_bytes;
        result->payload_bytes = file.total_bytes;
        result->chunks = file.chunks;
        result->raw_chunks = raw_chunks;
    }
    return timer.finish(stats, transformed ? 4 : 1);
}

}  // namespace

extern "C" int mcrt_exr_open(mcrt_ctx* ctx, const char* path, mcrt_exr_file** out) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (out) *out = nullptr;
    if (!path || !out) return ctxFail(ctx, MCRT_ERR_INVALID, "mcrt_exr_open: path or out is NULL");
    mcrt_exr_file* f = new mcrt_exr_file();
    std::string why;
    if (int rc = exrReadOpen(path, f->file, why)) {
        delete f;
        return ctxFail(ctx, rc, "mcrt_exr_open: " + why);
    }
    *out = f;
    return MCRT_OK;
}

extern "C" void mcrt_exr_close(mcrt_exr_file* f) { delete f; }

extern "C" int mcrt_exr_file_info(const mcrt_exr_file* f, mcrt_exr_info* info) {
    if (!f || !info) return MCRT_ERR_INVALID;
    const ExrFile& file = f->file;
    memset(info, 0, sizeof(*info));
    info->width = file.width;
    info->height = file.height;
    for (int i = 0; i < 4; i++) info->data_window[i] = file.data_window[i], info->display_window[i] = file.display_window[i];
    info->channels = (uint32_t)file.channels.size();
    info->attributes = (uint32_t)file.attributes.size();
    info->compression = file.compression;
    info->line_order = file.line_order;
    info->lines_per_chunk = file.lines_per_chunk;
    info->chunks = file.chunks;
    info->file_bytes = file.file_bytes;
    return MCRT_OK;
}

extern "C" int mcrt_exr_file_channel(const mcrt_exr_file* f, uint32_t i, const char** name, uint32_t* pixel_type) {
    if (!f || i >= f->file.channels.size()) return MCRT_ERR_INVALID;
    if (name) *name = f->file.channels[i].name.c_str();
    if (pixel_type) *pixel_type = f->file.channels[i].pixel_type;
    return MCRT_OK;
}

extern "C" int mcrt_exr_file_attribute(const mcrt_exr_file* f, uint32_t i, const char** name, const char** type, const void** value, uint32_t* size) {
    if (!f || i >= f->file.attributes.size()) return MCRT_ERR_INVALID;
    const ExrFileAttribute& a = f->file.attributes[i];
    if (name) *name = a.name.c_str();
    if (type) *type = a.type.c_str();
    if (value) *value = a.value.data();
    if (size) *size = (uint32_t)a.value.size();
    return MCRT_OK;
}

extern "C" int mcrt_exr_load_device(mcrt_ctx* ctx, mcrt_exr_file* f, const mcrt_exr_target* d_targets, uint32_t count, const mcrt_exr_load_params* params,
                                    mcrt_exr_load_result* result, mcrt_stats* stats) {
    return load(ctx, "mcrt_exr_load_device", false, f, d_targets, count, params, result, stats);
}

extern "C" int mcrt_exr_load(mcrt_ctx* ctx, mcrt_exr_file* f, const mcrt_exr_target* targets, uint32_t count, const mcrt_exr_load_params* params,
                             mcrt_exr_load_result* result, mcrt_stats* stats) {
    return load(ctx, "mcrt_exr_load", true, f, targets, count, params, result, stats);
}
