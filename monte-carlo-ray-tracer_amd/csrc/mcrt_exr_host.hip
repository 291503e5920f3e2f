// OpenEXR output (include/mcrt.h mcrt_exr_save*), host side: the two entry points. No kernel here: the pack is libmcrt_exr.so
// (csrc/mcrt_exr.hip; DESIGN.md "Image passes" says why); validation, the header, deflate and the file are csrc/mcrt_exr_file.hpp.
// The device form uploads the sorted channel table, launches the pack and brings the packed buffer - a half to a quarter of the FP64
// frames' bytes - to pinned host memory in one copy; no source frame leaves the device. The host form first stages every distinct source
// buffer on the device, once however many channels name it.
// Scratch slots of the family: 0 the channel table, 1 the packed buffer, 2 the host form's staged sources.
#include <algorithm>
#include <map>

#include "mcrt_exr_file.hpp"
#include "mcrt_exr_launch.hpp"
#include "mcrt_pass_host.hpp"

using namespace mcrt;

namespace {

struct PinnedBuffer {
    void* p = nullptr;
    ~PinnedBuffer() {
        if (p) (void)hipHostFree(p);
    }
};

// table: the plan's channels with data pointers the device can read
int packOnDevice(mcrt_ctx* ctx, const char* what, const ExrPlan& plan, const std::vector<ExrChannelRec>& table, PinnedBuffer& host, PassTimer& timer,
                 const unsigned char** packed) {
    hipStream_t stream = (hipStream_t)ctxStream(ctx);
    const size_t table_bytes = table.size() * sizeof(ExrChannelRec);
    ExrChannelRec* d_table = (ExrChannelRec*)ctxPassScratch(ctx, kPassExr, 0, table_bytes);
    const ExrPack shape = exrPackOf(plan, nullptr, nullptr);
    const size_t out_bytes = (size_t)exrPackedWords(shape) * 4;
    unsigned char* d_out = (unsigned char*)ctxPassScratch(ctx, kPassExr, 1, out_bytes);
    if (!d_table || !d_out) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the packed buffer could not be allocated");
    if (exrPackBlocks(shape) == 0) return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": the packed buffer is past what one launch fills");
    MCRT_HIP_TRY(ctx, hipHostMalloc(&host.p, out_bytes, hipHostMallocDefault));
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(d_table, table.data(), table_bytes, hipMemcpyHostToDevice, stream));
    MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));  // (the table is pageable host memory of this frame)
    if (int rc = timer.begin(stream)) return rc;
    MCRT_HIP_TRY(ctx, (hipError_t)launchExrPack(stream, exrPackOf(plan, d_table, d_out)));
    if (int rc = timer.end(stream)) return rc;
    MCRT_HIP_TRY(ctx, hipMemcpyAsync(host.p, d_out, (size_t)plan.total_bytes, hipMemcpyDeviceToHost, stream));
    MCRT_HIP_TRY(ctx, hipStreamSynchronize(stream));
    *packed = (const unsigned char*)host.p;
    return MCRT_OK;
}

int save(mcrt_ctx* ctx, const char* what, bool host_data, const char* path, uint32_t width, uint32_t height, const mcrt_exr_channel* channels, uint32_t count,
         const mcrt_exr_attribute* attributes, uint32_t attribute_count, const mcrt_exr_params* params, mcrt_exr_result* result, mcrt_stats* stats) {
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = ctxIdle(ctx, what)) return rc;
    PassTimer timer(ctx);
    PinnedBuffer host;
    std::string why;
    const auto pack = [&](const ExrPlan& plan, const unsigned char** packed) -> int {
        std::vector<ExrChannelRec> table = plan.table;
        if (host_data) {
            // the distinct source buffers, each as long as the farthest element one of its channels reads, in one allocation
            const uint64_t pixels = (uint64_t)width * height;
            std::map<const void*, size_t> extent;
            for (const ExrChannelRec& c : table) {
                const size_t bytes = (size_t)(((pixels - 1) * c.stride + c.offset + 1) * (c.pixel_type == MCRT_EXR_UINT ? 4 : 8));
                size_t& e = extent[c.data];
                e = std::max(e, bytes);
            }
            std::map<const void*, size_t> at;
            size_t total = 0;
            for (const auto& b : extent) {
                at[b.first] = total;
                total += (b.second + 7) / 8 * 8;
            }
            unsigned char* base = (unsigned char*)ctxPassScratch(ctx, kPassExr, 2, total);
            if (!base) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the frames' device copy could not be allocated");
            for (const auto& b : extent) MCRT_HIP_TRY(ctx, hipMemcpy(base + at[b.first], b.first, b.second, hipMemcpyHostToDevice));
            for (ExrChannelRec& c : table) c.data = base + at[c.data];
        }
        return packOnDevice(ctx, what, plan, table, host, timer, packed);
    };
    const int rc = exrSave(path, width, height, channels, count, attributes, attribute_count, params, result, why, pack);
    if (rc) return why.empty() ? rc : ctxFail(ctx, rc, std::string(what) + ": " + why);
    return timer.finish(stats, 1);
}

}  // namespace

extern "C" int mcrt_exr_save_device(mcrt_ctx* ctx, const char* path, uint32_t width, uint32_t height, const mcrt_exr_channel* d_channels, uint32_t count,
                                    const mcrt_exr_attribute* attributes, uint32_t attribute_count, const mcrt_exr_params* params, mcrt_exr_result* result,
                                    mcrt_stats* stats) {
    return save(ctx, "mcrt_exr_save_device", false, path, width, height, d_channels, count, attributes, attribute_count, params, result, stats);
}

extern "C" int mcrt_exr_save(mcrt_ctx* ctx, const char* path, uint32_t width, uint32_t height, const mcrt_exr_channel* channels, uint32_t count,
                             const mcrt_exr_attribute* attributes, uint32_t attribute_count, const mcrt_exr_params* params, mcrt_exr_result* result,
                             mcrt_stats* stats) {
    return save(ctx, "mcrt_exr_save", true, path, width, height, channels, count, attributes, attribute_count, params, result, stats);
}
