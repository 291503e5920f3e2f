// The row scatter of the sharded host-pointer forms (mcrt_pass_host.hpp shardFramesDown): a shard's owned rows come back from the device
// packed, and go to their places in the caller's full frame. No HIP here: tests/emu/row_scatter_main.cpp compiles this header alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mcrt {

// packed row r (r < rows) -> row idx[r] of the frame, row_bytes each; every other row of the frame is left alone
inline void scatterRows(void* frame, const void* packed, const uint32_t* idx, uint32_t rows, size_t row_bytes) {
    for (uint32_t r = 0; r < rows; r++)
        memcpy((unsigned char*)frame + (size_t)idx[r] * row_bytes, (const unsigned char*)packed + (size_t)r * row_bytes, row_bytes);
}

}  // namespace mcrt
