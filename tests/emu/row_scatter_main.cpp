// Stand-alone check of the sharded host-pointer forms' row scatter (csrc/mcrt_rows.hpp, which is all this includes of the product): a
// program of its own so that tests/test_row_scatter.py can build it with the address and undefined-behaviour sanitizers and run it as a
// child process. No library, no GPU: the row indices of every configuration come from the test (mcrt_shard_rows through the binding).
//
// Input (argv[1], text), one configuration per line: height width element_bytes elements_per_pixel rows idx[0] .. idx[rows-1]
// Per configuration the frame - height rows between one guard row before and one after, every byte a sentinel - takes the packed rows;
// then every byte is compared with the plain statement of what it must hold: row idx[r] the packed row r, every other row and both guard
// rows the sentinel. Exit status 0 and "ok <n> configurations", or 1 and the first byte that differs (2: input that makes no sense).
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_rows.hpp"

namespace {
constexpr unsigned char kSentinel = 0xA5;
unsigned char packedByte(size_t config, size_t offset) { return (unsigned char)((offset * 7 + config * 13) % 163); }  // (never the sentinel)
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s configurations.txt\n", argv[0]), 2;
    std::ifstream in(argv[1]);
    std::string line;
    size_t configs = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        size_t height, width, elem, per_pixel, rows;
        if (!(ls >> height >> width >> elem >> per_pixel >> rows)) return fprintf(stderr, "line %zu: five numbers expected\n", configs + 1), 2;
        std::vector<uint32_t> idx(rows);
        std::vector<long> owner(height, -1);  // packed row that goes to frame row y, or -1
        for (size_t r = 0; r < rows; r++) {
            if (!(ls >> idx[r]) || idx[r] >= height || owner[idx[r]] != -1) return fprintf(stderr, "line %zu: row index %zu\n", configs + 1, r), 2;
            owner[idx[r]] = (long)r;
        }
        const size_t row_bytes = width * elem * per_pixel;
        std::vector<unsigned char> frame((height + 2) * row_bytes, kSentinel), packed(rows * row_bytes);
        for (size_t i = 0; i < packed.size(); i++) packed[i] = packedByte(configs, i);
        mcrt::scatterRows(frame.data() + row_bytes, packed.data(), idx.data(), (uint32_t)rows, row_bytes);
        for (size_t y = 0; y < height + 2; y++)
            for (size_t b = 0; b < row_bytes; b++) {
                const long r = (y == 0 || y == height + 1) ? -1 : owner[y - 1];
                const unsigned char want = r < 0 ? kSentinel : packedByte(configs, (size_t)r * row_bytes + b);
                if (frame[y * row_bytes + b] != want)
                    return fprintf(stderr, "configuration %zu (%s): frame row %ld byte %zu holds %u, not %u\n", configs + 1, line.c_str(), (long)y - 1, b,
                                   frame[y * row_bytes + b], want), 1;
            }
        configs++;
    }
    printf("ok %zu configurations\n", configs);
    return configs ? 0 : 2;
}
