// tests/emu/matte_emu.cpp — TEST HARNESS ONLY (built by tests/test_matte_emulation.py into tests/emu/_build/).
//
// The ranking of the ID mattes on the host: csrc/mcrt_matte.hpp unchanged - the text the two kernels of csrc/mcrt_matte.hip run - on
// wave_emu.hpp's emulated workgroup (4 wavefronts of 64 fibers, __syncthreads a rendezvous of all of them, shuffles served from a
// snapshot of the lanes' operands), driven chunk by chunk the way mcrt_render_matte_device drives it. The tile form's LDS is an array
// here of exactly matteTileLdsWords(spp, tile) words, filled with a pattern before every workgroup and fenced behind. Not a CPU
// fallback: nothing in the product links or loads it.
#define MCRT_WAVE_EMU 1
#include "wave_emu.hpp"

#include "../../monte-carlo-ray-tracer_amd/csrc/mcrt_matte.hpp"

using namespace mcrt;

extern "C" {

// keys: [spp][pixels] sample-major (with map: surfaces, 0xFFFFFFFF a miss). out: host arrays of `pixels` pixels, null = not wanted.
// form: 1 tile, 2 memory. chunk_pixels: 0 = one ranking, else rankings of that many pixels (the last ragged), each from a sample-major
// copy of its own pixels' records as a chunk of the render has them. Returns 0, -1 for what the entry points refuse, -2 when the tile
// form wrote past its LDS.
int matte_emu_rank(uint64_t pixels, uint32_t spp, const uint32_t* keys, const uint32_t* map, uint32_t ranks, const uint32_t* codes,
                   const mcrt_matte_buffers* out, int form, uint64_t chunk_pixels) {
    if (pixels == 0 || pixels > 0xFFFFFFFFull || spp == 0 || pixels * spp > kMatteMaxSamples || !keys || !out || matteRanksError(ranks)) return -1;
    if (form != kMatteFormTile && form != kMatteFormMemory) return -1;
    if (form == kMatteFormTile && matteTilePixels(spp) == 0) return -1;
    if (out->layer && !codes) return -1;
    if (!chunk_pixels || chunk_pixels > pixels) chunk_pixels = pixels;
    std::vector<uint32_t> chunk(chunk_pixels * spp), work, lds;
    for (uint64_t first = 0; first < pixels; first += chunk_pixels) {
        MatteRank mr{};
        mr.pixels = (uint32_t)std::min<uint64_t>(chunk_pixels, pixels - first);
        for (uint32_t i = 0; i < spp; i++)
            for (uint32_t p = 0; p < mr.pixels; p++) chunk[(uint64_t)i * mr.pixels + p] = keys[(uint64_t)i * pixels + first + p];
        mr.keys = chunk.data();
        mr.map = map;
        mr.codes = codes;
        mr.out = *out;
        mr.first_pixel = first;
        mr.spp = spp;
        mr.ranks = ranks;
        wemu::launch().block_dim = kMatteBlock;
        if (form == kMatteFormTile) {
            mr.tile = matteTilePixels(spp);
            const uint32_t words = matteTileLdsWords(spp, mr.tile);
            lds.assign(words + 64, 0u);
            const uint32_t blocks = (mr.pixels + mr.tile - 1) / mr.tile;  // launchMatteRank's grid
            for (uint32_t blk = 0; blk < blocks; blk++) {
                for (uint32_t i = 0; i < words; i++) lds[i] = 0xDEADBEEFu;  // (a word the staging forgot shows as a key)
                for (uint32_t i = words; i < words + 64; i++) lds[i] = 0x0FE0CE00u + i;
                wemu::launch().block_idx = blk;
                wemu::launch().grid_dim = blocks;
                wemu::runGroup((int)kMatteWaves, [&](int tid) { matteRankTileBlock(mr, blk, (uint32_t)tid, lds.data()); });
                for (uint32_t i = words; i < words + 64; i++)
                    if (lds[i] != 0x0FE0CE00u + i) return -2;
            }
        } else {
            work.assign((size_t)mr.pixels * spp * 2, 0xDEADBEEFu);
            mr.work = work.data();
            const uint32_t blocks = (mr.pixels + kMatteWaves - 1) / kMatteWaves;
            for (uint32_t blk = 0; blk < blocks; blk++) {
                wemu::launch().block_idx = blk;
                wemu::launch().grid_dim = blocks;
                wemu::runGroup((int)kMatteWaves, [&](int tid) {  // matteRankMemoryKernel
                    const uint64_t p = (uint64_t)blk * kMatteWaves + (uint32_t)tid / 64u;
                    if (p < mr.pixels) matteRankMemoryWave(mr, (uint32_t)p, (uint32_t)tid % 64u);
                });
            }
        }
    }
    return 0;
}

// The pixels of a tile at spp samples per pixel, 0 where the tile form does not run, and the words of LDS its launch asks for.
uint32_t matte_emu_tile_pixels(uint32_t spp) { return matteTilePixels(spp); }
uint32_t matte_emu_tile_lds_words(uint32_t spp) { return matteTilePixels(spp) ? matteTileLdsWords(spp, matteTilePixels(spp)) : 0; }

}  // extern "C"
