"""What only the dual-buffer filter has (tests/side_libraries.py holds what libmcrt_denoise_dual.so may contain). The tile kernel's LDS is
DYNAMIC (its size depends on the radii and passes 64 KiB): the code object declares none, and what the launch asks for is
csrc/mcrt_denoise_dual.hpp's denoiseDualTileLdsBytes(R, F), held here to its statement and to a CU's 160 KiB. And what the calls refuse
as far as no GPU is needed."""
import ctypes as C

import test_denoise_dual_emulation as dd


def test_the_tile_form_s_lds_is_the_stated_function_of_the_radii():
    """Records [9][(16 + 2 (R + F))^2], the terms of one offset [6][(16 + 2 F)^2], its row sums [2][16 + 2 F][16], in doubles."""
    L = dd._emu()
    for R in range(1, 9):
        for F in range(1, 4):
            side, e = 16 + 2 * (R + F), 16 + 2 * F
            want = 8 * (9 * side * side + 6 * e * e + 2 * e * 16)
            assert L.denoise_dual_emu_tile_lds_bytes(R, F) == want, (R, F)
            assert want <= 160 * 1024, (R, F)
    assert L.denoise_dual_emu_tile_lds_bytes(5, 2) == 89120
    assert L.denoise_dual_emu_tile_lds_max_bytes() == L.denoise_dual_emu_tile_lds_bytes(8, 3) == 132832


def test_a_null_context_is_refused_and_the_structs_keep_their_sizes(pkg):
    L = pkg.lib()
    bufs, par = pkg.DenoiseDualBuffers(), pkg.DenoiseDualParams()
    assert L.mcrt_denoise_dual(None, 1, 1, 4, None, None, None, C.byref(par), C.byref(bufs), None) == -1  # MCRT_ERR_INVALID
    assert L.mcrt_denoise_dual_device(None, 1, 1, 4, None, None, None, C.byref(par), C.byref(bufs), None) == -1
    assert C.sizeof(pkg.DenoiseDualParams) == 40 and C.sizeof(pkg.DenoiseDualBuffers) == 32
