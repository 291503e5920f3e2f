"""What only the variance-guided filter has (tests/side_libraries.py holds what libmcrt_denoise_var.so may contain): the tile kernel's LDS
in the table is the LDS that csrc/mcrt_denoise_var.hpp's constant states."""
import test_denoise_var_emulation as dv
from side_libraries import TABLE


def test_the_tile_kernel_s_lds_is_the_header_s_constant():
    lds = dv._emu().denoise_var_emu_tile_lds_bytes()  # kDenoiseVarTileLdsBytes
    assert lds == 16 * 20 * 20 * 8 and 3 * lds <= 160 * 1024  # the 16 x 16 tile with its halo, 16 doubles per record; three per CU
    assert TABLE["mcrt_denoise_var"]["lds"] == {"denoiseVarTileKernel": lds}  # (the plain and the prep kernel: none)
