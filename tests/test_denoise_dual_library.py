"""The dual-buffer filter's kernels are a code object of their own, like the other image passes'. libmcrt_denoise_dual.so holds exactly
denoiseDualPrepKernel, denoiseDualPlainKernel and denoiseDualTileKernel, all without spills or scratch. The tile kernel's LDS is DYNAMIC
(its size depends on the radii and passes 64 KiB): the code object declares none, and what the launch asks for is
csrc/mcrt_denoise_dual.hpp's denoiseDualTileLdsBytes(R, F), held here to its statement and to a CU's 160 KiB. None of the other libraries
holds one of the kernels, and libmcrt_hip.so finds the new library next to itself (RUNPATH $ORIGIN)."""
import ctypes as C
import importlib.util
import os
import subprocess

import test_denoise_dual_emulation as dd
from conftest import ROOT

CSRC = os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc")
KERNELS = ["denoiseDualPlainKernel", "denoiseDualPrepKernel", "denoiseDualTileKernel"]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_denoise_dual_kernels_live_beside_the_render_path(pkg):
    pkg.lib()
    table = _tool("kernel_spill_table")
    kernels = {k["name"]: k for k in table.kernels_of(os.path.join(CSRC, "libmcrt_denoise_dual.so"))}
    assert sorted(kernels) == KERNELS
    for name, k in kernels.items():
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["lds"] == 0, (name, k)  # the tile kernel's is dynamic
        assert k["max_wg"] == (1024 if name == "denoiseDualTileKernel" else 256), (name, k)  # the tile form: up to 16 waves on one tile
    for lib in sorted(f for f in os.listdir(CSRC) if f.startswith("libmcrt_") and f.endswith(".so") and f != "libmcrt_denoise_dual.so"):
        assert not [k["name"] for k in table.kernels_of(os.path.join(CSRC, lib)) if "denoisedual" in k["name"].lower()], lib


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


def test_the_libraries_find_the_denoise_dual_library_next_to_themselves():
    for lib in ("libmcrt_hip.so", "libmcrt_hip_tol.so"):
        path = os.path.join(CSRC, lib)
        if lib.endswith("_tol.so") and not os.path.exists(path):
            continue  # (MCRT_SKIP_TOLERANCE_BUILD=1 builds)
        dyn = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
        assert "[libmcrt_denoise_dual.so]" in dyn, lib
        assert any("$ORIGIN" in l for l in dyn.splitlines() if "RUNPATH" in l or "RPATH" in l), lib


def test_the_calls_are_exported_and_the_abi_version_stays(pkg):
    L = pkg.lib()
    assert hasattr(L, "mcrt_denoise_dual") and hasattr(L, "mcrt_denoise_dual_device")
    assert L.mcrt_abi_version() == 2
    bufs, par = pkg.DenoiseDualBuffers(), pkg.DenoiseDualParams()
    assert L.mcrt_denoise_dual(None, 1, 1, 4, None, None, None, C.byref(par), C.byref(bufs), None) == -1  # MCRT_ERR_INVALID
    assert L.mcrt_denoise_dual_device(None, 1, 1, 4, None, None, None, C.byref(par), C.byref(bufs), None) == -1
    assert C.sizeof(pkg.DenoiseDualParams) == 40 and C.sizeof(pkg.DenoiseDualBuffers) == 32
