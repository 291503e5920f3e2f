"""The variance-guided filter's kernels are a code object of their own, like the a-trous filter's. libmcrt_denoise_var.so holds exactly
denoiseVarPrepKernel, denoiseVarPlainKernel and denoiseVarTileKernel, all without spills or scratch, the tile kernel with the LDS that
csrc/mcrt_denoise_var.hpp's constant states; none of the other libraries holds one of them, and libmcrt_hip.so finds the new library next
to itself (RUNPATH $ORIGIN)."""
import importlib.util
import os
import subprocess

import test_denoise_var_emulation as dv
from conftest import ROOT

CSRC = os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc")
KERNELS = ["denoiseVarPlainKernel", "denoiseVarPrepKernel", "denoiseVarTileKernel"]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_denoise_var_kernels_live_beside_the_render_path(pkg):
    pkg.lib()
    table = _tool("kernel_spill_table")
    kernels = {k["name"]: k for k in table.kernels_of(os.path.join(CSRC, "libmcrt_denoise_var.so"))}
    assert sorted(kernels) == KERNELS
    for name, k in kernels.items():
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    lds = dv._emu().denoise_var_emu_tile_lds_bytes()  # kDenoiseVarTileLdsBytes
    assert lds == 16 * 20 * 20 * 8 and 3 * lds <= 160 * 1024  # the 16 x 16 tile with its halo, 16 doubles per record; three per CU
    assert kernels["denoiseVarTileKernel"]["lds"] == lds
    assert kernels["denoiseVarPlainKernel"]["lds"] == 0 and kernels["denoiseVarPrepKernel"]["lds"] == 0
    for lib in ("libmcrt_hip.so", "libmcrt_aov.so", "libmcrt_denoise.so", "libmcrt_pixel_stats.so", "libmcrt_robust.so"):
        assert not [k["name"] for k in table.kernels_of(os.path.join(CSRC, lib)) if "denoisevar" in k["name"].lower()], lib


def test_the_libraries_find_the_denoise_var_library_next_to_themselves():
    for lib in ("libmcrt_hip.so", "libmcrt_hip_tol.so"):
        path = os.path.join(CSRC, lib)
        if lib.endswith("_tol.so") and not os.path.exists(path):
            continue  # (MCRT_SKIP_TOLERANCE_BUILD=1 builds)
        dyn = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
        assert "[libmcrt_denoise_var.so]" in dyn, lib
        assert any("$ORIGIN" in l for l in dyn.splitlines() if "RUNPATH" in l or "RPATH" in l), lib


def test_the_calls_are_exported_and_the_abi_version_stays(pkg):
    L = pkg.lib()
    assert hasattr(L, "mcrt_denoise_variance") and hasattr(L, "mcrt_denoise_variance_device")
    assert L.mcrt_abi_version() == 2
