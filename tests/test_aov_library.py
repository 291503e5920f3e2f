"""The first-hit AOV pass's kernels are a code object of their own. libmcrt_aov.so holds exactly aovRayKernel and aovResolveKernel, both
without spills or scratch (the issue's aim for them); libmcrt_hip.so - the render path's device code, listed function by function in
tests/golden/device_code_hashes.json - holds neither, and finds the other library next to itself (RUNPATH $ORIGIN)."""
import importlib.util
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_aov_kernels_live_beside_the_render_path(pkg):
    pkg.lib()
    table = _tool("kernel_spill_table")
    aov = {k["name"]: k for k in table.kernels_of(os.path.join(CSRC, "libmcrt_aov.so"))}
    assert sorted(aov) == ["aovRayKernel", "aovResolveKernel"]
    for name, k in aov.items():
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    assert not [k["name"] for k in table.kernels_of(os.path.join(CSRC, "libmcrt_hip.so")) if "aov" in k["name"].lower()]


def test_the_libraries_find_the_aov_library_next_to_themselves():
    for lib in ("libmcrt_hip.so", "libmcrt_hip_tol.so"):
        path = os.path.join(CSRC, lib)
        if lib.endswith("_tol.so") and not os.path.exists(path):
            continue  # (MCRT_SKIP_TOLERANCE_BUILD=1 builds)
        dyn = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
        assert "[libmcrt_aov.so]" in dyn, lib
        assert any("$ORIGIN" in l for l in dyn.splitlines() if "RUNPATH" in l or "RPATH" in l), lib
