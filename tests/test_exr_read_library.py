"""The kernels of the OpenEXR input are a code object of their own, like the pack of the output before them. libmcrt_exr_read.so holds
exactly the four exrRead kernels, without spills or scratch; no other library of build.SIDE_LIBS, nor libmcrt_hip.so - the render path's
device code, listed function by function in tests/golden/device_code_hashes.json -, holds a kernel of that name; the main libraries find
the new one next to themselves (RUNPATH $ORIGIN); zlib is not linked; and the binding lays the new structs out as the header does."""
import ctypes as C
import importlib
import importlib.util
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc")
LIB = os.path.join(CSRC, "libmcrt_exr_read.so")
KERNELS = ["exrReadGatherKernel", "exrReadScanKernel", "exrReadSumKernel", "exrReadUndoKernel"]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_four_kernels_live_beside_the_render_path(pkg):
    pkg.lib()
    table = _tool("kernel_spill_table")
    kernels = {k["name"]: k for k in table.kernels_of(LIB)}
    assert sorted(kernels) == KERNELS
    for name, k in kernels.items():
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    for name in KERNELS[1:]:
        assert kernels[name]["lds"] == 256 // 64 * 4, name   # a word per wave of the workgroup's scan
    assert kernels["exrReadGatherKernel"]["lds"] == 0        # (its table of requested channels is dynamic LDS, sized per launch)
    build = importlib.import_module("monte-carlo-ray-tracer_amd.build")
    side = [lib for lib, _ in build.SIDE_LIBS]
    assert LIB in side and side[-1] == LIB and "mcrt_exr_read_host.hip" in build.TUS
    for lib in [l for l in side if l != LIB] + [build.LIB]:
        names = [k["name"] for k in table.kernels_of(lib)]
        assert names and not [n for n in names if n.startswith("exrRead")], lib
    assert [k["name"] for k in table.kernels_of(os.path.join(CSRC, "libmcrt_exr.so"))] == ["exrPackKernel"]


def test_the_libraries_find_the_read_library_next_to_themselves_and_link_no_zlib():
    assert os.path.exists(os.path.join(CSRC, "libmcrt_hip.so"))
    for lib in ("libmcrt_hip.so", "libmcrt_hip_tol.so", "libmcrt_exr_read.so"):
        path = os.path.join(CSRC, lib)
        if lib.endswith("_tol.so") and not os.path.exists(path):
            continue  # (MCRT_SKIP_TOLERANCE_BUILD=1 builds)
        dyn = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
        needed = [l for l in dyn.splitlines() if "NEEDED" in l]
        assert not [l for l in needed if "libz" in l], (lib, needed)
        if lib != "libmcrt_exr_read.so":
            assert "[libmcrt_exr_read.so]" in dyn, lib
            assert any("$ORIGIN" in l for l in dyn.splitlines() if "RUNPATH" in l or "RPATH" in l), lib


def test_the_calls_are_exported_and_the_abi_version_stays(pkg):
    L = pkg.lib()
    for name in ("mcrt_exr_open", "mcrt_exr_close", "mcrt_exr_file_info", "mcrt_exr_file_channel", "mcrt_exr_file_attribute", "mcrt_exr_load", "mcrt_exr_load_device"):
        assert hasattr(L, name), name
    assert L.mcrt_abi_version() == 2
    for name in ("ExrInfo", "ExrTarget", "ExrLoadParams", "ExrLoadResult", "exr_unlayer"):
        assert hasattr(pkg, name), name
    assert hasattr(pkg.Context, "exr_load")


def test_the_binding_lays_the_structs_out_as_the_header_does(pkg, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcrt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n",sizeof(mcrt_exr_info),'
                   'sizeof(mcrt_exr_target),sizeof(mcrt_exr_load_params),sizeof(mcrt_exr_load_result),offsetof(mcrt_exr_info,display_window),'
                   'offsetof(mcrt_exr_info,lines_per_chunk),offsetof(mcrt_exr_info,file_bytes),offsetof(mcrt_exr_target,stride),'
                   'offsetof(mcrt_exr_load_result,raw_chunks),(int)MCRT_EXR_COMPRESSION_ZIPS);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(pkg.ExrInfo), C.sizeof(pkg.ExrTarget), C.sizeof(pkg.ExrLoadParams), C.sizeof(pkg.ExrLoadResult), pkg.ExrInfo.display_window.offset,
                     pkg.ExrInfo.lines_per_chunk.offset, pkg.ExrInfo.file_bytes.offset, pkg.ExrTarget.stride.offset, pkg.ExrLoadResult.raw_chunks.offset, 2]
    assert C.sizeof(pkg.ExrTarget) == 32 and C.sizeof(pkg.ExrInfo) == 72


def test_exr_unlayer_is_the_inverse_of_exr_layers(pkg):
    """Every documented name, from frames with a value of their own each: exr_layers' views, taken apart and put together again, are the
    frames; names it does not know - a matte's R, G, B, A among them - come back under "other"."""
    h, w = 3, 5
    rng = np.random.default_rng(1)
    f3, f1 = lambda: rng.random((h, w, 3)), lambda: rng.random((h, w))
    u1 = lambda: rng.integers(0, 1 << 32, size=(h, w), dtype=np.uint32)
    aov = {k: (u1() if t == np.uint32 else f3() if n == 3 else f1()) for k, (t, n) in pkg.AOV_CHANNELS.items()}
    given = dict(rgb=f3(), aov=aov, stats={"variance": f3(), "half_a": f3(), "half_b": f3()}, highlights={"tops": rng.random((h, w, 4, 3)), "level": f1()},
                 robust={"robust": f3(), "removed": f3(), "clamped": u1()},
                 denoised={"denoise": {"rgb": f3()}, "denoise_variance": {"rgb": f3(), "variance": f3()}, "denoise_dual": {"rgb": f3(), "variance": f3(), "error": f3()}},
                 errors={"squared_error": f1(), "relative": f1(), "ssim": f1()})
    matte = {"layer": rng.random((h, w, 2, 2))}
    layers = pkg.exr_layers(mattes={"crypto": matte}, **given)
    flat = {n: v for n, (v, _) in layers.items()}
    flat["someone.elses"] = f1()
    back = pkg.exr_unlayer(flat)
    assert sorted(back) == sorted(list(given) + ["other"])
    assert sorted(back["other"]) == ["crypto00.A", "crypto00.B", "crypto00.G", "crypto00.R", "someone.elses"]

    def same(a, b, where):
        if isinstance(b, dict):
            assert sorted(a) == sorted(b), where
            for k in b:
                same(a[k], b[k], where + "." + k)
        else:
            assert a.dtype == b.dtype and a.shape == b.shape, where
            np.testing.assert_array_equal(a, b, err_msg=where)

    for k in given:
        same(back[k], given[k], k)
    assert list(pkg.exr_layers(**{k: v for k, v in back.items() if k != "other"})) == [n for n in layers if not n.startswith("crypto")]
    part = pkg.exr_unlayer({"R": flat["R"], "G": flat["G"], "normal.X": flat["normal.X"], "tops0.R": flat["tops0.R"]})   # no layer is whole
    assert list(part) == ["other"] and sorted(part["other"]) == ["G", "R", "normal.X", "tops0.R"]
