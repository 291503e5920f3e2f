"""What only the frame comparison has (tests/side_libraries.py holds what libmcrt_compare.so may contain): the device code is without a
call (so no libm routine: it is + - * /, compare and select), three SSIM workgroups fit a CU, the binding's struct layouts, exr_layers'
names of the error maps."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

from side_libraries import CSRC, TABLE, c_values, tool as _tool

LIB = os.path.join(CSRC, "libmcrt_compare.so")


def test_three_ssim_workgroups_fit_a_cu():
    assert TABLE["mcrt_compare"]["lds"]["compareSsimKernel"] == 2 * 42 * 26 * 8 + 5 * 26 * 32 * 8 <= 160 * 1024 // 3  # three workgroups per CU


def test_the_device_code_calls_nothing(pkg, tmp_path):
    """Every kernel is one function: the code object defines the three kernels as its only functions, refers to no symbol outside itself -
    no libm / ocml routine was linked in or left undefined - and its text holds no call and no square-root, logarithm or exponential
    instruction."""
    pkg.lib()
    table = _tool("kernel_spill_table")
    local = str(tmp_path / "lib.so")
    shutil.copy(LIB, local)
    subprocess.run([os.path.join(table.LLVM, "llvm-objdump"), "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    objects = [str(tmp_path / f) for f in sorted(os.listdir(str(tmp_path))) if "gfx950" in f]
    assert len(objects) == 1, objects
    rows = subprocess.run([os.path.join(table.LLVM, "llvm-readelf"), "--symbols", "--wide", objects[0]], check=True, capture_output=True, text=True).stdout.splitlines()
    rows = [r.split() for r in rows if re.match(r"\s*\d+:", r)]
    named = [r for r in rows if len(r) >= 8]
    assert named and not [r for r in named if r[6] == "UND"], named
    functions = sorted({r[7] for r in named if r[3] == "FUNC"})  # (.dynsym and .symtab list them both)
    assert len(functions) == 3 and all(any(k in f for k in ("comparePixelsKernel", "compareLevelKernel", "compareSsimKernel")) for f in functions), functions
    text = subprocess.run([os.path.join(table.LLVM, "llvm-objdump"), "-d", objects[0]], check=True, capture_output=True, text=True).stdout
    assert "v_add_f64" in text and "v_mul_f64" in text  # (the disassembly is there)
    for op in ("s_swappc", "s_call", "s_setpc", "v_sqrt", "v_rsq", "v_log", "v_exp"):
        assert op not in text, op
    assert len(table.kernels_of(LIB)) == 3


def test_the_binding_lays_the_structs_out_as_the_header_does(pkg, tmp_path):
    sizes = c_values(tmp_path, ["sizeof(mcrt_compare_params)", "sizeof(mcrt_compare_maps)", "sizeof(mcrt_compare_result)", "offsetof(mcrt_compare_params,want_ssim)",
                                "offsetof(mcrt_compare_result,max_abs_pixel)", "offsetof(mcrt_compare_result,pixels)", "offsetof(mcrt_compare_result,ssim_excluded)",
                                "offsetof(mcrt_compare_result,mean_ssim)"], "%zu %zu %zu %zu %zu %zu %zu %zu")
    assert sizes == [C.sizeof(pkg.CompareParams), C.sizeof(pkg.CompareMaps), C.sizeof(pkg.CompareResult), pkg.CompareParams.want_ssim.offset,
                     pkg.CompareResult.max_abs_pixel.offset, pkg.CompareResult.pixels.offset, pkg.CompareResult.ssim_excluded.offset,
                     pkg.CompareResult.mean_ssim.offset]
    assert C.sizeof(pkg.CompareParams) == 32 and C.sizeof(pkg.CompareResult) == 160
    assert c_values(tmp_path, ["(double)MCRT_SSIM_G0"], "%a", parse=float.fromhex) == [0.26601172486179436]


def test_exr_layers_of_errors_names_types_and_views(pkg):
    """error.se, error.rel, error.ssim: the maps themselves (nothing copied), FLOAT whatever the defaults of colour are; after the
    channels there were; today's arguments give what they gave."""
    h, w = 3, 5
    maps = {"squared_error": np.arange(h * w, dtype=np.float64).reshape(h, w), "relative": np.ones((h, w)), "ssim": np.zeros((h, w)), "mse": 1.0, "compared": 15}
    rgb = np.zeros((h, w, 3))
    layers = pkg.exr_layers(rgb=rgb, errors=maps)
    assert list(layers) == ["R", "G", "B", "error.se", "error.rel", "error.ssim"]
    for key, name in (("squared_error", "error.se"), ("relative", "error.rel"), ("ssim", "error.ssim")):
        view, kind = layers[name]
        assert kind == "float" and view is maps[key]
    assert list(pkg.exr_layers(rgb=rgb)) == list(pkg.exr_layers(rgb=rgb, errors=None)) == list(pkg.exr_layers(rgb=rgb, errors={})) == ["R", "G", "B"]
    assert list(pkg.exr_layers(rgb=rgb, errors={"relative": maps["relative"], "ssim": None})) == ["R", "G", "B", "error.rel"]
    assert layers["R"][1] == "half"
