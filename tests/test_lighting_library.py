"""The lighting passes are a code object of their own, like the image passes before them. libmcrt_lighting.so holds exactly the pass's two
kernels, without scratch and within the registers profiles/NOTES_lighting.md records (its table is read here: the numbers are upper
bounds); libmcrt_hip.so - the render path's device code, listed function by function in tests/golden/device_code_hashes.json - and the
other side libraries hold no kernel of these names (whole names: robustHighlightsKernel contains "light"), and the main libraries find
the new one next to themselves (RUNPATH $ORIGIN). What the calls refuse is checked here as far as no GPU is needed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc")
KERNELS = ["lightingRayKernel", "lightingResolveKernel"]
CHANNELS = ["emission", "sky", "direct", "light", "unoccluded"]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def recorded_resources():
    """The table of profiles/NOTES_lighting.md: kernel -> dict of vgpr, vgpr_spill, sgpr_spill, scratch, lds."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "NOTES_lighting.md")):
        m = re.match(r"\|\s*`(lighting\w+Kernel)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", line)
        if m:
            rows[m.group(1)] = dict(zip(("vgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds"), (int(x) for x in m.groups()[1:])))
    return rows


def test_the_lighting_kernels_live_beside_the_render_path(pkg):
    pkg.lib()
    table = _tool("kernel_spill_table")
    kernels = {k["name"]: k for k in table.kernels_of(os.path.join(CSRC, "libmcrt_lighting.so"))}
    assert sorted(kernels) == KERNELS
    recorded = recorded_resources()
    assert sorted(recorded) == KERNELS
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (name, k)  # (spilled SGPRs go to lanes of a VGPR, not to memory)
        for word, bound in recorded[name].items():
            assert k[word] <= bound, (name, word, k[word], bound)
        assert k["lds"] == 6 * 4 * 256 * 4 + 440 * 8  # the Sobol byte tables and the sine / cosine table
    others = sorted(f for f in os.listdir(CSRC) if f.startswith("libmcrt_") and f.endswith(".so") and f != "libmcrt_lighting.so")
    assert len(others) >= 13, others
    for lib in others:
        names = [k["name"] for k in table.kernels_of(os.path.join(CSRC, lib))]
        assert names and not [n for n in names if n in KERNELS], lib


def test_the_libraries_find_the_lighting_library_next_to_themselves():
    assert os.path.exists(os.path.join(CSRC, "libmcrt_hip.so"))
    for lib in ("libmcrt_hip.so", "libmcrt_hip_tol.so"):
        path = os.path.join(CSRC, lib)
        if lib.endswith("_tol.so") and not os.path.exists(path):
            continue  # (MCRT_SKIP_TOLERANCE_BUILD=1 builds)
        dyn = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
        assert "[libmcrt_lighting.so]" in dyn, lib
        assert any("$ORIGIN" in l for l in dyn.splitlines() if "RUNPATH" in l or "RPATH" in l), lib


def test_the_calls_are_exported_and_the_abi_version_stays(pkg):
    L = pkg.lib()
    for name in ("mcrt_render_lighting", "mcrt_render_lighting_device"):
        assert hasattr(L, name), name
    assert L.mcrt_abi_version() == 2
    for name in ("LightingBuffers", "LIGHTING_CHANNELS"):
        assert hasattr(pkg, name), name
    for name in ("render_lighting", "render_lighting_device"):
        assert hasattr(pkg.Context, name), name
    assert list(pkg.LIGHTING_CHANNELS) == [k for k, _ in pkg.LightingBuffers._fields_] == CHANNELS


def test_the_binding_lays_the_struct_out_as_the_header_does(pkg, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcrt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",sizeof(mcrt_lighting_buffers),'
                   + ",".join("offsetof(mcrt_lighting_buffers,%s)" % k for k in CHANNELS) + ');return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(pkg.LightingBuffers)] + [getattr(pkg.LightingBuffers, k).offset for k in CHANNELS]


def test_a_null_context_is_refused(pkg):
    L = pkg.lib()
    cam, bufs = pkg.CameraDesc(), pkg.LightingBuffers()
    assert L.mcrt_render_lighting(None, C.byref(cam), 1, C.byref(bufs), None) == -1  # MCRT_ERR_INVALID
    assert L.mcrt_render_lighting_device(None, C.byref(cam), 1, C.byref(bufs), None) == -1


def test_exr_layers_of_the_lighting_passes_names_and_types(pkg):
    """lighting.emission.R/G/B ... lighting.unoccluded.R/G/B: colour, HALF, views of the arrays given; today's arguments give what they gave."""
    h, w = 3, 5
    res = {k: np.random.default_rng(i).random((h, w, 3)) for i, k in enumerate(CHANNELS)}
    rgb = np.zeros((h, w, 3))
    layers = pkg.exr_layers(rgb=rgb, lighting=res)
    assert list(layers) == ["R", "G", "B"] + ["lighting.%s.%s" % (k, c) for k in CHANNELS for c in "RGB"]
    assert all(kind == "half" for _, kind in layers.values()) and all(len(n) <= 31 for n in layers)
    assert np.array_equal(layers["lighting.light.G"][0], res["light"][..., 1])
    _, ptr, source, stride, offset = pkg._exr_source(layers["lighting.unoccluded.B"][0])
    assert (ptr, source, stride, offset) == (res["unoccluded"].ctypes.data, pkg.EXR_SRC_F64, 3, 2)
    assert pkg.exr_layers(lighting=res, pixel_types={"lighting.direct": "float"})["lighting.direct.R"][1] == "float"
    assert list(pkg.exr_layers(lighting={"sky": res["sky"]})) == ["lighting.sky.R", "lighting.sky.G", "lighting.sky.B"]
    assert list(pkg.exr_layers(rgb=rgb)) == list(pkg.exr_layers(rgb=rgb, lighting=None)) == list(pkg.exr_layers(rgb=rgb, lighting={})) == ["R", "G", "B"]


def test_exr_unlayer_gives_the_lighting_dict_back(pkg):
    h, w = 3, 5
    res = {k: np.random.default_rng(i).random((h, w, 3)) for i, k in enumerate(CHANNELS)}
    back = pkg.exr_unlayer({name: view for name, (view, _) in pkg.exr_layers(rgb=np.zeros((h, w, 3)), lighting=res).items()})
    assert sorted(back) == ["lighting", "rgb"] and sorted(back["lighting"]) == sorted(res)
    for k in res:
        assert np.array_equal(back["lighting"][k], res[k]), k
