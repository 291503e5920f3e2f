"""The light groups are a code object of their own, like the image passes before them. libmcrt_light_groups.so holds exactly the pass's
four kernels, without scratch and within the registers profiles/NOTES_light_groups.md records (its table is read here: the numbers are
upper bounds); libmcrt_hip.so - the render path's device code, listed function by function in tests/golden/device_code_hashes.json - and
the other side libraries hold no kernel of these names, and the main libraries find the new one next to themselves (RUNPATH $ORIGIN).
What the calls refuse is checked here as far as no GPU is needed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc")
KERNELS = ["lightGroupsBeginKernel", "lightGroupsRayKernel", "lightGroupsResolveKernel", "lightGroupsStepKernel"]
SHADING = ("lightGroupsRayKernel", "lightGroupsStepKernel")
FIELDS = ["num_groups", "flags", "sky_plane", "max_depth", "surface_group"]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def recorded_resources():
    """The table of profiles/NOTES_light_groups.md: kernel -> dict of vgpr, vgpr_spill, sgpr_spill, scratch, lds."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "NOTES_light_groups.md")):
        m = re.match(r"\|\s*`(lightGroups\w+Kernel)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", line)
        if m:
            rows[m.group(1)] = dict(zip(("vgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds"), (int(x) for x in m.groups()[1:])))
    return rows


def test_the_light_group_kernels_live_beside_the_render_path(pkg):
    pkg.lib()
    table = _tool("kernel_spill_table")
    kernels = {k["name"]: k for k in table.kernels_of(os.path.join(CSRC, "libmcrt_light_groups.so"))}
    assert sorted(kernels) == KERNELS
    recorded = recorded_resources()
    assert sorted(recorded) == KERNELS
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (name, k)  # (spilled SGPRs go to lanes of a VGPR, not to memory)
        for word, bound in recorded[name].items():
            assert k[word] <= bound, (name, word, k[word], bound)
        # the Sobol byte tables, the sine / cosine table and 8 history entries for each of 256 lanes - or nothing
        assert k["lds"] == (6 * 4 * 256 * 4 + 440 * 8 + 8 * 256 * 8 if name in SHADING else 0), name
    others = sorted(f for f in os.listdir(CSRC) if f.startswith("libmcrt_") and f.endswith(".so") and f != "libmcrt_light_groups.so")
    assert len(others) >= 14, others
    for lib in others:
        names = [k["name"] for k in table.kernels_of(os.path.join(CSRC, lib))]
        assert names and not [n for n in names if n in KERNELS], lib


def test_the_libraries_find_the_light_group_library_next_to_themselves():
    assert os.path.exists(os.path.join(CSRC, "libmcrt_hip.so"))
    for lib in ("libmcrt_hip.so", "libmcrt_hip_tol.so"):
        path = os.path.join(CSRC, lib)
        if lib.endswith("_tol.so") and not os.path.exists(path):
            continue  # (MCRT_SKIP_TOLERANCE_BUILD=1 builds)
        dyn = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
        assert "[libmcrt_light_groups.so]" in dyn, lib
        assert any("$ORIGIN" in l for l in dyn.splitlines() if "RUNPATH" in l or "RPATH" in l), lib


def test_the_calls_are_exported_and_the_abi_version_stays(pkg):
    L = pkg.lib()
    for name in ("mcrt_render_light_groups", "mcrt_render_light_groups_device", "mcrt_light_group_planes"):
        assert hasattr(L, name), name
    assert L.mcrt_abi_version() == 2
    for name in ("LightGroupParams", "LIGHT_GROUPS_MAX", "LIGHT_GROUPS_SKY_PLANE", "light_group_map"):
        assert hasattr(pkg, name), name
    for name in ("render_light_groups", "render_light_groups_device"):
        assert hasattr(pkg.Context, name), name
    assert [k for k, _ in pkg.LightGroupParams._fields_] == FIELDS


def test_the_binding_lays_the_struct_out_as_the_header_does(pkg, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcrt.h"\nint main(void){printf("%zu %u %u ' + "%zu " * len(FIELDS)
                   + '\\n",sizeof(mcrt_light_group_params),MCRT_LIGHT_GROUPS_MAX,(unsigned)MCRT_LIGHT_GROUPS_SKY_PLANE,'
                   + ",".join("offsetof(mcrt_light_group_params,%s)" % k for k in FIELDS) + ');return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(pkg.LightGroupParams), pkg.LIGHT_GROUPS_MAX, pkg.LIGHT_GROUPS_SKY_PLANE] + [getattr(pkg.LightGroupParams, k).offset for k in FIELDS]
    assert sizes[0] == 24


def test_the_number_of_planes(pkg):
    L = pkg.lib()
    assert L.mcrt_light_group_planes(None) == 2  # one group and the sky

    def planes(groups, sky=None):
        return L.mcrt_light_group_planes(C.byref(pkg.LightGroupParams(groups, 0 if sky is None else pkg.LIGHT_GROUPS_SKY_PLANE, sky or 0, 0, None)))
    assert [planes(0), planes(1), planes(1, 0), planes(1, 1), planes(3), planes(3, 1), planes(3, 3), planes(15), planes(15, 15), planes(15, 0)] == [2, 2, 1, 2, 4, 3, 4, 16, 16, 15]
    assert planes(16) == 0 and planes(1, 2) == 0 and planes(15, 16) == 0  # out of range
    par = pkg.LightGroupParams(1, 0, 9, 0, None)  # sky_plane without its flag is not read
    assert L.mcrt_light_group_planes(C.byref(par)) == 2


def test_a_null_context_is_refused(pkg):
    L = pkg.lib()
    cam, par = pkg.CameraDesc(), pkg.LightGroupParams()
    out = np.zeros(3)
    assert L.mcrt_render_light_groups(None, C.byref(cam), 1, C.byref(par), out.ctypes.data, None) == -1  # MCRT_ERR_INVALID
    assert L.mcrt_render_light_groups_device(None, C.byref(cam), 1, None, out.ctypes.data, None) == -1


def test_exr_layers_of_the_light_groups_names_and_types(pkg):
    """lightgroup.<name>.R/G/B: colour, HALF, views of the array given; today's arguments give what they gave; exr_unlayer gives the planes back."""
    h, w = 3, 5
    planes = np.random.default_rng(5).random((3, h, w, 3))
    names = ["material1", "material2", "sky"]
    rgb = np.zeros((h, w, 3))
    layers = pkg.exr_layers(rgb=rgb, light_groups=(planes, names))
    assert list(layers) == ["R", "G", "B"] + ["lightgroup.%s.%s" % (k, c) for k in names for c in "RGB"]
    assert all(kind == "half" for _, kind in layers.values()) and all(len(n) <= 31 for n in layers)
    assert np.array_equal(layers["lightgroup.material2.G"][0], planes[1][..., 1])
    _, ptr, source, stride, offset = pkg._exr_source(layers["lightgroup.sky.B"][0])
    assert (ptr, source, stride, offset) == (planes[2].ctypes.data, pkg.EXR_SRC_F64, 3, 2)
    assert pkg.exr_layers(light_groups=(planes, names), pixel_types={"lightgroup.sky": "float"})["lightgroup.sky.R"][1] == "float"
    assert list(pkg.exr_layers(rgb=rgb)) == list(pkg.exr_layers(rgb=rgb, light_groups=None)) == ["R", "G", "B"]
    back = pkg.exr_unlayer({name: view for name, (view, _) in layers.items()})
    assert sorted(back) == ["light_groups", "rgb"] and back["light_groups"][1] == names
    assert np.array_equal(back["light_groups"][0], planes)
