"""What only the path classes have (tests/side_libraries.py holds what libmcrt_path_classes.so may contain, within the registers
profiles/NOTES_path_classes.md records): the binding's struct layout and class numbers, the number of planes, the presets, and what the
calls refuse as far as no GPU is needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from side_libraries import CSRC, ROOT, c_values

FIELDS = ["flags", "max_depth", "class_plane"]
NAMES = ["emission", "background", "diffuse_direct", "diffuse_indirect", "glossy_direct", "glossy_indirect", "transmission_direct", "transmission_indirect"]


def test_the_binding_has_the_header_s_fields_and_class_names(pkg):
    assert [k for k, _ in pkg.PathClassParams._fields_] == FIELDS
    assert list(pkg.PATH_CLASS_NAMES) == NAMES


def test_the_binding_lays_the_struct_out_as_the_header_does(pkg, tmp_path):
    """... and numbers the classes as the header does."""
    sizes = c_values(tmp_path, ["sizeof(mcrt_path_class_params)", "MCRT_PATH_CLASSES", "(unsigned)MCRT_PATH_CLASSES_MAP"]
                     + ["offsetof(mcrt_path_class_params,%s)" % k for k in FIELDS] + ["(int)MCRT_PATH_CLASS_" + n.upper() for n in NAMES],
                     "%zu %u %u " + "%zu " * len(FIELDS) + "%d " * 8)
    assert sizes == [C.sizeof(pkg.PathClassParams), pkg.PATH_CLASSES, pkg.PATH_CLASSES_MAP] + [getattr(pkg.PathClassParams, k).offset for k in FIELDS] + list(range(8))
    assert sizes[0] == 16 and C.sizeof(pkg.PathClassParams().class_plane) == 8


def test_the_number_of_planes(pkg):
    L = pkg.lib()
    assert L.mcrt_path_class_planes(None) == 8

    def planes(entries, flag=True):
        par = pkg.PathClassParams(pkg.PATH_CLASSES_MAP if flag else 0, 0)
        par.class_plane[:] = entries
        return L.mcrt_path_class_planes(C.byref(par))
    assert planes([0] * 8) == 1 and planes(list(range(8))) == 8 and planes([0, 1, 2, 2, 3, 3, 4, 4]) == 5 and planes([0, 0, 0, 0, 0, 0, 0, 7]) == 8
    assert planes([3] * 8) == 4  # (planes 0 .. 2 without a class: they come back as zeros)
    assert planes([0, 1, 2, 3, 4, 5, 6, 8]) == 0 and planes([255] + [0] * 7) == 0  # out of range
    assert planes([9] * 8, flag=False) == 8  # class_plane without its flag is not read
    assert pkg.lib().mcrt_path_class_planes(C.byref(pkg.Context._path_class_params(None, 3))) == 8


def test_a_null_context_is_refused(pkg):
    L = pkg.lib()
    cam, par = pkg.CameraDesc(), pkg.PathClassParams()
    out = np.zeros(3)
    assert L.mcrt_render_path_classes(None, C.byref(cam), 1, C.byref(par), out.ctypes.data, None) == -1  # MCRT_ERR_INVALID
    assert L.mcrt_render_path_classes_device(None, C.byref(cam), 1, None, out.ctypes.data, None) == -1


def test_path_class_map_presets(pkg):
    plane, names = pkg.path_class_map()
    assert plane.dtype == np.uint8 and list(plane) == list(range(8)) and names == NAMES
    plane, names = pkg.path_class_map(merge="lobes")
    assert list(plane) == [0, 1, 2, 2, 3, 3, 4, 4] and names == ["emission", "background", "diffuse", "glossy", "transmission"]
    plane, names = pkg.path_class_map(merge="one")
    assert list(plane) == [0] * 8 and names == ["beauty"]
    with pytest.raises(ValueError):
        pkg.path_class_map(merge="lights")
    par = pkg.Context._path_class_params(pkg.path_class_map("lobes")[0], 2)
    assert (par.flags, par.max_depth, list(par.class_plane)) == (pkg.PATH_CLASSES_MAP, 2, [0, 1, 2, 2, 3, 3, 4, 4])
    assert pkg.lib().mcrt_path_class_planes(C.byref(par)) == len(pkg.path_class_map("lobes")[1])


def test_exr_layers_of_the_path_classes_names_and_types(pkg):
    """pathclass.<name>.R/G/B: colour, HALF, views of the array given; today's arguments give what they gave; exr_unlayer gives the planes
    back. One name is longer than the 31 bytes of OpenEXR's short names: Context.exr_save then asks for the long-names file."""
    h, w = 3, 5
    planes = np.random.default_rng(6).random((8, h, w, 3))
    rgb = np.zeros((h, w, 3))
    layers = pkg.exr_layers(rgb=rgb, path_classes=(planes, NAMES))
    assert list(layers) == ["R", "G", "B"] + ["pathclass.%s.%s" % (k, c) for k in NAMES for c in "RGB"]
    assert all(kind == "half" for _, kind in layers.values())
    assert sorted(n for n in layers if len(n) > 31) == ["pathclass.transmission_indirect.%s" % c for c in "BGR"] and all(len(n) <= 255 for n in layers)
    assert np.array_equal(layers["pathclass.glossy_direct.G"][0], planes[4][..., 1])
    _, ptr, source, stride, offset = pkg._exr_source(layers["pathclass.background.B"][0])
    assert (ptr, source, stride, offset) == (planes[1].ctypes.data, pkg.EXR_SRC_F64, 3, 2)
    assert pkg.exr_layers(path_classes=(planes, NAMES), pixel_types={"pathclass.emission": "float"})["pathclass.emission.R"][1] == "float"
    assert list(pkg.exr_layers(rgb=rgb)) == list(pkg.exr_layers(rgb=rgb, path_classes=None)) == ["R", "G", "B"]
    back = pkg.exr_unlayer({name: view for name, (view, _) in layers.items()})
    assert sorted(back) == ["path_classes", "rgb"] and back["path_classes"][1] == NAMES
    assert np.array_equal(back["path_classes"][0], planes)
    lobes = pkg.path_class_map("lobes")[1]
    both = pkg.exr_layers(light_groups=(planes[:2], ["lights", "sky"]), path_classes=(planes[:5], lobes))
    back = pkg.exr_unlayer({name: view for name, (view, _) in both.items()})
    assert back["light_groups"][1] == ["lights", "sky"] and back["path_classes"][1] == lobes and all(len(n) <= 31 for n in both)


def test_long_channel_names_are_an_option_of_the_exr_writer(pkg, tmp_path):
    """MCRT_EXR_LONG_NAMES: the plan of a file (mcrt_exr_file.hpp, no GPU needed for a refusal) takes names of up to 255 bytes with the
    flag and refuses 32 without it, as before."""
    src = tmp_path / "plan.cpp"
    src.write_text('#include <cstdio>\n#include <string>\n#include "mcrt_exr_file.hpp"\nint main(){ using namespace mcrt; double d[3]={0,0,0}; std::string n33(33,\'x\'), n256(256,\'x\'), why;\n'
                   'mcrt_exr_channel c{n33.c_str(), d, MCRT_EXR_SRC_F64, MCRT_EXR_HALF, 3, 0}; mcrt_exr_params p{}; p.compression = MCRT_EXR_COMPRESSION_SET | MCRT_EXR_COMPRESSION_NONE;\n'
                   'ExrPlan a, b, e; int r0 = exrPlan("f", 1, 1, &c, 1, nullptr, 0, &p, a, why); p.flags = MCRT_EXR_LONG_NAMES; int r1 = exrPlan("f", 1, 1, &c, 1, nullptr, 0, &p, b, why);\n'
                   'c.name = n256.c_str(); int r2 = exrPlan("f", 1, 1, &c, 1, nullptr, 0, &p, e, why);\n'
                   'std::printf("%d %d %d %d %d\\n", r0, r1, r2, (int)b.header[4], (int)b.header[5]); return 0; }\n')
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", str(exe), str(src), "-ldl", "-pthread"])
    assert subprocess.check_output([str(exe)]).split() == [b"-1", b"0", b"-1", b"2", b"4"]
    assert pkg.EXR_LONG_NAMES == 2
