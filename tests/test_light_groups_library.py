"""What only the light groups have (tests/side_libraries.py holds what libmcrt_light_groups.so may contain, within the registers
profiles/NOTES_light_groups.md records): the binding's struct layout, the number of planes, and what the calls refuse as far as no GPU is
needed."""
import ctypes as C

import numpy as np

from side_libraries import c_values

FIELDS = ["num_groups", "flags", "sky_plane", "max_depth", "surface_group"]


def test_the_struct_of_the_binding_has_the_header_s_fields(pkg):
    assert [k for k, _ in pkg.LightGroupParams._fields_] == FIELDS


def test_the_binding_lays_the_struct_out_as_the_header_does(pkg, tmp_path):
    sizes = c_values(tmp_path, ["sizeof(mcrt_light_group_params)", "MCRT_LIGHT_GROUPS_MAX", "(unsigned)MCRT_LIGHT_GROUPS_SKY_PLANE"]
                     + ["offsetof(mcrt_light_group_params,%s)" % k for k in FIELDS], "%zu %u %u " + "%zu " * len(FIELDS))
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
