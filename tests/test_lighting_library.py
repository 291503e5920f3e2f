"""What only the lighting passes have (tests/side_libraries.py holds what libmcrt_lighting.so may contain, within the registers
profiles/NOTES_lighting.md records): the binding's channels and struct layout, and what the calls refuse as far as no GPU is needed."""
import ctypes as C

import numpy as np

from side_libraries import c_values

CHANNELS = ["emission", "sky", "direct", "light", "unoccluded"]


def test_the_channels_of_the_binding_are_the_struct_s_fields(pkg):
    assert list(pkg.LIGHTING_CHANNELS) == [k for k, _ in pkg.LightingBuffers._fields_] == CHANNELS


def test_the_binding_lays_the_struct_out_as_the_header_does(pkg, tmp_path):
    sizes = c_values(tmp_path, ["sizeof(mcrt_lighting_buffers)"] + ["offsetof(mcrt_lighting_buffers,%s)" % k for k in CHANNELS], "%zu %zu %zu %zu %zu %zu")
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
