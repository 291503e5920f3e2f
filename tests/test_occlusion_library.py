"""What only the occlusion pass has (tests/side_libraries.py holds what libmcrt_occlusion.so may contain): the binding's channels and struct
layouts, and what the calls refuse as far as no GPU is needed: a NULL context by the library, the parameters by the validation the host
side calls (csrc/mcrt_occlusion.hpp occlusionSettingsOf, built into the CPU tier's emulation)."""
import ctypes as C
import math

import numpy as np

from side_libraries import c_values


def test_the_channels_of_the_binding_are_the_struct_s_fields(pkg):
    assert list(pkg.OCCLUSION_CHANNELS) == [k for k, _ in pkg.OcclusionBuffers._fields_]


def test_the_binding_lays_the_structs_out_as_the_header_does(pkg, tmp_path):
    sizes = c_values(tmp_path, ["sizeof(mcrt_occlusion_params)", "sizeof(mcrt_occlusion_buffers)", "offsetof(mcrt_occlusion_params,flags)",
                                "offsetof(mcrt_occlusion_params,max_distance)", "offsetof(mcrt_occlusion_buffers,sky)", "offsetof(mcrt_occlusion_buffers,bent_normal)",
                                "MCRT_OCCLUSION_GEOMETRIC", "MCRT_OCCLUSION_MAX_RAYS"], "%zu %zu %zu %zu %zu %zu %u %u")
    assert sizes == [C.sizeof(pkg.OcclusionParams), C.sizeof(pkg.OcclusionBuffers), pkg.OcclusionParams.flags.offset, pkg.OcclusionParams.max_distance.offset,
                     pkg.OcclusionBuffers.sky.offset, pkg.OcclusionBuffers.bent_normal.offset, pkg.OCCLUSION_GEOMETRIC, pkg.OCCLUSION_MAX_RAYS]
    assert sizes[0] == 16


def test_a_null_context_is_refused(pkg):
    L = pkg.lib()
    cam, par, bufs = pkg.CameraDesc(), pkg.OcclusionParams(), pkg.OcclusionBuffers()
    assert L.mcrt_render_occlusion(None, C.byref(cam), 1, C.byref(par), C.byref(bufs), None) == -1  # MCRT_ERR_INVALID
    assert L.mcrt_render_occlusion_device(None, C.byref(cam), 1, None, C.byref(bufs), None) == -1


def test_parameters_outside_the_definition_are_refused(pkg):
    """rays above 64, a negative or non-finite max_distance, unknown flag bits; NULL and rays == 0 mean one ray."""
    import test_occlusion_emulation as occ
    L = occ.load_occlusion_emu()

    def settings(par):
        rays = C.c_uint32(0)
        why = L.occlusion_emu_settings(C.byref(par) if par is not None else None, C.byref(rays))
        return (why.decode() if why else None), rays.value

    assert settings(None) == (None, 1)
    assert settings(pkg.OcclusionParams(0, 0, 0.0)) == (None, 1)
    assert settings(pkg.OcclusionParams(64, pkg.OCCLUSION_GEOMETRIC, 2.5)) == (None, 64)
    assert "rays" in settings(pkg.OcclusionParams(65, 0, 0.0))[0]
    assert "flag" in settings(pkg.OcclusionParams(1, 2, 0.0))[0] and "flag" in settings(pkg.OcclusionParams(1, 0x80000001, 0.0))[0]
    for bad in (-1.0, -1e-300, math.inf, -math.inf, math.nan):
        assert "max_distance" in settings(pkg.OcclusionParams(1, 0, bad))[0], bad
    assert settings(pkg.OcclusionParams(1, 0, np.finfo(np.float64).max)) == (None, 1)


def test_exr_layers_of_the_occlusion_pass_names_and_types(pkg):
    """occlusion.ao, occlusion.sky, occlusion.bent.X/Y/Z: HALF like the AOV pass's coverage and normals, views of the arrays given; today's
    arguments give what they gave."""
    h, w = 3, 5
    res = {"ao": np.random.default_rng(1).random((h, w)), "sky": np.zeros((h, w)), "bent_normal": np.arange(h * w * 3, dtype=np.float64).reshape(h, w, 3)}
    rgb = np.zeros((h, w, 3))
    layers = pkg.exr_layers(rgb=rgb, occlusion=res)
    assert list(layers) == ["R", "G", "B", "occlusion.ao", "occlusion.sky", "occlusion.bent.X", "occlusion.bent.Y", "occlusion.bent.Z"]
    assert all(kind == "half" for _, kind in layers.values()) and all(len(n) <= 31 for n in layers)
    assert layers["occlusion.ao"][0] is res["ao"] and np.array_equal(layers["occlusion.bent.Y"][0], res["bent_normal"][..., 1])
    _, ptr, source, stride, offset = pkg._exr_source(layers["occlusion.bent.Z"][0])
    assert (ptr, source, stride, offset) == (res["bent_normal"].ctypes.data, pkg.EXR_SRC_F64, 3, 2)
    assert pkg.exr_layers(occlusion=res, pixel_types={"occlusion.bent": "float", "occlusion.ao": "float"})["occlusion.bent.X"][1] == "float"
    assert list(pkg.exr_layers(occlusion={"sky": res["sky"]})) == ["occlusion.sky"]
    assert list(pkg.exr_layers(rgb=rgb)) == list(pkg.exr_layers(rgb=rgb, occlusion=None)) == list(pkg.exr_layers(rgb=rgb, occlusion={})) == ["R", "G", "B"]


def test_exr_unlayer_gives_the_occlusion_dict_back(pkg):
    h, w = 3, 5
    res = {"ao": np.random.default_rng(2).random((h, w)), "sky": np.ones((h, w)), "bent_normal": np.arange(h * w * 3, dtype=np.float64).reshape(h, w, 3)}
    back = pkg.exr_unlayer({name: view for name, (view, _) in pkg.exr_layers(rgb=np.zeros((h, w, 3)), occlusion=res).items()})
    assert sorted(back) == ["occlusion", "rgb"] and sorted(back["occlusion"]) == sorted(res)
    for k in res:
        assert np.array_equal(back["occlusion"][k], res[k]), k
    assert pkg.exr_unlayer({"occlusion.sky": res["sky"], "occlusion.bent.X": res["ao"]}) == {"occlusion": {"sky": res["sky"]}, "other": {"occlusion.bent.X": res["ao"]}}
