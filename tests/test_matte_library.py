"""What only the ID mattes have (tests/side_libraries.py holds what libmcrt_matte.so may contain; the tile form's keys are dynamic LDS,
sized per launch): the binding's struct layouts, exr_layers' names, strides and offsets, the attributes that name a layer."""
import ctypes as C

import numpy as np

from side_libraries import c_values


def test_the_binding_lays_the_structs_out_as_the_header_does(pkg, tmp_path):
    sizes = c_values(tmp_path, ["sizeof(mcrt_matte_params)", "sizeof(mcrt_matte_buffers)", "offsetof(mcrt_matte_params,surface_key)", "offsetof(mcrt_matte_params,names)",
                                "offsetof(mcrt_matte_params,reserved)", "offsetof(mcrt_matte_buffers,distinct)", "MCRT_MATTE_MATERIAL", "MCRT_MATTE_SURFACE",
                                "MCRT_MATTE_CUSTOM"], "%zu %zu %zu %zu %zu %zu %d %d %d")
    assert sizes == [C.sizeof(pkg.MatteParams), C.sizeof(pkg.MatteBuffers), pkg.MatteParams.surface_key.offset, pkg.MatteParams.names.offset,
                     pkg.MatteParams.reserved.offset, pkg.MatteBuffers.distinct.offset, pkg.MATTE_KEYS["material"], pkg.MATTE_KEYS["surface"],
                     pkg.MATTE_KEYS["custom"]]


def test_exr_layers_of_mattes_names_types_strides_and_offsets(pkg):
    """NAME00.R (id of rank 0), .G (its coverage), .B / .A (rank 1), NAME01.* (ranks 2 and 3) ...: views of the one "layer" buffer with
    stride 2 * ranks and offsets 0 .. 2 * ranks - 1, FLOAT whatever pixel_types says; today's arguments give what they gave."""
    h, w, ranks = 3, 5, 6
    layer = np.arange(h * w * ranks * 2, dtype=np.float64).reshape(h, w, ranks, 2)
    rgb = np.zeros((h, w, 3))
    layers = pkg.exr_layers(rgb=rgb, mattes={"CryptoMaterial": {"layer": layer}}, pixel_types={"CryptoMaterial00": "half", "CryptoMaterial01.G": "half", "R": "float"})
    names = ["CryptoMaterial%02d.%s" % (l, c) for l in range(ranks // 2) for c in "RGBA"]
    assert list(layers) == ["R", "G", "B"] + names
    assert all(len(n) <= 31 for n in layers)
    for i, name in enumerate(names):
        view, kind = layers[name]
        assert kind == "float" and view.shape == (h, w)
        assert np.array_equal(view, layer.reshape(h, w, 2 * ranks)[..., i])
        _, ptr, source, stride, offset = pkg._exr_source(view)
        assert (ptr, source, stride, offset) == (layer.ctypes.data, pkg.EXR_SRC_F64, 2 * ranks, i), name
    assert layers["R"][1] == "float" and layers["G"][1] == "half"
    assert list(pkg.exr_layers(rgb=rgb)) == list(pkg.exr_layers(rgb=rgb, mattes=None)) == list(pkg.exr_layers(rgb=rgb, mattes={})) == ["R", "G", "B"]
    two = pkg.exr_layers(mattes={"CryptoMaterial": {"layer": layer}, "CryptoObject": {"layer": layer[:, :, :2]}})
    assert len(two) == 4 * 3 + 4 and "CryptoObject00.A" in two and "CryptoObject01.R" not in two


def test_matte_attributes_name_the_layer(pkg):
    res = {"manifest": pkg.matte_manifest("material", 2)}
    attrs = pkg.matte_attributes("CryptoMaterial", res)
    k = "cryptomatte/%s/" % ("%08x" % pkg.matte_code("CryptoMaterial"))[:7]
    assert k == "cryptomatte/be359d6/"
    assert attrs == {k + "name": "CryptoMaterial", k + "hash": "MurmurHash3_32", k + "conversion": "uint32_to_float32", k + "manifest": res["manifest"]}
    assert all(len(n) <= 31 for n in attrs)
