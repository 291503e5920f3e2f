"""What only the pack of the OpenEXR output has (tests/side_libraries.py holds what libmcrt_exr.so may contain, and that zlib is not
linked: it is looked up when a ZIP file is first saved): the binding's struct layouts, exr_layers' names and types, the views."""
import ctypes as C

from side_libraries import c_values


def test_the_binding_lays_the_structs_out_as_the_header_does(pkg, tmp_path):
    sizes = c_values(tmp_path, ["sizeof(mcrt_exr_channel)", "sizeof(mcrt_exr_attribute)", "sizeof(mcrt_exr_params)", "sizeof(mcrt_exr_result)",
                                "offsetof(mcrt_exr_channel,stride)", "offsetof(mcrt_exr_result,chunks)"], "%zu %zu %zu %zu %zu %zu")
    assert sizes == [C.sizeof(pkg.ExrChannel), C.sizeof(pkg.ExrAttribute), C.sizeof(pkg.ExrParams), C.sizeof(pkg.ExrResult),
                     pkg.ExrChannel.stride.offset, pkg.ExrResult.chunks.offset]


def test_exr_layers_names_and_types(pkg):
    """The documented names and default types, from dicts shaped like the render_* and denoise_* methods' - no device needed."""
    import numpy as np
    h, w = 3, 5
    f3, f1 = np.zeros((h, w, 3)), np.zeros((h, w))
    aov = {k: (np.zeros((h, w) + ((n,) if n > 1 else ()), dtype=t)) for k, (t, n) in pkg.AOV_CHANNELS.items()}
    layers = pkg.exr_layers(rgb=f3, aov=aov, stats={"rgb": f3, "variance": f3, "half_a": f3, "half_b": f3},
                            highlights={"rgb": f3, "tops": np.zeros((h, w, 4, 3)), "level": f1},
                            robust={"robust": f3, "removed": f3, "clamped": np.zeros((h, w), dtype=np.uint32)},
                            denoised={"denoise": f3, "denoise_variance": (f3, f3), "denoise_dual": {"rgb": f3, "variance": f3}})
    rgb3, xyz = lambda p: [p + c for c in ("R", "G", "B")], lambda p: [p + c for c in ("X", "Y", "Z")]
    want = {n: "half" for n in rgb3("") + xyz("normal.") + xyz("shading_normal.") + rgb3("albedo.") + ["coverage.A"] + rgb3("half_a.") + rgb3("half_b.")
            + [n for k in range(4) for n in rgb3("tops%d." % k)] + rgb3("robust.") + rgb3("removed.") + rgb3("denoise.") + rgb3("denoise_variance.") + rgb3("denoise_dual.")}
    want.update({n: "float" for n in ["depth.Z", "level.Y"] + xyz("position.") + rgb3("variance.") + rgb3("denoise_variance.variance.") + rgb3("denoise_dual.variance.")})
    want.update({n: "uint" for n in ("surface.id", "material.id", "clamped.count")})
    assert {n: t for n, (_, t) in layers.items()} == want
    assert all(v.shape == (h, w) for v, _ in layers.values())
    assert all(len(n) <= 31 for n in layers)
    over = pkg.exr_layers(rgb=f3, aov={"normal": f3}, pixel_types={"R": "float", "normal": "float"})
    assert {n: t for n, (_, t) in over.items()} == {"R": "float", "G": "half", "B": "half", "normal.X": "float", "normal.Y": "float", "normal.Z": "float"}


def test_views_of_one_buffer_name_that_buffer(pkg):
    """Last-axis views become stride and offset of the packed buffer they look into; a view that is no such thing is copied."""
    import numpy as np
    h, w = 4, 6
    rgb, tops, ids = np.zeros((h, w, 3)), np.zeros((h, w, 4, 3)), np.zeros((h, w), dtype=np.uint32)
    for c in range(3):
        _, ptr, source, stride, offset = pkg._exr_source(rgb[..., c])
        assert (ptr, source, stride, offset) == (rgb.ctypes.data, pkg.EXR_SRC_F64, 3, c)
    _, ptr, source, stride, offset = pkg._exr_source(tops[:, :, 2, 1])
    assert (ptr, source, stride, offset) == (tops.ctypes.data, pkg.EXR_SRC_F64, 12, 7)
    _, ptr, source, stride, offset = pkg._exr_source(ids)
    assert (ptr, source, stride, offset) == (ids.ctypes.data, pkg.EXR_SRC_U32, 1, 0)
    kept, ptr, _, stride, offset = pkg._exr_source(rgb[::2, :, 0])   # rows skipped: not one stride per pixel
    assert (stride, offset) == (1, 0) and kept.shape == (2, w) and ptr == kept.ctypes.data and kept.flags["C_CONTIGUOUS"]
    one = pkg._exr_source(rgb[:1, :1, 2])                             # a single pixel: any stride serves
    assert one[1] + 8 * one[4] == rgb.ctypes.data + 16
