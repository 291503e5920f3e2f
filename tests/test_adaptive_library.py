"""What only adaptive sampling has (tests/side_libraries.py holds what libmcrt_adaptive.so may contain, within the registers
profiles/NOTES_adaptive.md records): the binding's struct layouts and parameters, and what the calls refuse as far as no GPU is needed."""
import ctypes as C

import numpy as np

from side_libraries import c_values

PARAM_FIELDS = ["target_relative_error", "floor", "max_spp", "min_batches", "window"]
RESULT_FIELDS = ["batches", "min_count", "max_count", "samples", "active"]


def test_the_structs_of_the_binding_have_the_header_s_fields(pkg):
    assert [k for k, _ in pkg.AdaptiveParams._fields_] == PARAM_FIELDS and [k for k, _ in pkg.AdaptiveResult._fields_] == RESULT_FIELDS


def test_the_binding_lays_the_structs_out_as_the_header_does(pkg, tmp_path):
    sizes = c_values(tmp_path, ["sizeof(mcrt_adaptive_params)", "sizeof(mcrt_adaptive_result)", "(unsigned)MCRT_CONVERGE_TRACE", "(unsigned)MCRT_ADAPTIVE_WINDOW_NONE"]
                     + ["offsetof(mcrt_adaptive_params,%s)" % k for k in PARAM_FIELDS] + ["offsetof(mcrt_adaptive_result,%s)" % k for k in RESULT_FIELDS],
                     "%zu %zu %u %u " + "%zu " * (len(PARAM_FIELDS) + len(RESULT_FIELDS)))
    assert sizes == [C.sizeof(pkg.AdaptiveParams), C.sizeof(pkg.AdaptiveResult), pkg.CONVERGE_TRACE, pkg.ADAPTIVE_WINDOW_NONE] + \
        [getattr(pkg.AdaptiveParams, k).offset for k in PARAM_FIELDS] + [getattr(pkg.AdaptiveResult, k).offset for k in RESULT_FIELDS]
    assert sizes[0] == 32


def test_the_parameters_of_the_binding(pkg):
    par = pkg.Context._adaptive_params(0.25)
    assert (par.target_relative_error, par.floor, par.max_spp, par.min_batches, par.window) == (0.25, 0.0, 0, 0, 0)
    par = pkg.Context._adaptive_params(0.25, 64, 0.5, 0, 3)
    assert (par.floor, par.max_spp, par.min_batches, par.window) == (0.5, 64, 3, pkg.ADAPTIVE_WINDOW_NONE)  # radius 0 is not "the default"
    assert pkg.Context._adaptive_params(0.25, window=4).window == 4


def test_a_null_context_is_refused(pkg):
    L = pkg.lib()
    cam, par = pkg.CameraDesc(), pkg.AdaptiveParams()
    out = np.zeros(3)
    count = np.zeros(1, dtype=np.uint32)
    assert L.mcrt_render_adaptive(None, C.byref(cam), 1, C.byref(par), out.ctypes.data, None, count.ctypes.data, None, None) == -1  # MCRT_ERR_INVALID
    assert L.mcrt_render_adaptive_device(None, C.byref(cam), 1, None, out.ctypes.data, None, None, None, None) == -1
    flags = np.ones(4, dtype=np.uint8)
    assert L.mcrt_adaptive_list(None, 4, flags.ctypes.data, count.ctypes.data, C.byref(C.c_uint32())) == -1


def test_exr_layers_of_an_adaptive_render_names_and_types(pkg):
    """samples.count: UINT, a view of the count map; the statistics under their existing names; today's arguments give what they gave."""
    h, w = 3, 5
    rng = np.random.default_rng(8)
    res = {"rgb": rng.random((h, w, 3)), "variance": rng.random((h, w, 3)), "half_a": rng.random((h, w, 3)), "count": rng.integers(4, 64, (h, w)).astype(np.uint32),
           "result": {"batches": 3}}
    layers = pkg.exr_layers(rgb=res["rgb"], adaptive=res)
    assert list(layers) == ["R", "G", "B", "samples.count"] + ["%s.%s" % (k, c) for k in ("variance", "half_a") for c in "RGB"]
    assert layers["samples.count"][1] == "uint" and layers["variance.R"][1] == "float" and layers["half_a.G"][1] == "half"
    assert layers["samples.count"][0] is res["count"] or np.shares_memory(layers["samples.count"][0], res["count"])
    _, ptr, source, stride, offset = pkg._exr_source(layers["samples.count"][0])
    assert (ptr, source, stride, offset) == (res["count"].ctypes.data, pkg.EXR_SRC_U32, 1, 0)
    assert list(pkg.exr_layers(rgb=res["rgb"])) == list(pkg.exr_layers(rgb=res["rgb"], adaptive=None)) == ["R", "G", "B"]
    stats_names = list(pkg.exr_layers(stats={k: res[k] for k in ("variance", "half_a")}))
    assert stats_names == [n for n in layers if n.split(".")[0] in ("variance", "half_a")]
