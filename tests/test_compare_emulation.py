"""Frame comparison (mcrt_frame_compare*), CPU tier: csrc/mcrt_compare.hpp - the text the three kernels of csrc/mcrt_compare.hip run - on
emulated wavefronts (tests/emu/compare_emu.cpp on wave_emu.hpp, driven launch by launch as the library drives them) against the
definition of include/mcrt.h ("Frame comparison") written out HERE in numpy, operation by operation in the stated order; the treesum is
restated here from the header's words (blocks of 256, stride 128 .. 1, again on the block values).

Bound: == on the bits of every field and every map. Derived, not measured: both sides execute the same IEEE-754 double operations
(+ - * /, compare, select) in the same order, none of them a libm call, neither side contracted (the harness is built with
-ffp-contract=off, numpy's ufuncs are one operation each); sqrt and log10 of the final scalars are the host's in both (numpy's sqrt is
correctly rounded like the C library's; log10 is the one routine that could differ between two C libraries, and both sides call the same).

Shapes (width x height): 70 x 13 (no multiple of a wavefront, a workgroup or a tile), 11 x 11 (one SSIM centre), 10 x 40 and 40 x 10 (no
centre), 12 x 11, and 257 x 256 - 65 792 pixels, a third treesum level with a ragged last block, a ragged centre grid. The small shapes
run the full cross of input case x mask x want_ssim x maps x tile shape; at 257 x 256 every input case runs with and without the mask
(SSIM and all maps on, the library's tile), and the random case runs the other settings: what the settings change - which stores
happen, how centres map to workgroups - does not depend on the frame's content."""
import ctypes as C
import functools
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TESTS
from emu_build import build_emu

SMALL = ((70, 13), (11, 11), (10, 40), (40, 10), (12, 11))
LARGE = (257, 256)
CASES = ("random", "same", "zeros", "nan_rgb", "inf_ref", "nan_both", "ties", "hdr")
MAPS = ("squared_error", "relative", "ssim")
SENTINEL = -7.25
NONE64, NONE32 = 2 ** 64 - 1, 2 ** 32 - 1


class Params(C.Structure):
    _fields_ = [("eps", C.c_double), ("peak", C.c_double), ("ssim_range", C.c_double), ("want_ssim", C.c_int32), ("reserved", C.c_uint32)]


class Maps(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in MAPS]


class Result(C.Structure):
    _fields_ = ([(k, C.c_double) for k in ("sum_se", "sum_ae", "sum_rel", "sum_ssim", "max_abs")] + [("max_abs_pixel", C.c_uint64), ("max_abs_channel", C.c_uint32),
                ("reserved", C.c_uint32)] + [(k, C.c_uint64) for k in ("pixels", "compared", "nonfinite", "masked", "differing", "ssim_centres", "ssim_excluded")] +
                [(k, C.c_double) for k in ("mse", "mae", "relmse", "rmse", "psnr", "mean_ssim")])


FIELDS = [k for k, _ in Result._fields_ if k != "reserved"]


def load_compare_emu():
    L = C.CDLL(build_emu("compare_emu.cpp"))
    vp = C.c_void_p
    L.compare_emu.argtypes = [C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(Params), C.POINTER(Maps), C.POINTER(Result), C.c_int, C.c_int]
    L.compare_emu_weight.argtypes = [C.c_uint32]
    L.compare_emu_weight.restype = C.c_double
    L.compare_emu_ssim_lds_bytes.restype = C.c_uint32
    return L


@functools.lru_cache(maxsize=None)
def _emu():
    return load_compare_emu()


def header_weights():
    """g[-5 .. 5] from the literals of include/mcrt.h: the definition."""
    text = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    lit = {int(k): float.fromhex(v) for k, v in re.findall(r"#define MCRT_SSIM_G(\d) (0x[0-9a-fA-F.]+p[-+]?\d+)", text)}
    assert sorted(lit) == [0, 1, 2, 3, 4, 5], lit
    return np.array([lit[abs(i)] for i in range(-5, 6)])


def bits(x):
    return struct.pack("<d", float(x))


def numpy_treesum(values):
    """include/mcrt.h's treesum: the values in blocks of 256 consecutive ones (the last may be shorter: len values); inside a block, for
    stride = 128 .. 1: t[k] = t[k] + t[k + stride] for every k < stride with k + stride < len; the block values the same way again."""
    t = np.array(values, dtype=np.float64).ravel()
    assert t.size > 0
    with np.errstate(all="ignore"):
        while True:
            blocks = -(-t.size // 256)
            padded = np.zeros(blocks * 256)
            padded[:t.size] = t
            padded = padded.reshape(blocks, 256)
            length = np.minimum(256, t.size - 256 * np.arange(blocks))[:, None]
            stride = 128
            while stride:
                pair = np.arange(stride)[None, :] + stride < length
                padded[:, :stride] = np.where(pair, padded[:, :stride] + padded[:, stride:2 * stride], padded[:, :stride])
                stride //= 2
            t = padded[:, 0].copy()
            if blocks == 1:
                return float(t[0])


def numpy_compare(rgb, ref, mask=None, eps=0.01, peak=1.0, ssim_range=1.0, ssim=True):
    """include/mcrt.h "Frame comparison" -> dict of the result's fields and the three maps ("ssim" None without SSIM)."""
    rgb, ref = np.asarray(rgb, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    height, width = rgb.shape[:2]
    r = {}
    with np.errstate(all="ignore"):
        masked = ~(mask > 0) if mask is not None else np.zeros((height, width), dtype=bool)
        finite = np.all(rgb - rgb == 0.0, axis=2) & np.all(ref - ref == 0.0, axis=2)
        nonfinite = ~masked & ~finite
        compared = ~masked & finite
        differs = ~masked & np.any(rgb.view(np.uint64) != ref.view(np.uint64), axis=2)
        d = rgb - ref
        a = np.where(d < 0, 0.0 - d, d)
        se = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        ae = (a[..., 0] + a[..., 1]) + a[..., 2]
        q = (d * d) / (ref * ref + eps)
        rel = (q[..., 0] + q[..., 1]) + q[..., 2]
        se, ae, rel = (np.where(compared, v, 0.0) for v in (se, ae, rel))
        r["sum_se"], r["sum_ae"], r["sum_rel"] = numpy_treesum(se), numpy_treesum(ae), numpy_treesum(rel)
        r["pixels"], r["compared"], r["nonfinite"], r["masked"], r["differing"] = (int(x) for x in (height * width, compared.sum(), nonfinite.sum(), masked.sum(), differs.sum()))
        if r["compared"]:
            flat = np.where(compared[..., None], a, -1.0).ravel()
            at = int(np.argmax(flat))  # the first of the largest: the lowest pixel, then the lowest channel
            r["max_abs"], r["max_abs_pixel"], r["max_abs_channel"] = float(flat[at]), at // 3, at % 3
            n = float(3 * r["compared"])
            r["mse"], r["mae"], r["relmse"] = r["sum_se"] / n, r["sum_ae"] / n, r["sum_rel"] / n
            r["rmse"] = float(np.sqrt(r["mse"]))
            r["psnr"] = float("inf") if r["mse"] == 0.0 else 10.0 * _log10(peak * peak / r["mse"])
        else:
            r["max_abs"], r["max_abs_pixel"], r["max_abs_channel"] = 0.0, NONE64, NONE32
            r["mse"] = r["mae"] = r["relmse"] = r["rmse"] = r["psnr"] = 0.0
        r["squared_error"], r["relative"], r["ssim"] = se, rel, None
        r["sum_ssim"], r["ssim_centres"], r["ssim_excluded"], r["mean_ssim"] = 0.0, 0, 0, 0.0
        if ssim:
            r["ssim"] = np.zeros((height, width))
        if ssim and width >= 11 and height >= 11:
            g = header_weights()
            cw, ch = width - 10, height - 10
            lum = lambda x: (0.2126 * x[..., 0] + 0.7152 * x[..., 1]) + 0.0722 * x[..., 2]
            lx, lr = lum(rgb), lum(ref)
            w = []
            for f in (lx, lr, lx * lx, lr * lr, lx * lr):
                h = np.zeros((height, cw))
                for k in range(11):
                    h = h + g[k] * f[:, k:k + cw]
                v = np.zeros((ch, cw))
                for k in range(11):
                    v = v + g[k] * h[k:k + ch, :]
                w.append(v)
            mx, mr = w[0], w[1]
            sxx, srr, sxr = w[2] - mx * mx, w[3] - mr * mr, w[4] - mx * mr
            c1, c2 = (0.01 * ssim_range) * (0.01 * ssim_range), (0.03 * ssim_range) * (0.03 * ssim_range)
            s = ((2.0 * (mx * mr) + c1) * (2.0 * sxr + c2)) / (((mx * mx + mr * mr) + c1) * ((sxx + srr) + c2))
            fin = s - s == 0.0
            s = np.where(fin, s, 0.0)
            r["sum_ssim"], r["ssim_centres"], r["ssim_excluded"] = numpy_treesum(s), cw * ch, int((~fin).sum())
            if r["ssim_centres"] > r["ssim_excluded"]:
                r["mean_ssim"] = r["sum_ssim"] / float(r["ssim_centres"] - r["ssim_excluded"])
            r["ssim"][5:height - 5, 5:width - 5] = s
    return r


def _log10(x):
    """The C library's log10, which the host side of the library calls."""
    libm = C.CDLL("libm.so.6")
    libm.log10.restype = C.c_double
    libm.log10.argtypes = [C.c_double]
    return libm.log10(float(x))


def emu_compare(rgb, ref, mask=None, eps=None, peak=None, ssim_range=None, ssim=True, maps=MAPS, tile=0, vec=-1, params=True):
    """The emulation -> dict of the result's fields, the maps asked for (others: None) and "launches". Maps come back with the
    sentinel they were filled with where nothing was written."""
    rgb, ref = np.ascontiguousarray(rgb, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)
    height, width = rgb.shape[:2]
    par = Params(eps or 0.0, peak or 0.0, ssim_range or 0.0, 1 if ssim else 0, 0)
    out = {k: np.full((height, width), SENTINEL) for k in maps}
    m, res = Maps(**{k: v.ctypes.data for k, v in out.items()}), Result()
    rc = _emu().compare_emu(width, height, rgb.ctypes.data, ref.ctypes.data, mask.ctypes.data if mask is not None else None,
                            C.byref(par) if params else None, C.byref(m) if maps else None, C.byref(res), tile, vec)
    assert rc > 0, "compare_emu: %d" % rc
    r = {k: getattr(res, k) for k in FIELDS}
    r.update({k: out.get(k) for k in MAPS})
    r["launches"] = rc
    return r


def assert_same(got, want, maps=MAPS, ssim=True, what=""):
    """Every field and every map asked for, bit for bit."""
    for k in FIELDS:
        if isinstance(want[k], float):
            assert bits(got[k]) == bits(want[k]), (what, k, got[k], want[k])
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])
    for k in MAPS:
        if k in maps and (ssim or k != "ssim"):
            np.testing.assert_array_equal(np.asarray(got[k]).view(np.uint64), want[k].view(np.uint64), err_msg="%s %s" % (what, k))
        elif k in maps:  # the ssim map without SSIM: not written
            assert np.all(np.asarray(got[k]) == SENTINEL), (what, k)
        else:
            assert got[k] is None, (what, k)


@functools.lru_cache(maxsize=None)
def frames(case, width, height):
    """(rgb, ref, mask) of an input case, read-only. Planted values sit at pixel n // 3 (also the mask's NaN: a pixel that is both
    counts as masked), at n // 2 (the frame's middle: inside an SSIM window wherever there is one) and at n - 2."""
    rng = np.random.default_rng(0x5EED0A0F + 131 * width + height)
    n = width * height
    ref = rng.random((n, 3))
    rgb = ref + (rng.random((n, 3)) - 0.5) * 0.125
    nan2 = np.frombuffer(struct.pack("<Q", 0x7FF8000000000123), dtype=np.float64)[0]  # a NaN with a payload
    if case == "same":
        rgb = ref.copy()
    elif case == "zeros":
        rgb = ref.copy()
        ref[n // 3], rgb[n // 3] = (0.0, 0.5, 0.0), (-0.0, 0.5, 0.0)
        ref[n // 2, 2], rgb[n // 2, 2] = -0.0, 0.0
    elif case == "nan_rgb":
        rgb[n // 3, 1], rgb[n // 2, 0], rgb[n - 2, 2] = np.nan, np.inf, -np.inf
    elif case == "inf_ref":
        ref[n // 3, 0], ref[n // 2, 2], ref[0, 1] = np.inf, np.nan, -np.inf
    elif case == "nan_both":  # equal bits: not differing, still not compared
        for p, c, v in ((n // 3, 0, np.nan), (n // 2, 1, nan2), (n - 2, 2, np.inf)):
            rgb[p] = ref[p]
            rgb[p, c] = ref[p, c] = v
        rgb[1, 0], ref[1, 0] = np.nan, nan2  # two NaNs of different bits: differing
    elif case == "ties":  # 0.5 three times: channels 1 and 2 of pixel n // 2 and, later, channel 0 of pixel n - 2 -> pixel n // 2, channel 1
        rgb = ref.copy()
        ref[n // 2], rgb[n // 2] = (0.25, 0.25, 0.75), (0.25, 0.75, 0.25)
        ref[n - 2, 0], rgb[n - 2, 0] = 0.25, 0.75
    elif case == "hdr":  # values far from [0, 1], a negative one, a large error
        ref = ref * 1000.0
        rgb = ref * (1.0 + (rng.random((n, 3)) - 0.5) * 0.5)
        rgb[n // 2] = (-3.0, 1e150, 1e-300)
    else:
        assert case == "random", case
    mask = np.where(rng.random(n) < 0.1, 0.0, rng.random(n) + 0.001)
    mask[n // 3], mask[5], mask[n - 1] = np.nan, -1.0, -0.0
    mask[n // 2] = mask[n - 2] = mask[0] = mask[1] = 1.0  # (the other planted pixels take part)
    out = rgb.reshape(height, width, 3), ref.reshape(height, width, 3), mask.reshape(height, width)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wanted(case, width, height, with_mask, ssim=True):
    """The numpy definition of an input case, computed once and shared (the GPU tier reads it too); read-only."""
    rgb, ref, mask = frames(case, width, height)
    r = numpy_compare(rgb, ref, mask if with_mask else None, ssim=ssim)
    for k in MAPS:
        if r[k] is not None:
            r[k].setflags(write=False)
    return r


MAP_SETS = (MAPS, (), ("squared_error",), ("relative",), ("ssim",))


@pytest.mark.parametrize("width,height", SMALL)
@pytest.mark.parametrize("case", CASES)
def test_small_frames_full_cross(case, width, height):
    rgb, ref, mask = frames(case, width, height)
    for with_mask, ssim, maps, tile in itertools.product((False, True), (True, False), MAP_SETS, (0, 1)):
        if not ssim and tile:
            continue  # (the tile is the SSIM kernel's alone)
        want = wanted(case, width, height, with_mask, ssim)
        got = emu_compare(rgb, ref, mask if with_mask else None, ssim=ssim, maps=maps, tile=tile)
        assert_same(got, want, maps, ssim, (case, with_mask, ssim, maps, tile))


@pytest.mark.parametrize("with_mask", (False, True))
@pytest.mark.parametrize("case", CASES)
def test_large_frame_every_case(case, with_mask):
    rgb, ref, mask = frames(case, *LARGE)
    got = emu_compare(rgb, ref, mask if with_mask else None)
    assert_same(got, wanted(case, *LARGE, with_mask), what=(case, with_mask))
    assert got["launches"] == 2 + 2  # pixels, SSIM, and two upper levels: 257 blocks -> 2 -> 1


def test_large_frame_other_settings():
    rgb, ref, mask = frames("random", *LARGE)
    for ssim, maps, tile in ((False, MAPS, 0), (True, MAPS, 1), (True, MAPS, 2), (True, ("squared_error",), 0), (True, ("relative",), 0), (True, ("ssim",), 1), (True, (), 0)):
        got = emu_compare(rgb, ref, mask, ssim=ssim, maps=maps, tile=tile)
        assert_same(got, wanted("random", *LARGE, True, ssim), maps, ssim, (ssim, maps, tile))


def test_what_the_special_cases_say():
    """The properties the cases were built for, stated on the numpy definition (which the tests above hold the kernels to)."""
    for width, height in SMALL + (LARGE,):
        n = width * height
        same = wanted("same", width, height, False)
        assert same["sum_se"] == same["sum_ae"] == same["sum_rel"] == 0.0 and same["differing"] == 0 and same["psnr"] == float("inf") and same["max_abs"] == 0.0
        assert (same["max_abs_pixel"], same["max_abs_channel"]) == (0, 0) and same["compared"] == n
        if width >= 11 and height >= 11:
            assert np.all(same["ssim"][5:height - 5, 5:width - 5] == 1.0) and same["ssim_excluded"] == 0
            assert same["ssim_centres"] == (width - 10) * (height - 10) and same["mean_ssim"] == 1.0
        else:
            assert same["ssim_centres"] == 0 and same["mean_ssim"] == 0.0 and not same["ssim"].any()
        zeros = wanted("zeros", width, height, False)
        assert zeros["differing"] == 2 and zeros["sum_se"] == 0.0 and zeros["compared"] == n
        assert wanted("zeros", width, height, True)["differing"] == 1  # (pixel n // 3 is masked)
        for case, differing in (("nan_rgb", n), ("inf_ref", n), ("nan_both", n - 3)):
            r = wanted(case, width, height, False)
            assert (r["nonfinite"], r["compared"], r["differing"]) == (4 if case == "nan_both" else 3, n - (4 if case == "nan_both" else 3), differing), case
            assert np.isfinite([r["sum_se"], r["sum_ae"], r["sum_rel"], r["sum_ssim"]]).all()
            assert (r["ssim_excluded"] > 0) == (width >= 11 and height >= 11)
            m = wanted(case, width, height, True)
            assert m["nonfinite"] < r["nonfinite"] and m["masked"] + m["nonfinite"] + m["compared"] == n
        ties = wanted("ties", width, height, False)
        assert (ties["max_abs"], ties["max_abs_pixel"], ties["max_abs_channel"]) == (0.5, n // 2, 1)
    nothing = numpy_compare(*frames("random", 11, 11)[:2], mask=np.zeros((11, 11)))
    assert (nothing["compared"], nothing["max_abs"], nothing["max_abs_pixel"], nothing["max_abs_channel"], nothing["mse"], nothing["psnr"]) == (0, 0.0, NONE64, NONE32, 0.0, 0.0)
    assert nothing["ssim_centres"] == 1 and nothing["mean_ssim"] != 0.0  # (SSIM ignores the mask)


def test_nothing_compared_and_the_parameters():
    rgb, ref, _ = frames("random", 12, 11)
    zero = np.zeros((11, 12))
    assert_same(emu_compare(rgb, ref, zero), numpy_compare(rgb, ref, zero), what="all masked")
    for eps, peak, rng_ in ((0.25, 255.0, 4.0), (1e-6, 0.5, 1000.0)):
        got = emu_compare(rgb, ref, None, eps=eps, peak=peak, ssim_range=rng_)
        assert_same(got, numpy_compare(rgb, ref, None, eps, peak, rng_), what=(eps, peak, rng_))
    assert_same(emu_compare(rgb, ref, None, params=False), numpy_compare(rgb, ref), what="params NULL")
    bad = Result()
    for par in (Params(-1.0, 0, 0, 1, 0), Params(0, float("nan"), 0, 1, 0), Params(0, 0, float("inf"), 1, 0)):
        assert _emu().compare_emu(12, 11, rgb.ctypes.data, ref.ctypes.data, None, C.byref(par), None, C.byref(bad), 0, -1) == -1
    assert _emu().compare_emu(0, 11, rgb.ctypes.data, ref.ctypes.data, None, None, None, C.byref(bad), 0, -1) == -1
    assert _emu().compare_emu(12, 11, None, ref.ctypes.data, None, None, None, C.byref(bad), 0, -1) == -1


def test_both_load_forms_and_a_frame_that_is_not_16_byte_aligned():
    """The 16-byte loads run where both frames are 16-byte aligned, the 8-byte loads otherwise: the same bits either way."""
    width, height = 70, 13
    rgb, ref, mask = frames("nan_rgb", width, height)
    want = wanted("nan_rgb", width, height, True)
    assert rgb.ctypes.data % 16 == 0 and ref.ctypes.data % 16 == 0  # (numpy's allocations are)
    assert_same(emu_compare(rgb, ref, mask, vec=0), want, what="8-byte loads")
    store = np.zeros(width * height * 3 + 1)
    odd = store[1:].reshape(height, width, 3)
    odd[...] = rgb
    assert odd.ctypes.data % 16 == 8
    par, res = Params(0, 0, 0, 1, 0), Result()
    rc = _emu().compare_emu(width, height, odd.ctypes.data, ref.ctypes.data, mask.ctypes.data, C.byref(par), None, C.byref(res), 0, -1)
    assert rc > 0
    assert_same({**{k: getattr(res, k) for k in FIELDS}, **{k: None for k in MAPS}}, want, (), what="unaligned frame")


def test_the_header_weights():
    """The literals against numpy's exp-and-normalise: within 1 ulp each, symmetric, and what the kernels take."""
    g = header_weights()
    i = np.arange(-5, 6, dtype=np.float64)
    w = np.exp(-(i * i) / 4.5)
    w = w / w.sum()
    assert np.all(np.abs(g - w) <= np.spacing(w))
    assert np.array_equal(g, g[::-1]) and len(set(g.tolist())) == 6
    assert [_emu().compare_emu_weight(k) for k in range(11)] == g.tolist()
    assert abs(g.sum() - 1.0) < 1e-15
    assert _emu().compare_emu_ssim_lds_bytes() == 50752  # three workgroups per 160 KB


def test_stand_alone_sanitizer_run(tmp_path):
    """tests/emu/compare_emu.cpp as a program of its own (its own main, no Python) on the 70 x 13 case, under AddressSanitizer and
    UndefinedBehaviorSanitizer: once, as a subprocess."""
    exe = str(tmp_path / "compare_emu_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DCOMPARE_EMU_MAIN", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread", "-o", exe, os.path.join(TESTS, "emu", "compare_emu.cpp"), "-ldl"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, (run.returncode, run.stdout, run.stderr[-2000:])
    assert run.stdout.startswith("compared ")


def test_the_probe_restates_the_same_definition():
    """tools/compare_probe.py --numpy carries a restatement of its own (a tool does not import the tests): it is this file's."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("compare_probe", os.path.join(ROOT, "tools", "compare_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    for case, (width, height) in (("nan_rgb", (70, 13)), ("ties", (12, 11)), ("hdr", (40, 10)), ("same", (11, 11))):
        rgb, ref, mask = frames(case, width, height)
        for with_mask in (False, True):
            want = wanted(case, width, height, with_mask)
            assert probe.same(probe.restate(rgb, ref, mask if with_mask else None), want) == [], (case, with_mask)
    rgb, ref, _ = frames("random", 70, 13)
    assert probe.same(probe.restate(rgb, ref, None, 0.25, 255.0, 4.0, False), numpy_compare(rgb, ref, None, 0.25, 255.0, 4.0, False)) == []
