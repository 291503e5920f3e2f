"""Firefly suppression (mcrt_render_highlights*, mcrt_robust_resolve*), CPU tier: csrc/mcrt_robust.hpp - the text the two kernels of
csrc/mcrt_robust.hip run - driven on the host (tests/emu/robust_emu.cpp: each kernel as a loop over its lanes) against the text of
include/mcrt.h ("Firefly suppression") written out HERE in numpy, sample by sample and tap by tap in the stated order. The samples are
the oracle's own per-sample radiance (test_pixel_stats_emulation.oracle_case) and hand-made stores.

Bound: assert_array_equal on the bits. Derived, not measured: both sides execute the same IEEE-754 double operations (+ - * /, compare,
select) in the same order, none of them a libm call, neither side contracted (the harness is built with -ffp-contract=off, numpy's
ufuncs are one operation each) - so every bit agrees, NaNs included. The one tolerance is the energy identity
L(S / n) ~ ((n - K) level + sum_k L(tops_k)) / n: the two sides add the same n non-negative samples in different orders and take the
luminance before or after, 3 (n + 2) roundings of relative size 2^-53 at most on either side, for n <= 16 below 1e-14 - held to the
1e-12 the GPU tests use."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_pixel_stats_emulation as ps
from emu_build import build_emu

WIDTH, HEIGHT, SEED = ps.WIDTH, ps.HEIGHT, ps.SEED
TOPS = 4
ORACLE_SCENES = ps.ORACLE_SCENES
SENTINEL = -7.25
bits = ps.bits


def load_robust_emu():
    L = C.CDLL(build_emu("robust_emu.cpp"))
    vp = C.c_void_p
    L.robust_highlights_emu.argtypes = [vp, C.c_uint64, C.c_uint32, vp, vp]
    L.robust_resolve_emu.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_double, C.c_double, C.c_uint32, vp, vp, vp]
    return L


@functools.lru_cache(maxsize=None)
def _emu():
    return load_robust_emu()


def robust_tops(n):
    return min(TOPS, n // 4)


def luminance(x):
    return (0.2126 * x[..., 0] + 0.7152 * x[..., 1]) + 0.0722 * x[..., 2]


def numpy_highlights(store):
    """include/mcrt.h's "Highlights of a render" in numpy on a store [n][...][3], sample by sample -> dict tops [...][4][3], level [...]
    and index [...][4] (the list's sample indices, -1 = empty place)."""
    store = np.asarray(store, dtype=np.float64)
    n, shape = store.shape[0], store.shape[1:-1]
    x = store.reshape(n, -1, 3)
    P, K = x.shape[1], robust_tops(n)
    with np.errstate(all="ignore"):
        lum = luminance(x)  # [n][P]
        el = np.zeros((TOPS, P))
        ei = np.full((TOPS, P), -1, dtype=np.int64)
        count = np.zeros(P, dtype=np.int64)
        for i in range(n):
            li = lum[i]
            pos = np.full(P, K)  # K: the sample does not enter
            for e in reversed(range(K)):  # (the FIRST entry it exceeds)
                pos = np.where((e < count) & (li > el[e]), e, pos)
            pos = np.where((pos == K) & (count < K), count, pos)  # appended
            pos = np.where(np.isnan(li), K, pos)
            for e in reversed(range(K)):
                if e > 0:
                    el[e] = np.where(pos < e, el[e - 1], el[e])
                    ei[e] = np.where(pos < e, ei[e - 1], ei[e])
                el[e] = np.where(pos == e, li, el[e])
                ei[e] = np.where(pos == e, i, ei[e])
            count = np.where(pos < K, np.minimum(count + 1, K), count)
        tops = np.zeros((P, TOPS, 3))
        cols = np.arange(P)
        for k in range(TOPS):
            have = ei[k] >= 0
            tops[have, k] = x[ei[k][have], cols[have]]
        rest = np.zeros((P, 3))
        for i in range(n):
            listed = (ei == i).any(axis=0)
            rest = np.where(listed[:, None], rest, rest + x[i])
        level = luminance(rest / float(n - K))
    return {"tops": tops.reshape(shape + (TOPS, 3)), "level": level.reshape(shape), "index": ei.T.reshape(shape + (TOPS,))}


def numpy_resolve(rgb, tops, level, spp, kappa=8.0, floor=0.0, radius=1):
    """include/mcrt.h's "Robust resolve" in numpy on full frames -> dict out, removed, clamped."""
    rgb, tops, level = np.asarray(rgb, dtype=np.float64), np.asarray(tops, dtype=np.float64), np.asarray(level, dtype=np.float64)
    H, W = level.shape
    K, R = robust_tops(spp), int(radius)
    with np.errstate(all="ignore"):
        M = np.full((H, W), -np.inf)
        ys, xs = np.mgrid[0:H, 0:W]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                lq = level[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                M = np.where(inside & (M < lq), lq, M)
        t = kappa * M
        T = np.where(t > floor, t, floor)
        removed = np.zeros((H, W, 3))
        count = np.zeros((H, W), dtype=np.uint32)
        for k in range(K):
            x = tops[:, :, k, :]
            lk = luminance(x)
            hit = lk > T
            f = T / lk
            removed = np.where(hit[..., None], removed + (x - x * f[..., None]), removed)
            count = count + hit.astype(np.uint32)
        q = removed / float(spp)
        o = rgb - q
        o = np.where(o < 0.0, 0.0, o)
        out = np.where((count > 0)[..., None], o, rgb)
    return {"out": out, "removed": q, "clamped": count}


def emu_highlights(store, channels=("tops", "level")):
    """The emulation on a store [spp][pixels][3] -> dict tops [pixels][4][3], level [pixels]; channels left out get a NULL pointer and
    come back as the sentinel they were filled with."""
    store = np.ascontiguousarray(store, dtype=np.float64)
    spp, pixels = store.shape[:2]
    out = {"tops": np.full((pixels, TOPS, 3), SENTINEL), "level": np.full(pixels, SENTINEL)}
    K = _emu().robust_highlights_emu(store.ctypes.data, pixels, spp, *[out[k].ctypes.data if k in channels else None for k in ("tops", "level")])
    assert K == robust_tops(spp)
    return out


def emu_resolve(rgb, tops, level, spp, kappa=8.0, floor=0.0, radius=1, in_place=False, buffers=("removed", "clamped")):
    rgb = np.array(rgb, dtype=np.float64, order="C")
    tops, level = np.ascontiguousarray(tops, dtype=np.float64), np.ascontiguousarray(level, dtype=np.float64)
    H, W = level.shape
    assert rgb.shape == (H, W, 3) and tops.shape == (H, W, TOPS, 3)
    out = rgb if in_place else np.full((H, W, 3), SENTINEL)
    removed, clamped = np.full((H, W, 3), SENTINEL), np.full((H, W), 77, dtype=np.uint32)
    rc = _emu().robust_resolve_emu(W, H, spp, rgb.ctypes.data, tops.ctypes.data, level.ctypes.data, kappa, floor, radius, out.ctypes.data,
                                   removed.ctypes.data if "removed" in buffers else None, clamped.ctypes.data if "clamped" in buffers else None)
    assert rc == 0, rc
    return {"out": out, "removed": removed, "clamped": clamped}


def assert_same(got, want, keys, msg=""):
    for k in keys:
        if got[k].dtype == np.uint32:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (msg, k))
        else:
            np.testing.assert_array_equal(bits(got[k]), bits(want[k].reshape(got[k].shape)), err_msg="%s %s" % (msg, k))


@functools.lru_cache(maxsize=None)
def oracle_highlights(scene, sqrtspp, integrator=None):
    """The oracle's frame and store of ps.oracle_case with the numpy highlights and the numpy robust frame (defaults): computed once."""
    frame, store, stats = ps.oracle_case(scene, sqrtspp, integrator)
    hl = numpy_highlights(store)
    res = numpy_resolve(frame, hl["tops"], hl["level"], sqrtspp * sqrtspp)
    for a in tuple(hl.values()) + tuple(res.values()):
        a.setflags(write=False)
    return frame, store, hl, res


def energy_identity_error(mean, tops, level, n):
    """|L(S / n) - ((n - K) level + sum_k L(tops_k)) / n| relative to the former (module docstring)."""
    K = robust_tops(n)
    with np.errstate(all="ignore"):
        back = float(n - K) * level
        for k in range(K):
            back = back + luminance(tops[..., k, :])
        lm = luminance(mean)
        return np.abs(back / float(n) - lm) / np.maximum(np.abs(lm), 1e-300)


@pytest.mark.parametrize("sqrtspp", [1, 2, 3, 4])  # K = 0, 1, 2, 4
@pytest.mark.parametrize("scene", ORACLE_SCENES)
def test_text_on_the_oracles_samples_is_the_header_in_numpy(scene, sqrtspp):
    frame, store, hl, res = oracle_highlights(scene, sqrtspp)
    n = sqrtspp * sqrtspp
    K = robust_tops(n)
    assert K == {1: 0, 2: 1, 3: 2, 4: 4}[sqrtspp]
    got = emu_highlights(store.reshape(n, -1, 3))
    assert_same(got, hl, ("tops", "level"), "%s sqrtspp %d" % (scene, sqrtspp))
    # the list is what a stable sort gives (no NaN in an oracle's store): luminance descending, index ascending
    lum = luminance(store)  # [n][H][W]
    order = np.argsort(-lum, axis=0, kind="stable")[:K]
    np.testing.assert_array_equal(np.moveaxis(order, 0, -1), hl["index"][..., :K])
    assert (hl["index"][..., K:] == -1).all() and not hl["tops"][..., K:, :].any()
    mean = ps.oracle_case(scene, sqrtspp)[2]["mean"]
    if K == 0:
        np.testing.assert_array_equal(bits(hl["level"]), bits(luminance(mean)))
    err = energy_identity_error(mean, hl["tops"], hl["level"], n)
    print("%s sqrtspp %d: energy identity, max relative error %.3e" % (scene, sqrtspp, err.max()))
    assert err.max() <= 1e-12
    # the resolve of that frame, defaults
    r = emu_resolve(frame, hl["tops"], hl["level"], n)
    assert_same(r, res, ("out", "removed", "clamped"), "%s sqrtspp %d" % (scene, sqrtspp))
    untouched = res["clamped"] == 0
    np.testing.assert_array_equal(bits(res["out"][untouched]), bits(frame[untouched]))
    assert (res["clamped"] <= K).all() and (res["out"] <= frame).all() and (res["out"] >= 0).all()
    if K == 0:
        assert untouched.all() and not res["removed"].any()


def _store(spp, pixels, seed):
    rng = np.random.default_rng(seed)
    return rng.random((spp, pixels, 3)) * rng.choice([1e-3, 1.0, 40.0], size=(1, pixels, 1))


@pytest.mark.parametrize("pixels", [1, 63, 65, 257])  # less than a wave, a wave and a lane, a workgroup and a lane
@pytest.mark.parametrize("spp", list(range(1, 18)))   # K = 0 .. 4; 8 and 16: whole batches of 8 planes, 17: a batch with a rest
def test_hand_made_stores(pixels, spp):
    store = _store(spp, pixels, 1000 * spp + pixels)
    assert_same(emu_highlights(store), numpy_highlights(store), ("tops", "level"), "%d pixels, %d spp" % (pixels, spp))


@pytest.mark.parametrize("spp", [4, 9, 16, 17])
def test_equal_luminances_go_to_the_lower_index(spp):
    """Samples in a few luminance classes (channel values of few bits, so that equal means equal): within a class the list keeps the
    lower indices, in ascending order; with ALL samples equal the list is samples 0 .. K-1 and the level their luminance."""
    rng = np.random.default_rng(spp)
    K = robust_tops(spp)
    store = np.repeat(rng.integers(1, 4, size=(spp, 257, 1)).astype(np.float64) * 0.25, 3, axis=2)
    want = numpy_highlights(store)
    assert_same(emu_highlights(store), want, ("tops", "level"))
    np.testing.assert_array_equal(np.argsort(-store[:, :, 0], axis=0, kind="stable")[:K].T, want["index"][:, :K])
    same = np.full((spp, 65, 3), 0.375)
    got = emu_highlights(same)
    assert_same(got, numpy_highlights(same), ("tops", "level"))
    np.testing.assert_array_equal(numpy_highlights(same)["index"][:, :K], np.tile(np.arange(K), (65, 1)))
    assert (got["tops"][:, :K] == 0.375).all() and not got["tops"][:, K:].any()
    np.testing.assert_array_equal(bits(got["level"]), bits(np.full(65, luminance(np.full(3, 0.375)))))


@pytest.mark.parametrize("spp", [4, 9, 16])
def test_a_planted_firefly_is_kept_aside_and_clamped(spp):
    W, H = 13, 5
    K = robust_tops(spp)
    store = _store(spp, W * H, 77)
    store[:, :, :] = np.random.default_rng(1).random((spp, W * H, 3)) * 0.5 + 0.25  # one scale: no pixel outshines its neighbours
    clean = numpy_highlights(store)
    planted = store.copy()
    planted[spp - 1, 31] = 1e9
    got = emu_highlights(planted)
    want = numpy_highlights(planted)
    assert_same(got, want, ("tops", "level"))
    assert (got["tops"][31, 0] == 1e9).all() and want["index"][31, 0] == spp - 1
    assert got["level"][31] < 1.0  # the level does not see it
    others = np.arange(W * H) != 31
    np.testing.assert_array_equal(bits(got["level"][others]), bits(clean["level"][others]))
    frame = planted.sum(axis=0).reshape(H, W, 3) / spp
    args = (frame, got["tops"].reshape(H, W, TOPS, 3), got["level"].reshape(H, W), spp)
    r = emu_resolve(*args)
    assert_same(r, numpy_resolve(*args), ("out", "removed", "clamped"))
    y, x = divmod(31, W)
    assert r["clamped"][y, x] >= 1 and r["clamped"].sum() == r["clamped"][y, x]
    assert (r["out"][y, x] < 8.0 * 1.0 + 1.0).all() and (frame[y, x] > 1e7).all()
    assert K >= 1


def test_nan_inf_and_negative_samples():
    spp, pixels = 16, 257
    store = _store(spp, pixels, 9)
    clean = emu_highlights(store)
    dirty = store.copy()
    dirty[4, 100, 1] = np.nan          # its luminance is NaN: never in the list, it reaches the level
    dirty[3, 256, 2] = np.inf          # the last pixel: the first entry of its list, the level stays finite
    dirty[:, 200, :] = -dirty[:, 200, :]  # negative samples are ordered like any other
    dirty[:, 50, 0] = np.nan           # every sample NaN: an empty list
    got = emu_highlights(dirty)
    want = numpy_highlights(dirty)
    assert_same(got, want, ("tops", "level"))
    other = np.ones(pixels, dtype=bool)
    other[[100, 256, 200, 50]] = False
    for k in ("tops", "level"):
        np.testing.assert_array_equal(bits(got[k][other]), bits(clean[k][other]), err_msg=k)
    assert np.isnan(got["level"][100]) and np.isfinite(got["tops"][100]).all() and 4 not in want["index"][100]
    assert np.isinf(got["tops"][256, 0, 2]) and want["index"][256, 0] == 3 and np.isfinite(got["level"][256])
    assert (got["tops"][200] < 0).all() and got["level"][200] < 0
    assert (want["index"][50] == -1).all() and not got["tops"][50].any() and np.isnan(got["level"][50])


@pytest.mark.parametrize("left_out", ["tops", "level"])
def test_a_null_channel_is_not_written(left_out):
    store = _store(9, 257, 11)
    full = emu_highlights(store)
    kept = "level" if left_out == "tops" else "tops"
    got = emu_highlights(store, channels=(kept,))
    assert (got[left_out] == SENTINEL).all()
    np.testing.assert_array_equal(bits(got[kept]), bits(full[kept]))
    none = emu_highlights(store, channels=())
    assert (none["tops"] == SENTINEL).all() and (none["level"] == SENTINEL).all()


def resolve_inputs(width, height, spp, seed):
    """A frame with its highlights from a hand-made store in which about one pixel in seven carries a bright sample."""
    rng = np.random.default_rng(seed)
    store = rng.random((spp, height * width, 3)) * 0.5 + 0.25
    bright = rng.random(height * width) < 0.15
    store[rng.integers(0, spp), bright] *= rng.choice([30.0, 1e4], size=(int(bright.sum()), 1))
    hl = numpy_highlights(store)
    frame = ps.numpy_pixel_stats(store)["mean"].reshape(height, width, 3)
    return frame, hl["tops"].reshape(height, width, TOPS, 3), hl["level"].reshape(height, width)


FRAMES = [(1, 1), (9, 1), (1, 9), (70, 13), (257, 3)]  # (width, height)


@pytest.mark.parametrize("radius", [1, 2, 8])  # 8: larger than most of the frames
@pytest.mark.parametrize("width,height", FRAMES)
def test_resolve_is_the_header_in_numpy(width, height, radius):
    for spp in (4, 9, 16, 3):
        frame, tops, level = resolve_inputs(width, height, spp, 100 * width + radius + spp)
        want = numpy_resolve(frame, tops, level, spp, radius=radius)
        got = emu_resolve(frame, tops, level, spp, radius=radius)
        assert_same(got, want, ("out", "removed", "clamped"), "%dx%d radius %d spp %d" % (width, height, radius, spp))
        if spp == 3:
            assert not want["clamped"].any()
        elif width * height > 500 and radius == 1:  # (the two frames large enough for the planted samples to be a fraction)
            assert want["clamped"].any() and (want["clamped"] == 0).any()
        # kappa and floor take part
        want2 = numpy_resolve(frame, tops, level, spp, kappa=1.0, floor=0.6, radius=radius)
        assert_same(emu_resolve(frame, tops, level, spp, kappa=1.0, floor=0.6, radius=radius), want2, ("out", "removed", "clamped"))
        # in place, and with the two buffers left out
        here = emu_resolve(frame, tops, level, spp, radius=radius, in_place=True, buffers=())
        np.testing.assert_array_equal(bits(here["out"]), bits(want["out"]))
        assert (here["removed"] == SENTINEL).all() and (here["clamped"] == 77).all()


@pytest.mark.parametrize("width,height", FRAMES)
def test_a_floor_above_everything_gives_the_frames_bits(width, height):
    frame, tops, level = resolve_inputs(width, height, 16, width)
    got = emu_resolve(frame, tops, level, 16, floor=1e300)
    np.testing.assert_array_equal(bits(got["out"]), bits(frame))
    assert not got["removed"].any() and not got["clamped"].any()
    assert_same(got, numpy_resolve(frame, tops, level, 16, floor=1e300), ("out", "removed", "clamped"))


def test_a_nan_level_is_never_taken_and_an_inf_level_switches_the_clamp_off_in_its_window():
    W, H, spp = 70, 13, 16
    frame, tops, level = resolve_inputs(W, H, spp, 5)
    base = numpy_resolve(frame, tops, level, spp)
    dirty = level.copy()
    dirty[4, 20] = np.nan
    dirty[9, 50] = np.inf
    frame2, tops2 = frame.copy(), tops.copy()
    frame2[2, 60, 1] = np.nan     # a NaN of the frame stays in its pixel
    tops2[11, 5, 0, 0] = np.nan   # a top whose luminance is NaN is not clamped
    tops2[9, 49, 0] = 1e12        # next to the Inf level: not clamped either
    frame2[9, 49] = 1e12 / spp
    want = numpy_resolve(frame2, tops2, dirty, spp)
    got = emu_resolve(frame2, tops2, dirty, spp)
    assert_same(got, want, ("out", "removed", "clamped"))
    assert not got["clamped"][8:11, 49:52].any()
    np.testing.assert_array_equal(bits(got["out"][8:11, 49:52]), bits(frame2[8:11, 49:52]))
    assert np.isnan(got["out"][2, 60, 1]) and np.isfinite(got["out"][2, 60, [0, 2]]).all()
    far = np.ones((H, W), dtype=bool)
    far[3:6, 19:22] = far[8:11, 49:52] = False
    far[2, 60] = far[11, 5] = False
    for k in ("out", "removed", "clamped"):
        np.testing.assert_array_equal(got[k][far], base[k][far], err_msg=k)
    # the NaN level's window: M is the largest of the other levels, so the pixel itself is still resolved
    assert np.isfinite(got["out"][4, 20]).all()
    alone = emu_resolve(frame[:1, :1], tops[:1, :1], np.full((1, 1), np.nan), spp)  # every level NaN: M stays -inf, T = floor = 0
    assert_same(alone, numpy_resolve(frame[:1, :1], tops[:1, :1], np.full((1, 1), np.nan), spp), ("out", "removed", "clamped"))
    assert alone["clamped"][0, 0] == 4


def test_what_the_library_refuses_the_harness_refuses():
    frame, tops, level = resolve_inputs(9, 1, 16, 1)
    for bad in ({"kappa": 0.5}, {"kappa": np.inf}, {"floor": -1.0}, {"floor": np.nan}, {"radius": 9}):
        args = dict(kappa=8.0, floor=0.0, radius=1)
        args.update(bad)
        out = np.zeros_like(frame)
        assert _emu().robust_resolve_emu(9, 1, 16, frame.ctypes.data, tops.ctypes.data, level.ctypes.data, args["kappa"], args["floor"], args["radius"],
                                         out.ctypes.data, None, None) == -1, bad
