"""Accumulated rendering (mcrt_frame_merge*), CPU tier: csrc/mcrt_accumulate.hpp - the text the kernel of csrc/mcrt_accumulate.hip runs -
driven on the host (tests/emu/accumulate_emu.cpp: the kernel as a loop over its lanes) against the text of include/mcrt.h ("Accumulated
rendering") written out HERE in numpy, operation by operation in the stated order.

Bounds. Emulation against numpy: assert_array_equal on the bits - both sides execute the same IEEE-754 double operations (+ - * /, compare,
select) in the same order, none of them a libm call, neither side contracted (the harness is built with -ffp-contract=off, numpy's ufuncs
are one operation each).
Meaning - the merge of two summaries against the statistics of the concatenated samples (the oracle's own per-sample radiance at two
seeds): tops are copies of samples and ties resolve as in the concatenation, so assert_array_equal; mean, halves and level add the same
non-negative terms in two orders, at most a few (n + 3) roundings of 2^-53, under 1e-14 for n <= 32, held to the 1e-12 relative the robust
tests use; the variance's d = m_b - m_a cancels in units of the mean, so its bound is |merged - direct| <= 1e-12 (direct + m m) per channel.
Derived, not fitted; the figures are printed before they are asserted.
Exact case: stores of small integers, 16 + 16 samples, whose sums are multiples of 16 and whose sums of squared deviations are multiples of
15 - every intermediate of both routes is then exact up to the one last division, which divides the same two numbers on both sides."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_pixel_stats_emulation as ps
import test_robust_emulation as rb
from emu_build import build_emu

SEED = ps.SEED
TOPS = 4
SENTINEL = -7.25
bits = ps.bits
luminance = rb.luminance
CHANNELS = {"rgb": (3,), "variance": (3,), "half_a": (3,), "half_b": (3,), "tops": (TOPS, 3), "level": ()}  # mcrt_frame_summary order
GROUPS = {"mean": ("rgb", "variance"), "halves": ("half_a", "half_b"), "highlights": ("tops", "level")}
ERR_INVALID, ERR_UNSUPPORTED = -1, -7
PIXEL_COUNTS = [1, 63, 64, 65, 257]  # less than a wave, a wave, a wave and a lane, a workgroup and a lane
COUNT_PAIRS = [(1, 1), (1, 4), (4, 9), (9, 9), (9, 16), (16, 16), (16, 25)]  # n_a odd and even; highlights from (16, 16) on
MEANING_SCENES = ("hexagon_room_diffuse", "coffee_maker_qsah")


def load_accumulate_emu():
    L = C.CDLL(build_emu("accumulate_emu.cpp"))
    vp = C.c_void_p
    L.frame_merge_emu.argtypes = [C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, vp]
    return L


@functools.lru_cache(maxsize=None)
def _emu():
    return load_accumulate_emu()


def wanted_channels(n_a, n_b, groups=None):
    """The channels of the groups (default: every group the counts allow)."""
    if groups is None:
        groups = ["mean", "halves"] + (["highlights"] if min(n_a, n_b) >= 16 else [])
    return [c for g in groups for c in GROUPS[g]]


def numpy_summary(store):
    """The summary a render delivers of a store [n][pixels][3], by the header's text in numpy: rgb (the mean, unclamped), variance,
    half_a, half_b, tops, level."""
    st, hl = ps.numpy_pixel_stats(store), rb.numpy_highlights(store)
    return {"rgb": st["mean"], "variance": st["variance"], "half_a": st["half_a"], "half_b": st["half_b"], "tops": hl["tops"], "level": hl["level"]}


def numpy_wmean(c1, x1, c2, x2):
    w1, w2 = float(c1) * x1, float(c2) * x2
    return (((w1 + w2) if c2 > 0 else w1) if c1 > 0 else w2) / float(c1 + c2)


def numpy_frame_merge(A, n_a, B, n_b, channels=None):
    """include/mcrt.h's mcrt_frame_merge in numpy on dicts of [pixels]... arrays -> dict of the channels wanted."""
    channels = wanted_channels(n_a, n_b) if channels is None else channels
    a, b = float(n_a), float(n_b)
    t = a + b
    out = {}
    with np.errstate(all="ignore"):
        if "rgb" in channels:
            out["rgb"] = (a * A["rgb"] + b * B["rgb"]) / t
        if "variance" in channels:
            d = B["rgb"] - A["rgb"]
            Q = ((a - 1.0) * A["variance"] + (b - 1.0) * B["variance"]) + (d * d) * ((a * b) / t)
            out["variance"] = Q / (t - 1.0)
        if "half_a" in channels:
            e_a, o_a, e_b, o_b = (n_a + 1) // 2, n_a // 2, (n_b + 1) // 2, n_b // 2
            if n_a % 2 == 0:
                out["half_a"] = numpy_wmean(e_a, A["half_a"], e_b, B["half_a"])
                out["half_b"] = numpy_wmean(o_a, A["half_b"], o_b, B["half_b"])
            else:
                out["half_a"] = numpy_wmean(e_a, A["half_a"], o_b, B["half_b"])
                out["half_b"] = numpy_wmean(o_a, A["half_b"], e_b, B["half_a"])
        if "tops" in channels:
            E = np.array(A["tops"], dtype=np.float64).reshape(-1, TOPS, 3)
            tb = np.asarray(B["tops"], dtype=np.float64).reshape(-1, TOPS, 3)
            EL = luminance(E)  # [P][4]
            gone = np.zeros(E.shape[0])
            for j in range(TOPS):
                x, l = tb[:, j], luminance(tb[:, j])
                pos = np.full(E.shape[0], TOPS)  # TOPS: x exceeds no entry (a NaN l never does)
                for e in reversed(range(TOPS)):  # (the FIRST entry it exceeds)
                    pos = np.where(l > EL[:, e], e, pos)
                gone = gone + np.where(pos < TOPS, EL[:, TOPS - 1], l)
                for e in reversed(range(TOPS)):
                    if e > 0:
                        E[:, e] = np.where((pos < e)[:, None], E[:, e - 1], E[:, e])
                        EL[:, e] = np.where(pos < e, EL[:, e - 1], EL[:, e])
                    E[:, e] = np.where((pos == e)[:, None], x, E[:, e])
                    EL[:, e] = np.where(pos == e, l, EL[:, e])
            out["tops"] = E.reshape(np.shape(A["tops"]))
            out["level"] = (((a - 4.0) * np.asarray(A["level"]) + (b - 4.0) * np.asarray(B["level"])) + gone.reshape(np.shape(A["level"]))) / (t - 4.0)
    return out


def _pointers(d, names):
    return (C.c_void_p * 6)(*[d[k].ctypes.data if k in names and k in d else None for k in CHANNELS])


def emu_frame_merge(A, n_a, B, n_b, channels=None, in_place=False, pixels=None, expect=0):
    """The emulation -> dict of ALL six channels: those left out of `channels` get a NULL pointer and come back as the sentinel they
    were filled with. in_place: the outputs are (copies of) A's own buffers."""
    channels = wanted_channels(n_a, n_b) if channels is None else channels
    A = {k: np.array(v, dtype=np.float64, order="C") for k, v in A.items()}
    B = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in B.items()}
    P = next(iter(A.values())).size // int(np.prod(CHANNELS[next(iter(A))], dtype=np.int64))
    out = {k: (A[k] if in_place and k in channels else np.full((P,) + CHANNELS[k], SENTINEL)) for k in CHANNELS}
    rc = _emu().frame_merge_emu(P if pixels is None else pixels, _pointers(A, CHANNELS), n_a, _pointers(B, CHANNELS), n_b, _pointers(out, channels))
    assert rc == expect, (rc, expect)
    return out


def assert_same(got, want, keys, msg=""):
    for k in keys:
        np.testing.assert_array_equal(bits(got[k]), bits(np.asarray(want[k]).reshape(got[k].shape)), err_msg="%s %s" % (msg, k))


def _store(spp, pixels, seed):
    rng = np.random.default_rng(seed)
    return rng.random((spp, pixels, 3)) * rng.choice([1e-3, 1.0, 40.0], size=(1, pixels, 1))


@functools.lru_cache(maxsize=None)
def hand_made(pixels, n_a, n_b):
    """Two summaries of hand-made stores, their numpy merge and the emulation's: computed once, shared with the GPU tests."""
    A, B = numpy_summary(_store(n_a, pixels, 100 * n_a + pixels)), numpy_summary(_store(n_b, pixels, 7000 + 100 * n_b + pixels))
    if min(n_a, n_b) < 16:
        for s in (A, B):
            del s["tops"], s["level"]
    want = numpy_frame_merge(A, n_a, B, n_b)
    for d in (A, B, want):
        for v in d.values():
            v.setflags(write=False)
    return A, B, want


@pytest.mark.parametrize("n_a,n_b", COUNT_PAIRS)
@pytest.mark.parametrize("pixels", PIXEL_COUNTS)
def test_text_is_the_header_in_numpy(pixels, n_a, n_b):
    A, B, want = hand_made(pixels, n_a, n_b)
    names = wanted_channels(n_a, n_b)
    assert ("tops" in names) == (min(n_a, n_b) >= 16) and sorted(want) == sorted(names)
    got = emu_frame_merge(A, n_a, B, n_b)
    assert_same(got, want, names, "%d pixels, %d + %d" % (pixels, n_a, n_b))
    for k in CHANNELS:
        if k not in names:
            assert (got[k] == SENTINEL).all(), k
    # the outputs may be A's own buffers
    here = emu_frame_merge(A, n_a, B, n_b, in_place=True)
    assert_same(here, want, names, "in place")


@pytest.mark.parametrize("n_a,n_b", [(9, 16), (16, 16), (16, 25)])
def test_a_group_left_out_is_not_written(n_a, n_b):
    A, B, want = hand_made(257, n_a, n_b)
    every = wanted_channels(n_a, n_b)
    for group, names in GROUPS.items():
        if names[0] not in every:
            continue
        got = emu_frame_merge(A, n_a, B, n_b, channels=list(names))
        assert_same(got, want, names, group)
        for k in CHANNELS:
            if k not in names:
                assert (got[k] == SENTINEL).all(), (group, k)
    mean_only = emu_frame_merge(A, n_a, B, n_b, channels=["rgb"])
    assert_same(mean_only, want, ("rgb",))
    assert (mean_only["variance"] == SENTINEL).all()


def test_nan_and_inf_stay_in_their_pixel():
    n_a, n_b, P = 16, 25, 257
    A, B, want = hand_made(P, n_a, n_b)
    A = {k: v.copy() for k, v in A.items()}
    B = {k: v.copy() for k, v in B.items()}
    A["rgb"][100, 1] = np.nan
    B["variance"][7, 0] = np.inf
    A["half_a"][256, 2] = np.nan
    B["tops"][50, 0, :] = np.inf      # an Inf entry: the first of the merged list
    A["tops"][51, 2, 1] = np.nan      # an entry of A whose luminance is NaN is never displaced
    B["tops"][52, 1, 0] = np.nan      # an entry of B whose luminance is NaN never enters; it reaches the level
    B["level"][200] = -np.inf
    dirty = numpy_frame_merge(A, n_a, B, n_b)
    got = emu_frame_merge(A, n_a, B, n_b)
    assert_same(got, dirty, list(CHANNELS))
    touched = {"rgb": [100], "variance": [100, 7], "half_a": [256], "half_b": [], "tops": [50, 51, 52], "level": [50, 51, 52, 200]}
    for k, rows in touched.items():
        other = np.ones(P, dtype=bool)
        other[rows] = False
        np.testing.assert_array_equal(bits(got[k][other]), bits(want[k][other]), err_msg=k)
    assert np.isnan(got["rgb"][100, 1]) and np.isfinite(got["rgb"][100, [0, 2]]).all()
    assert np.isinf(got["variance"][7, 0]) and np.isnan(got["half_a"][256, 2])
    assert np.isinf(got["tops"][50, 0]).all() and np.isnan(got["tops"][51, 2, 1]) and np.isfinite(got["tops"][52]).all()
    assert np.isnan(got["level"][52]) and got["level"][200] == -np.inf


def test_ties_go_to_a_and_to_the_lower_index():
    """Entries in a few luminance classes (channel values of few bits, so that equal means equal), B's tagged in the last bit of blue,
    which the luminance does not see: the merged list is what a stable sort of A's entries followed by B's gives."""
    rng = np.random.default_rng(3)
    P = 257

    def side():
        l = -np.sort(-rng.integers(1, 4, size=(P, TOPS)).astype(np.float64), axis=1) * 0.25
        return np.repeat(l[:, :, None], 3, axis=2)
    A = {"tops": side(), "level": rng.random(P)}
    plain = side()
    B = {"tops": plain.copy(), "level": rng.random(P)}
    B["tops"][:, :, 2] = np.nextafter(plain[:, :, 2], 2.0)
    assert (luminance(B["tops"]) == luminance(plain)).all() and (B["tops"][:, :, 2] != plain[:, :, 2]).all()
    got = emu_frame_merge(A, 16, B, 16, channels=["tops", "level"])
    assert_same(got, numpy_frame_merge(A, 16, B, 16, channels=["tops", "level"]), ("tops", "level"))
    both = np.concatenate([A["tops"], B["tops"]], axis=1)  # [P][8][3]
    order = np.argsort(-luminance(both), axis=1, kind="stable")[:, :TOPS]
    np.testing.assert_array_equal(bits(got["tops"]), bits(np.take_along_axis(both, order[:, :, None], axis=1)))
    assert (order >= TOPS).any() and (order < TOPS).any()
    same = {"tops": np.full((65, TOPS, 3), 0.375), "level": np.full(65, 0.25)}
    other = {"tops": same["tops"].copy(), "level": np.full(65, 0.25)}
    other["tops"][:, :, 2] = np.nextafter(0.375, 2.0)
    alone = emu_frame_merge(same, 16, other, 16, channels=["tops", "level"])
    np.testing.assert_array_equal(bits(alone["tops"]), bits(same["tops"]))  # all equal: A's entries stay


def test_what_the_library_refuses_the_harness_refuses():
    A, B, _ = hand_made(63, 16, 16)
    every = list(CHANNELS)
    emu_frame_merge(A, 0, B, 16, channels=every, expect=ERR_INVALID)
    emu_frame_merge(A, 16, B, 0, channels=every, expect=ERR_INVALID)
    emu_frame_merge(A, 0xFFFFFFF0, B, 16, channels=every, expect=ERR_INVALID)  # n_a + n_b past uint32_t
    emu_frame_merge(A, 16, B, 16, channels=every, pixels=0, expect=ERR_INVALID)
    emu_frame_merge(A, 16, B, 16, channels=[], expect=ERR_INVALID)
    emu_frame_merge(A, 16, B, 16, channels=["variance"], expect=ERR_INVALID)      # the variance needs rgb
    emu_frame_merge(A, 16, B, 16, channels=["half_a"], expect=ERR_INVALID)        # half a group
    emu_frame_merge(A, 16, B, 16, channels=["tops"], expect=ERR_INVALID)
    for k in ("rgb", "variance", "half_b", "level"):                              # a wanted group without its inputs
        emu_frame_merge({c: v for c, v in A.items() if c != k}, 16, B, 16, channels=every, expect=ERR_INVALID)
        emu_frame_merge(A, 16, {c: v for c, v in B.items() if c != k}, 16, channels=every, expect=ERR_INVALID)
    for n_a, n_b in ((15, 16), (16, 15), (9, 9)):                                 # highlights below full lists on both sides
        emu_frame_merge(A, n_a, B, n_b, channels=every, expect=ERR_UNSUPPORTED)
        emu_frame_merge(A, n_a, B, n_b, channels=["rgb", "variance", "half_a", "half_b"])
    # 2^32 pixels: refused before anything is read
    emu_frame_merge(A, 16, B, 16, channels=every, pixels=1 << 32, expect=ERR_INVALID)


@functools.lru_cache(maxsize=None)
def oracle_halves(scene, sqrtspp):
    """The oracle's per-sample stores of one camera at SEED and SEED + 1 as [n][pixels][3], their summaries, and the summary of the
    concatenation: computed once."""
    sa = ps.oracle_case(scene, sqrtspp, seed=SEED)[1]
    sb = ps.oracle_case(scene, sqrtspp, seed=SEED + 1)[1]
    n = sqrtspp * sqrtspp
    sa, sb = sa.reshape(n, -1, 3), sb.reshape(n, -1, 3)
    return numpy_summary(sa), numpy_summary(sb), numpy_summary(np.concatenate([sa, sb], axis=0))


@pytest.mark.parametrize("sqrtspp", [3, 4])
@pytest.mark.parametrize("scene", MEANING_SCENES)
def test_merge_of_the_halves_is_the_statistics_of_the_whole(scene, sqrtspp):
    A, B, whole = oracle_halves(scene, sqrtspp)
    n = sqrtspp * sqrtspp
    names = wanted_channels(n, n)
    assert ("tops" in names) == (sqrtspp == 4)
    assert not np.array_equal(A["rgb"], B["rgb"])  # two seeds: two sets of samples
    want = numpy_frame_merge({k: A[k] for k in names}, n, {k: B[k] for k in names}, n)
    got = emu_frame_merge({k: A[k] for k in names}, n, {k: B[k] for k in names}, n)
    assert_same(got, want, names, "%s sqrtspp %d" % (scene, sqrtspp))

    def rel(x, y):
        return float((np.abs(x - y) / np.maximum(np.abs(y), 1e-300)).max())
    for k in ("rgb", "half_a", "half_b") + (("level",) if sqrtspp == 4 else ()):
        e = rel(want[k], whole[k])
        print("%s sqrtspp %d: %s, max relative error %.3e" % (scene, sqrtspp, k, e))
        assert e <= 1e-12, k
    m = whole["rgb"]
    excess = np.abs(want["variance"] - whole["variance"]) / np.maximum(whole["variance"] + m * m, 1e-300)
    print("%s sqrtspp %d: variance, max |merged - direct| / (direct + m m) %.3e" % (scene, sqrtspp, excess.max()))
    assert (np.abs(want["variance"] - whole["variance"]) <= 1e-12 * (whole["variance"] + m * m)).all()
    if sqrtspp == 4:
        np.testing.assert_array_equal(bits(want["tops"]), bits(whole["tops"]))


def exact_stores(pixels, seed):
    """Two stores [16][pixels][3] of small integers: every pixel and channel of each sums to a multiple of 16 and has a sum of squared
    deviations that is a multiple of 15."""
    rng = np.random.default_rng(seed)
    need = 2 * pixels * 3
    found = np.zeros((0, 16))
    while found.shape[0] < need:
        cand = rng.integers(0, 8, size=(200000, 16)).astype(np.float64)
        S = cand.sum(axis=1)
        Q = (cand * cand).sum(axis=1) - S * S / 16.0
        found = np.concatenate([found, cand[(S % 16 == 0) & (Q % 15 == 0) & (Q > 0)]])
    found = found[:need].reshape(2, pixels, 3, 16)
    return np.ascontiguousarray(np.moveaxis(found[0], 2, 0)), np.ascontiguousarray(np.moveaxis(found[1], 2, 0))


@pytest.mark.parametrize("pixels", [65, 257])
def test_exact_case(pixels):
    sa, sb = exact_stores(pixels, pixels)
    A, B, whole = numpy_summary(sa), numpy_summary(sb), numpy_summary(np.concatenate([sa, sb], axis=0))
    assert (A["rgb"] == np.round(A["rgb"])).all() and ((15.0 * A["variance"]) % 15 == 0).all()
    got = emu_frame_merge(A, 16, B, 16, channels=["rgb", "variance"])
    np.testing.assert_array_equal(bits(got["rgb"]), bits(whole["rgb"]))
    np.testing.assert_array_equal(bits(got["variance"]), bits(whole["variance"]))
    assert_same(got, numpy_frame_merge(A, 16, B, 16, ["rgb", "variance"]), ("rgb", "variance"))
