"""Dual-buffer denoised output (mcrt_denoise_dual*), CPU tier: csrc/mcrt_denoise_dual.hpp - the text the three kernels of
csrc/mcrt_denoise_dual.hip run - driven on the host (tests/emu/denoise_dual_emu.cpp: the plain form as a loop, the tile form on
wave_emu.hpp's emulated workgroup with its barriers) against the definition of include/mcrt.h ("Dual-buffer denoised output") written
out HERE in numpy, window offset by window offset and patch element by patch element in the stated order.

Bound: assert_array_equal. Derived, not measured: both sides execute the same IEEE-754 double operations (+ - * /, compare, select) in
the same order, none of them a libm call, neither side contracted (the harness is built with -ffp-contract=off, numpy's ufuncs are
one operation each) - so every bit agrees, NaNs included."""
import ctypes as C
import functools

import numpy as np
import pytest

from emu_build import build_emu

# explicit parameters everywhere (not the defaults: retuning those must not touch a test)
PARAMS = dict(k=0.6, alpha=0.9, epsilon=1e-9)
OUTPUTS = ("rgb", "variance", "half_a", "half_b")
# (width, height, window_radius, patch_radius, spp): one pixel; exactly one tile; ragged tiles; a window taller than the frame; ragged both
# ways over 9 x 5 tiles; the limits of both radii. Odd spp (n_a != n_b) and even.
SHAPES = [(1, 1, 3, 1, 4), (16, 16, 5, 2, 5), (17, 33, 3, 1, 9), (70, 13, 8, 2, 4), (131, 67, 5, 2, 9), (37, 21, 8, 3, 5)]


def load_denoise_dual_emu():
    L = C.CDLL(build_emu("denoise_dual_emu.cpp"))
    vp = C.c_void_p
    L.denoise_dual_emu.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_int, vp]
    L.denoise_dual_emu_tile_lds_bytes.argtypes = [C.c_uint32, C.c_uint32]
    L.denoise_dual_emu_tile_lds_bytes.restype = C.c_uint32
    L.denoise_dual_emu_tile_lds_max_bytes.restype = C.c_uint32
    return L


@functools.lru_cache(maxsize=None)
def _emu():
    return load_denoise_dual_emu()


def _pkg():
    import importlib
    return importlib.import_module("monte-carlo-ray-tracer_amd")


def emu_denoise_dual(half_a, half_b, variance, spp, form, want=OUTPUTS, in_place=False, **params):
    """The emulation's outputs as a dict. form: "plain", "tile" (the workgroup the launch uses) or the tile form's lanes (256, 512, 1024). in_place: half_a, half_b and variance of the outputs are written over
    (copies of) the inputs."""
    pkg = _pkg()
    a, b, v = (np.array(x, dtype=np.float64, order="C") for x in (half_a, half_b, variance))
    height, width = a.shape[:2]
    res = {k: np.full_like(a, -7.0) for k in want}
    if in_place:
        res.update({k: arr for k, arr in (("half_a", a), ("half_b", b), ("variance", v)) if k in want})
    bufs = pkg.DenoiseDualBuffers(**{k: arr.ctypes.data for k, arr in res.items()})
    par = pkg.DenoiseDualParams(**params)
    rc = _emu().denoise_dual_emu(width, height, spp, a.ctypes.data, b.ctypes.data, v.ctypes.data, C.byref(par), {"plain": 0, "tile": 1}.get(form, form), C.byref(bufs))
    assert rc == 0, "denoise_dual_emu: %d" % rc
    return res


def _max0(x):
    return np.where(x < 0.0, 0.0, x)


def _taps(H, W, radius):
    """(dy, dx, p, q): the slices of the pixels p whose tap q = p + (dx, dy) is inside the frame; dy outer, dx inner."""
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                yield dy, dx, (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def numpy_denoise_dual(A, B, v, spp, window_radius, patch_radius, k, alpha, epsilon):
    """include/mcrt.h's "Dual-buffer denoised output" in numpy: whole-frame arrays per window offset and patch element, both halves stacked
    on a leading axis (index 0: the weights computed from A, 1: from B), every sum in the stated order."""
    A, B, v = (np.asarray(x, dtype=np.float64) for x in (A, B, v))
    H, W = A.shape[:2]
    R, F = window_radius, patch_radius
    n = int(spp)
    n_a, n_b = (n + 1) // 2, n // 2
    ia, ib = 1.0 / float(n_a), 1.0 / float(n_b)
    fa, fb = float(n_a) / float(n), float(n_b) / float(n)
    k2 = k * k
    kk = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)
    with np.errstate(all="ignore"):
        s3, ks = np.zeros((H, W, 3)), np.zeros((H, W))
        for dy, dx, p, q in _taps(H, W, 1):
            kw = kk[dy + 1] * kk[dx + 1]
            s3[p] = s3[p] + kw * v[q]
            ks[p] = ks[p] + kw
        V0 = s3 * (1.0 / ks)[..., None]
        P = R + F
        X = np.zeros((2, H + 2 * P, W + 2 * P, 3))
        VX = np.zeros_like(X)
        inside = np.zeros((H + 2 * P, W + 2 * P), dtype=bool)
        X[0, P:P + H, P:P + W], X[1, P:P + H, P:P + W] = A, B
        VX[0, P:P + H, P:P + W], VX[1, P:P + H, P:P + W] = V0 * ia, V0 * ib
        inside[P:P + H, P:P + W] = True
        Y = (B, A)  # the half that the weights of X[0] (from A), X[1] (from B) are applied to
        total, wsum = np.zeros((2, H, W, 3)), np.zeros((2, H, W))
        for dy, dx, p, q in _taps(H, W, R):
            if dx == 0 and dy == 0:
                w = np.ones((2, H, W))
            else:
                S, cnt = np.zeros((2, H, W)), np.zeros((H, W), dtype=np.int64)
                for j in range(-F, F + 1):
                    row = np.zeros((2, H, W))
                    for i in range(-F, F + 1):
                        ep = (slice(P + j, P + j + H), slice(P + i, P + i + W))
                        eq = (slice(P + j + dy, P + j + dy + H), slice(P + i + dx, P + i + dx + W))
                        valid = inside[ep] & inside[eq]
                        cnt = cnt + valid
                        vp, vq = VX[(slice(None),) + ep], VX[(slice(None),) + eq]
                        delta = X[(slice(None),) + ep] - X[(slice(None),) + eq]
                        vm = np.where(vq < vp, vq, vp)
                        num = delta * delta - alpha * (vp + vm)
                        den = epsilon + k2 * (vp + vq)
                        t = num / den
                        row = np.where(valid, ((row + t[..., 0]) + t[..., 1]) + t[..., 2], row)
                    S = S + row
                D = S / (3 * cnt).astype(np.float64)
                w = _max0(1.0 - _max0(D))
                w = w * w
            for h in (0, 1):  # (in the order of the text: A's sums, with the weights from B, first - the two do not meet)
                total[h][p] = total[h][p] + w[h][p][..., None] * Y[h][q]
                wsum[h][p] = wsum[h][p] + w[h][p]
        Bf, Af = total[0] * (1.0 / wsum[0])[..., None], total[1] * (1.0 / wsum[1])[..., None]
        dl = Af - Bf
        return {"rgb": (fa * Af) + (fb * Bf), "variance": ((dl * dl) * (fa * fb)) * float(n), "half_a": Af, "half_b": Bf}


def make_halves(width, height, spp, seed):
    """-> (A, B, v): a smooth base with an edge, per-sample spread sigma, halves with noise of variance sigma^2 / n_x around it, and a
    sample variance consistent with that noise (sigma^2 times a seeded factor), with a few exact zeros."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    base = np.stack([0.4 + 0.3 * np.sin(0.21 * x) * np.cos(0.17 * y), 0.5 + 0.02 * x, 0.3 + 0.4 * (x + 2 * y > 0.9 * (width + height))], axis=-1)
    sigma = 0.05 + 0.2 * base
    n_a, n_b = (spp + 1) // 2, spp // 2
    A = base + rng.standard_normal(base.shape) * sigma / np.sqrt(n_a)
    B = base + rng.standard_normal(base.shape) * sigma / np.sqrt(n_b)
    v = sigma ** 2 * rng.uniform(0.3, 2.5, size=base.shape)
    v[rng.random((height, width)) < 0.04] = 0.0
    return np.ascontiguousarray(A), np.ascontiguousarray(B), np.ascontiguousarray(v)


@functools.lru_cache(maxsize=None)
def shape_case(width, height, R, F, spp):
    """The inputs of a shape and their numpy result: computed once, shared (tests/test_gpu_denoise_dual.py reads make_halves too)."""
    A, B, v = make_halves(width, height, spp, 1000 + width + 7 * height)
    want = numpy_denoise_dual(A, B, v, spp, R, F, **PARAMS)
    for arr in (A, B, v) + tuple(want.values()):
        arr.setflags(write=False)
    return A, B, v, want


def both_forms_equal(A, B, v, spp, want, msg="", **kw):
    for form in ("plain", "tile"):
        got = emu_denoise_dual(A, B, v, spp, form, **kw)
        for name in OUTPUTS:
            np.testing.assert_array_equal(got[name], want[name], err_msg="%s %s %s" % (name, form, msg))


@pytest.mark.parametrize("width,height,R,F,spp", SHAPES)
def test_emulation_is_the_numpy_restatement(width, height, R, F, spp):
    A, B, v, want = shape_case(width, height, R, F, spp)
    both_forms_equal(A, B, v, spp, want, window_radius=R, patch_radius=F, **PARAMS)
    assert all(np.isfinite(want[k]).all() for k in OUTPUTS)
    if width * height > 1:
        assert not np.array_equal(want["half_a"], A) and not np.array_equal(want["half_b"], B) and (want["variance"] > 0).any()
        # the filter filtered, and not everything: weights strictly between 0 and 1 exist when the mean is neither the pixel nor the window's
        assert np.abs(want["half_a"] - A).max() > 1e-3


@pytest.mark.parametrize("lanes", [256, 512, 1024])
def test_the_tile_form_does_not_depend_on_its_workgroup(lanes):
    """256, 512 or 1024 lanes on one tile (option MCRT_DENOISE_DUAL_LANES): the staging, the terms and the row sums are dealt to however
    many lanes there are, the first 256 own the pixels - the same operations on the same numbers."""
    for shape in (SHAPES[2], SHAPES[5]):
        A, B, v, want = shape_case(*shape)
        got = emu_denoise_dual(A, B, v, shape[4], lanes, window_radius=shape[2], patch_radius=shape[3], **PARAMS)
        for name in OUTPUTS:
            np.testing.assert_array_equal(got[name], want[name], err_msg="%s %d lanes" % (name, lanes))


def test_one_pixel_is_itself():
    """1 x 1: only the centre tap, w = 1.0: sum = 0.0 + 1.0 * Y, 1.0 / 1.0 = 1.0: the halves come back bit for bit."""
    A, B, v, want = shape_case(*SHAPES[0])
    assert want["half_a"].tobytes() == A.tobytes() and want["half_b"].tobytes() == B.tobytes()


def test_no_optional_output_gives_the_same_frame():
    A, B, v, want = shape_case(*SHAPES[2])
    _, _, R, F, spp = SHAPES[2]
    for form in ("plain", "tile"):
        got = emu_denoise_dual(A, B, v, spp, form, want=("rgb",), window_radius=R, patch_radius=F, **PARAMS)
        assert sorted(got) == ["rgb"]
        np.testing.assert_array_equal(got["rgb"], want["rgb"])


def test_identical_halves_have_no_error():
    """A = B and even n: n_a = n_b, so VA = VB, both weight sets and both sums are the same operations on the same numbers - half_a ==
    half_b bit for bit, dl = 0 and variance == 0 exactly."""
    A, _, v = make_halves(40, 23, 6, 3)
    for form in ("plain", "tile"):
        got = emu_denoise_dual(A, A, v, 6, form, window_radius=4, patch_radius=2, **PARAMS)
        assert got["half_a"].tobytes() == got["half_b"].tobytes()
        assert (got["variance"] == 0.0).all()
        assert not np.array_equal(got["half_a"], A)


STEP = dict(window_radius=3, patch_radius=2, k=0.5, alpha=1.0, epsilon=1e-10)


def _step(width, height, edge, lo=0.3, hi=1.3):
    f = np.empty((height, width, 3))
    f[:, :edge], f[:, edge:] = lo, hi
    return f


def test_a_step_edge_far_above_the_variance_is_kept():
    """Both halves the same noise-free step of height 1 (levels 0.3 | 1.3), v = 1e-6 everywhere, n = 4: vX = 5e-7, den = 1e-10 + 0.25 x 1e-6
    = 2.501e-7 for every element. A tap q on the other side of the edge from p: its centre element has delta^2 = 1 in all three channels,
    each term (1 - 1e-6) / 2.501e-7 > 3.9e6; every other of the at most 25 x 3 terms is at least -alpha 2 vX / den > -4. So S > 1.1e7,
    D > 1.1e7 / 75 >> 1, 1 - x < 0 and w = 0 EXACTLY, far from any rounding. A tap on p's own side with all its elements on matching sides
    has delta = 0, num < 0, D < 0, w = 1; whatever the others get, every tap with w > 0 holds the pixel's own level L. The output is then
    (sum of w L) x (1 / sum of w) over N <= 49 taps with weights >= 0. Numerator: N products that round, and N - 1 additions that round
    (0.0 + x does not) - a term passes through at most N roundings; denominator: N - 1; the reciprocal and the last product one each:
    2 N + 1 = 99 half-ulps to first order; rgb = 0.5 A_f + 0.5 B_f adds one rounding: 100, 102 with room for the second order."""
    W, H, edge = 24, 9, 11
    f = _step(W, H, edge)
    v = np.full_like(f, 1e-6)
    for form in ("plain", "tile"):
        got = emu_denoise_dual(f, f, v, 4, form, **STEP)
        for name in ("half_a", "half_b", "rgb"):
            np.testing.assert_allclose(got[name], f, rtol=102 * 2.0 ** -53, atol=0, err_msg="%s %s" % (name, form))
        assert (got["variance"] == 0.0).all()


def test_the_weights_come_from_the_other_half():
    """B: the noise-free step of the test above. A: edge-free noise around 0.8, a quarter of the spread that v = 1e-6 states. half_a's
    weights come from B: exactly 0 across B's edge (derivation above), so half_a left of the edge does not see A right of it - replace A
    there by other noise and the left columns keep their bits, while the right ones change. half_b's weights come from A, which has no
    edge: B is mixed across its edge - with every weight 1 the column left of the edge would be 0.3 + 3/7, the one right of it 1.3 - 3/7."""
    W, H, edge = 24, 9, 11
    B = _step(W, H, edge)
    v = np.full_like(B, 1e-6)
    sd = 0.25 * np.sqrt(1e-6 / 2.0)
    A = 0.8 + sd * np.random.default_rng(5).standard_normal(B.shape)
    A2 = A.copy()
    A2[:, edge:] = 0.8 + sd * np.random.default_rng(6).standard_normal(A2[:, edge:].shape)
    for form in ("plain", "tile"):
        got, got2 = (emu_denoise_dual(a, B, v, 4, form, **STEP) for a in (A, A2))
        assert got["half_a"][:, :edge].tobytes() == got2["half_a"][:, :edge].tobytes()
        assert (got["half_a"][:, edge:] != got2["half_a"][:, edge:]).all()
        assert (got["half_b"][:, edge - 1] > 0.5).all() and (got["half_b"][:, edge - 1] < 0.9).all()
        assert (got["half_b"][:, edge] > 0.7).all() and (got["half_b"][:, edge] < 1.1).all()


def _cheb(width, height, z):
    y, x = np.mgrid[0:height, 0:width]
    return np.maximum(np.abs(y - z[0]), np.abs(x - z[1]))


@pytest.mark.parametrize("z", [(9, 14), (0, 27)])
def test_a_nan_reaches_exactly_the_pixels_the_header_names(z):
    """R = 3, F = 2, 33 x 19. A NaN in A at z: half_b (weights from A) is NaN exactly within Chebyshev distance R + F = 5 of z, half_a (A
    is what is averaged there, a NaN product even at weight 0) exactly within R = 3; rgb and variance hold both. A NaN in v at z: the
    prefilter spreads it one pixel, both weight sets read it: both halves NaN exactly within R + F + 1 = 6. Every pixel further away keeps
    the bits of the NaN-free run, in all four outputs."""
    W, H, R, F = 33, 19, 3, 2
    A, B, v = make_halves(W, H, 4, 12)
    par = dict(PARAMS, window_radius=R, patch_radius=F)
    d = _cheb(W, H, z)
    clean = emu_denoise_dual(A, B, v, 4, "plain", **par)
    An, vn = A.copy(), v.copy()
    An[z[0], z[1], 1] = np.nan
    vn[z[0], z[1], 2] = np.nan
    want = numpy_denoise_dual(An, B, v, 4, R, F, **PARAMS)
    both_forms_equal(An, B, v, 4, want, "NaN in A", **par)
    nan = {k: np.isnan(want[k]).any(axis=2) for k in OUTPUTS}
    assert np.array_equal(nan["half_b"], d <= R + F) and np.array_equal(nan["half_a"], d <= R)
    assert np.array_equal(nan["rgb"], d <= R + F) and np.array_equal(nan["variance"], d <= R + F)
    for k in OUTPUTS:
        assert want[k][d > R + F].tobytes() == clean[k][d > R + F].tobytes(), k
    want = numpy_denoise_dual(A, B, vn, 4, R, F, **PARAMS)
    both_forms_equal(A, B, vn, 4, want, "NaN in v", **par)
    for k in OUTPUTS:
        assert np.array_equal(np.isnan(want[k]).any(axis=2), d <= R + F + 1), k
        assert want[k][d > R + F + 1].tobytes() == clean[k][d > R + F + 1].tobytes(), k


def test_a_huge_variance_opens_every_weight():
    """v = 1e30: vX >= 2.5e29 while delta^2 < 10, so every num = delta^2 - alpha (vp + vm) < 0 and every den > 0: every row, S and D are
    negative, x = 0 and w = 1 exactly. half_a is then the in-frame window mean of A in the stated order: ((0.0 + A(q_0)) + A(q_1)) + ...
    times 1.0 / (the number of in-frame taps, summed as 1.0s)."""
    W, H, R = 29, 17, 4
    A, B, _ = make_halves(W, H, 4, 13)
    v = np.full_like(A, 1e30)
    mean = {}
    for name, Y in (("half_a", A), ("half_b", B)):
        s, c = np.zeros_like(Y), np.zeros((H, W))
        for dy, dx, p, q in _taps(H, W, R):
            s[p] = s[p] + 1.0 * Y[q]
            c[p] = c[p] + 1.0
        mean[name] = s * (1.0 / c)[..., None]
    for form in ("plain", "tile"):
        got = emu_denoise_dual(A, B, v, 4, form, window_radius=R, patch_radius=1, **PARAMS)
        for name in mean:
            np.testing.assert_array_equal(got[name], mean[name], err_msg="%s %s" % (name, form))


def test_in_place_equals_out_of_place():
    """Every output over its input (the prep pass has copied what the filter reads), and rgb over an input."""
    width, height, R, F, spp = SHAPES[2]
    A, B, v, want = shape_case(*SHAPES[2])
    pkg = _pkg()
    for form in ("plain", "tile"):
        got = emu_denoise_dual(A, B, v, spp, form, in_place=True, window_radius=R, patch_radius=F, **PARAMS)
        for name in OUTPUTS:
            np.testing.assert_array_equal(got[name], want[name], err_msg="%s %s" % (name, form))
        a, b, vv = A.copy(), B.copy(), v.copy()
        bufs = pkg.DenoiseDualBuffers(rgb=vv.ctypes.data)
        par = pkg.DenoiseDualParams(window_radius=R, patch_radius=F, **PARAMS)
        assert _emu().denoise_dual_emu(width, height, spp, a.ctypes.data, b.ctypes.data, vv.ctypes.data, C.byref(par), form == "tile", C.byref(bufs)) == 0
        np.testing.assert_array_equal(vv, want["rgb"], err_msg=form)
        assert a.tobytes() == A.tobytes() and b.tobytes() == B.tobytes()


def test_defaults_and_refusals_of_the_settings():
    """A zero field is the default - whatever it is, it is within the limits and the forms agree on it; radii above 8 and 3, fewer than 2
    samples, missing frames and a k, alpha or epsilon that is negative or not finite are refused."""
    pkg = _pkg()
    A, B, v = make_halves(9, 7, 4, 14)
    got = [emu_denoise_dual(A, B, v, 4, form) for form in ("plain", "tile")]
    for name in OUTPUTS:
        np.testing.assert_array_equal(got[0][name], got[1][name])
    out = np.empty_like(A)
    bufs = pkg.DenoiseDualBuffers(rgb=out.ctypes.data)
    P = pkg.DenoiseDualParams

    def run(par, w=9, h=7, spp=4, a=A, b=B, vv=v, o=bufs):
        ptr = lambda x: x.ctypes.data if x is not None else None
        return _emu().denoise_dual_emu(w, h, spp, ptr(a), ptr(b), ptr(vv), C.byref(par), 1, C.byref(o) if o is not None else None)

    assert run(P(window_radius=8, patch_radius=3)) == 0
    assert run(P(window_radius=9)) == -1 and run(P(patch_radius=4)) == -1
    assert run(P(), w=0) == -1 and run(P(), h=0) == -1
    assert run(P(), w=65536, h=65536) == -1  # width * height = 2^32 (refused before a pixel is touched)
    assert run(P(), spp=0) == -1 and run(P(), spp=1) == -1 and run(P(), spp=2) == 0
    assert run(P(), a=None) == -1 and run(P(), b=None) == -1 and run(P(), vv=None) == -1
    assert run(P(), o=None) == -1 and run(P(), o=pkg.DenoiseDualBuffers(variance=out.ctypes.data)) == -1
    for field in ("k", "alpha", "epsilon"):
        for bad in (-1.0, float("inf"), float("-inf"), float("nan")):
            assert run(P(**{field: bad})) == -1, (field, bad)
        assert run(P(**{field: 1e-300})) == 0
    assert C.sizeof(P) == 40 and C.sizeof(pkg.DenoiseDualBuffers) == 32
