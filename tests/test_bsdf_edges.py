"""The lobe functions at the edges of their domain (tests/golden/kat_bsdf_edges, made by tests/golden/make_bsdf_edges.py from the
reference's own functions): what the committed vectors have to contain, and bsdfKernel's own text (csrc/mcrt_kernels.hpp) run on the
host against them. The oracle's tier is in tests/test_oracle_vs_reference.py, the GPU's in tests/test_gpu_parity.py. CPU only.

The device tier drives bsdfKernel the way tests/emu/wave_kernel_emu.cpp drives the other kernels - workgroups of emulated wavefronts,
since the kernel stages the sincos table in LDS behind a __syncthreads - with BsdfKatConsts filled and the grid sized by the functions
mcrt_bsdf calls (fillBsdfKatConsts, bsdfGrid: csrc/mcrt_launch.hpp)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import golden_path
from kat_bits import BSDF_COLUMNS, assert_same_bits, edge_groups, load_edge_group, mismatches

GROUPS = edge_groups()
DBL_MIN = 2.2250738585072014e-308


def test_there_are_groups():
    assert len(GROUPS) >= 4


# ---- the comparison rule ---------------------------------------------------------------------------------------------------------------
def test_assert_same_bits_rule():
    want = np.array([[0.0, -0.0, np.nan, 1.0, np.inf]])
    assert_same_bits(want.copy(), want)
    other_nan = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]  # another sign, another payload
    got = want.copy()
    got[0, 2] = other_nan
    assert_same_bits(got, want)
    for col, value in ((0, -0.0), (1, 0.0), (2, 1.0), (3, np.nan), (3, np.nextafter(1.0, 2.0)), (4, -np.inf)):
        got = want.copy()
        got[0, col] = value
        assert mismatches(got, want).sum() == 1 and mismatches(got, want)[0, col]
        with pytest.raises(AssertionError, match="column %d" % col):
            assert_same_bits(got, want, inputs=np.zeros((1, 11)))


# ---- what the vectors have to contain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_fixture_is_not_trivial(group):
    """Per group and column 0-16: at most a third of the reference's values are NaN and at least half are finite and nonzero - a set
    that is mostly NaN, zero or infinite would pass with almost any arithmetic. One kind of column cannot meet the second bound and is
    held to its own: a diffuse column (13-15) whose reflectance component is 0 in this group's consts is reflectance / pi times a factor,
    so every value of it is a zero or (0 x NaN) a NaN; the group's other diffuse columns carry the bound."""
    consts, inp, out = load_edge_group(group)
    assert 0 < len(inp) <= 4000
    nan = np.isnan(out[:, :17]).mean(axis=0)
    live = (np.isfinite(out[:, :17]) & (out[:, :17] != 0)).mean(axis=0)
    print(group, "NaN %", np.round(100 * nan, 1).tolist())
    print(group, "finite and nonzero %", np.round(100 * live, 1).tolist())
    dead = [13 + k for k in range(3) if consts[1 + k] == 0.0]
    assert len(dead) <= 1
    for c in range(17):
        assert nan[c] <= 1 / 3, (group, c, BSDF_COLUMNS[c], nan[c])
        if c in dead:
            assert ((out[:, c] == 0) | np.isnan(out[:, c])).all()
        else:
            assert live[c] >= 0.5, (group, c, BSDF_COLUMNS[c], live[c])
    assert (out[:, 17] == 0).all() and not np.signbit(out[:, 17]).any()


def test_fixture_reaches_the_edges():
    """Over all groups the reference's outputs hold a -0.0, a subnormal, an infinity, an F == 1.0 returned by `g2 < 0` of
    Fresnel::dielectric (total internal reflection) and an F == 0.0; the inputs hold a vector on the `len2 == 0` branch of
    GGX::visibleMicrofacet; the consts hold a roughness on either side of C::EPSILON."""
    neg_zero = subnormal = inf = f_one = f_zero = len2_zero = 0
    roughness = []
    for group in GROUPS:
        consts, inp, out = load_edge_group(group)
        o = out[:, :17]
        neg_zero += int(((o == 0) & np.signbit(o)).sum())
        subnormal += int(((o != 0) & (np.abs(o) < DBL_MIN)).sum())
        inf += int(np.isinf(o).sum())
        n1, n2, cos_theta = inp[:, 6], inp[:, 7], inp[:, 5]
        g2 = (n2 / n1) * (n2 / n1) + cos_theta * cos_theta - 1.0  # material/fresnel.cpp:18, the same operations in the same order
        assert (out[g2 < 0, 0] == 1.0).all()
        f_one += int((g2 < 0).sum())
        f_zero += int((out[:, 0] == 0.0).sum())
        with np.errstate(all="ignore"):  # material/ggx.cpp:69-72
            v = np.stack([inp[:, 8] * inp[:, 3], inp[:, 8] * inp[:, 4], inp[:, 5]], axis=1)
            vh = v / np.sqrt((v * v).sum(axis=1))[:, None]
            len2_zero += int((vh[:, 0] * vh[:, 0] + vh[:, 1] * vh[:, 1] == 0).sum())
        roughness.append(consts[0])
    print("-0.0 %d, subnormal %d, inf %d, F == 1 by g2 < 0 %d, F == 0 %d, len2 == 0 %d" % (neg_zero, subnormal, inf, f_one, f_zero, len2_zero))
    assert min(neg_zero, subnormal, inf, f_one, f_zero, len2_zero) >= 1
    assert min(roughness) < 1e-9 and 1e-9 in roughness and min(r for r in roughness if r > 1e-9) == np.nextafter(1e-9, 1.0)


def test_fixture_inputs_are_the_generators():
    """The committed consts and inputs are what tests/golden/make_bsdf_edges.py writes today (its answers need the reference binary)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_bsdf_edges", golden_path("make_bsdf_edges.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert [name for name, _ in gen.GROUPS] == GROUPS
    for name, consts in gen.GROUPS:
        c, inp, _ = load_edge_group(name)
        assert c.tobytes() == np.array(consts, dtype=np.float64).tobytes()
        assert inp.tobytes() == gen.rows(name == "g0").tobytes()


# ---- device code on the host -----------------------------------------------------------------------------------------------------------
def emu_bsdf(lib, inp, consts, grid_cap=0):
    lib.wemu_bsdf.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.wemu_bsdf.restype = C.c_int
    inp = np.ascontiguousarray(inp, dtype=np.float64)
    consts = np.ascontiguousarray(consts, dtype=np.float64)
    out = np.full((len(inp), 18), np.nan)
    assert lib.wemu_bsdf(len(inp), inp.ctypes.data, consts.ctypes.data, out.ctypes.data, grid_cap) == 0
    return out


@pytest.mark.parametrize("group", GROUPS)
def test_bsdf_kernel_on_host_edges(wave_kernel_emu, group):
    consts, inp, ref = load_edge_group(group)
    assert_same_bits(emu_bsdf(wave_kernel_emu, inp, consts), ref, inputs=inp, columns=BSDF_COLUMNS, what="bsdfKernel on the host, " + group)


def test_bsdf_kernel_on_host_stride(wave_kernel_emu):
    """Two workgroups for g0's vectors: every lane takes the stride loop several times, the last time past the end for some."""
    consts, inp, ref = load_edge_group(GROUPS[0])
    assert len(inp) > 3 * 512 and len(inp) % 512
    assert_same_bits(emu_bsdf(wave_kernel_emu, inp, consts, grid_cap=2), ref, inputs=inp, columns=BSDF_COLUMNS, what="bsdfKernel on the host, 2 workgroups")


def test_bsdf_kernel_on_host_kat(wave_kernel_emu, manifest):
    d = golden_path(manifest["cases"]["hexagon_room"]["kat"])
    inp = np.fromfile(os.path.join(d, "bsdf_in.f64")).reshape(-1, 11)
    ref = np.fromfile(os.path.join(d, "bsdf_out.f64")).reshape(-1, 18)
    consts = np.fromfile(os.path.join(d, "bsdf_consts.f64"))
    assert_same_bits(emu_bsdf(wave_kernel_emu, inp, consts), ref, inputs=inp, columns=BSDF_COLUMNS, what="bsdfKernel on the host, kat_hexagon_room")
