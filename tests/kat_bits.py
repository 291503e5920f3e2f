"""The comparison rule of the known-answer tests: the reference's bits, with no tolerance anywhere.

np.testing.assert_array_equal compares values, so it takes -0.0 for +0.0 and (by default) any NaN for any NaN, and it names no
input. assert_same_bits compares the words: where the reference value is a NaN the result must be a NaN (any sign, any payload:
the default NaN of x86 has the sign bit set, the GPU's has not), everywhere else every bit must be the reference's, the sign of a
zero included."""
import os

import numpy as np

EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_bsdf_edges")
# out[n][18] of mcrt_bsdf (include/mcrt.h)
BSDF_COLUMNS = ["F_dielectric", "F_conductor.r", "F_conductor.g", "F_conductor.b", "GGX_reflection.f", "GGX_reflection.pdf", "GGX_transmission.f",
                "GGX_transmission.pdf", "microfacet.x", "microfacet.y", "microfacet.z", "GGX_D(m)", "GGX_Lambda(wo)", "diffuse.r", "diffuse.g", "diffuse.b",
                "diffuse.pdf", "zero"]


def _words(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float64, np.float32), a.dtype
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def mismatches(got, want):
    """Boolean array: where `got` is not `want` by the rule above."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    return np.where(nan, ~np.isnan(got), _words(got) != _words(want))


def assert_same_bits(got, want, inputs=None, columns=None, what=""):
    """got == want bit for bit (NaN for NaN). inputs: the row-aligned inputs, printed for the first failing rows; columns: names
    of the last axis."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = mismatches(got, want)
    if not bad.any():
        return
    bad2 = bad.reshape(len(bad), -1) if bad.ndim > 1 else bad.reshape(-1, 1)
    g2, w2 = got.reshape(bad2.shape), want.reshape(bad2.shape)
    lines = ["%s: %d of %d values are not the reference's bits (%d of %d rows)" % (what or "KAT", int(bad2.sum()), bad2.size, int(bad2.any(axis=1).sum()), len(bad2))]
    for c in np.nonzero(bad2.any(axis=0))[0]:
        name = columns[c] if columns is not None and c < len(columns) else "column %d" % c
        idx = np.nonzero(bad2[:, c])[0]
        lines.append("  column %d (%s): %d rows, first %s" % (c, name, len(idx), idx[:8].tolist()))
        for i in idx[:4]:
            lines.append("    row %d: got %r (%#018x) want %r (%#018x)%s" % (
                i, float(g2[i, c]), int(_words(g2[i:i + 1, c])[0]), float(w2[i, c]), int(_words(w2[i:i + 1, c])[0]),
                "" if inputs is None else " in %s" % np.array2string(np.asarray(inputs)[i], floatmode="unique", max_line_width=400)))
    raise AssertionError("\n".join(lines))


def edge_groups():
    """The groups of tests/golden/kat_bsdf_edges (made by tests/golden/make_bsdf_edges.py from the reference's own functions), sorted."""
    return sorted(f[:-len("_consts.f64")] for f in os.listdir(EDGES) if f.endswith("_consts.f64"))


def load_edge_group(group):
    """(consts[10], in[n][11], out[n][18]) of one group."""
    consts = np.fromfile(os.path.join(EDGES, group + "_consts.f64"))
    inp = np.fromfile(os.path.join(EDGES, group + "_in.f64")).reshape(-1, 11)
    out = np.fromfile(os.path.join(EDGES, group + "_out.f64")).reshape(-1, 18)
    assert consts.shape == (10,) and len(inp) == len(out)
    return consts, inp, out
