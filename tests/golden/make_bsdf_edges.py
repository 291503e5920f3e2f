#!/usr/bin/env python3
"""Writes tests/golden/kat_bsdf_edges/: the lobe functions of mcrt_bsdf (Fresnel::dielectric / conductor, GGX::reflection /
transmission / visibleMicrofacet / D / Lambda, Material::diffuseReflection) at the EDGES of their domain, answered by the reference's
own functions (oracle/_ref/mcrt_ref bsdf: the row body of the kat mode on inputs from a file). Needs the reference binary, so it
runs where tests/golden/make_golden.py runs; the outputs are committed.

kat_hexagon_room/bsdf_*.f64 holds 4000 random vectors from the middle of the domain: no component is 0, wo.z is never 0 or 1,
alpha is in [0.01, 0.9], n1 != n2 and no critical angle, one roughness, one complex IOR. Here every factor of a vector has a list of
edge values and a short list of benign ones; each edge list is crossed with benign values of the other factors, and the pairs that
interact are crossed with each other: wo x wi, wo x (n1, n2), wo x alpha x (u, v), alpha x (u, v). No random numbers.

  g<k>_consts.f64  consts[10] of mcrt_bsdf   g<k>_in.f64  in[n][11]   g<k>_out.f64  out[n][18], the reference's

What the set has to contain is asserted on the committed files by tests/test_bsdf_edges.py."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.path.join(ROOT, "oracle", "_ref", "mcrt_ref")
OUT = os.path.join(HERE, "kat_bsdf_edges")

# consts[10] = roughness, reflectance[3] of the diffuse material, complex IOR real[3], imaginary[3]
GROUPS = [
    ("g0", [0.7, 0.8, 0.6, 0.4, 0.27, 0.68, 1.32, 3.6, 2.6, 2.3]),              # kat_hexagon_room's
    # Material::computeProperties: rough = roughness > C::EPSILON (1e-9). At and far below it: Lambertian, whatever Oren-Nayar would give
    ("g1", [1e-9, 0.0, 1.0, 0.2, 0.27, 0.68, 1.32, 3.6, 2.6, 2.3]),
    ("g2", [1e-160, 1.0, 0.0, 0.2, 0.27, 0.68, 1.32, 3.6, 2.6, 2.3]),
    # ... the next double above it: Oren-Nayar, with its 0 / 0 when a direction is the normal
    ("g3", [float(np.nextafter(1e-9, 1.0)), 0.2, 1.0, 0.0, 0.27, 0.68, 1.32, 3.6, 2.6, 2.3]),
    # a complex IOR with a real part of 1 and imaginary parts 0, tiny (its square is 0) and small
    ("g4", [0.7, 0.8, 0.6, 0.4, 1.0, 1.0, 1.0, 0.0, 1e-160, 1e-7]),
    # ... and with components of 1e3 and 1e-3
    ("g5", [0.7, 0.8, 0.6, 0.4, 1e3, 1e-3, 1e3, 1e-3, 1e3, 1e3]),
]

N_EDGES = [(1.0, 1.0), (1.5, 1.5), (1.5, 1.0), (1.5, 1.0 + 2.0 ** -52), (1.0, 1000.0), (1000.0, 1.0), (2.5, 1.0)]
N_BENIGN = [(1.2, 1.7), (1.6, 1.1)]


def at_cos(c):
    """A direction with wo.z = c at an azimuth whose sine and cosine are exact in binary to a few bits (0.6, 0.8)."""
    s = math.sqrt(1.0 - c * c)
    return (s * 0.6, s * 0.8, c)


def unit(x, y, z):
    l = math.sqrt(x * x + y * y + z * z)
    return (x / l, y / l, z / l)


def wo_edges():
    e = [(0.0, 0.0, 1.0), (-0.0, -0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]
    e += [at_cos(c) for c in (1e-3, 1e-8, 1e-160, 1.0 - 2.0 ** -53, -0.5)]
    for n1, n2 in N_EDGES:  # total internal reflection begins where g2 = (n2 / n1)^2 + cos^2 - 1 changes sign (Fresnel::dielectric)
        if n2 < n1:
            c = math.sqrt(1.0 - (n2 / n1) ** 2)
            e += [at_cos(c), at_cos(float(np.nextafter(c, 0.0))), at_cos(float(np.nextafter(c, 2.0)))]
    return e


WO_EDGES = wo_edges()
WO_BENIGN = [unit(0.3, -0.4, 0.866), unit(-0.5, 0.2, 0.5)]
# wi as the ABI takes it, before its fold into the upper hemisphere (|z| + 1e-3, renormalised); "same" = wo, "mirror" = wo mirrored in
# xy (the half vector is the normal)
WI_EDGES = [(0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), unit(0.3, -0.5, -0.81), "same", "mirror"]
WI_BENIGN = [unit(-0.2, 0.5, 0.7), unit(0.6, 0.1, 0.4)]
ALPHA_EDGES = [1e-160, 1e-8, 1e-3, 1.0]
ALPHA_BENIGN = [0.15, 0.6]
# visibleMicrofacet: r = sqrt(u), phi = 2 pi v. phi at 0, at multiples of pi / 2 and at 2 pi; 1 - t1^2 - t2^2 at, above and below 0
UV_EDGES = [(0.0, 0.0), (1.0, 1.0), (1.0 - 2.0 ** -53, 0.25), (0.5, 0.5), (2.0 ** -1074, 0.75), (0.3, 1.0 - 2.0 ** -53), (1.0, 0.0)]
UV_BENIGN = [(0.37, 0.81), (0.62, 0.13)]


def rows(microfacet_cross):
    """microfacet_cross: with wo x alpha x (u, v), which only GGX::visibleMicrofacet and D(m) read and no constant touches (g0 has it)."""
    out = []

    def add(wi, wo, n, alpha, uv):
        if wi == "same":
            wi = wo
        elif wi == "mirror":
            wi = (-wo[0], -wo[1], wo[2])
        out.append(list(wi) + list(wo) + list(n) + [alpha] + list(uv))

    def benign(k):  # the k-th of a fixed cycle of benign combinations (the lists have two entries each)
        return (WI_BENIGN[k & 1], WO_BENIGN[(k >> 1) & 1], N_BENIGN[(k >> 2) & 1], ALPHA_BENIGN[(k >> 3) & 1], UV_BENIGN[(k >> 4) & 1])

    combos = [0, 7, 10, 21, 28, 31]
    # the benign middle: the full cross of the benign lists
    for k in range(32):
        add(*benign(k))
    # each edge list against benign values of the other factors
    for k in combos:
        wi, wo, n, al, uv = benign(k)
        for e in WO_EDGES:
            add(wi, e, n, al, uv)
        for e in WI_EDGES:
            add(e, wo, n, al, uv)
        for e in N_EDGES:
            add(wi, wo, e, al, uv)
        for e in ALPHA_EDGES:
            add(wi, wo, n, e, uv)
        for e in UV_EDGES:
            add(wi, wo, n, al, e)
    # the pairs that interact
    for k in combos[:2]:
        wi, wo, n, al, uv = benign(k)
        for eo in WO_EDGES:
            for ei in WI_EDGES:
                add(ei, eo, n, al, uv)
            for en in N_EDGES:
                add(wi, eo, en, al, uv)
    wi, wo, n, al, uv = benign(combos[2])
    for eo in WO_EDGES if microfacet_cross else []:
        for ea in ALPHA_EDGES:
            for eu in UV_EDGES:
                add(wi, eo, n, ea, eu)
    for k in combos:
        wi, wo, n, al, uv = benign(k)
        for ea in ALPHA_EDGES:
            for eu in UV_EDGES:
                add(wi, wo, n, ea, eu)
    return np.array(out, dtype=np.float64)


def main():
    if not os.path.exists(REF):
        sys.exit("%s is missing: build it first (oracle/Makefile, target ref)" % REF)
    os.makedirs(OUT, exist_ok=True)
    for name, consts in GROUPS:
        inp = rows(name == "g0")
        assert inp.shape[1] == 11 and len(inp) <= 4000, inp.shape
        base = os.path.join(OUT, name)
        np.array(consts, dtype=np.float64).tofile(base + "_consts.f64")
        inp.tofile(base + "_in.f64")
        with tempfile.TemporaryDirectory() as tmp:
            raw = os.path.join(tmp, "out.f64")
            subprocess.run([REF, "bsdf", "--consts", base + "_consts.f64", "--in", base + "_in.f64", "--out", raw], check=True, stdout=subprocess.DEVNULL)
            out = np.fromfile(raw).reshape(-1, 18)
        assert len(out) == len(inp)
        out.tofile(base + "_out.f64")
        nan = np.isnan(out[:, :17]).mean(axis=0)
        live = (np.isfinite(out[:, :17]) & (out[:, :17] != 0)).mean(axis=0)
        print("%s: %d rows; NaN at most %.1f %% (column %d); finite and nonzero at least %.1f %% (column %d)"
              % (name, len(out), 100 * nan.max(), nan.argmax(), 100 * live.min(), live.argmin()))


if __name__ == "__main__":
    main()
