#!/usr/bin/env python3
"""Compare two frames with the library's frame comparison (include/mcrt.h "Frame comparison", Context.frame_compare) and print the result.

    python tools/compare_probe.py FRAME REF [--width W --height H] [--mask MASK] [--eps X] [--peak X] [--ssim-range X] [--no-ssim]
                                  [--device D] [--numpy] [--exr OUT.exr]

FRAME, REF: [H, W, 3] float64 as .npy (what bench.py --dump-outputs writes) or raw little-endian binary64 (then --width and --height say
the shape; what host/mcrt_render writes). MASK: [H, W] float64 the same way; a pixel takes part where it is > 0. Prints one JSON line of
mcrt_compare_result. --numpy also evaluates the header's definition in numpy on the host - written out in this file, operation by
operation - and prints it and whether every field and every map equals the library's, bit for bit. --exr writes FRAME with the error
maps (error.se, error.rel, error.ssim) into one OpenEXR file."""
import argparse
import importlib
import json
import os
import re
import struct
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIELDS = ("sum_se", "sum_ae", "sum_rel", "sum_ssim", "max_abs", "max_abs_pixel", "max_abs_channel", "pixels", "compared", "nonfinite", "masked", "differing",
          "ssim_centres", "ssim_excluded", "mse", "mae", "relmse", "rmse", "psnr", "mean_ssim")
MAPS = ("squared_error", "relative", "ssim")


def load(path, width, height, channels):
    if path.endswith(".npy"):
        a = np.load(path)
    else:
        assert width and height, "%s is raw: --width and --height say its shape" % path
        a = np.fromfile(path, dtype="<f8")
        assert a.size == width * height * channels, "%s holds %d values, %d x %d x %d are %d" % (path, a.size, width, height, channels, width * height * channels)
        a = a.reshape((height, width, 3) if channels == 3 else (height, width))
    assert a.dtype == np.float64 and a.ndim == (3 if channels == 3 else 2), (path, a.dtype, a.shape)
    return np.ascontiguousarray(a)


def weights():
    """g[-5 .. 5]: the literals of include/mcrt.h."""
    text = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    lit = {int(k): float.fromhex(v) for k, v in re.findall(r"#define MCRT_SSIM_G(\d) (0x[0-9a-fA-F.]+p[-+]?\d+)", text)}
    return np.array([lit[abs(i)] for i in range(-5, 6)])


def treesum(values):
    """Blocks of 256 consecutive values, stride 128 .. 1 pairing k with k + stride where both exist, again on the block values."""
    t = np.array(values, dtype=np.float64).ravel()
    while True:
        blocks = -(-t.size // 256)
        pad = np.zeros(blocks * 256)
        pad[:t.size] = t
        pad = pad.reshape(blocks, 256)
        length = np.minimum(256, t.size - 256 * np.arange(blocks))[:, None]
        stride = 128
        while stride:
            pair = np.arange(stride)[None, :] + stride < length
            pad[:, :stride] = np.where(pair, pad[:, :stride] + pad[:, stride:2 * stride], pad[:, :stride])
            stride //= 2
        t = pad[:, 0].copy()
        if blocks == 1:
            return float(t[0])


def restate(rgb, ref, mask=None, eps=0.01, peak=1.0, ssim_range=1.0, ssim=True):
    """The definition of include/mcrt.h in numpy -> dict of the result's fields and the maps."""
    import math
    height, width = rgb.shape[:2]
    r = {}
    with np.errstate(all="ignore"):
        masked = ~(mask > 0) if mask is not None else np.zeros((height, width), dtype=bool)
        finite = np.all(rgb - rgb == 0.0, axis=2) & np.all(ref - ref == 0.0, axis=2)
        compared = ~masked & finite
        d = rgb - ref
        a = np.where(d < 0, 0.0 - d, d)
        q = (d * d) / (ref * ref + eps)
        se = np.where(compared, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], 0.0)
        ae = np.where(compared, (a[..., 0] + a[..., 1]) + a[..., 2], 0.0)
        rel = np.where(compared, (q[..., 0] + q[..., 1]) + q[..., 2], 0.0)
        r.update(sum_se=treesum(se), sum_ae=treesum(ae), sum_rel=treesum(rel), pixels=height * width, compared=int(compared.sum()),
                 nonfinite=int((~masked & ~finite).sum()), masked=int(masked.sum()),
                 differing=int((~masked & np.any(rgb.view(np.uint64) != ref.view(np.uint64), axis=2)).sum()))
        r.update(max_abs=0.0, max_abs_pixel=2 ** 64 - 1, max_abs_channel=2 ** 32 - 1, mse=0.0, mae=0.0, relmse=0.0, rmse=0.0, psnr=0.0)
        if r["compared"]:
            flat = np.where(compared[..., None], a, -1.0).ravel()
            at = int(np.argmax(flat))
            n = float(3 * r["compared"])
            r.update(max_abs=float(flat[at]), max_abs_pixel=at // 3, max_abs_channel=at % 3, mse=r["sum_se"] / n, mae=r["sum_ae"] / n, relmse=r["sum_rel"] / n)
            r["rmse"] = math.sqrt(r["mse"])
            r["psnr"] = float("inf") if r["mse"] == 0.0 else (10.0 * math.log10(peak * peak / r["mse"]) if r["mse"] > 0 else float("nan"))
        r.update(squared_error=se, relative=rel, ssim=np.zeros((height, width)) if ssim else None, sum_ssim=0.0, ssim_centres=0, ssim_excluded=0, mean_ssim=0.0)
        if ssim and width >= 11 and height >= 11:
            g, cw, ch = weights(), width - 10, height - 10
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
            r.update(sum_ssim=treesum(s), ssim_centres=cw * ch, ssim_excluded=int((~fin).sum()))
            if r["ssim_centres"] > r["ssim_excluded"]:
                r["mean_ssim"] = r["sum_ssim"] / float(r["ssim_centres"] - r["ssim_excluded"])
            r["ssim"][5:height - 5, 5:width - 5] = s
    return r


def same(got, want):
    """Names of the fields and maps whose bits differ."""
    bad = []
    for k in FIELDS:
        if (struct.pack("<d", got[k]) != struct.pack("<d", want[k])) if isinstance(want[k], float) else got[k] != want[k]:
            bad.append(k)
    for k in MAPS:
        if want[k] is not None and k in got and not np.array_equal(np.asarray(got[k]).view(np.uint64), want[k].view(np.uint64)):
            bad.append(k)
    return bad


def printable(r):
    return {k: (repr(r[k]) if isinstance(r[k], float) and not np.isfinite(r[k]) else r[k]) for k in FIELDS}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("frame")
    ap.add_argument("ref")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--mask", default=None)
    ap.add_argument("--eps", type=float, default=None)
    ap.add_argument("--peak", type=float, default=None)
    ap.add_argument("--ssim-range", type=float, default=None)
    ap.add_argument("--no-ssim", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--exr", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("monte-carlo-ray-tracer_amd")
    rgb, ref = load(args.frame, args.width, args.height, 3), load(args.ref, args.width, args.height, 3)
    assert rgb.shape == ref.shape, (rgb.shape, ref.shape)
    mask = load(args.mask, rgb.shape[1], rgb.shape[0], 1) if args.mask else None
    ctx = pkg.Context(args.device)
    stats = {}
    want_maps = args.numpy or bool(args.exr)
    got = ctx.frame_compare(rgb, ref, mask, eps=args.eps, peak=args.peak, ssim_range=args.ssim_range, ssim=not args.no_ssim, maps=want_maps, stats=stats)
    print(json.dumps(dict(printable(got), kernel_ms=stats["kernel_ms"], total_ms=stats["total_ms"], kernel_launches=stats["kernel_launches"])))
    if args.numpy:
        want = restate(rgb, ref, mask, args.eps or 0.01, args.peak or 1.0, args.ssim_range or 1.0, not args.no_ssim)
        bad = same(got, want)
        print(json.dumps(dict(printable(want), numpy=True, equal=not bad, differing_fields=bad)))
    if args.exr:
        res = ctx.exr_save(args.exr, pkg.exr_layers(rgb=rgb, errors=got))
        print(json.dumps(dict(res, exr=args.exr)))
    ctx.close()
    return 1 if args.numpy and bad else 0


if __name__ == "__main__":
    sys.exit(main())
