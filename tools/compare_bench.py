#!/usr/bin/env python3
"""Timing of the frame comparison at 1920 x 1080 on one MI355X (profiles/NOTES_compare.md): seeded random frames in device memory; per
variant 3 untimed and 30 timed calls, wall time around the call and the call's own kernel_ms (HIP events around its launches); then what
the call replaces - two frame downloads and the numpy restatement of tools/compare_probe.py - timed once, and the library's result held
to that restatement bit for bit. mcrt_frame_noise_device on the same frame runs first: its level 0 is the existing reader of the same bytes.

    python tools/compare_bench.py
    rocprofv3 --kernel-trace --stats -d OUT -o compare --output-format csv -- python tools/compare_bench.py --profiled

--profiled: 10 timed calls per variant and no numpy part - the run for the per-kernel times of the trace."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
profiled = "--profiled" in sys.argv
pkg = importlib.import_module("monte-carlo-ray-tracer_amd")
W, H = 1920, 1080
rng = np.random.default_rng(5)
ref = rng.random((H, W, 3))
rgb = ref + (rng.random((H, W, 3)) - 0.5) * 0.125
var = rng.random((H, W, 3))
mask = np.where(rng.random((H, W)) < 0.1, 0.0, 1.0)
d_rgb, d_ref, d_var, d_mask = (torch.from_numpy(a).to("cuda:0") for a in (rgb, ref, var, mask))
maps = {k: torch.empty((H, W), dtype=torch.float64, device="cuda:0") for k in pkg.COMPARE_MAPS}
torch.cuda.synchronize()
ctx = pkg.Context(0)
reps = 10 if profiled else 30


def timed(fn):
    for _ in range(3):
        fn()
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        if st:
            kern.append(st["kernel_ms"])
    return dict(wall_ms_median=round(statistics.median(wall), 4), wall_ms_min=round(min(wall), 4),
                kernel_ms_median=round(statistics.median(kern), 4) if kern else None, kernel_ms_min=round(min(kern), 4) if kern else None)


par0 = pkg.CompareParams(0, 0, 0, 0, 0)
par1 = pkg.CompareParams(0, 0, 0, 1, 0)
ptrs = {k: v.data_ptr() for k, v in maps.items()}
out = {}
out["frame_noise_device"] = timed(lambda: ctx.frame_noise_device(W * H, 16, d_rgb.data_ptr(), d_var.data_ptr()) and None)
out["compare_no_ssim"] = timed(lambda: ctx.frame_compare_device(W, H, d_rgb.data_ptr(), d_ref.data_ptr(), None, None, par0)[1])
out["compare_no_ssim_mask"] = timed(lambda: ctx.frame_compare_device(W, H, d_rgb.data_ptr(), d_ref.data_ptr(), d_mask.data_ptr(), None, par0)[1])
out["compare_ssim"] = timed(lambda: ctx.frame_compare_device(W, H, d_rgb.data_ptr(), d_ref.data_ptr(), None, None, par1)[1])
out["compare_ssim_all_maps"] = timed(lambda: ctx.frame_compare_device(W, H, d_rgb.data_ptr(), d_ref.data_ptr(), d_mask.data_ptr(), ptrs, par1)[1])
out["compare_host_form_ssim"] = timed(lambda: ctx.frame_compare(rgb, ref, stats=(s := {})) and s)
bytes_px = W * H * 48
out["bytes_two_frames"] = bytes_px
for k in ("compare_no_ssim",):
    out[k + "_GBps_by_kernel_ms_min"] = round(bytes_px / out[k]["kernel_ms_min"] / 1e6, 1)
if not profiled:
    import compare_probe
    t0 = time.perf_counter()
    h_rgb, h_ref = d_rgb.cpu().numpy(), d_ref.cpu().numpy()
    t1 = time.perf_counter()
    want0 = compare_probe.restate(h_rgb, h_ref, None, ssim=False)
    t2 = time.perf_counter()
    want1 = compare_probe.restate(h_rgb, h_ref, mask)
    t3 = time.perf_counter()
    out["replaced"] = dict(download_two_frames_ms=round((t1 - t0) * 1e3, 2), numpy_no_ssim_ms=round((t2 - t1) * 1e3, 2), numpy_ssim_mask_ms=round((t3 - t2) * 1e3, 2))
    got0 = ctx.frame_compare(d_rgb, d_ref, ssim=False)
    got1 = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in ctx.frame_compare(d_rgb, d_ref, d_mask, maps=True).items()}
    bad = compare_probe.same(got0, dict(want0, ssim=None, squared_error=None, relative=None)) + compare_probe.same(got1, want1)
    out["equal_to_numpy_at_1080p"] = not bad
    out["differing_fields"] = bad
    out["mean_ssim"], out["mse"] = want1["mean_ssim"], want1["mse"]
print(json.dumps(out, indent=1))
ctx.close()
