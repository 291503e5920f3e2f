#!/usr/bin/env python3
"""The occlusion pass (mcrt_render_occlusion_device) on one scene: the range and mean of every channel and the pass's time - HIP-event
milliseconds from mcrt_stats, one warm-up, then the median of --runs runs; Mray/s = (camera rays + occlusion slots traced) / that time -,
next to the first-hit AOV pass of the same camera (the closest-hit search of the camera rays alone, between its own two kernels).

  python tools/occlusion_probe.py [--scene hexagon_room] [--width 1920 --height 1080 --sqrtspp 4] [--rays 1,4] [--distance 0]
                                  [--geometric] [--runs 5] [--no-aov]

Prints one JSON line per number of rays (--rays "" : none), then one for the AOV pass. For the share of each kernel, run it under a kernel trace with
--runs 1: the pass's kernels are occlusionRayKernel and occlusionResolveKernel, the AOV pass's aovRayKernel and aovResolveKernel, the
search is the trace or intersect kernel between them."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sqrtspp", type=int, default=4)
    ap.add_argument("--rays", default="1,4")
    ap.add_argument("--distance", type=float, default=0.0)
    ap.add_argument("--geometric", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--no-aov", action="store_true")
    args = ap.parse_args()
    import torch
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", args.scene + ".mcrt"))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = args.width, args.height, args.sqrtspp
    cam.shard_index, cam.shard_count = 0, 1
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    bufs = {k: torch.empty((cam.height, cam.width) + ((n,) if n > 1 else ()), dtype=torch.float64, device="cuda:0") for k, (_, n) in m.OCCLUSION_CHANNELS.items()}
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    for rays in [int(r) for r in args.rays.split(",") if r]:
        kw = dict(rays=rays, max_distance=args.distance, geometric=args.geometric)
        ctx.render_occlusion_device(cam, args.seed, ptrs, **kw)  # warm-up (scratch allocated here)
        runs = [ctx.render_occlusion_device(cam, args.seed, ptrs, **kw) for _ in range(max(args.runs, 1))]
        ms = statistics.median(r["kernel_ms"] for r in runs)
        length = bufs["bent_normal"].square().sum(dim=-1).sqrt()
        rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "spp": cam.sqrtspp ** 2, "rays": rays, "max_distance": args.distance,
               "geometric": args.geometric, "traced": runs[0]["rays"], "paths": runs[0]["paths"], "launches": runs[0]["kernel_launches"],
               "ms_median": round(ms, 3), "ms_runs": [round(r["kernel_ms"], 3) for r in runs], "Mray_s": round(runs[0]["rays"] / ms / 1e3, 1)}
        for k in ("ao", "sky"):
            rec[k] = {"min": bufs[k].min().item(), "max": bufs[k].max().item(), "mean": round(bufs[k].mean().item(), 6)}
        rec["bent_length"] = {"min": length.min().item(), "max": length.max().item(), "mean": round(length.mean().item(), 6)}
        print(json.dumps(rec), flush=True)
    if not args.no_aov:
        aov = {k: torch.empty((cam.height, cam.width) + ((n,) if n > 1 else ()), dtype=torch.float64 if dt.__name__ == "float64" else torch.int32, device="cuda:0")
               for k, (dt, n) in m.AOV_CHANNELS.items()}
        torch.cuda.synchronize()
        aptrs = {k: v.data_ptr() for k, v in aov.items()}
        ctx.render_aov_device(cam, args.seed, aptrs)
        runs = [ctx.render_aov_device(cam, args.seed, aptrs) for _ in range(max(args.runs, 1))]
        ms = statistics.median(r["kernel_ms"] for r in runs)
        print(json.dumps({"scene": args.scene, "pass": "aov", "traced": runs[0]["rays"], "ms_median": round(ms, 3), "ms_runs": [round(r["kernel_ms"], 3) for r in runs],
                          "Mray_s": round(runs[0]["rays"] / ms / 1e3, 1), "coverage_mean": round(aov["coverage"].mean().item(), 6)}), flush=True)
    ctx.close()
    img.close()


if __name__ == "__main__":
    main()
