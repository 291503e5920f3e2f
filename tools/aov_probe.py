#!/usr/bin/env python3
"""Time of the first-hit AOV pass (mcrt_render_aov_device) next to the beauty frame of the same camera: HIP-event milliseconds from
mcrt_stats, one warm-up, then the median of --runs runs; Mray/s = camera rays / that time. The beauty frame is rendered once after
its own warm-up; its rays per path say how much longer a path is than the first hit the AOV pass stops at.

  python tools/aov_probe.py [--width 1920 --height 1080 --sqrtspp 4] [--runs 5] [--scenes hexagon_room,coffee_maker_qsah]

Prints one JSON line per scene."""
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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sqrtspp", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--scenes", default="hexagon_room,coffee_maker_qsah")
    ap.add_argument("--no-beauty", action="store_true")
    args = ap.parse_args()
    import torch
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    for name in args.scenes.split(","):
        img = m.SceneImage(os.path.join(ROOT, "tests", "golden", name + ".mcrt"))
        cam = img.camera
        cam.width, cam.height, cam.sqrtspp = args.width, args.height, args.sqrtspp
        cam.shard_index, cam.shard_count = 0, 1
        ctx = m.Context(0)
        ctx.upload_scene(img.scene)
        bufs = {k: torch.empty((cam.height, cam.width) + ((n,) if n > 1 else ()), dtype=torch.float64 if dt.__name__ == "float64" else torch.int32, device="cuda:0")
                for k, (dt, n) in m.AOV_CHANNELS.items()}
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        ctx.render_aov_device(cam, args.seed, ptrs)  # warm-up (scratch allocated here)
        runs = [ctx.render_aov_device(cam, args.seed, ptrs) for _ in range(max(args.runs, 1))]
        ms = statistics.median(r["kernel_ms"] for r in runs)
        rec = {"scene": name, "width": cam.width, "height": cam.height, "spp": cam.sqrtspp ** 2, "aov_rays": runs[0]["rays"], "aov_ms_median": round(ms, 3),
               "aov_ms_runs": [round(r["kernel_ms"], 3) for r in runs], "aov_Mray_s": round(runs[0]["rays"] / ms / 1e3, 1), "aov_launches": runs[0]["kernel_launches"],
               "coverage_mean": float(bufs["coverage"].mean().item())}
        if not args.no_beauty:
            rgb = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            for _ in range(2):  # warm-up, then the one that counts
                ctx.render_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr())
                st = ctx.render_finish()
            rec.update({"beauty_ms": round(st["kernel_ms"], 3), "beauty_rays_per_path": round(st["rays"] / st["paths"], 3),
                        "beauty_Mray_s": round(st["rays"] / st["kernel_ms"] / 1e3, 1), "beauty_kernel": m.KERNEL_NAMES[st["kernel_id"]].split(" ")[0]})
        print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


if __name__ == "__main__":
    main()
