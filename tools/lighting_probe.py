#!/usr/bin/env python3
"""The lighting passes (mcrt_render_lighting_device) on one scene, next to a path-traced render of the same camera, seed and sample count
on the same build: the mean of every channel, the share of the beauty frame that is direct light - mean((emission + direct) + sky) /
mean(beauty): what the path tracer's path cut after its second vertex carries - and the pass's time beside the render's, both HIP-event
milliseconds from mcrt_stats: one warm-up, then the median of --runs runs.

  python tools/lighting_probe.py [--scene hexagon_room] [--width 1920 --height 1080 --sqrtspp 16] [--runs 5] [--no-render]
                                 [--chunk-rays N]

The default frame is the benchmark's (bench.py c2: hexagon_room, 1920 x 1080 at 256 samples a pixel). Prints one JSON line. The pass
traces 3 rays per sample through the general closest-hit search, the render as many as its paths are long through whichever kernel form
the scene gets, so the ratio of the two times is a finding, not a bar. For the share of each kernel, run it under a kernel trace with
--runs 1: the pass's kernels are lightingRayKernel and lightingResolveKernel, the camera rays' aovRayKernel,
the search is the trace or intersect kernel between them."""
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
    ap.add_argument("--sqrtspp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--chunk-rays", type=int, default=0, help="option MCRT_AOV_CHUNK_RAYS: shadow and bounce slots per chunk (0: the default)")
    args = ap.parse_args()
    import torch
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", args.scene + ".mcrt"))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = args.width, args.height, args.sqrtspp
    cam.shard_index, cam.shard_count = 0, 1
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    if args.chunk_rays:
        ctx.set_option("MCRT_AOV_CHUNK_RAYS", args.chunk_rays)
    bufs = {k: torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0") for k in m.LIGHTING_CHANNELS}
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    ctx.render_lighting_device(cam, args.seed, ptrs)  # warm-up (scratch allocated here)
    runs = [ctx.render_lighting_device(cam, args.seed, ptrs) for _ in range(max(args.runs, 1))]
    ms = statistics.median(r["kernel_ms"] for r in runs)
    rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "spp": cam.sqrtspp ** 2, "traced": runs[0]["rays"], "paths": runs[0]["paths"],
           "launches": runs[0]["kernel_launches"], "chunk_rays": args.chunk_rays or None, "kernel_ms": round(ms, 3), "kernel_ms_runs": [round(r["kernel_ms"], 3) for r in runs],
           "Mray_s": round(runs[0]["rays"] / ms / 1e3, 1), "mean": {k: round(v.mean().item(), 6) for k, v in bufs.items()}}
    lit, unoccluded = bufs["light"].sum().item(), bufs["unoccluded"].sum().item()
    rec["shadow_matte_mean"] = round(lit / unoccluded, 6) if unoccluded > 0 else None
    if not args.no_render:
        rgb = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        render = []
        for _ in range(max(args.runs, 1) + 1):
            ctx.render_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr())
            render.append(ctx.render_finish())
        rms = statistics.median(r["kernel_ms"] for r in render[1:])
        cut = (bufs["emission"] + bufs["direct"]) + bufs["sky"]
        rec["render"] = {"kernel_id": render[-1]["kernel_id"], "kernel_ms": round(rms, 3), "kernel_ms_runs": [round(r["kernel_ms"], 3) for r in render[1:]],
                         "rays": render[-1]["rays"], "rays_per_path": round(render[-1]["rays"] / render[-1]["paths"], 3), "mean": round(rgb.mean().item(), 6)}
        rec["direct_share_of_beauty"] = round(cut.mean().item() / rgb.mean().item(), 6)
        rec["pass_over_render"] = round(ms / rms, 4)
    print(json.dumps(rec), flush=True)
    ctx.close()
    img.close()


if __name__ == "__main__":
    main()
