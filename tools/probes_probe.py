#!/usr/bin/env python3
"""The light probes (mcrt_render_probes) on one scene: what the projection costs beside the plain resolve of the same walk, and a
plausibility figure for the irradiance the coefficients give. HIP-event milliseconds from mcrt_stats: one warm-up, then --runs runs,
the median first.

  python tools/probes_probe.py [--scene hexagon_room] [--runs 5] [--what frame,probes,irradiance]

frame       1920 x 1080 at 16 samples (--width --height --sqrtspp), the camera's own rays: render_light_groups_device (the plain resolve)
            beside render_probes_device at orders 0 and 2, the same walk.
probes      64 probes x 4096 rays and 4096 probes x 1024 rays from points inside the scene: the probe rays alone
            (probe_rays_device), then - under a RAYS source fed with them, so that both calls walk the same rays -
            render_light_groups_device beside render_probes_device at orders 0 and 2, and render_probes_device with positions (the
            same bytes, checked).
irradiance  probe_irradiance at the normals of --points surface points (an AOV frame's first hits, lifted 1e-9 along the normal) from
            1024 uniform rays each, beside gather_irradiance there with 1024 cosine-weighted rays, and the gather against itself at
            another seed: the mean over the points of the relative difference of the summed planes' luminance-free mean channel.

A call's kernel_ms is the whole call - camera rays, searches, walk, resolve -, so "projection_ms" is a difference of two medians: the
probes call minus the light groups call over the same rays (it also holds the call's one device-to-device copy of the first rays'
directions). Prints one JSON line."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sqrtspp", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--what", default="frame,probes,irradiance")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", args.scene + ".mcrt"))
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    groups, names = m.light_group_map(img.scene, by="material")
    lg = dict(groups=groups, num_groups=len(names) - 1)
    planes = len(names)
    what = args.what.split(",")
    rec = {"scene": args.scene, "planes": planes}

    def timed(call):
        call()  # warm-up (scratch allocated here)
        ms = [round(call()["kernel_ms"], 4) for _ in range(max(args.runs, 1))]
        return {"kernel_ms": statistics.median(ms), "kernel_ms_runs": ms}

    def compare(cam, positions=None):
        """The plain resolve beside the projection over the same first rays -> dict."""
        pixels, spp = cam.width * cam.height, cam.sqrtspp ** 2
        out = torch.empty((planes * 9 * pixels * 3,), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        r = {"pixels": pixels, "spp": spp, "lanes_per_pixel": {"plain": 1, "order0": planes * 3, "order2": planes * 27}}
        r["light_groups"] = timed(lambda: ctx.render_light_groups_device(cam, args.seed, out.data_ptr(), **lg))
        for order in (0, 2):
            t = timed(lambda: ctx.render_probes_device(cam, args.seed, out.data_ptr(), order=order, **lg))
            t["projection_ms"] = round(t["kernel_ms"] - r["light_groups"]["kernel_ms"], 4)
            t["share_of_call"] = round(t["projection_ms"] / t["kernel_ms"], 5)
            r["probes_order%d" % order] = t
        return r, out

    if "frame" in what:
        cam = img.camera
        cam.width, cam.height, cam.sqrtspp = args.width, args.height, args.sqrtspp
        cam.shard_index, cam.shard_count = 0, 1
        rec["frame"], _ = compare(cam)
        rec["frame"].update(width=cam.width, height=cam.height)
    if "probes" in what:
        rec["probes"] = []
        for probes, sqrtspp in ((64, 64), (4096, 32)):
            cam = m.CameraDesc()
            cam.width, cam.height, cam.sqrtspp, cam.shard_count = probes, 1, sqrtspp, 1
            spp = sqrtspp * sqrtspp
            points = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, (probes, 3))).to("cuda:0")
            start = torch.empty((spp, probes, 3), dtype=torch.float64, device="cuda:0")
            direction = torch.empty_like(start)
            torch.cuda.synchronize()
            rays = timed(lambda: ctx.probe_rays_device(cam, args.seed, points.data_ptr(), start.data_ptr(), direction.data_ptr()))
            rays["TB_s"] = round((48 * spp * probes + 24 * probes) / (rays["kernel_ms"] * 1e-3) / 1e12, 3)
            ctx.set_ray_source("rays", start, direction)
            r, fed = compare(cam)
            fed = fed.clone()
            ctx.clear_ray_source()
            own = torch.empty_like(fed)
            torch.cuda.synchronize()
            r["probes_order2_positions"] = timed(lambda: ctx.render_probes_device(cam, args.seed, own.data_ptr(), positions=points.data_ptr(), order=2, **lg))
            r["positions_same_bits_as_fed_rays"] = bool((own.view(torch.int64) == fed.view(torch.int64)).all().item())
            r["probe_rays"] = rays
            rec["probes"].append(r)
    if "irradiance" in what:
        side = max(int(math.isqrt(args.points)), 2)
        cam = img.camera
        cam.width, cam.height, cam.sqrtspp = side, side, 1
        cam.shard_index, cam.shard_count = 0, 1
        aov = ctx.render_aov(cam, args.seed)
        hit = aov["coverage"].reshape(-1) > 0
        position, normal = aov["position"].reshape(-1, 3)[hit], aov["shading_normal"].reshape(-1, 3)[hit]
        n = position.shape[0]
        cam.width, cam.height, cam.sqrtspp = n, 1, 32
        baked = ctx.bake_probes(position + normal * 1e-9, rays=1024, order=2, global_seed=args.seed, **lg)
        e_probe = m.probe_irradiance(baked["sh"][:, :, None], normal[None]).sum(axis=0)[0]  # [n, 3], the planes summed
        gather = [ctx.gather_irradiance(cam, seed, position.reshape(1, n, 3), normal.reshape(1, n, 3), **lg).sum(axis=0)[0] for seed in (args.seed, args.seed + 1)]
        value = lambda e: e.mean(axis=1)
        rel = lambda a, b: float(np.mean(np.abs(value(a) - value(b)) / np.maximum(value(b), 1e-300)))
        rec["irradiance"] = {"points": n, "rays": 1024, "mean_gather": float(value(gather[0]).mean()), "mean_probe": float(value(e_probe).mean()),
                             "probe_vs_gather_mean_relative_difference": round(rel(e_probe, gather[0]), 5),
                             "gather_vs_gather_other_seed_mean_relative_difference": round(rel(gather[1], gather[0]), 5)}
    print(json.dumps(rec), flush=True)
    ctx.close()
    img.close()


if __name__ == "__main__":
    main()
