#!/usr/bin/env python3
"""The ray sources (mcrt_set_ray_source) on one scene: with no source the time of the AOV pass, of the light groups in one plane and of
the ray kernel alone (mcrt_camera_rays_device: one launch, its own event pair) - the numbers a build of another commit is compared by -,
then the ray kernel alone under each kind of source with the bytes it moves, and Context.gather_irradiance's walk (the light groups under
a SURFACE source made of the AOV pass's own frames) beside render_lens at the same sample count. HIP-event milliseconds from mcrt_stats:
one warm-up, then --runs runs, the median first.

  python tools/ray_source_probe.py [--scene hexagon_room] [--width 1920 --height 1080 --sqrtspp 4] [--runs 5] [--package DIR]
  python tools/ray_source_probe.py --dump [--kind surface|rays] [--width 4 --height 3 --sqrtspp 1]

--package DIR: the directory that holds the monte-carlo-ray-tracer_amd package to load (default: this tree) - a build of another commit,
for the same measurement there; a package without mcrt_set_ray_source measures the no-source rows only. --dump prints one JSON line per
first ray of a small frame under a source made of the AOV frame (surface) or of the camera's own rays (rays) instead of timing anything.
Prints one JSON line otherwise. Bytes: RAYS reads 48 and writes 48 per ray; SURFACE reads 48 per pixel (counted once per sample here
only where it says so) and writes 48 per ray."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--sqrtspp", type=int, default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--dump", action="store_true")
    ap.add_argument("--kind", default="surface", choices=("surface", "rays"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import torch
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", args.scene + ".mcrt"))
    cam = img.camera
    small = args.dump
    cam.width, cam.height, cam.sqrtspp = args.width or (4 if small else 1920), args.height or (3 if small else 1080), args.sqrtspp or (1 if small else 4)
    cam.shard_index, cam.shard_count = 0, 1
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    has_source = hasattr(m.Context, "set_ray_source")
    pixels, spp = cam.width * cam.height, cam.sqrtspp ** 2
    n = pixels * spp

    aov = {k: torch.empty((pixels * c,), dtype=torch.float64 if dt == m.np.float64 else torch.int32, device="cuda:0") for k, (dt, c) in m.AOV_CHANNELS.items()}
    plane = torch.empty((pixels, 3), dtype=torch.float64, device="cuda:0")
    rays = [torch.empty((n, 3), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    out = [torch.empty((n, 3), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    aov_ptrs = {k: v.data_ptr() for k, v in aov.items()}

    if args.dump:
        ctx.render_aov_device(cam, args.seed, aov_ptrs)
        if args.kind == "surface":
            ctx.set_ray_source("surface", aov["position"].view(pixels, 3), aov["normal"].view(pixels, 3))
        else:
            ctx.camera_rays_device(cam, args.seed, rays[0].data_ptr(), rays[1].data_ptr())
            ctx.set_ray_source("rays", rays[0].view(spp, pixels, 3), rays[1].view(spp, pixels, 3))
        start, direction = ctx.camera_rays(cam, args.seed)
        for i in range(start.shape[0]):
            for y in range(cam.height):
                for x in range(cam.width):
                    print(json.dumps({"x": x, "y": y, "sample": i, "start": start[i, y, x].tolist(), "direction": direction[i, y, x].tolist()}))
        ctx.close()
        return

    def timed(call):
        call()  # warm-up (scratch allocated here)
        runs = [call() for _ in range(max(args.runs, 1))]
        ms = [round(r["kernel_ms"], 4) for r in runs]
        return {"kernel_ms": statistics.median(ms), "kernel_ms_runs": ms, "rays": runs[0]["rays"], "launches": runs[0]["kernel_launches"]}

    def with_rate(t, nbytes):
        t["bytes"] = nbytes
        t["TB_s"] = round(nbytes / (t["kernel_ms"] * 1e-3) / 1e12, 3)
        return t

    rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "spp": spp, "package": os.path.abspath(args.package)}
    walk = lambda: ctx.render_light_groups_device(cam, args.seed, plane.data_ptr(), sky_plane=0, num_groups=1)
    none = {"render_aov": timed(lambda: ctx.render_aov_device(cam, args.seed, aov_ptrs)), "render_light_groups": timed(walk)}
    none["beauty_mean"] = round(plane.mean().item(), 6)
    if hasattr(ctx, "camera_rays_device"):
        none["camera_rays"] = with_rate(timed(lambda: ctx.camera_rays_device(cam, args.seed, rays[0].data_ptr(), rays[1].data_ptr())), 48 * n)
    rec["none"] = none
    if has_source:
        into = lambda: ctx.camera_rays_device(cam, args.seed, out[0].data_ptr(), out[1].data_ptr())
        ctx.set_ray_source("rays", rays[0].view(spp, pixels, 3), rays[1].view(spp, pixels, 3))  # the camera's own rays, fed back
        rec["rays"] = {"camera_rays": with_rate(timed(into), 96 * n), "same_bits": bool((out[0] == rays[0]).all().item() and (out[1] == rays[1]).all().item()),
                       "render_light_groups": timed(walk)}
        rec["rays"]["beauty_mean"] = round(plane.mean().item(), 6)
        ctx.set_ray_source("rays", rays[0][:pixels].view(pixels, 3), rays[1][:pixels].view(pixels, 3), per_pixel=True)
        rec["rays_per_pixel"] = {"camera_rays": with_rate(timed(into), 48 * n + 48 * pixels)}
        ctx.set_ray_source("surface", aov["position"].view(pixels, 3), aov["normal"].view(pixels, 3))  # the AOV frame of the run above
        rec["surface"] = {"camera_rays": with_rate(timed(into), 48 * pixels + 48 * n), "gather_walk": timed(walk)}
        rec["surface"]["camera_rays"]["TB_s_read_per_sample"] = round(96 * n / (rec["surface"]["camera_rays"]["kernel_ms"] * 1e-3) / 1e12, 3)
        rec["surface"]["irradiance_mean"] = round(plane.mean().item() * 3.141592653589793, 6)
        ctx.clear_ray_source()
        rec["gather_over_render_lens"] = round(rec["surface"]["gather_walk"]["kernel_ms"] / none["render_light_groups"]["kernel_ms"], 3)
    print(json.dumps(rec), flush=True)
    ctx.close()
    img.close()


if __name__ == "__main__":
    main()
