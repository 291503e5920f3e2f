#!/usr/bin/env python3
"""The denoise filters (mcrt_denoise_device, the variance-guided mcrt_denoise_variance_device and the dual-buffer mcrt_denoise_dual_device) measured on the same frames in one
session: their time next to the beauty frame and the AOV pass of the same camera, and what they do to the error of a low-sample frame.

  python tools/denoise_probe.py [--width 1920 --height 1080 --sqrtspp 4] [--runs 5] [--scenes hexagon_room]
      Time: HIP-event milliseconds from mcrt_stats, one warm-up, then the median of --runs runs, for 1 .. iterations iterations in the
      tile form, the plain form and the default choice; "step_ms" are the differences (the first includes the prep pass, the default
      count's last one the remodulation); "variance_tile" / "variance_plain" / "variance_default" are the guided filter's. One JSON line
      per scene.

  python tools/denoise_probe.py --errors [--width 192 --height 108] [--truth-sqrtspp 32] [--scenes a,b,...] [--grid]
      Error: per scene and sqrtspp 1, 2, 4 the mean squared error (all channels, pixels with coverage > 0) of the unfiltered and of the
      filtered frame (default parameters) against a render at --truth-sqrtspp with another seed. The guided filter (default parameters) runs on the same frame with the variance of
      render_pixel_stats: "mse_variance_guided", and "calibration" = the mean over those pixels of g(out_variance) / spp over the mean of
      the filtered frame's squared error (channels added). --grid adds a small grid of parameters for each filter ("grid", "variance_grid":
      [sigma_variance, sigma_floor, ratio]). One JSON line per (scene, sqrtspp).

  python tools/denoise_probe.py --dual [--width 1920 --height 1080 --sqrtspp 4] [--runs 5] [--scenes hexagon_room] [--radii 5,2:8,3]
      The dual-buffer filter (mcrt_denoise_dual_device) on the half-buffers of one render: HIP-event milliseconds (one warm-up, then the
      median of --runs runs) of the tile form, the plain form (--plain-runs of it, default 1: it is slow on purpose) and the default choice
      per (window_radius, patch_radius) of --radii ("0,0" = the defaults), and the variance-guided filter's at its defaults on the same
      frame in the same session as the yardstick. One JSON line per scene.

  python tools/denoise_probe.py --dual --errors [--width 192 --height 108] [--truth-sqrtspp 32] [--scenes a,b,...] [--grid]
      Per scene and sqrtspp 2, 4: the mean squared error (all channels, pixels with coverage > 0) of the unfiltered frame and of the frames
      filtered by mcrt_denoise_dual, mcrt_denoise_variance and mcrt_denoise (default parameters) against a render at --truth-sqrtspp with
      another seed, and "calibration" / "calibration_variance_guided" = the mean of g(variance) / spp over the mean of the filtered
      frame's squared error (channels added) for the two filters that estimate their error. --grid adds "dual_grid":
      [window_radius, patch_radius, k, ratio, calibration]. One JSON line per (scene, sqrtspp)."""
import argparse
import importlib
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

GUIDES = ("shading_normal", "normal", "position", "coverage", "albedo")
VARIANCE_GRID = dict(sigma_variance=(2.0, 3.0, 4.0, 6.0), sigma_floor=(0.02, 0.05, 0.1))
GRID = dict(iterations=(3, 5), sigma_color=(1.0, 2.0, 4.0), sigma_plane=(0.1, 0.3), normal_power_log2=(5, 7))


def setup(m, name, width, height, sqrtspp):
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", name + ".mcrt"))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = width, height, sqrtspp
    cam.shard_index, cam.shard_count = 0, 1
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    return img, cam, ctx


def timing(m, args):
    import torch
    for name in args.scenes.split(","):
        img, cam, ctx = setup(m, name, args.width, args.height, args.sqrtspp)
        bufs = {k: torch.empty((cam.height, cam.width) + ((3,) if m.AOV_CHANNELS[k][1] == 3 else ()), dtype=torch.float64, device="cuda:0") for k in GUIDES}
        rgb = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
        out, var, out_var = torch.empty_like(rgb), torch.empty_like(rgb), torch.empty_like(rgb)
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        ctx.render_pixel_stats_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr(), {"variance": var.data_ptr()})
        for _ in range(2):  # warm-up, then the ones that count
            aov = ctx.render_aov_device(cam, args.seed, ptrs)
            ctx.render_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr())
            beauty = ctx.render_finish()
        rec = {"scene": name, "width": cam.width, "height": cam.height, "spp": cam.sqrtspp ** 2, "beauty_ms": round(beauty["kernel_ms"], 3),
               "aov_ms": round(aov["kernel_ms"], 3), "pixels": cam.width * cam.height}
        for form in ("tile", "plain", None):
            ctx.set_option("MCRT_DENOISE_FORM", form)
            total = []
            for n in range(1, args.iterations + 1):
                ctx.denoise_device(cam.width, cam.height, rgb.data_ptr(), ptrs, out.data_ptr(), iterations=n)
                runs = [ctx.denoise_device(cam.width, cam.height, rgb.data_ptr(), ptrs, out.data_ptr(), iterations=n)["kernel_ms"] for _ in range(max(args.runs, 1))]
                total.append(statistics.median(runs))
            rec[form or "default"] = {"total_ms": [round(t, 4) for t in total], "step_ms": [round(b - a, 4) for a, b in zip([0.0] + total, total)]}
        ctx.set_option("MCRT_DENOISE_FORM", None)
        guided = lambda n: ctx.denoise_variance_device(cam.width, cam.height, cam.sqrtspp ** 2, rgb.data_ptr(), var.data_ptr(), ptrs, out.data_ptr(),
                                                       out_var.data_ptr(), iterations=n)["kernel_ms"]
        for form in ("tile", "plain", None):
            ctx.set_option("MCRT_DENOISE_VAR_FORM", form)
            total = []
            for n in range(1, args.iterations + 1):
                guided(n)
                total.append(statistics.median([guided(n) for _ in range(max(args.runs, 1))]))
            rec["variance_" + (form or "default")] = {"total_ms": [round(t, 4) for t in total], "step_ms": [round(b - a, 4) for a, b in zip([0.0] + total, total)]}
        print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


def errors(m, args):
    import numpy as np
    combos = [dict(zip(GRID, v)) for v in itertools.product(*GRID.values())] if args.grid else []
    vcombos = [dict(zip(VARIANCE_GRID, v)) for v in itertools.product(*VARIANCE_GRID.values())] if args.grid else []
    for name in args.scenes.split(","):
        img, cam, ctx = setup(m, name, args.width, args.height, args.truth_sqrtspp)
        truth, _ = ctx.sample_image(cam, args.seed ^ 0x00ABCDEF, m.INTEGRATOR_PATH_TRACER)
        for sqrtspp in (1, 2, 4):
            cam.sqrtspp = sqrtspp
            stats = ctx.render_pixel_stats(cam, args.seed, m.INTEGRATOR_PATH_TRACER, channels=("variance",))
            noisy, variance, spp = stats["rgb"], stats["variance"], sqrtspp ** 2
            guides = ctx.render_aov(cam, args.seed, channels=GUIDES)
            covered = guides["coverage"] > 0
            mse = lambda frame: float(((frame - truth)[covered] ** 2).mean())
            before, after = mse(noisy), mse(ctx.denoise(noisy, guides))
            rec = {"scene": name, "width": cam.width, "height": cam.height, "spp": sqrtspp ** 2, "truth_spp": args.truth_sqrtspp ** 2,
                   "mse_unfiltered": before, "mse_filtered": after, "ratio": round(after / before, 4)}
            guided, guided_var = ctx.denoise_variance(noisy, variance, guides, spp)
            rec["mse_variance_guided"] = mse(guided)
            rec["ratio_variance_guided"] = round(rec["mse_variance_guided"] / before, 4)
            estimate = float((guided_var[covered].sum(axis=-1) / spp).mean())
            rec["calibration"] = round(estimate / float((((guided - truth)[covered]) ** 2).sum(axis=-1).mean()), 4)
            if combos:
                rec["grid"] = [[c["iterations"], c["sigma_color"], c["sigma_plane"], c["normal_power_log2"], round(mse(ctx.denoise(noisy, guides, **c)) / before, 4)]
                               for c in combos]
                rec["variance_grid"] = [[c["sigma_variance"], c["sigma_floor"],
                                         round(mse(ctx.denoise_variance(noisy, variance, guides, spp, want_variance=False, **c)[0]) / before, 4)] for c in vcombos]
            print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


DUAL_GRID = dict(radii=((3, 1), (5, 2), (8, 3)), k=(0.3, 0.45, 0.6, 0.8, 1.0))


def dual_timing(m, args):
    import torch
    radii = [tuple(int(x) for x in r.split(",")) for r in args.radii.split(":")]
    for name in args.scenes.split(","):
        img, cam, ctx = setup(m, name, args.width, args.height, args.sqrtspp)
        spp = cam.sqrtspp ** 2
        frame = lambda: torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
        rgb, var, half_a, half_b, out, out_var = (frame() for _ in range(6))
        bufs = {k: torch.empty((cam.height, cam.width) + ((3,) if m.AOV_CHANNELS[k][1] == 3 else ()), dtype=torch.float64, device="cuda:0") for k in GUIDES}
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        ctx.render_pixel_stats_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr(), {"variance": var.data_ptr(), "half_a": half_a.data_ptr(), "half_b": half_b.data_ptr()})
        ctx.render_aov_device(cam, args.seed, ptrs)
        rec = {"scene": name, "width": cam.width, "height": cam.height, "spp": spp, "pixels": cam.width * cam.height}
        dual = lambda R, F: ctx.denoise_dual_device(cam.width, cam.height, spp, half_a.data_ptr(), half_b.data_ptr(), var.data_ptr(),
                                                    {"rgb": out.data_ptr(), "variance": out_var.data_ptr()}, window_radius=R, patch_radius=F)["kernel_ms"]
        for R, F in radii:
            for lanes in (256, 512, 1024):  # the tile form's workgroup
                ctx.set_option("MCRT_DENOISE_DUAL_FORM", "tile")
                ctx.set_option("MCRT_DENOISE_DUAL_LANES", str(lanes))
                dual(R, F)
                rec["dual_%d_%d_tile_%d" % (R, F, lanes)] = round(statistics.median([dual(R, F) for _ in range(max(args.runs, 1))]), 4)
            ctx.set_option("MCRT_DENOISE_DUAL_LANES", None)
            for form in ("tile", "plain", None):
                ctx.set_option("MCRT_DENOISE_DUAL_FORM", form)
                if form != "plain":
                    dual(R, F)  # warm-up
                runs = [dual(R, F) for _ in range(max(args.plain_runs if form == "plain" else args.runs, 1))]
                rec["dual_%d_%d_%s" % (R, F, form or "default")] = round(statistics.median(runs), 4)
        ctx.set_option("MCRT_DENOISE_DUAL_FORM", None)
        guided = lambda: ctx.denoise_variance_device(cam.width, cam.height, spp, rgb.data_ptr(), var.data_ptr(), ptrs, out.data_ptr(), out_var.data_ptr())["kernel_ms"]
        guided()
        rec["variance_guided_default"] = round(statistics.median([guided() for _ in range(max(args.runs, 1))]), 4)
        print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


def dual_errors(m, args):
    import numpy as np
    for name in args.scenes.split(","):
        img, cam, ctx = setup(m, name, args.width, args.height, args.truth_sqrtspp)
        truth, _ = ctx.sample_image(cam, args.seed ^ 0x00ABCDEF, m.INTEGRATOR_PATH_TRACER)
        for sqrtspp in (2, 4):
            cam.sqrtspp = sqrtspp
            raw, spp = ctx.render_pixel_stats(cam, args.seed, m.INTEGRATOR_PATH_TRACER), sqrtspp ** 2
            guides = ctx.render_aov(cam, args.seed, channels=GUIDES)
            covered = guides["coverage"] > 0
            mse = lambda frame: float(((frame - truth)[covered] ** 2).mean())
            calibration = lambda frame, variance: float((variance[covered].sum(axis=-1) / spp).mean()) / float((((frame - truth)[covered]) ** 2).sum(axis=-1).mean())
            before = mse(raw["rgb"])
            dual = ctx.denoise_dual(raw["half_a"], raw["half_b"], raw["variance"], spp)
            guided, guided_var = ctx.denoise_variance(raw["rgb"], raw["variance"], guides, spp)
            rec = {"scene": name, "width": cam.width, "height": cam.height, "spp": spp, "truth_spp": args.truth_sqrtspp ** 2, "mse_unfiltered": before,
                   "ratio_dual": round(mse(dual["rgb"]) / before, 4), "ratio_variance_guided": round(mse(guided) / before, 4),
                   "ratio_denoise": round(mse(ctx.denoise(raw["rgb"], guides)) / before, 4),
                   "calibration": round(calibration(dual["rgb"], dual["variance"]), 4), "calibration_variance_guided": round(calibration(guided, guided_var), 4)}
            if args.grid:
                rec["dual_grid"] = []
                for (R, F), k in itertools.product(DUAL_GRID["radii"], DUAL_GRID["k"]):
                    d = ctx.denoise_dual(raw["half_a"], raw["half_b"], raw["variance"], spp, window_radius=R, patch_radius=F, k=k)
                    rec["dual_grid"].append([R, F, k, round(mse(d["rgb"]) / before, 4), round(calibration(d["rgb"], d["variance"]), 4)])
            print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--dual", action="store_true")
    ap.add_argument("--radii", default="0,0:8,3")
    ap.add_argument("--plain-runs", type=int, default=1)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--sqrtspp", type=int, default=4)
    ap.add_argument("--truth-sqrtspp", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--scenes")
    args = ap.parse_args()
    args.width = args.width or (192 if args.errors else 1920)
    args.height = args.height or (108 if args.errors else 1080)
    args.scenes = args.scenes or ("hexagon_room_diffuse,hexagon_room,hexagon_room_ggx,coffee_maker_qsah" if args.errors else "hexagon_room")
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    if args.dual:
        (dual_errors if args.errors else dual_timing)(m, args)
    else:
        (errors if args.errors else timing)(m, args)


if __name__ == "__main__":
    main()
