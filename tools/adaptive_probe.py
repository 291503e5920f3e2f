#!/usr/bin/env python3
"""Adaptive sampling (mcrt_render_adaptive_device) on one scene: the schedule - the pixels listed for every batch, the histogram of the
sample counts - and the measurements profiles/NOTES_adaptive.md records, all in one process and one context.

  python tools/adaptive_probe.py [--scene hexagon_room] [--width 1920 --height 1080 --sqrtspp 4] --target T [--max-spp N] [--window R]
                                 [--floor F] [--runs 3] [--reference-spp 4096] [--no-gain] [--chunk-rays N]

schedule      one run with option MCRT_ADAPTIVE_LOG, whose per-batch lines (stderr of the library, captured here) give the list's length, the
              form of the batch (render: mcrt_render_pixel_stats_device and a merge; walk: the path walk over the list) and the host-clock
              milliseconds of the rule with the list (criterion, count, scan, the read-back of the length, scatter) and of the batch.
              A second such run with MCRT_ADAPTIVE_FULL_BATCH=walk gives the walk's time at 100 % of the frame.
times         one warm-up, then --runs runs of the adaptive call and of mcrt_render_converged_device (path tracer, no target) at the same
              total number of samples - result.samples / pixels rounded to a batch -: the median of total_ms and of kernel_ms.
gain          both frames against a reference of another seed at --reference-spp samples a pixel (mcrt_render_converged_device, batches
              of 256) with mcrt_frame_compare: MSE and relMSE.
overhead      the rule with the list per batch against one full batch of mcrt_render_pixel_stats_device.
Prints one JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def logged_run(call):
    """Runs call() with the process's stderr (file descriptor 2: the library writes there) into a file; -> (its result, the JSON lines)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        lines = tmp.read().decode(errors="replace").splitlines()
    return out, [json.loads(l) for l in lines if l.startswith('{"adaptive_batch"')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sqrtspp", type=int, default=4)
    ap.add_argument("--target", type=float, required=True)
    ap.add_argument("--max-spp", type=int, default=0)
    ap.add_argument("--window", type=int, default=None)
    ap.add_argument("--floor", type=float, default=0.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--no-gain", action="store_true")
    ap.add_argument("--chunk-rays", type=int, default=0, help="option MCRT_AOV_CHUNK_RAYS (0: the default)")
    args = ap.parse_args()
    import torch
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", args.scene + ".mcrt"))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = args.width, args.height, args.sqrtspp
    cam.shard_index, cam.shard_count = 0, 1
    pixels, n = cam.width * cam.height, args.sqrtspp ** 2
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    if args.chunk_rays:
        ctx.set_option("MCRT_AOV_CHUNK_RAYS", args.chunk_rays)
    dev = "cuda:0"
    frame = lambda: torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device=dev)
    rgb, variance, count = frame(), frame(), torch.empty((cam.height, cam.width), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    kw = dict(max_spp=args.max_spp, floor=args.floor, window=args.window)

    def run():
        return ctx.render_adaptive_device(cam, args.seed, rgb.data_ptr(), args.target, stats_pointers={"variance": variance.data_ptr()}, count_ptr=count.data_ptr(), **kw)

    run()  # warm-up: scratch is allocated here
    timed = [run() for _ in range(max(args.runs, 1))]
    result = timed[0][0]
    med = lambda key: round(statistics.median(s[key] for _, s in timed), 3)
    values, numbers = torch.unique(count, return_counts=True)
    rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "batch": n, "target": args.target, "max_spp": args.max_spp or max(1024, n),
           "window": 1 if args.window is None else args.window, "batches": result["batches"], "samples": result["samples"], "mean_spp": round(result["samples"] / pixels, 3),
           "min_count": result["min_count"], "max_count": result["max_count"], "active": result["active"],
           "active_fraction": [round(a / pixels, 5) for a in result["active"]], "count_histogram": {int(v): int(c) for v, c in zip(values.tolist(), numbers.tolist())},
           "adaptive": {"total_ms": med("total_ms"), "kernel_ms": med("kernel_ms"), "total_ms_runs": [round(s["total_ms"], 3) for _, s in timed], "rays": timed[0][1]["rays"],
                        "launches": timed[0][1]["kernel_launches"]}}
    ctx.set_option("MCRT_ADAPTIVE_LOG", 1)
    _, lines = logged_run(run)
    rec["batches_logged"] = [{"listed": l["listed"], "fraction": round(l["listed"] / pixels, 5), "form": l["form"], "list_ms": l["list_ms"], "batch_ms": l["batch_ms"]} for l in lines]
    ctx.set_option("MCRT_ADAPTIVE_FULL_BATCH", "walk")
    run()
    _, lines = logged_run(run)
    ctx.set_option("MCRT_ADAPTIVE_FULL_BATCH", None)
    ctx.set_option("MCRT_ADAPTIVE_LOG", None)
    rec["walk_batches_logged"] = [{"listed": l["listed"], "fraction": round(l["listed"] / pixels, 5), "form": l["form"], "batch_ms": l["batch_ms"]} for l in lines]

    # one full batch of the statistics render: the yardstick of the per-batch overhead
    batch = []
    for _ in range(max(args.runs, 1) + 1):
        batch.append(ctx.render_pixel_stats_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr(), pointers={"variance": variance.data_ptr()}))
    full_ms = statistics.median(s["kernel_ms"] for s in batch[1:])
    list_ms = [l["list_ms"] for l in rec["batches_logged"]]
    rec["overhead"] = {"full_batch_kernel_ms": round(full_ms, 3), "list_ms_median": round(statistics.median(list_ms), 3), "list_ms_max": round(max(list_ms), 3),
                       "share_of_a_full_batch": round(statistics.median(list_ms) / full_ms, 4)}

    # the converged render at the same total number of samples
    equal_spp = max(n, int(round(result["samples"] / pixels / n)) * n)
    other, other_var = frame(), frame()
    torch.cuda.synchronize()

    def uniform():
        return ctx.render_converged_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, other.data_ptr(), 0.0, max_spp=equal_spp, stats_pointers={"variance": other_var.data_ptr()})
    uniform()
    utimed = [uniform() for _ in range(max(args.runs, 1))]
    rec["converged"] = {"spp": equal_spp, "total_ms": round(statistics.median(s["total_ms"] for _, s in utimed), 3),
                        "kernel_ms": round(statistics.median(s["kernel_ms"] for _, s in utimed), 3), "rays": utimed[0][1]["rays"]}
    rec["adaptive_over_converged_total_ms"] = round(rec["adaptive"]["total_ms"] / rec["converged"]["total_ms"], 4)
    run()  # (rgb holds the adaptive frame again)
    if not args.no_gain:
        ref_cam = img.camera
        ref_cam.width, ref_cam.height, ref_cam.sqrtspp = cam.width, cam.height, 16
        ref_cam.shard_index, ref_cam.shard_count = 0, 1
        ref = frame()
        torch.cuda.synchronize()
        ref_result, ref_stats = ctx.render_converged_device(ref_cam, args.seed + 0x1000, m.INTEGRATOR_PATH_TRACER, ref.data_ptr(), 0.0, max_spp=max(args.reference_spp, 256))
        errors = {}
        for name, f in (("adaptive", rgb), ("converged", other)):
            r = ctx.frame_compare(f, ref, ssim=False)
            errors[name] = {"mse": r["mse"], "relmse": r["relmse"], "nonfinite": r["nonfinite"]}
        rec["reference"] = {"spp": ref_result["spp"], "seed": args.seed + 0x1000, "total_ms": round(ref_stats["total_ms"], 1)}
        rec["errors"] = errors
        rec["adaptive_over_converged_mse"] = round(errors["adaptive"]["mse"] / errors["converged"]["mse"], 4) if errors["converged"]["mse"] else None
        rec["adaptive_over_converged_relmse"] = round(errors["adaptive"]["relmse"] / errors["converged"]["relmse"], 4) if errors["converged"]["relmse"] else None
    print(json.dumps(rec), flush=True)
    ctx.close()
    img.close()


if __name__ == "__main__":
    main()
