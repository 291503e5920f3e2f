#!/usr/bin/env python3
"""The path classes (mcrt_render_path_classes_device) on one scene, next to the light groups with the same number of planes and a
path-traced render, all of the same camera, seed and sample count on the same build and in the same process: every plane's sum as a share
of the beauty frame, the sum of the planes against that frame, and the three times, HIP-event milliseconds from mcrt_stats: one warm-up,
then the median of --runs runs with their spread.

  python tools/path_classes_probe.py [--scene hexagon_room] [--width 1920 --height 1080 --sqrtspp 4] [--merge all|lobes|one]
                                     [--depth D] [--runs 5] [--no-render] [--no-light-groups] [--chunk-rays N]

The light groups are the yardstick: the same walk, the same work per live sample, one word of state less. They run with every emitter in
group 0 and as many (empty) groups as give the same number of planes, so both passes clear, carry and resolve the same radiances.
--merge one puts every class into plane 0: the pass is then the path tracer scheduled another way, and the probe says whether plane 0 is
the render's frame bit for bit. Prints one JSON line. After the timed runs one more run is made with option MCRT_PATH_CLASSES_LOG, whose
per-chunk lines (stderr of the library, captured here) give the live-sample curve; that run is not timed."""
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
    """Runs call() with the process's stderr (file descriptor 2: the library writes there) into a file; -> the JSON lines it wrote."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        lines = tmp.read().decode(errors="replace").splitlines()
    return [json.loads(l) for l in lines if l.startswith('{"path_classes_chunk"')]


def timed(call, runs):
    """One warm-up (scratch is allocated there), then `runs` runs: -> (stats of the first timed run, the runs' kernel_ms, their median)."""
    call()
    stats = [call() for _ in range(max(runs, 1))]
    ms = [s["kernel_ms"] for s in stats]
    return stats[0], ms, statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sqrtspp", type=int, default=4)
    ap.add_argument("--merge", default="all", choices=("all", "lobes", "one"))
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--no-light-groups", action="store_true")
    ap.add_argument("--chunk-rays", type=int, default=0, help="option MCRT_AOV_CHUNK_RAYS: shadow and bounce slots of iteration 0 per chunk (0: the default)")
    args = ap.parse_args()
    import torch
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", args.scene + ".mcrt"))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = args.width, args.height, args.sqrtspp
    cam.shard_index, cam.shard_count = 0, 1
    class_plane, names = m.path_class_map(args.merge)
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    if args.chunk_rays:
        ctx.set_option("MCRT_AOV_CHUNK_RAYS", args.chunk_rays)
    planes = torch.empty((len(names), cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()

    def run():
        return ctx.render_path_classes_device(cam, args.seed, planes.data_ptr(), class_plane=class_plane, max_depth=args.depth)
    first, ms, med = timed(run, args.runs)
    sums = {k: planes[i].sum().item() for i, k in enumerate(names)}
    whole = sum(sums.values())
    rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "spp": cam.sqrtspp ** 2, "planes": names, "max_depth": args.depth,
           "traced": first["rays"], "paths": first["paths"], "rays_per_path": round(first["rays"] / first["paths"], 3), "launches": first["kernel_launches"],
           "chunk_rays": args.chunk_rays or None, "kernel_ms": round(med, 3), "kernel_ms_runs": [round(x, 3) for x in ms], "spread": round((max(ms) - min(ms)) / med, 4),
           "Mray_s": round(first["rays"] / med / 1e3, 1), "share_of_the_planes_sum": {k: round(v / whole, 6) if whole else 0.0 for k, v in sums.items()}}
    ctx.set_option("MCRT_PATH_CLASSES_LOG", 1)
    chunks = logged_run(run)
    ctx.set_option("MCRT_PATH_CLASSES_LOG", None)
    if chunks:
        longest = max(chunks, key=lambda c: len(c["live"]))
        rec["chunks"] = len(chunks)
        rec["iterations"] = [len(c["live"]) for c in chunks] if len(chunks) <= 8 else {"min": min(len(c["live"]) for c in chunks), "max": len(longest["live"])}
        rec["live_curve"] = [round(v / longest["samples"], 4) for v in longest["live"]]  # of the chunk with the most iterations, per sample
        rec["search_share_of_host_clock"] = round(sum(c["search_ms"] for c in chunks) / sum(c["chunk_ms"] for c in chunks), 4)
    total = planes.sum(dim=0)
    if not args.no_light_groups:
        p = len(names)
        kw = dict(groups=None, num_groups=1, sky_plane=0) if p == 1 else dict(groups=None, num_groups=p - 1, sky_plane=None)
        other = torch.empty((p, cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        gfirst, gms, gmed = timed(lambda: ctx.render_light_groups_device(cam, args.seed, other.data_ptr(), max_depth=args.depth, **kw), args.runs)
        rec["light_groups"] = {"planes": p, "kernel_ms": round(gmed, 3), "kernel_ms_runs": [round(x, 3) for x in gms], "spread": round((max(gms) - min(gms)) / gmed, 4),
                               "rays": gfirst["rays"], "launches": gfirst["kernel_launches"]}
        rec["pass_over_light_groups"] = round(med / gmed, 4)
        rec["rays_equal_light_groups"] = bool(gfirst["rays"] == first["rays"])
        if p == 1:
            rec["one_plane_is_the_light_groups_bit_for_bit"] = bool(torch.equal(total.view(torch.int64), other[0].view(torch.int64)))
        del other
    if not args.no_render:
        rgb = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        render = []
        for _ in range(max(args.runs, 1) + 1):
            ctx.render_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr())
            render.append(ctx.render_finish())
        rms = [r["kernel_ms"] for r in render[1:]]
        rmed = statistics.median(rms)
        rel = ((total - rgb).abs() / rgb.abs().clamp_min(1e-300)).nan_to_num(0.0)
        beauty = rgb.sum().item()
        rec["render"] = {"kernel_id": render[-1]["kernel_id"], "kernel_ms": round(rmed, 3), "kernel_ms_runs": [round(x, 3) for x in rms],
                         "spread": round((max(rms) - min(rms)) / rmed, 4), "rays": render[-1]["rays"], "rays_per_path": round(render[-1]["rays"] / render[-1]["paths"], 3),
                         "mean": round(rgb.mean().item(), 6)}
        rec["share_of_the_frame"] = {k: round(v / beauty, 6) for k, v in sums.items()}
        rec["planes_sum_over_beauty"] = round(whole / beauty, 9)
        rec["planes_sum_max_rel_error"] = float("%.3e" % rel.max().item())
        rec["planes_sum_is_beauty_bit_for_bit"] = bool(torch.equal(total.view(torch.int64), rgb.view(torch.int64)))
        rec["rays_over_render"] = round(first["rays"] / render[-1]["rays"], 4)
        rec["pass_over_render"] = round(med / rmed, 4)
    print(json.dumps(rec), flush=True)
    ctx.close()
    img.close()


if __name__ == "__main__":
    main()
