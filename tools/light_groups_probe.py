#!/usr/bin/env python3
"""The light groups (mcrt_render_light_groups_device) on one scene, next to a path-traced render of the same camera, seed and sample
count on the same build: the rays traced, the iterations and the live samples of every iteration, the sum of the planes against the
beauty frame, and the pass's time beside the render's, both HIP-event milliseconds from mcrt_stats: one warm-up, then the median of
--runs runs with their spread.

  python tools/light_groups_probe.py [--scene hexagon_room] [--width 1920 --height 1080 --sqrtspp 4] [--by material|light|one]
                                     [--one-plane] [--depth D] [--runs 5] [--no-render] [--chunk-rays N]

--one-plane puts every emitter and the sky into plane 0: the pass is then the path tracer scheduled another way, and the probe says
whether plane 0 is the render's frame bit for bit. Prints one JSON line. After the timed runs one more run is made with option
MCRT_LIGHT_GROUPS_LOG, whose per-chunk lines (stderr of the library, captured here) give the live-sample curve and the share of the host
clock spent in the closest-hit searches; that run is not timed."""
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
    return [json.loads(l) for l in lines if l.startswith('{"light_groups_chunk"')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sqrtspp", type=int, default=4)
    ap.add_argument("--by", default="light", choices=("material", "light", "one"))
    ap.add_argument("--one-plane", action="store_true")
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--chunk-rays", type=int, default=0, help="option MCRT_AOV_CHUNK_RAYS: shadow and bounce slots of iteration 0 per chunk (0: the default)")
    args = ap.parse_args()
    import torch
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", args.scene + ".mcrt"))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = args.width, args.height, args.sqrtspp
    cam.shard_index, cam.shard_count = 0, 1
    if args.one_plane:
        kw, names = dict(groups=None, num_groups=1, sky_plane=0), ["all"]
    else:
        groups, names = m.light_group_map(img.scene, by=args.by)
        kw = dict(groups=groups, num_groups=len(names) - 1, sky_plane=None)
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    if args.chunk_rays:
        ctx.set_option("MCRT_AOV_CHUNK_RAYS", args.chunk_rays)
    planes = torch.empty((len(names), cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()

    def run():
        return ctx.render_light_groups_device(cam, args.seed, planes.data_ptr(), max_depth=args.depth, **kw)
    run()  # warm-up (scratch allocated here)
    runs = [run() for _ in range(max(args.runs, 1))]
    ms = [r["kernel_ms"] for r in runs]
    med = statistics.median(ms)
    rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "spp": cam.sqrtspp ** 2, "planes": names, "max_depth": args.depth,
           "traced": runs[0]["rays"], "paths": runs[0]["paths"], "rays_per_path": round(runs[0]["rays"] / runs[0]["paths"], 3), "launches": runs[0]["kernel_launches"],
           "chunk_rays": args.chunk_rays or None, "kernel_ms": round(med, 3), "kernel_ms_runs": [round(x, 3) for x in ms], "spread": round((max(ms) - min(ms)) / med, 4),
           "Mray_s": round(runs[0]["rays"] / med / 1e3, 1), "mean": {k: round(planes[i].mean().item(), 6) for i, k in enumerate(names)}}
    ctx.set_option("MCRT_LIGHT_GROUPS_LOG", 1)
    chunks = logged_run(run)
    ctx.set_option("MCRT_LIGHT_GROUPS_LOG", None)
    if chunks:
        longest = max(chunks, key=lambda c: len(c["live"]))
        rec["chunks"] = len(chunks)
        rec["iterations"] = [len(c["live"]) for c in chunks] if len(chunks) <= 8 else {"min": min(len(c["live"]) for c in chunks), "max": len(longest["live"])}
        rec["live_curve"] = [round(v / longest["samples"], 4) for v in longest["live"]]  # of the chunk with the most iterations, per sample
        rec["search_share_of_host_clock"] = round(sum(c["search_ms"] for c in chunks) / sum(c["chunk_ms"] for c in chunks), 4)
    if not args.no_render:
        rgb = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        render = []
        for _ in range(max(args.runs, 1) + 1):
            ctx.render_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr())
            render.append(ctx.render_finish())
        rms = [r["kernel_ms"] for r in render[1:]]
        rmed = statistics.median(rms)
        total = planes.sum(dim=0)
        rel = ((total - rgb).abs() / rgb.abs().clamp_min(1e-300)).nan_to_num(0.0)
        rec["render"] = {"kernel_id": render[-1]["kernel_id"], "kernel_ms": round(rmed, 3), "kernel_ms_runs": [round(x, 3) for x in rms],
                         "spread": round((max(rms) - min(rms)) / rmed, 4), "rays": render[-1]["rays"], "rays_per_path": round(render[-1]["rays"] / render[-1]["paths"], 3),
                         "mean": round(rgb.mean().item(), 6)}
        rec["planes_sum_over_beauty"] = round(total.mean().item() / rgb.mean().item(), 9)
        rec["planes_sum_max_rel_error"] = float("%.3e" % rel.max().item())
        rec["planes_sum_is_beauty_bit_for_bit"] = bool(torch.equal(total.view(torch.int64), rgb.view(torch.int64)))
        rec["rays_over_render"] = round(runs[0]["rays"] / render[-1]["rays"], 4)
        rec["pass_over_render"] = round(med / rmed, 4)
    print(json.dumps(rec), flush=True)
    ctx.close()
    img.close()


if __name__ == "__main__":
    main()
