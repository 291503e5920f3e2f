#!/usr/bin/env python3
"""Accumulated rendering (mcrt_frame_merge*, mcrt_render_converged*) measured: what a merge costs next to the batch it follows and next
to the statistics kernel of the same frame, and what merging batches costs in error against one render of as many samples.

  python tools/accumulate_probe.py [--width 1920 --height 1080 --sqrtspp 4] [--runs 5] [--scene hexagon_room]
      Kernel: frame_merge_device on summaries of the frame's size (random contents, merged into buffers of their own),
      mcrt_stats.kernel_ms (HIP events around the launch), one warm-up, the median (and the smallest and largest) of --runs runs, for
      every group (600 bytes per pixel: two summaries of 25 doubles read, one written) and for {rgb, variance} alone (144 bytes);
      bytes per second and the share of --peak-TBps (6.3, the achievable HBM rate); next to pixelStatsKernel with all three channels on
      a store of sqrtspp^2 planes of the same frame, in the same session, interleaved.
      Call: one batch (render_highlights_device with every channel) beside the merge that follows it, and render_converged_device
      for four batches, wall clock and kernel_ms. One JSON line.

  python tools/accumulate_probe.py --errors [--width 192 --height 108] [--batches 4 --sqrtspp 4] [--truth-sqrtspp 64] [--seeds 8]
                                   [--seed N --truth-seed M] [--scenes a,b] [--oracle]
      Per scene: the summed squared error of --batches batches of sqrtspp^2 samples merged (seeds s, s + 1, ...: what
      render_converged accumulates) beside ONE render of as many samples (sqrtspp x sqrt(batches), seed s), both against a render at
      --truth-sqrtspp with seed --truth-seed; --seeds such pairs (s = --seed, + 16, ...), each ratio and the ratio of the sums. The price of giving up the
      stratification across batches. --oracle: every frame from the CPU oracle (the GPU's bits; no GPU needed). One JSON line each."""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


class PixelStatsPass(C.Structure):  # csrc/mcrt_pixel_stats.hpp
    _fields_ = [("samples", C.c_void_p), ("words", C.c_uint64), ("spp", C.c_uint32), ("vec", C.c_uint32), ("variance", C.c_void_p),
                ("half_a", C.c_void_p), ("half_b", C.c_void_p)]


def setup(m, name, width, height, sqrtspp, upload=True):
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", name + ".mcrt"))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = width, height, sqrtspp
    cam.shard_index, cam.shard_count = 0, 1
    ctx = None
    if upload:
        ctx = m.Context(0)
        ctx.upload_scene(img.scene)
    return img, cam, ctx


def spread(values):
    return [round(statistics.median(values), 4), round(min(values), 4), round(max(values), 4)]


def timing(m, args):
    import torch
    m.lib()
    twin = C.CDLL(os.path.join(os.path.dirname(m.LIB_PATH), "libmcrt_pixel_stats.so"))
    launch_stats = twin._ZN4mcrt16launchPixelStatsEPvRKNS_14PixelStatsPassE  # mcrt::launchPixelStats(void* stream, const PixelStatsPass&)
    launch_stats.argtypes = [C.c_void_p, C.POINTER(PixelStatsPass)]
    launch_stats.restype = C.c_int
    sqrtspp = int(args.sqrtspp)
    img, cam, ctx = setup(m, args.scene, args.width, args.height, sqrtspp)
    spp, pixels = sqrtspp * sqrtspp, cam.width * cam.height
    rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "batch_spp": spp, "peak_TBps": args.peak_TBps}
    shapes = m.FRAME_SUMMARY_CHANNELS
    summary = lambda: {k: torch.rand((pixels,) + s, dtype=torch.float64, device="cuda:0") for k, s in shapes.items()}
    a, b, out = summary(), summary(), summary()
    ptr = lambda d, names=None: {k: v.data_ptr() for k, v in d.items() if names is None or k in names}
    store = torch.rand((spp, pixels, 3), dtype=torch.float64, device="cuda:0")
    ps = PixelStatsPass(store.data_ptr(), pixels * 3, spp, 1 if store.data_ptr() % 16 == 0 and (pixels * 3) % 2 == 0 else 0,
                        out["variance"].data_ptr(), out["half_a"].data_ptr(), out["half_b"].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def merge(names):
        return lambda: ctx.frame_merge_device(pixels, ptr(a), spp, ptr(b), spp, ptr(out, names))["kernel_ms"]

    def stats_kernel():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = launch_stats(stream, C.byref(ps))
        e1.record()
        e1.synchronize()
        assert rc == 0, rc
        return e0.elapsed_time(e1)
    cases = (("merge_all", 600, merge(None)), ("merge_mean_variance", 144, merge(("rgb", "variance"))), ("pixel_stats", (2 * spp + 3) * 24, stats_kernel))
    for rep in range(2):  # (twice each, interleaved: the spread between the repeats is what a difference is read against)
        for label, bytes_per_pixel, fn in cases:
            fn()
            ms = spread([fn() for _ in range(max(args.runs, 1))])
            rec["kernel_%s_ms_%d" % (label, rep)] = ms
            rec["kernel_%s_TBps_%d" % (label, rep)] = round(bytes_per_pixel * pixels / ms[0] / 1e9, 3)
            rec["kernel_%s_share_of_peak_%d" % (label, rep)] = round(bytes_per_pixel * pixels / ms[0] / 1e9 / args.peak_TBps, 3)
    del store
    torch.cuda.empty_cache()
    # a batch beside the merge that follows it
    hl, st_names = ("tops", "level"), ("variance", "half_a", "half_b")
    batch_ms, batch_wall, merge_ms, merge_wall = [], [], [], []
    for i in range(max(args.runs, 1) + 1):
        t0 = time.perf_counter()
        st = ctx.render_highlights_device(cam, args.seed + i, m.INTEGRATOR_PATH_TRACER, b["rgb"].data_ptr(), ptr(b, hl), ptr(b, st_names))
        t1 = time.perf_counter()
        sm = ctx.frame_merge_device(pixels, ptr(a), spp, ptr(b), spp, ptr(out))
        t2 = time.perf_counter()
        if i:  # (the first pair warms up)
            batch_ms.append(st["kernel_ms"]), batch_wall.append((t1 - t0) * 1e3), merge_ms.append(sm["kernel_ms"]), merge_wall.append((t2 - t1) * 1e3)
    rec["batch_kernel_ms"], rec["batch_wall_ms"] = spread(batch_ms)[0], spread(batch_wall)[0]
    rec["merge_kernel_ms"], rec["merge_wall_ms"] = spread(merge_ms)[0], spread(merge_wall)[0]
    rec["merge_over_batch_kernel"] = round(rec["merge_kernel_ms"] / rec["batch_kernel_ms"], 5)
    t0 = time.perf_counter()
    res, st = ctx.render_converged_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, out["rgb"].data_ptr(), 0.0, 4 * spp, stats_pointers=ptr(out, st_names),
                                          pointers=ptr(out, hl))
    rec["converged_4_batches_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    rec["converged_4_batches_kernel_ms"] = round(st["kernel_ms"], 3)
    rec["converged_relative_error"] = [round(e, 6) for e in res["relative_error"]]
    print(json.dumps(rec), flush=True)
    ctx.close()
    img.close()


def errors(m, args):
    import numpy as np
    sqrtspp, J = int(args.sqrtspp), args.batches
    whole = int(round(sqrtspp * math.sqrt(J)))
    assert whole * whole == sqrtspp * sqrtspp * J, "--batches times sqrtspp^2 must be a square"
    if args.oracle:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib
    for name in args.scenes.split(","):
        img, cam, ctx = setup(m, name, args.width, args.height, sqrtspp, upload=not args.oracle)

        def render(s, seed):
            cam.sqrtspp = s
            if args.oracle:
                return oracle_lib.render(img, cam, seed, m.INTEGRATOR_PATH_TRACER)[0]
            return ctx.sample_image(cam, seed, m.INTEGRATOR_PATH_TRACER)[0]
        truth = render(args.truth_sqrtspp, args.truth_seed)
        sq = lambda frame: float(((frame - truth) ** 2).sum())
        merged, one = [], []
        for r in range(args.seeds):
            seed = args.seed + 16 * r
            frames = [render(sqrtspp, seed + j) for j in range(J)]
            mean = frames[0]
            for j in range(1, J):  # (the merge's mean, batch after batch)
                mean = (float(j * sqrtspp * sqrtspp) * mean + float(sqrtspp * sqrtspp) * frames[j]) / float((j + 1) * sqrtspp * sqrtspp)
            merged.append(sq(mean))
            one.append(sq(render(whole, seed)))
        rec = {"scene": name, "width": cam.width, "height": cam.height, "batches": J, "batch_spp": sqrtspp * sqrtspp, "spp": whole * whole,
               "truth_spp": args.truth_sqrtspp ** 2, "frames_from": "oracle" if args.oracle else "gpu", "seeds": args.seeds,
               "squared_error_merged": [round(x, 6) for x in merged], "squared_error_one_render": [round(x, 6) for x in one],
               "ratios": [round(x / y, 4) for x, y in zip(merged, one)], "ratio_of_sums": round(sum(merged) / sum(one), 4)}
        print(json.dumps(rec), flush=True)
        if ctx:
            ctx.close()
        img.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--sqrtspp", default="4")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--truth-sqrtspp", type=int, default=64)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=lambda v: int(v, 0))
    ap.add_argument("--truth-seed", type=lambda v: int(v, 0), default=12345)
    ap.add_argument("--peak-TBps", dest="peak_TBps", type=float, default=6.3)
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--scenes", default="hexagon_room_diffuse,coffee_maker_qsah")
    args = ap.parse_args()
    args.width = args.width or (192 if args.errors else 1920)
    args.height = args.height or (108 if args.errors else 1080)
    args.seed = args.seed if args.seed is not None else (0x5EED0A0F if args.errors else 0x12345678)
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    (errors if args.errors else timing)(m, args)


if __name__ == "__main__":
    main()
