#!/usr/bin/env python3
"""The firefly suppression (mcrt_render_highlights*, mcrt_robust_resolve*) measured: what the highlights launch costs next to the frame
and next to the statistics kernel that reads the same store, what the resolve costs, and what the robust frame does to the error.

  python tools/robust_probe.py [--width 1920 --height 1080 --sqrtspp 4,16] [--runs 5] [--scene hexagon_room]
      Kernel: robustHighlightsKernel alone on a store of the frame's size ([spp][pixels][3] FP64, random contents; launched through
      libmcrt_robust.so's own launch function, as the pass loops do), HIP events around the launches only, one warm-up, the median
      (and the smallest and largest) of --runs runs, for both channels (two reads of the store) and for the tops alone (one read);
      bytes per second = the store's bytes times the reads, over the time; next to pixelStatsKernel with all three channels (two
      reads of the same store too), in the same session.
      Call: render_highlights_device against render_device + render_finish, alternating, wall clock and mcrt_stats.kernel_ms (HIP
      events around the whole frame), the median of --runs pairs; then the resolve of that frame. One JSON line per sqrtspp.

  python tools/robust_probe.py --errors [--width 192 --height 108] [--truth-sqrtspp 32] [--scenes a,b,...] [--sqrtspp 2,4,8]
      Per scene and sample count, over the grid kappa {4, 8, 16} x radius {1, 2}: the summed squared error of the robust frame over
      the plain frame's, against a render at --truth-sqrtspp with another seed; the pixels and samples clamped and the share of the
      frame's luminance that `removed` takes; and mcrt_denoise (defaults, the AOV frame of the same camera) on the robust frame against
      mcrt_denoise on the plain frame, both as squared error over the plain unfiltered frame's. One JSON line each."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


class HighlightsPass(C.Structure):  # csrc/mcrt_robust.hpp
    _fields_ = [("samples", C.c_void_p), ("pixels", C.c_uint64), ("spp", C.c_uint32), ("reserved", C.c_uint32), ("tops", C.c_void_p),
                ("level", C.c_void_p)]


class PixelStatsPass(C.Structure):  # csrc/mcrt_pixel_stats.hpp
    _fields_ = [("samples", C.c_void_p), ("words", C.c_uint64), ("spp", C.c_uint32), ("vec", C.c_uint32), ("variance", C.c_void_p),
                ("half_a", C.c_void_p), ("half_b", C.c_void_p)]


def setup(m, name, width, height, sqrtspp):
    img = m.SceneImage(os.path.join(ROOT, "tests", "golden", name + ".mcrt"))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = width, height, sqrtspp
    cam.shard_index, cam.shard_count = 0, 1
    ctx = m.Context(0)
    ctx.upload_scene(img.scene)
    return img, cam, ctx


def event_ms(torch, fn, runs):
    """-> (median, smallest, largest) of `runs` timed calls after one warm-up."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(max(runs, 1)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def timing(m, args):
    import torch
    m.lib()
    here = os.path.dirname(m.LIB_PATH)
    side = C.CDLL(os.path.join(here, "libmcrt_robust.so"))
    launch = side._ZN4mcrt16launchHighlightsEPvRKNS_14HighlightsPassE  # mcrt::launchHighlights(void* stream, const HighlightsPass&)
    launch.argtypes = [C.c_void_p, C.POINTER(HighlightsPass)]
    launch.restype = C.c_int
    twin = C.CDLL(os.path.join(here, "libmcrt_pixel_stats.so"))
    launch_stats = twin._ZN4mcrt16launchPixelStatsEPvRKNS_14PixelStatsPassE  # mcrt::launchPixelStats(void* stream, const PixelStatsPass&)
    launch_stats.argtypes = [C.c_void_p, C.POINTER(PixelStatsPass)]
    launch_stats.restype = C.c_int
    for sqrtspp in [int(s) for s in args.sqrtspp.split(",")]:
        img, cam, ctx = setup(m, args.scene, args.width, args.height, sqrtspp)
        spp, pixels = sqrtspp * sqrtspp, cam.width * cam.height
        rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "spp": spp, "store_GB": round(spp * pixels * 24 / 1e9, 3)}
        # the kernels alone, alternating so that neither has the warmer device
        store = torch.rand((spp, pixels, 3), dtype=torch.float64, device="cuda:0")
        tops = torch.empty((pixels, 4, 3), dtype=torch.float64, device="cuda:0")
        level = torch.empty((pixels,), dtype=torch.float64, device="cuda:0")
        outs = [torch.empty((pixels, 3), dtype=torch.float64, device="cuda:0") for _ in range(3)]
        stream = torch.cuda.current_stream().cuda_stream
        both = HighlightsPass(store.data_ptr(), pixels, spp, 0, tops.data_ptr(), level.data_ptr())
        only_tops = HighlightsPass(store.data_ptr(), pixels, spp, 0, tops.data_ptr(), None)
        ps = PixelStatsPass(store.data_ptr(), pixels * 3, spp, 1 if store.data_ptr() % 16 == 0 and (pixels * 3) % 2 == 0 else 0,
                            *[o.data_ptr() for o in outs])

        def go(fn, arg):
            def run():
                rc = fn(stream, C.byref(arg))
                assert rc == 0, rc
            return run
        for rep in range(2):  # (twice each, interleaved: the spread between the repeats is what a difference is read against)
            for label, reads, fn in (("highlights", 2, go(launch, both)), ("pixel_stats", 2, go(launch_stats, ps)), ("tops_only", 1, go(launch, only_tops))):
                ms, lo, hi = event_ms(torch, fn, args.runs)
                rec["kernel_%s_ms_%d" % (label, rep)] = [round(ms, 4), round(lo, 4), round(hi, 4)]
                rec["kernel_%s_TBps_%d" % (label, rep)] = round(reads * store.numel() * 8 / ms / 1e9, 3)
        del store
        torch.cuda.empty_cache()
        # the whole call, alternating with the plain render
        rgb = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ptrs = {"tops": tops.data_ptr(), "level": level.data_ptr()}
        wall, kern = {"plain": [], "highlights": []}, {"plain": [], "highlights": []}
        for i in range(max(args.runs, 1) + 1):
            for which in ("plain", "highlights"):
                t0 = time.perf_counter()
                if which == "plain":
                    ctx.render_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr())
                    st = ctx.render_finish()
                else:
                    st = ctx.render_highlights_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr(), ptrs)
                if i:  # (the first pair warms up)
                    wall[which].append((time.perf_counter() - t0) * 1e3)
                    kern[which].append(st["kernel_ms"])
        for which in ("plain", "highlights"):
            rec["call_%s_wall_ms" % which] = round(statistics.median(wall[which]), 3)
            rec["call_%s_kernel_ms" % which] = round(statistics.median(kern[which]), 3)
        rec["call_difference_kernel_ms"] = round(rec["call_highlights_kernel_ms"] - rec["call_plain_kernel_ms"], 3)
        rec["kernel_id"], rec["kernel_launches"] = st["kernel_id"], st["kernel_launches"]
        # the resolve of that frame (to another frame; removed and clamped written)
        out = torch.empty_like(rgb)
        removed = torch.empty_like(rgb)
        clamped = torch.empty((cam.height, cam.width), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for radius in (1, 2):
            ms = []
            for i in range(max(args.runs, 1) + 1):
                st = ctx.robust_resolve_device(cam.width, cam.height, spp, rgb.data_ptr(), tops.data_ptr(), level.data_ptr(), out.data_ptr(),
                                               removed.data_ptr(), clamped.data_ptr(), radius=radius)
                if i:
                    ms.append(st["kernel_ms"])
            rec["resolve_radius%d_kernel_ms" % radius] = round(statistics.median(ms), 4)
        rec["clamped_pixels"] = int((clamped > 0).sum().item())
        print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


def errors(m, args):
    import numpy as np
    lum = lambda x: (0.2126 * x[..., 0] + 0.7152 * x[..., 1]) + 0.0722 * x[..., 2]
    for name in args.scenes.split(","):
        img, cam, ctx = setup(m, name, args.width, args.height, args.truth_sqrtspp)
        truth, _ = ctx.sample_image(cam, args.seed ^ 0x00ABCDEF, m.INTEGRATOR_PATH_TRACER)
        sq = lambda frame: float(((frame - truth) ** 2).sum())
        for sqrtspp in [int(s) for s in args.sqrtspp.split(",")]:
            cam.sqrtspp = sqrtspp
            spp = sqrtspp * sqrtspp
            hl = ctx.render_highlights(cam, args.seed, m.INTEGRATOR_PATH_TRACER)
            guides = ctx.render_aov(cam, args.seed, channels=m.DENOISE_GUIDES)
            plain = sq(hl["rgb"])
            plain_denoised = sq(ctx.denoise(hl["rgb"], guides))
            for kappa in (4.0, 8.0, 16.0):
                for radius in (1, 2):
                    r = ctx.robust_resolve(hl["rgb"], hl["tops"], hl["level"], spp, kappa=kappa, radius=radius)
                    rec = {"scene": name, "width": cam.width, "height": cam.height, "spp": spp, "truth_spp": args.truth_sqrtspp ** 2, "kappa": kappa,
                           "radius": radius, "squared_error_plain": plain, "robust_over_plain": round(sq(r["robust"]) / plain, 4),
                           "clamped_pixels": int((r["clamped"] > 0).sum()), "clamped_samples": int(r["clamped"].sum()),
                           "removed_share_of_luminance": round(float(lum(r["removed"]).sum() / lum(hl["rgb"]).sum()), 5),
                           "denoised_plain_over_plain": round(plain_denoised / plain, 4),
                           "denoised_robust_over_plain": round(sq(ctx.denoise(r["robust"], guides)) / plain, 4)}
                    print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--sqrtspp")
    ap.add_argument("--truth-sqrtspp", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--scenes", default="hexagon_room_diffuse,hexagon_room,hexagon_room_ggx,coffee_maker_qsah")
    args = ap.parse_args()
    args.width = args.width or (192 if args.errors else 1920)
    args.height = args.height or (108 if args.errors else 1080)
    args.sqrtspp = args.sqrtspp or ("2,4,8" if args.errors else "4,16")
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    (errors if args.errors else timing)(m, args)


if __name__ == "__main__":
    main()
