#!/usr/bin/env python3
"""The per-pixel sample statistics (mcrt_render_pixel_stats*) measured: what the statistics launch costs next to the frame, and whether
the summary's `noise` predicts the frame's error.

  python tools/pixel_stats_probe.py [--width 1920 --height 1080 --sqrtspp 4,16] [--runs 5] [--scene hexagon_room]
      Kernel: pixelStatsKernel alone on a store of the frame's size ([spp][pixels][3] FP64, random contents; launched through
      libmcrt_pixel_stats.so's own launch function, as the pass loops do), HIP events around the launches only, one warm-up, the median
      of --runs runs, for all three channels and for the half-buffers alone (one read of the store instead of two); bytes per second
      = the store's bytes times the reads, over the time; next to a device-to-device copy of the same store (read + write).
      Call: render_pixel_stats_device against render_device + render_finish, alternating, wall clock and mcrt_stats.kernel_ms (HIP
      events around the whole frame), the median of --runs pairs. One JSON line per sqrtspp.

  python tools/pixel_stats_probe.py --errors [--width 192 --height 108] [--truth-sqrtspp 32] [--scenes a,b,...]
      Per scene and sqrtspp 2, 4, 8: mcrt_frame_noise's `noise` (the predicted summed variance of the pixel means) next to the
      measured squared error, sum over pixels and channels of (frame - truth)^2 with truth a render at --truth-sqrtspp with another
      seed (whose own variance, noise * spp / truth_spp if it scaled like 1 / n, is inside the measurement). One JSON line each."""
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
    fn()  # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(max(runs, 1)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def timing(m, args):
    import torch
    m.lib()
    side = C.CDLL(os.path.join(os.path.dirname(m.LIB_PATH), "libmcrt_pixel_stats.so"))
    launch = side._ZN4mcrt16launchPixelStatsEPvRKNS_14PixelStatsPassE  # mcrt::launchPixelStats(void* stream, const PixelStatsPass&)
    launch.argtypes = [C.c_void_p, C.POINTER(PixelStatsPass)]
    launch.restype = C.c_int
    for sqrtspp in [int(s) for s in args.sqrtspp.split(",")]:
        img, cam, ctx = setup(m, args.scene, args.width, args.height, sqrtspp)
        spp, pixels = sqrtspp * sqrtspp, cam.width * cam.height
        rec = {"scene": args.scene, "width": cam.width, "height": cam.height, "spp": spp, "store_GB": round(spp * pixels * 24 / 1e9, 3)}
        # the kernel alone
        store = torch.rand((spp, pixels, 3), dtype=torch.float64, device="cuda:0")
        outs = [torch.empty((pixels, 3), dtype=torch.float64, device="cuda:0") for _ in range(3)]
        stream = torch.cuda.current_stream().cuda_stream
        for label, reads, chans in (("all", 2, (0, 1, 2)), ("halves", 1, (1, 2))):
            ps = PixelStatsPass(store.data_ptr(), pixels * 3, spp, 1 if store.data_ptr() % 16 == 0 and (pixels * 3) % 2 == 0 else 0,
                                *[outs[i].data_ptr() if i in chans else None for i in range(3)])

            def go():
                rc = launch(stream, C.byref(ps))
                assert rc == 0, rc
            ms = event_ms(torch, go, args.runs)
            rec["kernel_%s_ms" % label] = round(ms, 4)
            rec["kernel_%s_TBps" % label] = round(reads * store.numel() * 8 / ms / 1e9, 3)
        twin = torch.empty_like(store)
        ms = event_ms(torch, lambda: twin.copy_(store), args.runs)
        rec["copy_ms"], rec["copy_TBps_read_plus_write"] = round(ms, 4), round(2 * store.numel() * 8 / ms / 1e9, 3)
        del twin, store
        torch.cuda.empty_cache()
        # the whole call, alternating with the plain render
        rgb = torch.empty((cam.height, cam.width, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ptrs = {k: outs[i].data_ptr() for i, k in enumerate(m.PIXEL_STATS_CHANNELS)}
        wall, kern = {"plain": [], "stats": []}, {"plain": [], "stats": []}
        for i in range(max(args.runs, 1) + 1):
            for which in ("plain", "stats"):
                t0 = time.perf_counter()
                if which == "plain":
                    ctx.render_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr())
                    st = ctx.render_finish()
                else:
                    st = ctx.render_pixel_stats_device(cam, args.seed, m.INTEGRATOR_PATH_TRACER, rgb.data_ptr(), ptrs)
                if i:  # (the first pair warms up)
                    wall[which].append((time.perf_counter() - t0) * 1e3)
                    kern[which].append(st["kernel_ms"])
        for which in ("plain", "stats"):
            rec["call_%s_wall_ms" % which] = round(statistics.median(wall[which]), 3)
            rec["call_%s_kernel_ms" % which] = round(statistics.median(kern[which]), 3)
        rec["call_difference_kernel_ms"] = round(rec["call_stats_kernel_ms"] - rec["call_plain_kernel_ms"], 3)
        rec["kernel_id"], rec["kernel_launches"] = st["kernel_id"], st["kernel_launches"]
        print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


def errors(m, args):
    import numpy as np
    for name in args.scenes.split(","):
        img, cam, ctx = setup(m, name, args.width, args.height, args.truth_sqrtspp)
        truth, _ = ctx.sample_image(cam, args.seed ^ 0x00ABCDEF, m.INTEGRATOR_PATH_TRACER)
        for sqrtspp in (2, 4, 8):
            cam.sqrtspp = sqrtspp
            spp = sqrtspp * sqrtspp
            got = ctx.render_pixel_stats(cam, args.seed, m.INTEGRATOR_PATH_TRACER, channels=("variance",))
            fn = ctx.frame_noise(got["rgb"], got["variance"], spp)
            measured = float(((got["rgb"] - truth) ** 2).sum())
            rec = {"scene": name, "width": cam.width, "height": cam.height, "spp": spp, "truth_spp": args.truth_sqrtspp ** 2, "noise": fn["noise"],
                   "signal": fn["signal"], "relative_error": fn["relative_error"], "squared_error": measured,
                   "noise_over_squared_error": round(fn["noise"] / measured, 4) if measured > 0 else None}
            print(json.dumps(rec), flush=True)
        ctx.close()
        img.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--sqrtspp", default="4,16")
    ap.add_argument("--truth-sqrtspp", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x12345678)
    ap.add_argument("--scene", default="hexagon_room")
    ap.add_argument("--scenes", default="hexagon_room_diffuse,hexagon_room,hexagon_room_ggx,coffee_maker_qsah")
    args = ap.parse_args()
    args.width = args.width or (192 if args.errors else 1920)
    args.height = args.height or (108 if args.errors else 1080)
    m = importlib.import_module("monte-carlo-ray-tracer_amd")
    (errors if args.errors else timing)(m, args)


if __name__ == "__main__":
    main()
