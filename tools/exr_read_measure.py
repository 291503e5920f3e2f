#!/usr/bin/env python3
"""The OpenEXR input measured (profiles/NOTES_exr_read.md): ONE run at 1920 x 1080 on the file that profiles/NOTES_exr.md describes - the
full exr_layers set of a 16 spp render of hexagon_room_diffuse, 63 channels - written once without compression and once with ZIP by
Context.exr_save. Per file and form (torch device tensors, numpy arrays): one warm-up load, then 5 (device) or 2 (host) timed ones -
kernel_ms (the call's own HIP events around its launches), total_ms, payload_bytes; the bytes the kernels read and write, that traffic
over kernel_ms as a share of the 6.3 TB/s an MI355X achieves; and where the call's time goes on the host, from a load on ONE inflate
thread next to the default. The frames of the two files must be the same bits, and R must be the widened HALF of the render. Needs a GPU.

    python tools/exr_read_measure.py [OUT.json]"""
import importlib, json, os, statistics, sys, tempfile, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else None
sys.path.insert(0, ROOT)
m = importlib.import_module("monte-carlo-ray-tracer_amd")
W, H, S, SEED = 1920, 1080, 4, 0x5EED0A0F
img = m.SceneImage(os.path.join(ROOT, "tests", "golden", "hexagon_room_diffuse.mcrt"))
cam = img.camera
cam.width, cam.height, cam.sqrtspp = W, H, S
cam.shard_index, cam.shard_count, cam.shard_rows = 0, 1, 0
ctx = m.Context(0)
ctx.upload_image(img)
t0 = time.time()
hl = ctx.render_highlights(cam, SEED, m.INTEGRATOR_PATH_TRACER, stats_channels=m.PIXEL_STATS_CHANNELS)
aov = ctx.render_aov(cam, SEED)
rb = ctx.robust_resolve(hl["rgb"], hl["tops"], hl["level"], S * S)
dn = ctx.denoise(hl["rgb"], aov)
dv = ctx.denoise_variance(hl["rgb"], hl["variance"], aov, S * S)
dd = ctx.denoise_dual(hl["half_a"], hl["half_b"], hl["variance"], S * S)
print("rendered and filtered in %.1f s" % (time.time() - t0), flush=True)
layers = m.exr_layers(rgb=hl["rgb"], aov=aov, stats=hl, highlights=hl, robust=rb, denoised={"denoise": dn, "denoise_variance": dv, "denoise_dual": dd})
sizes = {"half": 2, "float": 4, "uint": 4}
px = W * H
payload = sum(px * sizes[t] for _, t in layers.values())
written = sum(px * (4 if t == "uint" else 8) for _, t in layers.values())
out = {"width": W, "height": H, "channels": len(layers), "types": {t: sum(1 for _, x in layers.values() if x == t) for t in sizes},
       "payload_bytes": payload, "destination_bytes_written": written, "inflate_threads_default": min(16, os.cpu_count() or 1)}
tmp = tempfile.mkdtemp()
frames = {}
for comp in ("none", "zip"):
    path = os.path.join(tmp, comp + ".exr")
    res = ctx.exr_save(path, layers, attributes={"mcrt:spp": S * S}, compression=comp)
    for form in ("device", "host"):
        reps = 6 if form == "device" else 3
        ks, ts = [], []
        for i in range(reps):
            st = {}
            got, _, info = ctx.exr_load(path, device=form == "device", stats=st)
            assert info["payload_bytes"] == payload and len(got) == len(layers)
            if i:  # (the first is the warm-up)
                ks.append(st["kernel_ms"]); ts.append(st["total_ms"])
            if form == "device" and i == reps - 1:
                frames[comp] = got
            del got
        key = "%s_%s" % (comp, form)
        # the scan reads the payload twice (tile sums, undo) and writes the plane once; the gather reads the value's bytes and writes the frames
        traffic = written + payload * (4 if comp == "zip" else 1)
        k = statistics.median(ks) * 1e-3
        out[key] = {"kernel_ms": [round(x, 3) for x in ks], "kernel_ms_median": statistics.median(ks), "total_ms": [round(x, 1) for x in ts],
                    "total_ms_median": statistics.median(ts), "kernel_launches": st["kernel_launches"], "file_bytes": info["file_bytes"], "chunks": info["chunks"],
                    "raw_chunks": info["raw_chunks"], "traffic_bytes": traffic, "traffic_TB_s": traffic / k / 1e12, "share_of_6.3_TB_s": traffic / k / 6.3e12}
        print(key, json.dumps(out[key]), flush=True)
    st = {}
    ctx.exr_load(path, device=True, threads=1, stats=st)
    out["%s_device_one_thread_total_ms" % comp] = round(st["total_ms"], 1)
    t0 = time.time()
    with open(path, "rb") as f:
        n = len(f.read())
    out["%s_plain_read_ms" % comp] = round((time.time() - t0) * 1e3, 1)
    assert n == res["file_bytes"]
out["none_equals_zip"] = list(frames["none"]) == list(frames["zip"]) and all(torch.equal(frames["none"][n], frames["zip"][n]) for n in frames["none"])
half = hl["rgb"][..., 0].astype(np.float16)   # (finite, in range: one rounding; the tests hold the rest)
out["R_is_the_widened_half"] = bool(np.array_equal(frames["zip"]["R"].cpu().numpy(), half.astype(np.float64)))
if OUT:
    json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out))
ctx.close()
__import__("shutil").rmtree(tmp)
