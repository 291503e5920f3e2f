#!/usr/bin/env python3
"""The OpenEXR output measured (profiles/NOTES_exr.md): ONE run at 1920 x 1080 with the full exr_layers set of a 16 spp render of
hexagon_room_diffuse - AOV, statistics, highlights, robust frame, the three denoisers. Per compression (NONE, ZIP) and form (torch device
tensors, numpy arrays): one warm-up save, then 5 (device) or 2 (host) timed ones - the pack kernel's kernel_ms (the call's own HIP events),
total_ms, the file's size; the bytes the kernel has to read (every channel's source elements once) and write (the packed buffer), that
traffic over kernel_ms as a share of the 6.3 TB/s an MI355X achieves; the sum of the raw FP64 / uint32 buffers for comparison. Needs a GPU.

    python tools/exr_measure.py [OUT.json]"""
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
def dev(a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")
def devd(d):
    return {k: dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
host = dict(rgb=hl["rgb"], aov=aov, stats=hl, highlights=hl, robust=rb, denoised={"denoise": dn, "denoise_variance": dv, "denoise_dual": dd})
layers_h = m.exr_layers(**host)
layers_d = m.exr_layers(rgb=dev(hl["rgb"]), aov=devd(aov), stats=devd(hl), highlights=devd(hl), robust=devd(rb),
                        denoised={"denoise": dev(dn), "denoise_variance": tuple(dev(x) for x in dv), "denoise_dual": devd(dd)})
torch.cuda.synchronize()
assert sorted(layers_h) == sorted(layers_d)
sizes = {"half": 2, "float": 4, "uint": 4}
px = W * H
read_bytes = sum(px * (4 if t == "uint" else 8) for _, t in layers_h.values())
packed = sum(px * sizes[t] for _, t in layers_h.values())
arrays = [hl[k] for k in ("rgb", "variance", "half_a", "half_b", "tops", "level")] + list(aov.values()) + list(rb.values()) + [dn, dv[0], dv[1], dd["rgb"], dd["variance"]]
f64_dump = sum(a.nbytes for a in arrays)
out = {"width": W, "height": H, "channels": len(layers_h), "types": {t: sum(1 for _, x in layers_h.values() if x == t) for t in sizes},
       "source_bytes_read": read_bytes, "packed_bytes": packed, "f64_dump_bytes": f64_dump, "f64_dump_files": len(arrays)}
tmp = tempfile.mkdtemp()
for comp in ("none", "zip"):
    for form, layers in (("device", layers_d), ("host", layers_h)):
        reps = 6 if form == "device" else 3
        ks, ts = [], []
        for i in range(reps):
            st = {}
            path = os.path.join(tmp, "%s_%s.exr" % (comp, form))
            res = ctx.exr_save(path, layers, attributes={"mcrt:spp": S * S}, compression=comp, stats=st)
            assert res["packed_bytes"] == packed
            if i:  # (the first is the warm-up)
                ks.append(st["kernel_ms"]); ts.append(st["total_ms"])
        key = "%s_%s" % (comp, form)
        out[key] = {"kernel_ms": [round(x, 3) for x in ks], "kernel_ms_median": statistics.median(ks), "total_ms": [round(x, 1) for x in ts],
                    "total_ms_median": statistics.median(ts), "file_bytes": res["file_bytes"], "chunks": res["chunks"], "raw_chunks": res["raw_chunks"]}
        k = statistics.median(ks) * 1e-3
        out[key]["traffic_TB_s"] = (read_bytes + packed) / k / 1e12
        out[key]["share_of_6.3_TB_s"] = (read_bytes + packed) / k / 6.3e12
        print(key, json.dumps(out[key]), flush=True)
# the files read back: NONE and ZIP hold the same bits
sys.path.insert(0, os.path.join(ROOT, "tools"))
import exr_probe
a, _, _ = exr_probe.read(os.path.join(tmp, "none_device.exr"))
b, _, _ = exr_probe.read(os.path.join(tmp, "zip_host.exr"))
out["none_equals_zip"] = all(a[n].tobytes() == b[n].tobytes() for n in a) and list(a) == list(b)
out["deflate_threads_default"] = min(16, os.cpu_count() or 1)
if OUT:
    json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out))
ctx.close()
__import__("shutil").rmtree(tmp)
