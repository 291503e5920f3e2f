"""OpenEXR input on the GPU (mcrt_exr_open .. mcrt_exr_load / mcrt_exr_load_device): the frames the kernels' bits give, against the numpy
restatement of include/mcrt.h that tests/test_exr_read_emulation.py keeps (and holds the host emulation to), in the host-pointer form and
in the torch-device form; the files are those of the Python writers there and in tests/test_exr_emulation.py, never the library's own
save - except where the round trip through the save is what is tested. What the C ABI promises besides: strided destinations whose other
elements keep their bytes, the refusals, a load while a render is in flight; Context.exr_load against tools/exr_probe.py; exr_unlayer on
the device; and the host program's --compare with an OpenEXR reference.

Bounds: bits everywhere. The widenings are integer arithmetic on the bits, so that no floating-point mode of the device can show: every
binary16 pattern and the binary32 subnormals, edges and NaNs are part of one file here."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_aov_emulation as aov
import test_exr_emulation as ex
import test_exr_read_emulation as rd
from conftest import golden_path

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, SEED = aov.WIDTH, aov.HEIGHT, aov.SEED   # 70 x 13: the smallest frame the image passes' GPU tests render
SCENE = "hexagon_room_diffuse"
_state = {}


@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    yield
    for k in [k for k in _state if isinstance(k, str)]:
        _state.pop(k).close()
    _state.clear()


def context(pkg, scene=None):
    key = scene or "no scene"
    if key not in _state:
        ctx = pkg.Context(0)
        if scene:
            ctx.upload_image(aov._image(scene))
        _state[key] = ctx
    return _state[key]


def host(a):
    """A loaded channel as a numpy array of the file's kind: a device tensor's int32 are the uint32 bits."""
    if hasattr(a, "data_ptr"):
        a = a.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a
    return a


def assert_loaded(got, file_chans, msg=""):
    for n, t, v in file_chans:
        if n in got:
            a = host(got[n])
            assert a.dtype == (np.uint32 if t == rd.UINT else np.float64) and a.shape == v.shape, (msg, n)
            np.testing.assert_array_equal(a.view(np.uint32 if t == rd.UINT else np.uint64), rd.widened(v, t), err_msg="%s %s" % (msg, n))


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("which", ex.CHANNEL_SETS)
def test_files_of_the_python_writer_load_bit_for_bit(pkg, tmp_path, which, form):
    ctx = context(pkg)
    path = str(tmp_path / "f.exr")
    for width in ex.WIDTHS:
        for height in ex.HEIGHTS:
            file_chans = ex.sorted_file_channels(ex.channel_set(which, width, height))
            line_bytes = width * sum(ex.FILE_DTYPES[t].itemsize for _, t, _ in file_chans)
            for compression in (0, 3):
                msg = "%s %d x %d %s %d" % (which, width, height, form, compression)
                data, raws = ex.py_exr_file(width, height, file_chans, compression, ex.ATTRIBUTES)
                open(path, "wb").write(data)
                stats = {}
                got, attrs, info = ctx.exr_load(path, device=form == "device", threads=2, stats=stats)
                assert list(got) == [n for n, _, _ in file_chans], msg
                assert_loaded(got, file_chans, msg)
                lines = 16 if compression else 1
                chunks = (height + lines - 1) // lines
                raws = raws if compression else chunks
                assert info == {"width": width, "height": height, "data_window": (0, 0, width - 1, height - 1), "display_window": (0, 0, width - 1, height - 1),
                                "compression": compression, "line_order": 0, "chunks": chunks, "raw_chunks": raws, "file_bytes": len(data),
                                "payload_bytes": height * line_bytes}, msg
                assert stats["kernel_launches"] == (1 if raws == chunks else 4) and stats["kernel_ms"] > 0 and stats["total_ms"] > 0, msg
                assert [(k, attrs[k]) for k in list(attrs)[8:]] == [(k, ("string", v)) for k, v in ex.ATTRIBUTES], msg


def pattern_file(compression):
    """256 x 256: H holds every binary16 pattern; F binary32 zeros, the subnormals' single bits and neighbours, exponent fields 0, 1, 254,
    255 at fractions 0, 1, 0x7fffff, quiet and signalling NaNs of both signs, the conversion list rounded to float, and random patterns."""
    h = np.arange(1 << 16, dtype=np.uint16).reshape(256, 256)
    with np.errstate(all="ignore"):
        listed = ex.conversion_list().astype(np.float32).view(np.uint32)
    edges = np.array([s | e << 23 | f for s in (0, 0x80000000) for e in (0, 1, 254, 255) for f in (0, 1, 0x400000, 0x7fffff)], dtype=np.uint32)
    subnormals = np.array([1 << k for k in range(23)] + [(1 << k) | 1 for k in range(1, 23)] + [(1 << k) - 1 for k in range(2, 24)], dtype=np.uint32)
    f = np.random.default_rng(2024).integers(0, 1 << 32, size=1 << 16, dtype=np.uint32)
    first = np.concatenate([listed, edges, subnormals])
    f[:first.size] = first
    f = f.reshape(256, 256)
    chans = [("F", rd.FLOAT, f.view("<f4")), ("H", rd.HALF, h.view("<f2"))]
    return rd.variant_file(256, 256, chans, compression)[0], chans


@pytest.mark.parametrize("form", ["host", "device"])
def test_every_half_pattern_and_the_float_edges_on_the_device(pkg, tmp_path, form):
    """... widen to the definition, uncompressed and through ZIP's scan; saved again as HALF and FLOAT the loaded frames give back the
    file's bits for every pattern that is no NaN, for 0x7e00 / 0xfe00 and for every quiet binary32 NaN."""
    ctx = context(pkg)
    for compression in (rd.NONE, rd.ZIP):
        data, chans = pattern_file(compression)
        path = str(tmp_path / ("patterns%d.exr" % compression))
        open(path, "wb").write(data)
        got, _, info = ctx.exr_load(path, device=form == "device")
        assert_loaded(got, chans, "compression %d" % compression)
        assert info["chunks"] == (16 if compression else 256) and (compression == 0 or info["raw_chunks"] < info["chunks"])
    again = str(tmp_path / "again.exr")
    ctx.exr_save(again, {"H": (got["H"], "half"), "F": (got["F"], "float")}, compression="none", half_inf=True)
    back, _, _ = ex.probe().read(again)
    hb, fb = chans[1][2].view(np.uint16), chans[0][2].view(np.uint32)
    h_nan, f_nan = ((hb & 0x7c00) == 0x7c00) & ((hb & 1023) != 0), ((fb & 0x7f800000) == 0x7f800000) & ((fb & 0x7fffff) != 0)
    h_same, f_same = ~h_nan | (hb == 0x7e00) | (hb == 0xfe00), ~f_nan | ((fb & 0x400000) != 0)
    assert h_same.sum() == 65536 - 2046 + 2 and (f_nan & f_same).sum() > 50 and (~f_same).sum() > 50
    np.testing.assert_array_equal(back["H"].view(np.uint16)[h_same], hb[h_same])
    np.testing.assert_array_equal(back["F"].view(np.uint32)[f_same], fb[f_same])


@pytest.mark.parametrize("form", ["host", "device"])
def test_scan_boundaries_and_variant_files(pkg, tmp_path, form):
    ctx = context(pkg)
    tile = rd._emu().exr_read_tile_bytes_emu()
    for label, data, chans, chunks, raws in rd.boundary_cases(tile):
        path = str(tmp_path / (label + ".exr"))
        open(path, "wb").write(data)
        stats = {}
        got, _, info = ctx.exr_load(path, device=form == "device", stats=stats)
        assert_loaded(got, chans, label)
        assert (info["chunks"], info["raw_chunks"], stats["kernel_launches"]) == (chunks, raws, 4), label
    for variant in rd.VARIANTS:
        data, file_chans, compression, raws, kw = rd.variant_case(variant)
        path = str(tmp_path / (variant + ".exr"))
        open(path, "wb").write(data)
        got, attrs, info = ctx.exr_load(path, device=form == "device")
        assert list(got) == [n for n, _, _ in file_chans], variant
        assert_loaded(got, file_chans, variant)
        x0, y0 = kw.get("origin", (0, 0))
        assert info["data_window"] == (x0, y0, x0 + 64, y0 + 39) and info["display_window"] == tuple(kw.get("display", info["data_window"])), variant
        assert (info["compression"], info["line_order"]) == (compression, kw.get("line_order", 0)), variant
        if variant == "attributes":
            assert attrs["exposure"] == ("float", 1.5) and attrs["offset"] == ("v2f", (0.25, -2.0)) and attrs["chromaticities"] == ("chromaticities", rd.EXTRA[2][2])
            assert attrs["made.up"] == ("a type nobody knows", rd.EXTRA[3][2]) and attrs["empty"] == ("another", b"") and attrs["mcrt:spp"] == ("string", "16")
            assert list(attrs)[8:] == [e[0] for e in rd.EXTRA]
        if variant == "long_names":
            assert rd.LONG_NAME in got


@pytest.mark.parametrize("form", ["host", "device"])
def test_strided_destinations_a_subset_and_sentinels_through_the_abi(pkg, tmp_path, form):
    """R, G into one [H,W,3] whose third plane no target names; the twelve tops channels into [H,W,5,3]; B alone into slot 2 of [H,W,4];
    surface.id of another file into the odd words of [H,W,2] uint32: in an order that is not the file's, and every other element keeps
    its sentinel - in the host form through the staging and the copy back."""
    import torch
    ctx = context(pkg)
    L = pkg.lib()
    w, h = 65, 17
    file_chans = ex.sorted_file_channels(ex.channel_set("strided_15", w, h))
    by = {n: (t, v) for n, t, v in file_chans}
    mixed = ex.sorted_file_channels(ex.channel_set("mixed_unsorted", w, h))
    for compression in (0, 3):
        paths = []
        for name, chans in (("s", file_chans), ("m", mixed)):
            paths.append(str(tmp_path / ("%s%d.exr" % (name, compression))))
            open(paths[-1], "wb").write(ex.py_exr_file(w, h, chans, compression)[0])
        rgb = np.full((h, w, 3), rd.SENTINEL_F64, dtype=np.uint64)
        tops = np.full((h, w, 5, 3), rd.SENTINEL_F64, dtype=np.uint64)
        lone = np.full((h, w, 4), rd.SENTINEL_F64, dtype=np.uint64)
        ids = np.full((h, w, 2), rd.SENTINEL_U32, dtype=np.uint32)
        if form == "device":
            dev = [torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to("cuda:0") for a in (rgb, tops, lone, ids)]
            torch.cuda.synchronize()
            base = [int(d.data_ptr()) for d in dev]
        else:
            base = [a.ctypes.data for a in (rgb, tops, lone, ids)]
        targets = [pkg.ExrTarget(("tops%d.%s" % (k, "RGB"[c])).encode(), base[1], 0, 15, 3 * k + c, 0) for k in (3, 1, 0, 2) for c in (2, 0, 1)]
        targets += [pkg.ExrTarget(b"B", base[2], 0, 4, 2, 0), pkg.ExrTarget(b"G", base[0], 0, 3, 1, 0), pkg.ExrTarget(b"R", base[0], 0, 3, 0, 0)]
        call = L.mcrt_exr_load_device if form == "device" else L.mcrt_exr_load
        for path, recs in ((paths[0], targets), (paths[1], [pkg.ExrTarget(b"surface.id", base[3], 1, 2, 1, 0)])):
            f = C.c_void_p()
            assert L.mcrt_exr_open(ctx._h, path.encode(), C.byref(f)) == 0
            res = pkg.ExrLoadResult()
            rc = call(ctx._h, f, (pkg.ExrTarget * len(recs))(*recs), len(recs), None, C.byref(res), None)
            L.mcrt_exr_close(f)
            assert rc == 0, L.mcrt_last_error(ctx._h)
            assert res.payload_bytes == h * w * (15 * 2 + 6 * 2 if path == paths[0] else 16)   # (six of the fifteen are FLOAT)
        if form == "device":
            rgb, tops, lone, ids = [d.cpu().numpy().view(a.dtype) for d, a in zip(dev, (rgb, tops, lone, ids))]
        for c in (0, 1):
            np.testing.assert_array_equal(rgb[..., c], rd.widened(by["RGB"[c]][1], by["RGB"[c]][0]))
        for k in range(4):
            for c in range(3):
                n = "tops%d.%s" % (k, "RGB"[c])
                np.testing.assert_array_equal(tops[:, :, k, c], rd.widened(by[n][1], by[n][0]), err_msg=n)
        np.testing.assert_array_equal(lone[..., 2], rd.widened(by["B"][1], by["B"][0]))
        np.testing.assert_array_equal(ids[..., 1], dict((n, v) for n, _, v in mixed)["surface.id"])
        assert (rgb[..., 2] == rd.SENTINEL_F64).all() and (tops[:, :, 4, :] == rd.SENTINEL_F64).all() and (lone[..., [0, 1, 3]] == rd.SENTINEL_F64).all()
        assert (ids[..., 0] == rd.SENTINEL_U32).all()


def test_refusals_through_the_abi(pkg, tmp_path):
    import torch
    ctx = context(pkg, SCENE)
    L, h = pkg.lib(), ctx._h
    good, _, head = rd.small_file()
    path = str(tmp_path / "good.exr")
    open(path, "wb").write(good)
    d = torch.zeros((18, 9, 3), dtype=torch.float64, device="cuda:0")
    ids = torch.zeros((18, 9), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def opened(data=None, name="x.exr"):
        p = path
        if data is not None:
            p = str(tmp_path / name)
            open(p, "wb").write(data)
        f = C.c_void_p()
        rc = L.mcrt_exr_open(h, p.encode(), C.byref(f))
        return rc, f, (L.mcrt_last_error(h) or b"").decode()

    def rec(name=b"R", data=d.data_ptr(), dest=0, stride=3, offset=0, reserved=0):
        return pkg.ExrTarget(name, data, dest, stride, offset, reserved)

    rc, f, _ = opened()
    assert rc == 0 and f

    def call(recs, count=None, params=None, fn=L.mcrt_exr_load_device, file=f):
        arr = (pkg.ExrTarget * max(len(recs), 1))(*recs) if recs is not None else None
        rc = fn(h, file, arr, len(recs) if count is None else count, C.byref(params) if params else None, None, None)
        return rc, (L.mcrt_last_error(h) or b"").decode()

    assert call([rec(), rec(b"surface.id", ids.data_ptr(), 1, 1)])[0] == 0
    invalid = [call(None, count=1), call([rec()], count=0), call([rec()] * 1025), call([rec()], file=None), call([rec()], params=pkg.ExrLoadParams(0, 1)),
               call([rec(name=None)]), call([rec(name=b"albedo.R")]), call([rec(data=None)]), call([rec(stride=0)]), call([rec(offset=3)]), call([rec(reserved=1)]),
               call([rec(dest=1)]), call([rec(dest=2)]), call([rec(b"surface.id")]), call([rec(b"B", ids.data_ptr(), 1, 1)]), call([rec(), rec(b"G")]),
               call([rec(), rec(b"G", d.data_ptr() + 8, 0, 3, 2)])]
    for i, (rc, msg) in enumerate(invalid):
        assert rc == ex.ERR_INVALID and msg.startswith("mcrt_exr_load_device: "), (i, rc, msg)
    assert "albedo.R" in invalid[6][1]
    rc, msg = call([rec(stride=0)], fn=L.mcrt_exr_load)
    assert rc == ex.ERR_INVALID and msg.startswith("mcrt_exr_load: ")
    assert L.mcrt_exr_open(h, None, C.byref(C.c_void_p())) == ex.ERR_INVALID and L.mcrt_exr_open(h, path.encode(), None) == ex.ERR_INVALID
    assert L.mcrt_exr_file_info(None, C.byref(pkg.ExrInfo())) == ex.ERR_INVALID and L.mcrt_exr_file_info(f, None) == ex.ERR_INVALID
    assert L.mcrt_exr_file_channel(f, 5, None, None) == ex.ERR_INVALID and L.mcrt_exr_file_channel(f, 4, None, None) == 0
    assert L.mcrt_exr_file_attribute(f, 8, None, None, None, None) == ex.ERR_INVALID and L.mcrt_exr_file_attribute(f, 7, None, None, None, None) == 0
    L.mcrt_exr_close(None)
    # files: what open refuses, and what only the load sees
    rc, g, msg = opened(good[:head + 8])
    assert rc == ex.ERR_IO and not g and msg.startswith("mcrt_exr_open: ") and "offset table" in msg
    rc, g, msg = opened(rd.small_file(version=2 | 0x200)[0])
    assert rc == ex.ERR_UNSUPPORTED and not g and "tiled" in msg
    rc, g, msg = opened(b"", "empty.exr")
    assert rc == ex.ERR_IO and not g
    first = np.frombuffer(good, dtype="<u8", count=1, offset=head)[0]
    rc, g, _ = opened(rd._patch(good, int(first) + 8, b"\xff" * 8), "stream.exr")
    assert rc == 0 and g
    rc, msg = call([rec()], file=g)
    assert rc == ex.ERR_IO and "chunk 0" in msg and "inflate" in msg
    L.mcrt_exr_close(g)
    # a load while a render is in flight, in both forms; served again once the render was collected
    cam = aov._image(SCENE).camera
    cam.width, cam.height, cam.sqrtspp = WIDTH, HEIGHT, 1
    cam.shard_index, cam.shard_count, cam.shard_rows = 0, 1, 0
    frame = torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float64, device="cuda:0")
    ctx.render_device(cam, SEED, pkg.INTEGRATOR_PATH_TRACER, frame.data_ptr())
    try:
        for fn in (L.mcrt_exr_load_device, L.mcrt_exr_load):
            rc, msg = call([rec()], fn=fn)
            assert rc == ex.ERR_INVALID and "in flight" in msg, (rc, msg)
        with pytest.raises(pkg.McrtError, match=r"\(-1\).*in flight"):
            ctx.exr_load(path)
    finally:
        ctx.render_finish()
    assert call([rec()])[0] == 0
    L.mcrt_exr_close(f)
    with pytest.raises(pkg.McrtError, match=r"mcrt_exr_load failed \(-1\).*albedo.R"):
        ctx.exr_load(path, channels=["R", "albedo.R"])
    with pytest.raises(pkg.McrtError, match=r"mcrt_exr_open failed \(-6\)"):
        ctx.exr_load(str(tmp_path / "not there.exr"))
    np.testing.assert_array_equal(d[..., 0].cpu().numpy().view(np.uint64), rd.widened(dict((n, v) for n, _, v in rd.small_chans())["R"], rd.HALF))


def synthetic_layers(pkg, h, w, seed=5):
    rng = np.random.default_rng(seed)
    f3, f1 = lambda: rng.random((h, w, 3)), lambda: rng.random((h, w))
    u1 = lambda: rng.integers(0, 1 << 32, size=(h, w), dtype=np.uint32)
    aov_ = {k: (u1() if t == np.uint32 else f3() if n == 3 else f1()) for k, (t, n) in pkg.AOV_CHANNELS.items()}
    return dict(rgb=f3(), aov=aov_, stats={"variance": f3(), "half_a": f3(), "half_b": f3()}, highlights={"tops": rng.random((h, w, 4, 3)), "level": f1()},
                robust={"robust": f3(), "removed": f3(), "clamped": u1()}, denoised={"denoise_dual": {"rgb": f3(), "variance": f3(), "error": f3()}},
                errors={"squared_error": f1(), "relative": f1(), "ssim": f1()})


def test_exr_load_against_the_probe_and_exr_unlayer_on_the_device(pkg, tmp_path):
    """A file of the library's own save with every documented layer: what Context.exr_load returns compares == with what
    tools/exr_probe.py reads - channels exactly widened, attributes, sizes -, a subset comes in the order asked for, and exr_unlayer
    puts the frames together again where they live: on the device, nothing but the file's bytes crossed."""
    import torch
    ctx = context(pkg)
    h, w = 33, 65
    given = synthetic_layers(pkg, h, w)
    layers = pkg.exr_layers(**given)
    path = str(tmp_path / "layers.exr")
    ctx.exr_save(path, layers, attributes={"mcrt:spp": 16, "mcrt:kernel": ""})
    want, want_attrs, want_info = ex.probe().read(path)
    for device in (False, True):
        got, attrs, info = ctx.exr_load(path, device=device)
        assert list(got) == list(want) and attrs == want_attrs and list(attrs) == list(want_attrs)
        for n, v in want.items():
            a = host(got[n])
            if v.dtype == np.uint32:
                np.testing.assert_array_equal(a, v, err_msg=n)
            else:
                np.testing.assert_array_equal(a.view(np.uint64), v.astype(np.float64).view(np.uint64), err_msg=n)   # (no NaN in these frames)
        assert {k: info[k] for k in ("width", "height", "compression", "chunks", "raw_chunks", "file_bytes")} == {k: want_info[k] for k in
                                                                                                                  ("width", "height", "compression", "chunks", "raw_chunks", "file_bytes")}
        back = pkg.exr_unlayer(got)
        assert sorted(back) == sorted(given)
        if device:
            assert back["rgb"].is_cuda and tuple(back["highlights"]["tops"].shape) == (h, w, 4, 3) and back["aov"]["surface"].dtype == torch.int32
        np.testing.assert_array_equal(host(back["rgb"]), np.stack([want[c].astype(np.float64) for c in "RGB"], axis=-1))
        np.testing.assert_array_equal(host(back["highlights"]["tops"])[:, :, 2, 1], want["tops2.G"].astype(np.float64))
        np.testing.assert_array_equal(host(back["aov"]["material"]), given["aov"]["material"])
        np.testing.assert_array_equal(host(back["denoised"]["denoise_dual"]["error"])[..., 2], want["denoise_dual.error.B"].astype(np.float64))
        np.testing.assert_array_equal(host(back["errors"]["relative"]), want["error.rel"].astype(np.float64))
        sub, _, _ = ctx.exr_load(path, channels=["surface.id", "depth.Z", "B"], device=device)
        assert list(sub) == ["surface.id", "depth.Z", "B"]
        np.testing.assert_array_equal(host(sub["surface.id"]), want["surface.id"])
        np.testing.assert_array_equal(host(sub["depth.Z"]), want["depth.Z"].astype(np.float64))


def test_host_program_compares_with_an_openexr_reference(pkg, tmp_path):
    """--compare REF.exr: the lines are those of the raw binary64 reference that holds the same values - R, G, B of the file --exr wrote,
    and FLOAT channels ref.R/G/B of the Python writer with --compare-layer -, but for the name of the reference; a file of another
    size ends the run with status 2."""
    build = __import__("importlib").import_module("monte-carlo-ray-tracer_amd.build")
    exe = build.build_host()
    common = [exe, golden_path(SCENE + ".mcrt"), str(tmp_path / "beauty.f64"), "--width", str(WIDTH), "--height", str(HEIGHT), "--sqrtspp", "2", "--seed", str(SEED)]
    first = str(tmp_path / "first.exr")
    subprocess.run(common + ["--exr", first], check=True, timeout=120, capture_output=True, text=True)
    beauty = np.fromfile(str(tmp_path / "beauty.f64")).reshape(HEIGHT, WIDTH, 3)
    halves = ex.numpy_half_bits(beauty)
    raw = str(tmp_path / "halves.f64")
    rd.widen_half_bits(halves).tofile(raw)
    layer = str(tmp_path / "layer.exr")
    chans = sorted([("ref." + "RGB"[c], rd.FLOAT, halves[..., c].view(np.float16).astype("<f4")) for c in range(3)] + [("R", rd.HALF, np.zeros((HEIGHT, WIDTH), "<f2"))])
    open(layer, "wb").write(rd.variant_file(WIDTH, HEIGHT, chans, rd.ZIPS, origin=(3, -2))[0])

    def lines(reference, *more):
        run = subprocess.run(common + ["--compare", reference] + list(more), check=True, timeout=120, capture_output=True, text=True)
        out = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"compare"')]
        assert len(out) == 1 and out[0].pop("compare") == reference
        assert out[0].pop("kernel_ms") > 0 and out[0].pop("total_ms") > 0   # (the call's times: not the frame's)
        return out[0]

    want = lines(raw)
    assert want["compared"] == WIDTH * HEIGHT and want["differing"] > 0 and 0 < want["mse"] < 1e-3
    assert lines(first) == want
    assert lines(layer, "--compare-layer", "ref") == want
    other = str(tmp_path / "other.exr")
    open(other, "wb").write(rd.variant_file(WIDTH, HEIGHT + 1, [(n, rd.HALF, np.zeros((HEIGHT + 1, WIDTH), "<f2")) for n in "BGR"], rd.ZIP)[0])
    run = subprocess.run(common + ["--compare", other], timeout=120, capture_output=True, text=True)
    assert run.returncode == 2 and "%d x %d" % (WIDTH, HEIGHT + 1) in run.stderr
    run = subprocess.run(common + ["--compare", layer], timeout=120, capture_output=True, text=True)   # (it has R but no G)
    assert run.returncode == 2 and "no channel named G" in run.stderr
