"""Lighting passes on the GPU (mcrt_render_lighting / mcrt_render_lighting_device): against the host emulation of the same text (built in
tests/test_lighting_emulation.py, which holds it to the oracle's path-traced frames; shared here), and the properties the C ABI
promises - the statistics, a frame that does not depend on chunks or shards, unrequested channels and unowned rows left alone, errors
refused - plus one cross-check that goes round the pass's own kernels: on the constructed scene, whose paths all end by their second
vertex, the render kernels' frame at sqrtspp 1 is (emission + direct) + sky bit for bit. 70 x 13 frames."""
import ctypes as C

import numpy as np
import pytest

import test_aov_emulation as aov
import test_lighting_emulation as lit

pytestmark = pytest.mark.gpu

CHANNELS = lit.CHANNELS
PIXELS, WIDTH, HEIGHT, SEED = lit.PIXELS, lit.WIDTH, lit.HEIGHT, lit.SEED
_state = {}


@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    yield
    for k in [k for k in _state if k[0] == "ctx"]:
        _state.pop(k).close()
    _state.clear()


def context(pkg, scene):
    """One context per scene for the whole module (the scene uploaded once). scene: the name of a scene image, or (floor, bvh) of the
    constructed scene."""
    key = ("ctx", scene)
    if key not in _state:
        ctx = pkg.Context(0)
        ctx.upload_scene(aov._image(scene).scene if isinstance(scene, str) else lit.constructed(*scene).scene)
        _state[key] = ctx
    return _state[key]


def camera(scene, sqrtspp, shard=None):
    return aov.camera(scene, sqrtspp, shard) if isinstance(scene, str) else lit.constructed_camera(sqrtspp, shard)


def gpu_frame(pkg, scene, sqrtspp):
    """The default (one chunk, unsharded) frame of a case, rendered once and shared: (dict channel -> [H,W,3], stats)."""
    key = ("frame", scene, sqrtspp)
    if key not in _state:
        stats = {}
        _state[key] = (context(pkg, scene).render_lighting(camera(scene, sqrtspp), SEED, stats=stats), stats)
    return _state[key]


def constructed_results(pkg, floor, bvh):
    """Everything the tests take of one constructed scene, from a context of its own that is closed again (twelve scenes: they are not
    all kept open): the lighting frames at sqrtspp 1 and 2 with their stats, and the path-traced frame at sqrtspp 1 with its stats."""
    key = ("constructed", floor, bvh)
    if key not in _state:
        ctx = pkg.Context(0)
        try:
            ctx.upload_scene(lit.constructed(floor, bvh).scene)
            res = {}
            for sqrtspp in (1, 2):
                stats = {}
                res[sqrtspp] = (ctx.render_lighting(lit.constructed_camera(sqrtspp), SEED, stats=stats), stats)
            res["beauty"] = ctx.sample_image(lit.constructed_camera(1), SEED, pkg.INTEGRATOR_PATH_TRACER)
        finally:
            ctx.close()
        _state[key] = res
    return _state[key]


def flat(frame):
    return {k: frame[k].reshape(-1, 3) for k in CHANNELS}


def assert_same_bits(a, b, what):
    for k in CHANNELS:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def check_stats(stats, samples, chunks=1):
    assert stats["paths"] == samples and stats["rays"] == 3 * samples and stats["kernel_launches"] == 5 * chunks
    assert stats["kernel_ms"] > 0 and stats["total_ms"] > 0


@pytest.mark.parametrize("sqrtspp", [1, 2])
@pytest.mark.parametrize("floor,bvh", lit.CONSTRUCTED)
def test_constructed_scene_is_the_emulations_bits(pkg, oracle, floor, bvh, sqrtspp):
    frame, stats = constructed_results(pkg, floor, bvh)[sqrtspp]
    check_stats(stats, PIXELS * sqrtspp * sqrtspp)
    what = "GPU %s floor, %s, sqrtspp %d" % (floor, "quaternary SAH" if bvh else "flat", sqrtspp)
    assert_same_bits(flat(frame), lit.constructed_case(floor, bvh, sqrtspp), what)
    lit.check_constructed(flat(frame), floor, bvh, sqrtspp, lit.constructed_oracle(floor, bvh, sqrtspp), what)  # ... and so the oracle's


@pytest.mark.parametrize("scene", list(lit.SCENES))
def test_scene_images_are_the_emulations_bits(pkg, scene):
    frame, stats = gpu_frame(pkg, scene, 1)
    check_stats(stats, PIXELS)
    assert_same_bits(flat(frame), lit.image_case(scene), scene)


@pytest.mark.parametrize("floor,bvh", lit.CONSTRUCTED)
def test_render_kernels_give_the_sum_of_the_parts(pkg, floor, bvh):
    """Round the pass's own kernels: mcrt_render of the constructed scene at sqrtspp 1 - whichever kernel form launchRender picks for it -
    against (emission + direct) + sky of the pass, bit for bit."""
    res = constructed_results(pkg, floor, bvh)
    (beauty, st), (frame, _) = res["beauty"], res[1]
    total = lit.recombined(frame)
    differ = (total.view(np.uint64) != beauty.view(np.uint64)).any(axis=2)
    print("%s floor, bvh %s: render kernel %d, %d of %d pixels differ" % (floor, bvh, st["kernel_id"], differ.sum(), PIXELS))
    assert not differ.any()


def test_lamp_seen_from_below_is_the_emulations_bits_and_the_render_kernels_sum(pkg):
    """The emission channel: the constructed scene's camera under the lamp (test_lighting_emulation holds the emulation to the oracle)."""
    scene = ("lambertian", False)
    ctx = context(pkg, scene)
    for sqrtspp in (1, 2):
        cam = lit.constructed_camera(sqrtspp, under_the_lamp=True)
        frame = ctx.render_lighting(cam, SEED)
        assert_same_bits(flat(frame), lit.emu_frame(lit.constructed(*scene).scene, cam, 1), "under the lamp, sqrtspp %d" % sqrtspp)
        assert (frame["emission"] > 0).any() and (frame["sky"] > 0).any()
    beauty, _ = ctx.sample_image(lit.constructed_camera(1, under_the_lamp=True), SEED, pkg.INTEGRATOR_PATH_TRACER)
    assert lit.recombined(ctx.render_lighting(lit.constructed_camera(1, under_the_lamp=True), SEED)).tobytes() == beauty.tobytes()


def test_frame_does_not_depend_on_chunking(pkg):
    """64 pixels per chunk: 15 chunks, the last one ragged (14 pixels); 64 K slots: one chunk; one slot's worth: one pixel per chunk."""
    scene, sqrtspp = "coffee_maker_qsah", 2
    ctx, cam = context(pkg, scene), camera(scene, sqrtspp)
    whole, stats = gpu_frame(pkg, scene, sqrtspp)
    check_stats(stats, PIXELS * 4)
    assert_same_bits(flat(whole), lit.emu_frame(aov._image(scene).scene, cam, lit.SCENES[scene]), scene + " sqrtspp 2")
    try:
        for chunk_rays, chunks in ((64 * 4 * 2, 15), (65536, 1), (1, 910)):
            ctx.set_option("MCRT_AOV_CHUNK_RAYS", chunk_rays)
            stats = {}
            chunked = ctx.render_lighting(cam, SEED, stats=stats)
            check_stats(stats, PIXELS * 4, chunks)
            assert_same_bits(chunked, whole, "MCRT_AOV_CHUNK_RAYS=%d" % chunk_rays)
    finally:
        ctx.set_option("MCRT_AOV_CHUNK_RAYS", None)


@pytest.mark.parametrize("count", [1, 2, 3])
def test_shards_reassemble_to_the_frame_and_leave_other_rows_alone(pkg, count):
    """shard_rows 2 over 13 rows, dealt round robin (the last group ragged). Device form: packed owned rows; host form: the full frame,
    rows of other shards untouched."""
    import torch
    scene, sqrtspp = "coffee_maker_qsah", 2
    ctx = context(pkg, scene)
    whole, _ = gpu_frame(pkg, scene, sqrtspp)
    glued = {k: np.zeros_like(whole[k]) for k in CHANNELS}
    seen = 0
    for index in range(count):
        cam = camera(scene, sqrtspp, (index, count, 2))
        rows = pkg.shard_rows(cam)
        seen += len(rows)
        dev = {k: torch.full((len(rows), WIDTH, 3), -1, dtype=torch.float64, device="cuda:0") for k in CHANNELS}
        torch.cuda.synchronize()
        stats = ctx.render_lighting_device(cam, SEED, {k: v.data_ptr() for k, v in dev.items()})
        check_stats(stats, len(rows) * WIDTH * 4)
        for k, v in dev.items():
            glued[k][rows] = v.cpu().numpy()
        out = {k: np.full_like(whole[k], 7) for k in CHANNELS}  # host form into sentinel-filled full frames
        got = ctx.render_lighting(cam, SEED, out=out)
        others = np.setdiff1d(np.arange(HEIGHT), rows)
        for k in CHANNELS:
            assert got[k][rows].tobytes() == whole[k][rows].tobytes(), "shard %d %s" % (index, k)
            assert (got[k][others] == 7).all(), "shard %d wrote rows it does not own (%s)" % (index, k)
    assert seen == HEIGHT
    assert_same_bits(glued, whole, "%d shards reassembled" % count)


def test_unrequested_channels_are_left_as_they_were(pkg):
    import torch
    scene, sqrtspp = ("ggx", True), 2
    ctx, cam = context(pkg, scene), camera(scene, sqrtspp)
    whole, _ = gpu_frame(pkg, scene, sqrtspp)
    part = ctx.render_lighting(cam, SEED, channels=["light"])
    assert sorted(part) == ["light"] and part["light"].tobytes() == whole["light"].tobytes()
    part = ctx.render_lighting(cam, SEED, channels=["unoccluded", "sky"])
    assert sorted(part) == ["sky", "unoccluded"] and part["sky"].tobytes() == whole["sky"].tobytes() and part["unoccluded"].tobytes() == whole["unoccluded"].tobytes()
    # device form: one allocation of five frames, only the third (direct's place) handed over
    block = torch.full((5, HEIGHT, WIDTH, 3), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_lighting_device(cam, SEED, {"direct": block[2].data_ptr(), "light": None})
    got = block.cpu().numpy()
    assert got[2].tobytes() == whole["direct"].tobytes() and (got[:2] == -1).all() and (got[3:] == -1).all()


def test_calls_are_refused_without_a_scene_while_a_render_is_pending_and_on_bad_parameters(pkg):
    import torch
    scene = ("lambertian", False)
    cam = camera(scene, 1)
    buf = torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    fresh = pkg.Context(0)
    try:
        with pytest.raises(pkg.McrtError, match=r"\(-4\)"):
            fresh.render_lighting(cam, SEED)
        with pytest.raises(pkg.McrtError, match=r"\(-4\)"):
            fresh.render_lighting_device(cam, SEED, {"light": buf.data_ptr()})
    finally:
        fresh.close()
    ctx = context(pkg, scene)
    with pytest.raises(pkg.McrtError, match="no channel"):
        ctx.render_lighting(cam, SEED, channels=[])
    assert pkg.lib().mcrt_render_lighting_device(ctx._h, C.byref(cam), SEED, C.byref(pkg.LightingBuffers()), None) == -1
    assert b"no channel" in pkg.lib().mcrt_last_error(ctx._h)
    with pytest.raises(pkg.McrtError, match="shard_index"):
        ctx.render_lighting(camera(scene, 1, (3, 3, 2)), SEED)
    with pytest.raises(pkg.McrtError, match="shard_index"):
        ctx.render_lighting_device(camera(scene, 1, (5, 2, 1)), SEED, {"light": buf.data_ptr()})
    ctx.render_device(cam, SEED, pkg.INTEGRATOR_PATH_TRACER, buf.data_ptr())
    try:
        with pytest.raises(pkg.McrtError, match="in flight"):
            ctx.render_lighting(cam, SEED)
        with pytest.raises(pkg.McrtError, match="in flight"):
            ctx.render_lighting_device(cam, SEED, {"light": buf.data_ptr()})
    finally:
        ctx.render_finish()
    frame = ctx.render_lighting(cam, SEED, channels=["light"])  # ... and served again once the render was collected
    assert frame["light"].tobytes() == gpu_frame(pkg, scene, 1)[0]["light"].tobytes()


def test_exr_file_of_the_layers_round_trips(pkg, tmp_path):
    """exr_layers(lighting=...) -> exr_save -> exr_load: the fifteen channels under their names, every one the HALF (or, asked for, FLOAT)
    rounding of its binary64 word, widened exactly; exr_unlayer gives the dict back."""
    scene, sqrtspp = ("ggx", True), 2
    ctx = context(pkg, scene)
    frame, _ = gpu_frame(pkg, scene, sqrtspp)
    names = ["lighting.%s.%s" % (k, c) for k in CHANNELS for c in "RGB"]
    path = str(tmp_path / "lighting.exr")
    ctx.exr_save(path, pkg.exr_layers(lighting=frame, pixel_types={"lighting.unoccluded": "float"}))
    channels, _, info = ctx.exr_load(path)
    assert sorted(channels) == sorted(names) and (info["width"], info["height"]) == (WIDTH, HEIGHT)
    for k in CHANNELS:
        narrow = np.float32 if k == "unoccluded" else np.float16
        for i, c in enumerate("RGB"):
            np.testing.assert_array_equal(channels["lighting.%s.%s" % (k, c)], frame[k][..., i].astype(narrow).astype(np.float64), err_msg=k + "." + c)
    back = pkg.exr_unlayer(channels)
    assert sorted(back) == ["lighting"] and sorted(back["lighting"]) == sorted(CHANNELS)
    assert np.array_equal(back["lighting"]["direct"], frame["direct"].astype(np.float16).astype(np.float64))
    assert (frame["direct"] > 0).any() and (frame["unoccluded"] > frame["light"]).any()


def test_host_program_writes_the_bindings_arrays_and_the_exr_channels(pkg, tmp_path):
    import subprocess
    from conftest import golden_path
    build = __import__("importlib").import_module("monte-carlo-ray-tracer_amd.build")
    exe = build.build_host()
    scene, sqrtspp, seed = "coffee_maker_qsah", 2, 77
    prefix, exr = str(tmp_path / "lighting"), str(tmp_path / "lighting.exr")
    subprocess.run([exe, golden_path(scene + ".mcrt"), str(tmp_path / "beauty.f64"), "--width", str(WIDTH), "--height", str(HEIGHT), "--sqrtspp", str(sqrtspp),
                    "--seed", str(seed), "--lighting", prefix, "--exr", exr], check=True, timeout=120, capture_output=True)
    ctx = context(pkg, scene)
    frame = ctx.render_lighting(camera(scene, sqrtspp), seed)
    for k in CHANNELS:
        assert open("%s.%s.f64" % (prefix, k), "rb").read() == frame[k].tobytes(), k
    channels, _, _ = ctx.exr_load(exr)
    names = ["lighting.%s.%s" % (k, c) for k in CHANNELS for c in "RGB"]
    assert sorted(n for n in channels if n.startswith("lighting")) == sorted(names)
    again = str(tmp_path / "layers.exr")
    ctx.exr_save(again, pkg.exr_layers(lighting=frame))
    back, _, _ = ctx.exr_load(again)
    for n in names:  # the same file from the binding's layers
        assert back[n].tobytes() == channels[n].tobytes(), n
