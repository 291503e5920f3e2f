"""Accumulated rendering on the GPU (mcrt_frame_merge*, mcrt_render_converged*): the merge kernel against the host emulation of its text
(tests/test_accumulate_emulation.py holds it, with the numpy restatement of include/mcrt.h), host form and device form, in place and
into buffers of its own, groups left out left alone; the stopping loop against the same renders merged by hand - one batch is the
render itself, three batches are three renders at consecutive seeds merged through frame_merge, the reported trace is frame_noise of
those frames, a target inside the trace stops where the trace says -; refusals; and one case through the wavefront pipeline.

Bounds: bits everywhere. The kernel and the emulation run one text (csrc/mcrt_accumulate.hpp), FP64 + - * / compare select in one
order, uncontracted on both sides; the loop is compared with the library's own calls made by hand, which run the same kernels on the
same inputs."""
import re

import numpy as np
import pytest

import test_accumulate_emulation as acc
import test_aov_emulation as aov
import test_pixel_stats_emulation as ps
from conftest import golden_path

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, SEED = ps.WIDTH, ps.HEIGHT, ps.SEED
EVERY = tuple(acc.CHANNELS)  # rgb, variance, half_a, half_b, tops, level
SCENE = "hexagon_room_diffuse"
_state = {}

SPLATS = (": a frame whose film splats (a reconstruction filter, or a box of another radius) keeps no samples: there is nothing to take "
          "the %s of")


def refused(pkg, code, text):
    """The call fails with `code` and, as the whole message of the library, `text`."""
    return pytest.raises(pkg.McrtError, match=r"\(%d\): %s$" % (code, re.escape(text)))


@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    yield
    for k in [k for k in _state if isinstance(k, str)]:
        _state.pop(k).close()
    _state.clear()


def context(pkg, scene=SCENE):
    if scene not in _state:
        ctx = pkg.Context(0)
        ctx.upload_image(aov._image(scene))
        _state[scene] = ctx
    return _state[scene]


def camera(scene=SCENE, sqrtspp=4, shard=None):
    cam = aov._image(scene).camera
    cam.width, cam.height, cam.sqrtspp = WIDTH, HEIGHT, sqrtspp
    cam.shard_index, cam.shard_count, cam.shard_rows = shard if shard else (0, 1, 0)
    return cam


def same_bits(a, b, keys, what=""):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def to_device(d):
    import torch
    dev = {k: torch.from_numpy(np.array(v, dtype=np.float64, order="C")).to("cuda:0") for k, v in d.items()}
    torch.cuda.synchronize()
    return dev


def pointers(dev):
    return {k: v.data_ptr() for k, v in dev.items()}


@pytest.mark.parametrize("n_a,n_b", acc.COUNT_PAIRS)
@pytest.mark.parametrize("pixels", acc.PIXEL_COUNTS)
def test_frame_merge_is_the_emulation(pkg, pixels, n_a, n_b):
    import torch
    ctx = context(pkg)
    A, B, _ = acc.hand_made(pixels, n_a, n_b)
    names = acc.wanted_channels(n_a, n_b)
    want = acc.emu_frame_merge(A, n_a, B, n_b)
    st = {}
    got = ctx.frame_merge(A, n_a, B, n_b, stats=st)
    assert sorted(got) == sorted(names) and st["kernel_launches"] == 1 and st["kernel_id"] == pkg.KERNEL_NONE
    same_bits(got, want, names, "host form")
    # the device form into buffers of its own, then in place: it equals the host form
    da, db = to_device(A), to_device(B)
    out = {k: torch.full((pixels,) + acc.CHANNELS[k], -9.0, dtype=torch.float64, device="cuda:0") for k in names}
    torch.cuda.synchronize()
    st = ctx.frame_merge_device(pixels, pointers(da), n_a, pointers(db), n_b, pointers(out))
    assert st["kernel_launches"] == 1
    for k in names:
        assert out[k].cpu().numpy().tobytes() == got[k].tobytes(), k
        assert da[k].cpu().numpy().tobytes() == A[k].tobytes(), k  # (A left alone)
    ctx.frame_merge_device(pixels, pointers(da), n_a, pointers(db), n_b)
    for k in names:
        assert da[k].cpu().numpy().tobytes() == got[k].tobytes(), k
        assert db[k].cpu().numpy().tobytes() == B[k].tobytes(), k


def test_a_group_left_out_is_left_alone_and_the_host_form_merges_in_place(pkg):
    import torch
    ctx = context(pkg)
    pixels, n_a, n_b = 257, 16, 25
    A, B, want = acc.hand_made(pixels, n_a, n_b)
    da, db = to_device(A), to_device(B)
    for group, names in acc.GROUPS.items():
        out = {k: torch.full((pixels,) + acc.CHANNELS[k], -9.0, dtype=torch.float64, device="cuda:0") for k in EVERY}
        torch.cuda.synchronize()
        ctx.frame_merge_device(pixels, pointers(da), n_a, pointers(db), n_b, {k: out[k].data_ptr() for k in names})
        for k in EVERY:
            a = out[k].cpu().numpy()
            assert a.tobytes() == want[k].tobytes() if k in names else (a == -9.0).all(), (group, k)
    mean_only = ctx.frame_merge({"rgb": A["rgb"]}, n_a, {"rgb": B["rgb"]}, n_b)
    assert list(mean_only) == ["rgb"] and mean_only["rgb"].tobytes() == want["rgb"].tobytes()
    mine = {k: v.copy() for k, v in A.items()}
    got = ctx.frame_merge(mine, n_a, B, n_b, in_place=True)
    for k in EVERY:
        assert got[k] is mine[k] and mine[k].tobytes() == want[k].tobytes(), k


def test_frame_merge_refusals_name_their_cause_and_leave_the_context_usable(pkg):
    import torch
    ctx = context(pkg)
    A, B, want = acc.hand_made(63, 16, 16)
    d = torch.zeros((63, 4, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    p = d.data_ptr()
    every = {k: p for k in EVERY}
    frame = torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device(camera(), SEED, pkg.INTEGRATOR_PATH_TRACER, frame.data_ptr())
    try:
        with pytest.raises(pkg.McrtError, match=r"\(-1\).*in flight"):
            ctx.frame_merge(A, 16, B, 16)
        with pytest.raises(pkg.McrtError, match=r"\(-1\).*in flight"):
            ctx.frame_merge_device(63, every, 16, every, 16)
    finally:
        ctx.render_finish()
    for n_a, n_b in ((0, 16), (16, 0), (0xFFFFFFF0, 16)):
        with pytest.raises(pkg.McrtError, match=r"\(-1\).*(count|uint32_t)"):
            ctx.frame_merge_device(63, every, n_a, every, n_b)
    for pixels in (0, 1 << 32):
        with pytest.raises(pkg.McrtError, match=r"\(-1\).*pixels"):
            ctx.frame_merge_device(pixels, every, 16, every, 16)
    for n_a, n_b in ((15, 16), (16, 9)):
        with pytest.raises(pkg.McrtError, match=r"\(-7\).*16 samples"):
            ctx.frame_merge_device(63, every, n_a, every, n_b)
        with pytest.raises(pkg.McrtError, match=r"\(-7\).*16 samples"):
            ctx.frame_merge(A, n_a, B, n_b)
    for out in ({"variance": p}, {"rgb": p, "half_a": p}, {"tops": p}, {}):
        with pytest.raises(pkg.McrtError, match=r"\(-1\)"):
            ctx.frame_merge_device(63, every, 16, every, 16, out)
    for k in ("rgb", "variance", "half_b", "level"):
        with pytest.raises(pkg.McrtError, match=r"\(-1\).*NULL"):
            ctx.frame_merge_device(63, {c: v for c, v in every.items() if c != k}, 16, every, 16, every)
    same_bits(ctx.frame_merge(A, 16, B, 16), want, EVERY)


def batches(pkg, scene=SCENE, kernel=None, count=3):
    """`count` render_highlights of the scene at SEED, SEED + 1, ... with every statistics channel, their frames merged by hand through
    frame_merge, and frame_noise of each merged frame: computed once -> (list of renders, list of merged summaries, list of
    frame_noise dicts, list of stats)."""
    key = ("batches", scene, kernel)
    if key not in _state:
        ctx, cam = context(pkg, scene), camera(scene)
        ctx.set_option("MCRT_KERNEL", kernel)
        try:
            renders, stats = [], []
            for j in range(count):
                st = {}
                renders.append(ctx.render_highlights(cam, SEED + j, stats_channels=pkg.PIXEL_STATS_CHANNELS, stats=st))
                stats.append(st)
        finally:
            ctx.set_option("MCRT_KERNEL", None)
        merged = [renders[0]]
        for j in range(1, count):
            merged.append(ctx.frame_merge(merged[-1], 16 * j, renders[j], 16))
        noise = [ctx.frame_noise(m["rgb"], m["variance"], 16 * (j + 1)) for j, m in enumerate(merged)]
        _state[key] = (renders, merged, noise, stats)
    return _state[key]


def test_a_target_met_at_once_gives_one_batch_the_render_itself(pkg):
    renders, _, noise, stats = batches(pkg)
    st = {}
    got = context(pkg).render_converged(camera(), SEED, 1e9, 0, channels=pkg.PIXEL_STATS_CHANNELS + tuple(pkg.HIGHLIGHT_CHANNELS), stats=st)
    r = got["result"]
    assert (r["batches"], r["spp"]) == (1, 16) and r["relative_error"] == [noise[0]["relative_error"]] and r["final"] == noise[0]
    same_bits(got, renders[0], EVERY)
    assert (got["variance"] > 0).any() and got["tops"].any()
    assert st["paths"] == stats[0]["paths"] and st["kernel_id"] == stats[0]["kernel_id"] == pkg.KERNEL_FLAT
    assert st["kernel_launches"] == stats[0]["kernel_launches"]


def test_no_target_runs_to_max_spp_and_equals_the_renders_merged_by_hand(pkg):
    import torch
    renders, merged, noise, stats = batches(pkg)
    ctx, cam = context(pkg), camera()
    st = {}
    got = ctx.render_converged(cam, SEED, 0.0, 48, channels=pkg.PIXEL_STATS_CHANNELS + tuple(pkg.HIGHLIGHT_CHANNELS), stats=st)
    r = got["result"]
    assert (r["batches"], r["spp"]) == (3, 48)
    same_bits(got, merged[2], EVERY)
    assert not np.array_equal(got["rgb"], renders[0]["rgb"])
    assert r["relative_error"] == [n["relative_error"] for n in noise] and r["final"] == noise[2]
    assert r["relative_error"][0] > r["relative_error"][1] > r["relative_error"][2] > 0
    assert st["paths"] == sum(s["paths"] for s in stats) and st["rays"] == sum(s["rays"] for s in stats)
    assert st["kernel_launches"] == sum(s["kernel_launches"] for s in stats) + 2 and st["kernel_id"] == pkg.KERNEL_FLAT
    # a max_spp that is no multiple of the batch: the batch that would exceed it is not rendered
    assert ctx.render_converged(cam, SEED, 0.0, 47)["result"]["spp"] == 32
    # channels left out: the frame and the variance are the same bits, nothing else is delivered
    few = ctx.render_converged(cam, SEED, 0.0, 48)
    assert sorted(few) == ["result", "rgb", "variance"]
    same_bits(few, merged[2], ("rgb", "variance"))
    # the device form on full frames equals the host form; a channel not named is left alone
    dev = {k: torch.full((HEIGHT, WIDTH) + acc.CHANNELS[k], -9.0, dtype=torch.float64, device="cuda:0") for k in EVERY}
    torch.cuda.synchronize()
    res, dst = ctx.render_converged_device(cam, SEED, pkg.INTEGRATOR_PATH_TRACER, dev["rgb"].data_ptr(), 0.0, 48,
                                           stats_pointers={"variance": dev["variance"].data_ptr(), "half_b": dev["half_b"].data_ptr()},
                                           pointers={"tops": dev["tops"].data_ptr()})
    assert res == r and dst["paths"] == st["paths"]
    for k in ("rgb", "variance", "half_b", "tops"):
        assert dev[k].cpu().numpy().tobytes() == merged[2][k].tobytes(), k
    assert (dev["half_a"] == -9.0).all() and (dev["level"] == -9.0).all()


def test_a_target_inside_the_trace_stops_where_the_trace_says(pkg):
    _, merged, noise, _ = batches(pkg)
    e = [n["relative_error"] for n in noise]
    target = 0.5 * (e[0] + e[1])
    assert e[1] < target < e[0]
    got = context(pkg).render_converged(camera(), SEED, target, 1024)
    assert (got["result"]["batches"], got["result"]["spp"]) == (2, 32) and got["result"]["final"] == noise[1]
    same_bits(got, merged[1], ("rgb", "variance"))
    # min_batches holds the loop open past a target already met
    held = context(pkg).render_converged(camera(), SEED, 1e9, 1024, min_batches=3)
    assert held["result"]["batches"] == 3
    same_bits(held, merged[2], ("rgb", "variance"))


def test_one_sample_batches_run_twice_at_least(pkg):
    ctx, cam = context(pkg), camera(sqrtspp=1)
    got = ctx.render_converged(cam, SEED, 1e9, 1024)
    r = got["result"]
    assert (r["batches"], r["spp"]) == (2, 2) and r["relative_error"][0] == 0.0 and r["relative_error"][1] > 0.0
    a, b = ctx.render_pixel_stats(cam, SEED), ctx.render_pixel_stats(cam, SEED + 1)
    assert not a["variance"].any()
    want = ctx.frame_merge(a, 1, b, 1)
    same_bits(got, want, ("rgb", "variance"))
    assert (got["variance"] > 0).any()


def test_render_converged_refusals(pkg, manifest):
    ctx = context(pkg)
    what = "mcrt_render_converged_device"
    with refused(pkg, -7, what + ": a sharded camera - the summary needs the whole frame: merge per shard with mcrt_frame_merge_device"):
        ctx.render_converged(camera(shard=(0, 3, 5)), SEED, 0.0, 48)
    with refused(pkg, -7, what + ": highlights need 16 samples per batch"):
        ctx.render_converged(camera(sqrtspp=3), SEED, 0.0, 48, channels=("variance", "tops"))
    assert ctx.render_converged(camera(sqrtspp=3), SEED, 0.0, 18)["result"]["spp"] == 18  # (without highlights 9 spp batches are fine)
    with refused(pkg, -1, what + ": max_spp is less than one batch"):
        ctx.render_converged(camera(), SEED, 0.0, 15)
    for bad in (-1.0, float("nan"), float("inf")):
        with refused(pkg, -1, what + ": target_relative_error must be finite and not negative"):
            ctx.render_converged(camera(), SEED, bad, 48)
    film = pkg.SceneImage(golden_path(manifest["cases"]["film_mitchell"]["image"]))
    fctx = pkg.Context(0)
    try:
        fctx.upload_image(film)
        fcam = film.camera
        fcam.width, fcam.height, fcam.sqrtspp = WIDTH, HEIGHT, 4
        with refused(pkg, -7, "mcrt_render_pixel_stats_device" + SPLATS % "statistics"):  # (the batch's own entry point names itself)
            fctx.render_converged(fcam, SEED, 0.0, 48)
        with refused(pkg, -7, "mcrt_render_highlights_device" + SPLATS % "highlights"):
            fctx.render_converged(fcam, SEED, 0.0, 48, channels=("variance", "level"))
    finally:
        fctx.close()
    fresh = pkg.Context(0)
    try:
        with refused(pkg, -4, what + " before mcrt_upload_scene"):
            fresh.render_converged(camera(), SEED, 0.0, 48)
    finally:
        fresh.close()
    assert ctx.render_converged(camera(), SEED, 1e9, 48)["result"]["batches"] == 1  # the context is still usable


def test_the_loop_through_the_wavefront_pipeline(pkg):
    scene = "coffee_maker_qsah"
    renders, merged, noise, stats = batches(pkg, scene, "wf", count=2)
    assert stats[0]["kernel_id"] == pkg.KERNEL_WAVEFRONT
    ctx = context(pkg, scene)
    ctx.set_option("MCRT_KERNEL", "wf")
    try:
        st = {}
        got = ctx.render_converged(camera(scene), SEED, 0.0, 32, channels=pkg.PIXEL_STATS_CHANNELS + tuple(pkg.HIGHLIGHT_CHANNELS), stats=st)
    finally:
        ctx.set_option("MCRT_KERNEL", None)
    assert st["kernel_id"] == pkg.KERNEL_WAVEFRONT and st["paths"] == stats[0]["paths"] + stats[1]["paths"]
    assert (got["result"]["batches"], got["result"]["spp"]) == (2, 32)
    assert got["result"]["relative_error"] == [n["relative_error"] for n in noise]
    same_bits(got, merged[1], EVERY)
