"""The image passes' scratch is one table in the context, a buffer per (family, slot) (csrc/mcrt_internal.hpp ctxPassScratch): what could
go wrong with it is a slot that two calls share by mistake, or a buffer kept from a larger frame that a smaller one reads past its own
end of. So on ONE context the host-pointer forms of all four families run in a row - render_aov, render_pixel_stats, render_highlights
with the statistics' channels, robust_resolve, denoise, frame_noise - at 16 x 12, then at 7 x 5 (every buffer now larger than needed),
then at 16 x 12 again, and every array of every call must be, bit for bit, what the same call gives on a context of its own. Then the
same with a _device form's outputs live in the caller's tensors across host-pointer calls of the other families. Bounds: bits - the
calls are deterministic and neither the context's history nor the size of a buffer is an input to them."""
import numpy as np
import pytest

import test_aov_emulation as aov

pytestmark = pytest.mark.gpu

SCENE, SEED, SQRTSPP = "hexagon_room_diffuse", 20240607, 2
SPP = SQRTSPP * SQRTSPP
SIZES = [(16, 12), (7, 5), (16, 12)]
_fresh = {}


def camera(width, height):
    cam = aov._image(SCENE).camera
    cam.width, cam.height, cam.sqrtspp = width, height, SQRTSPP
    cam.shard_index, cam.shard_count, cam.shard_rows = 0, 1, 0
    return cam


def calls(pkg, cam):
    """The six host-pointer calls in the issue's order: name -> function(ctx, results so far) -> dict of arrays (or of numbers)."""
    stats_channels = tuple(pkg.PIXEL_STATS_CHANNELS)
    return [
        ("render_aov", lambda c, r: c.render_aov(cam, SEED)),
        ("render_pixel_stats", lambda c, r: c.render_pixel_stats(cam, SEED)),
        ("render_highlights", lambda c, r: c.render_highlights(cam, SEED, stats_channels=stats_channels)),
        ("robust_resolve", lambda c, r: c.robust_resolve(r["render_highlights"]["rgb"], r["render_highlights"]["tops"], r["render_highlights"]["level"], SPP)),
        ("denoise", lambda c, r: {"rgb": c.denoise(r["render_pixel_stats"]["rgb"], r["render_aov"])}),
        ("frame_noise", lambda c, r: c.frame_noise(r["render_pixel_stats"]["rgb"], r["render_pixel_stats"]["variance"], SPP)),
    ]


def fresh(pkg, size):
    """Every call on a context of its own (its inputs the results of the calls before it), once per frame size."""
    if size not in _fresh:
        res = {}
        for name, call in calls(pkg, camera(*size)):
            ctx = pkg.Context(0)
            try:
                ctx.upload_image(aov._image(SCENE))
                res[name] = call(ctx, res)
            finally:
                ctx.close()
        assert res["render_pixel_stats"]["variance"].any() and res["render_highlights"]["level"].any() and res["render_aov"]["coverage"].any()
        assert res["denoise"]["rgb"].tobytes() != res["render_pixel_stats"]["rgb"].tobytes() and res["frame_noise"]["noise"] > 0
        _fresh[size] = res
    return _fresh[size]


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    c.upload_image(aov._image(SCENE))
    yield c
    c.close()


def test_one_context_gives_every_call_what_a_fresh_context_gives(pkg, ctx):
    for visit, size in enumerate(SIZES):
        want, res = fresh(pkg, size), {}
        for name, call in calls(pkg, camera(*size)):
            res[name] = call(ctx, want)  # (the inputs are the fresh contexts': a difference shows at the call that made it)
            assert_same(res[name], want[name], "visit %d, %d x %d: %s" % (visit, size[0], size[1], name))


def test_device_outputs_stay_what_they_were_across_host_calls_of_other_families(pkg, ctx):
    import torch
    size = SIZES[0]
    width, height = size
    cam, want = camera(*size), fresh(pkg, size)
    host = dict(calls(pkg, cam))

    def tensors(shapes, dtypes=None):
        t = {k: torch.full((height, width) + s, -9.0, dtype=torch.float64, device="cuda:0") for k, s in shapes.items()}
        for k, dt in (dtypes or {}).items():
            t[k] = torch.full((height, width), 77, dtype=dt, device="cuda:0")
        torch.cuda.synchronize()
        return t

    def ptrs(t, names):
        return {k: t[k].data_ptr() for k in names}

    def then(live, family_result, *names):
        """Host-pointer calls `names` while `live` holds a _device form's outputs; then those outputs against the fresh context's."""
        for name in names:
            assert_same(host[name](ctx, want), want[name], "%s with device outputs live" % name)
        for k, t in live.items():
            assert t.cpu().numpy().tobytes() == family_result[k].tobytes(), (names, k)

    stats_names = tuple(pkg.PIXEL_STATS_CHANNELS)
    live = tensors({k: (3,) for k in ("rgb",) + stats_names})
    ctx.render_pixel_stats_device(cam, SEED, pkg.INTEGRATOR_PATH_TRACER, live["rgb"].data_ptr(), ptrs(live, stats_names))
    then(live, want["render_pixel_stats"], "denoise", "render_aov", "render_highlights", "robust_resolve")

    live = tensors({"rgb": (3,), "tops": (pkg.ROBUST_TOPS, 3), "level": (), **{k: (3,) for k in stats_names}})
    ctx.render_highlights_device(cam, SEED, pkg.INTEGRATOR_PATH_TRACER, live["rgb"].data_ptr(), ptrs(live, ("tops", "level")), ptrs(live, stats_names))
    then(live, want["render_highlights"], "render_pixel_stats", "frame_noise", "denoise", "render_aov")

    shapes = {k: ((n,) if n > 1 else ()) for k, (dt, n) in pkg.AOV_CHANNELS.items() if dt == np.float64}
    ids = {k: torch.int32 for k, (dt, n) in pkg.AOV_CHANNELS.items() if dt != np.float64}
    live = tensors(shapes, ids)
    ctx.render_aov_device(cam, SEED, ptrs(live, live))
    then(live, want["render_aov"], "render_highlights", "robust_resolve", "render_pixel_stats", "denoise", "frame_noise")

    d = {k: torch.from_numpy(want["render_highlights"][k]).to("cuda:0") for k in ("rgb", "tops", "level")}
    live = tensors({"robust": (3,), "removed": (3,)}, {"clamped": torch.int32})
    ctx.robust_resolve_device(width, height, SPP, d["rgb"].data_ptr(), d["tops"].data_ptr(), d["level"].data_ptr(), live["robust"].data_ptr(),
                              live["removed"].data_ptr(), live["clamped"].data_ptr())
    then(live, want["robust_resolve"], "render_aov", "denoise", "render_pixel_stats", "frame_noise")


# The passes that trace camera rays (csrc/mcrt_camera_pass.hpp) all keep the camera-ray records in kPassAov slots 0 .. 4, each sized for
# its own chunk - 76 B a ray - and the second search's rays in slots 0 .. 4 of their own family. So the five of them run in a row on ONE
# context, in small chunks, at the three sizes above, and every array of every call must be, bit for bit, what the same call gives on a
# context of its own that takes the frame in one chunk. Bounds: bits - neither the chunking nor a context's history is an input.
CAMERA_CHUNK_RAYS = 40  # 10 pixels a chunk for the AOV pass and the mattes, 3 for the occlusion pass (12 rays a pixel), 5 for the lighting
                        # passes and the light groups (8 slots a pixel): 20, 64 and 39 chunks at 16 x 12, the last one ragged every time
_fresh_camera = {}


def camera_calls(cam):
    """The five camera-ray passes in the order they run: name -> function(ctx, stats) -> dict of arrays (or of numbers and texts). The
    room is closed, so an unbounded occlusion ray always hits and that frame is all zeros; a sixth call bounds the rays at 2 units, where
    the emulation's ao lies between 1/12 and 1."""
    def matte(c, st):
        res = c.render_matte(cam, SEED, aov=True, stats=st)
        res.update({"aov." + k: v for k, v in res.pop("aov").items()})
        return res
    return [
        ("render_aov", lambda c, st: c.render_aov(cam, SEED, stats=st)),
        ("render_matte", matte),
        ("render_occlusion", lambda c, st: c.render_occlusion(cam, SEED, rays=3, stats=st)),
        ("render_lighting", lambda c, st: c.render_lighting(cam, SEED, stats=st)),
        ("render_light_groups", lambda c, st: {"planes": c.render_light_groups(cam, SEED, stats=st)}),
        ("render_occlusion_near", lambda c, st: c.render_occlusion(cam, SEED, rays=3, max_distance=2.0, stats=st)),
    ]


def fresh_camera(pkg, size):
    """Every camera-ray pass on a context of its own, option MCRT_AOV_CHUNK_RAYS unset (one chunk), once per frame size."""
    if size not in _fresh_camera:
        res = {}
        for name, call in camera_calls(camera(*size)):
            ctx = pkg.Context(0)
            try:
                ctx.upload_image(aov._image(SCENE))
                assert ctx.get_option("MCRT_AOV_CHUNK_RAYS") is None
                res[name] = call(ctx, {})
            finally:
                ctx.close()
        assert res["render_aov"]["coverage"].any() and res["render_matte"]["coverage"].any() and res["render_occlusion_near"]["ao"].any()
        assert res["render_occlusion_near"]["bent_normal"].any() and not res["render_occlusion"]["ao"].any()
        assert res["render_lighting"]["direct"].any() and res["render_light_groups"]["planes"].any()
        _fresh_camera[size] = res
    return _fresh_camera[size]


def test_one_context_gives_every_camera_ray_pass_in_small_chunks_what_a_fresh_context_gives(pkg, ctx):
    try:
        ctx.set_option("MCRT_AOV_CHUNK_RAYS", CAMERA_CHUNK_RAYS)
        for visit, size in enumerate(SIZES):
            want, pixels = fresh_camera(pkg, size), size[0] * size[1]
            # launches per chunk (include/mcrt.h): 3, 3 + 1 with the AOV channels, 5, 5; the light groups' depend on the paths
            launches = {"render_aov": 3 * -(-pixels // 10), "render_matte": 4 * -(-pixels // 10), "render_occlusion": 5 * -(-pixels // 3),
                        "render_occlusion_near": 5 * -(-pixels // 3),
                        "render_lighting": 5 * -(-pixels // 5)}
            for name, call in camera_calls(camera(*size)):
                st = {}
                assert_same(call(ctx, st), want[name], "visit %d, %d x %d: %s" % (visit, size[0], size[1], name))
                assert st["paths"] == pixels * SPP, name
                if name in launches:
                    assert st["kernel_launches"] == launches[name], (name, size)
                else:
                    assert st["kernel_launches"] >= 4 * -(-pixels // 5), (name, size)  # rays, search, begin and resolve in every chunk
    finally:
        ctx.set_option("MCRT_AOV_CHUNK_RAYS", None)
