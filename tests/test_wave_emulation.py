"""The wave-cooperative photon search of the product (csrc/mcrt_waveknn.hpp) on the HOST: the device source unchanged, one wavefront
emulated as 64 fibers that meet at every cross-lane operation (tests/emu/wave_emu.hpp: ballots, readlane, DPP moves with their row
masks and bound_ctrl, shuffles, wave barriers; LDS as ordinary memory). What the GPU tier checks through the C ABI
(test_knn_exact, test_knn_large_k) is checked here without a GPU: the reference's own k-NN vectors, the oracle's search for other k,
both widths of the candidate buffer, and the frontier's spill list in both of its forms (state in registers / in LDS)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import golden_path


def _search(wave_emu, desc, pts, k, rows, spill_mode, upload_k=50):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(pts)
    cnt = np.zeros(n, dtype=np.uint32)
    idx = np.zeros((n, k), dtype=np.uint32)
    d2 = np.zeros((n, k))
    overflow = np.zeros(1, dtype=np.uint32)
    rc = wave_emu.wemu_knn(C.byref(desc), upload_k, n, pts.ctypes.data, k, rows, spill_mode, cnt.ctypes.data, idx.ctypes.data, d2.ctypes.data,
                           overflow.ctypes.data)
    assert rc == 0
    return cnt, idx, d2, int(overflow[0])


def test_wave_search_on_the_host_gives_the_reference_vectors(pkg, wave_emu, manifest):
    case = manifest["cases"]["hexagon_room_pm"]
    img = pkg.SceneImage(golden_path(case["image"]))
    k = img.param("k_nearest_photons")
    d = golden_path(case["kat"])
    for which, tag in ((0, "g"), (1, "c")):
        pts = np.fromfile(os.path.join(d, "knn_%s_points.f64" % tag)).reshape(-1, 3)[:400]
        cnt, idx, d2, overflow = _search(wave_emu, img.photons(which), pts, k, 4, 1, upload_k=k)
        assert overflow == 0
        np.testing.assert_array_equal(cnt, np.fromfile(os.path.join(d, "knn_%s_count.u32" % tag), dtype=np.uint32)[:400])
        np.testing.assert_array_equal(idx, np.fromfile(os.path.join(d, "knn_%s_index.u32" % tag), dtype=np.uint32).reshape(-1, k)[:400])
        np.testing.assert_array_equal(d2, np.fromfile(os.path.join(d, "knn_%s_d2.f64" % tag)).reshape(-1, k)[:400])


@pytest.mark.parametrize("k,rows", [(1, 4), (7, 4), (64, 4), (128, 4), (129, 16), (300, 16), (768, 16), (50, 16)])
def test_wave_search_on_the_host_equals_the_oracle(pkg, wave_emu, oracle, manifest, k, rows):
    case = manifest["cases"]["hexagon_room_pm"]
    img = pkg.SceneImage(golden_path(case["image"]))
    d = golden_path(case["kat"])
    for which, tag in ((0, "g"), (1, "c")):
        pts = np.fromfile(os.path.join(d, "knn_%s_points.f64" % tag)).reshape(-1, 3)[400:440]
        for mode in (1, 2):  # the spill list's state in registers / in LDS (unused here: same answers)
            cnt, idx, d2, overflow = _search(wave_emu, img.photons(which), pts, k, rows, mode)
            ocnt, oidx, od2 = oracle.knn(img.photons(which), pts, k)
            assert overflow == 0
            np.testing.assert_array_equal(cnt, ocnt)
            np.testing.assert_array_equal(d2, od2)
            np.testing.assert_array_equal(idx, oidx)


@pytest.mark.parametrize("count", [1, 49, 50, 51, 300])
def test_wave_search_on_the_host_small_maps(pkg, wave_emu, count):
    rng = np.random.default_rng(count)
    lo, hi = np.array([-3.0, -2.0, -1.0]), np.array([5.0, 2.0, 4.0])
    ph = np.zeros((count, 8), dtype=np.float32)
    ph[:, 3:6] = (lo + rng.random((count, 3)) * (hi - lo)).astype(np.float32)
    m = pkg.PhotonMap(ph, lo.tolist(), hi.tolist(), 200)
    pts = lo + rng.random((40, 3)) * (hi - lo)
    pos = np.ctypeslib.as_array(m.desc.photons, (count, 8))[:, 3:6].astype(np.float64)
    dd = pts[:, None, :] - pos[None, :, :]
    d2_all = (dd[:, :, 0] * dd[:, :, 0] + dd[:, :, 1] * dd[:, :, 1]) + dd[:, :, 2] * dd[:, :, 2]
    for k in (1, 50):
        want = np.sort(d2_all, axis=1)[:, :min(k, count)]
        cnt, idx, d2, overflow = _search(wave_emu, m.desc, pts, k, 4, 1)
        assert overflow == 0 and np.all(cnt == min(k, count))
        np.testing.assert_array_equal(d2[:, :min(k, count)], want)
        assert np.all(np.isinf(d2[:, min(k, count):])) and np.all(idx[:, min(k, count):] == 0xFFFFFFFF)
    m.close()


@pytest.mark.parametrize("leaf,k,rows,upload_k", [(1, 64, 4, 1), (2, 100, 4, 2), (4, 300, 16, 16)])
def test_frontier_spill_list_on_the_host(pkg, wave_emu, leaf, k, rows, upload_k):
    """Leaves far smaller than k, and record lists built for a far smaller k than the one asked for (upload_k: only octants of up to
    that many photons are scanned whole): more octants lie within the bound at once than the 128 frontier entries of a wave's
    registers. Without the list in memory the search reports an overflow; with it - its state kept in registers or in LDS - the
    brute-force answer."""
    rng = np.random.default_rng(leaf * 1000 + k)
    count = 6000
    lo, hi = np.array([-3.0, -2.0, -1.0]), np.array([5.0, 2.0, 4.0])
    ph = np.zeros((count, 8), dtype=np.float32)
    ph[:, 3:6] = (lo + rng.random((count, 3)) * (hi - lo)).astype(np.float32)
    m = pkg.PhotonMap(ph, lo.tolist(), hi.tolist(), leaf)
    pts = lo + rng.random((24, 3)) * (hi - lo)
    pos = np.ctypeslib.as_array(m.desc.photons, (count, 8))[:, 3:6].astype(np.float64)
    dd = pts[:, None, :] - pos[None, :, :]
    d2_all = (dd[:, :, 0] * dd[:, :, 0] + dd[:, :, 1] * dd[:, :, 1]) + dd[:, :, 2] * dd[:, :, 2]
    want = np.sort(d2_all, axis=1)[:, :k]
    _, _, _, overflow = _search(wave_emu, m.desc, pts, k, rows, 0, upload_k=upload_k)
    assert overflow == 1  # the case is a real one: 128 entries do not hold this frontier
    for mode in (1, 2):
        cnt, idx, d2, overflow = _search(wave_emu, m.desc, pts, k, rows, mode, upload_k=upload_k)
        assert overflow == 0 and np.all(cnt == k)
        np.testing.assert_array_equal(d2, want)
        np.testing.assert_array_equal(d2_all[np.arange(len(pts))[:, None], idx], want)
    m.close()


@pytest.mark.parametrize("name", ["coffee_maker_qsah", "coffee_maker_bsah", "hexagon_room", "quadric", "metals"])
def test_shared_leaf_walk_on_the_host_equals_the_oracle(pkg, wave_walk_emu, oracle, manifest, name):
    """traceWalkShared (csrc/mcrt_sharedleaf.hpp: the trace kernel's walk - deferred leaves tested by the whole wave, items numbered by
    a prefix sum and pulled with ds_bpermute, one pop site, the stack's top cached in registers) and traceWalkQ, 64 rays per emulated
    wavefront, full waves and waves with lanes that carry no ray: t, surface and uv of the oracle's Scene::intersect bit for bit,
    on the reference's KAT rays and on random rays (some with zero direction components: the exact-record walk)."""
    case = manifest["cases"].get(name)
    if case is None:
        pytest.skip("no such golden case")
    img = pkg.SceneImage(golden_path(case["image"]))
    sc = img.scene
    rng = np.random.default_rng(11)
    lo, hi = np.array(sc.bb_min[:]), np.array(sc.bb_max[:])
    n = 1500
    start = lo + (hi - lo) * rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:40, rng.integers(0, 3)] = 0.0
    d[:40] /= np.linalg.norm(d[:40], axis=1, keepdims=True)
    kat = os.path.join(golden_path(case["kat"]), "isect_rays.f64") if case.get("kat") else ""
    if kat and os.path.exists(kat):
        rays = np.fromfile(kat).reshape(-1, 6)[:1500]
        start, d = np.vstack([start, rays[:, :3]]), np.vstack([d, rays[:, 3:]])
    start, d = np.ascontiguousarray(start), np.ascontiguousarray(d)
    n = start.shape[0]
    t0, s0, uv0, _ = oracle.intersect(img, start, d)
    for which, holes in ((0, 0), (0, 3), (1, 0)):
        t, surf, uv = np.full(n, np.nan), np.zeros(n, dtype=np.uint32), np.zeros((n, 2))
        rc = wave_walk_emu.wemu_intersect(C.byref(sc), n, start.ctypes.data, d.ctypes.data, which, holes, t.ctypes.data, surf.ctypes.data, uv.ctypes.data)
        assert rc == 0
        hit = s0 != 0xFFFFFFFF
        np.testing.assert_array_equal(surf, s0, err_msg="walk %d holes %d" % (which, holes))
        np.testing.assert_array_equal(t[hit], t0[hit])
        np.testing.assert_array_equal(uv[hit], uv0[hit])


@pytest.mark.parametrize("k,rows", [(50, 4), (200, 16)])
def test_wave_radiance_estimate_on_the_host(pkg, wave_walk_emu, manifest, k, rows):
    """renderKernelPM's part 2 on the emulated wavefront - the asking lanes' Interactions staged in memory, one search per request by
    the whole wave, the record read back into 'scalar registers' (readfirstlane), the k photons evaluated by k lanes, the sums by the
    DPP reduction (waveSumD) - against the per-lane estimate functions of the legacy kernel (estimateCausticRadiance /
    estimateGlobalRadiance) at the first hits of a small frame's camera rays. Same photons, same per-photon arithmetic; only the
    order of the FP64 sum differs: 1e-12."""
    from conftest import camera_for
    case = manifest["cases"]["hexagon_room_pm"]
    img = pkg.SceneImage(golden_path(case["image"]))
    cam = camera_for(img, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 32, 18, 1
    n = cam.width * cam.height
    lane, wave = np.zeros((n, 6)), np.zeros((n, 6))
    valid = np.zeros(n, dtype=np.uint8)
    rc = wave_walk_emu.wemu_estimate(C.byref(img.scene), C.byref(img.photons(0)), C.byref(img.photons(1)), k, rows, C.byref(cam),
                                     manifest["seed"], n, lane.ctypes.data, wave.ctypes.data, valid.ctypes.data)
    assert rc == 0
    v = valid != 0
    assert v.sum() > n // 2 and (lane[v] != 0).any()
    rel = np.abs(wave[v] - lane[v]) / np.maximum(np.abs(lane[v]), 1e-3)
    print("estimates at %d hits, k = %d: max rel %.3e between the wave's and the lane's sums" % (v.sum(), k, rel.max()))
    assert rel.max() <= 1e-12
    assert (wave[~v] == 0).all()


def _random_rays(sc, n, seed, kat_dir=None):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(sc.bb_min[:]), np.array(sc.bb_max[:])
    start = lo + (hi - lo) * rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:40, rng.integers(0, 3)] = 0.0   # zero direction components: the exact-record walk
    d[:40] /= np.linalg.norm(d[:40], axis=1, keepdims=True)
    if kat_dir and os.path.exists(os.path.join(kat_dir, "isect_rays.f64")):
        rays = np.fromfile(os.path.join(kat_dir, "isect_rays.f64")).reshape(-1, 6)[:2000]
        start, d = np.vstack([start, rays[:, :3]]), np.vstack([d, rays[:, 3:]])
    return np.ascontiguousarray(start), np.ascontiguousarray(d)


# (form, workgroups, waves per workgroup, stack entries per lane in LDS, refill gate, leaf gate, log2 of the dealing block)
# form 3: round 4's visit (what MCRT_COUNT_TESTS and MCRT_WF_LEAN=0 run);
# forms 11 / 27 (round 5): the shared form with the lean visit (MCRT_WF_LEAN: FP32 ray kept, the pushes as one block of LDS writes) / ... one
# block per visit (trees without a node of more than four children; skipped otherwise). Stacks of 4 LDS entries make lanes leave the fast pushes.
TRACE_LAUNCHES = [(3, 3, 2, 16, 16, 16, 6), (3, 1, 4, 4, 16, 16, 6), (3, 2, 2, 16, 1, 1, 6), (3, 2, 3, 16, 48, 40, 7), (3, 5, 1, 8, 16, 16, 6),
                  (11, 3, 2, 16, 16, 16, 6), (11, 1, 4, 4, 16, 16, 6), (11, 2, 2, 3, 1, 1, 6), (11, 2, 3, 16, 48, 40, 7), (11, 5, 1, 8, 16, 16, 6),
                  (27, 3, 2, 16, 16, 16, 6), (27, 1, 4, 4, 16, 16, 6), (27, 2, 2, 3, 1, 1, 6), (27, 2, 3, 16, 48, 40, 7), (27, 5, 1, 8, 16, 16, 6)]


@pytest.mark.parametrize("name", ["coffee_maker_qsah", "coffee_maker_bsah", "hexagon_room", "quadric", "metals", "veach_mis"])
def test_trace_kernel_on_the_host_equals_the_oracle(pkg, wave_kernel_emu, oracle, manifest, name):
    """wfTraceKernel - the kernel half the bench's GPU time is spent in - as it is, on emulated workgroups: every form (shared leaf
    step = the default, deferred leaves, the first walk, eight-wide nodes), several launch shapes (one to five workgroups of one to
    four waves, 4 to 16 stack entries per lane in LDS with the rest spilled, refill and leaf gates from 'at once' to 'almost never',
    dealing blocks of 64 and 128): t, surface and uv of the oracle's Scene::intersect for every ray, bit for bit, and the kernel's own
    ray count. What this covers beyond the per-wave walk test: the queue dealt in blocks, the LDS cursor, batched refills and hit
    stores, the staging of the tree's top and root, __syncthreads."""
    case = manifest["cases"].get(name)
    if case is None:
        pytest.skip("no such golden case")
    img = pkg.SceneImage(golden_path(case["image"]))
    sc = img.scene
    start, d = _random_rays(sc, 3000, 23, golden_path(case["kat"]) if case.get("kat") else None)
    n = len(start)
    t0, s0, uv0, _ = oracle.intersect(img, start, d)
    hit = s0 != 0xFFFFFFFF
    ran = set()
    for form, grid, waves, lds_stack, refill, leaf, deal in TRACE_LAUNCHES:
        t, surf, uv = np.full(n, np.nan), np.full(n, 7, dtype=np.uint32), np.zeros((n, 2))
        stats = np.zeros(64, dtype=np.uint64)
        rc = wave_kernel_emu.wemu_trace_kernel(C.byref(sc), n, start.ctypes.data, d.ctypes.data, form, grid, waves, 0xFFFFFFFF, lds_stack, refill, leaf,
                                               deal, t.ctypes.data, surf.ctypes.data, uv.ctypes.data, stats.ctypes.data)
        if rc == -201 or (rc == -203 and form == 27):
            continue  # (no eight-wide nodes for this tree / a node with more than four children)
        ran.add(form)
        what = "form %d, %d x %d waves, stack %d, gates %d / %d" % (form, grid, waves, lds_stack, refill, leaf)
        assert rc == 0, what
        assert int(stats[1]) == n, what
        np.testing.assert_array_equal(surf, s0, err_msg=what)
        np.testing.assert_array_equal(t[hit], t0[hit], err_msg=what)
        np.testing.assert_array_equal(uv[hit], uv0[hit], err_msg=what)
    assert {3, 11} <= ran and (27 in ran or name != "coffee_maker_qsah")  # (a quaternary tree is single-block by construction)
    print("%s: forms run %s" % (name, sorted(ran)))


KERNEL_NAMES = {1: "renderKernel<path tracer, flat>", 2: "renderKernel (wave-synchronous)", 3: "renderKernelSM", 5: "renderKernelPM",
                16: "renderKernelFlatK (flat, cull records as a kernel argument)"}


def _emulated_frame(pkg, wave_kernel_emu, img, cam, seed, integrator, force=0, grid=1):
    out = np.zeros((cam.height, cam.width, 3))
    stats = np.zeros(64, dtype=np.uint64)
    kid = C.c_int(0)
    g, c = img.photons(0), img.photons(1)
    rc = wave_kernel_emu.wemu_render(C.byref(img.scene), C.byref(g) if g is not None else None, C.byref(c) if c is not None else None,
                                     img.param("k_nearest_photons") or 50, int(img.param("direct_visualization") or 0), C.byref(cam), seed, integrator,
                                     force, grid, out.ctypes.data, stats.ctypes.data, C.byref(kid))
    return rc, out, stats, kid.value


@pytest.mark.parametrize("name", ["hexagon_room", "hexagon_room_diffuse", "hexagon_room_ggx", "hexagon_room_dof", "coffee_maker_qsah", "coffee_maker_bsah",
                                  "veach_mis", "metals", "ggx_test", "oren_nayar_test", "ior_test", "quadric", "dragon_room", "shell_room"])
def test_frame_kernels_on_the_host_give_the_oracle_frame(pkg, wave_kernel_emu, oracle, manifest, name):
    """The FRAME KERNELS of the product - the flat megakernel of the headline config, the lane state machine, the wave-synchronous
    kernel - as they are, on emulated workgroups of 8 wavefronts (work units popped with wave-aggregated atomics, path regeneration,
    LDS staging of scene / tables / stacks, the per-sample store) followed by sampleResolveKernel: a small frame of every golden scene,
    by the kernel launchRender picks and by the wave-synchronous one, against the oracle's frame (which is the reference's, bit for
    bit: test_oracle_vs_reference.py) - bit for bit, with the oracle's ray count. No GPU."""
    case = manifest["cases"].get(name)
    if case is None:
        pytest.skip("no such golden case")
    from conftest import camera_for
    img = pkg.SceneImage(golden_path(case["image"]))
    cam = camera_for(img, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 28, 16, 2
    want, info = oracle.render(img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER)
    seen = set()
    for force, grid in ((0, 1), (2, 2), (6, 2)):  # (6: the flat megakernel with its cull records as a kernel argument, renderKernelFlatK)
        rc, out, stats, kid = _emulated_frame(pkg, wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, force, grid)
        if force == 6 and (rc == -206 or kid != 16):
            continue  # (not a flat scene, or more records than the argument block holds)
        assert rc == 0, "%s: rc %d" % (KERNEL_NAMES.get(kid), rc)
        seen.add(kid)
        assert int(stats[0]) == cam.width * cam.height * 4 and int(stats[1]) == info["rays"], KERNEL_NAMES.get(kid)
        np.testing.assert_array_equal(out, want, err_msg="%s: %s is not the oracle's frame" % (name, KERNEL_NAMES.get(kid)))
    print("%s: %s - the oracle's bits, %d rays" % (name, " and ".join(KERNEL_NAMES[k] for k in sorted(seen)), info["rays"]))


def test_photon_mapping_kernel_on_the_host(pkg, wave_kernel_emu, oracle, manifest):
    """renderKernelPM (1024 lanes = 16 emulated wavefronts: per-lane bounce code, estimates served by whole waves) on hexagon_room_pm's
    maps against the oracle's photon-mapped frame: the order of an estimate's FP64 sum is the only difference (1e-12)."""
    from conftest import camera_for
    case = manifest["cases"]["hexagon_room_pm"]
    img = pkg.SceneImage(golden_path(case["image"]))
    cam = camera_for(img, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 24, 12, 2
    want, info = oracle.render(img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER)
    rc, out, stats, kid = _emulated_frame(pkg, wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER)
    assert rc == 0 and kid == 5
    assert int(stats[1]) == info["rays"] and int(stats[4]) > 0
    rel = np.abs(out - want) / np.maximum(np.abs(want), 1e-3)
    print("hexagon_room_pm through renderKernelPM on the host: max rel %.3e, %d searches" % (rel.max(), int(stats[4])))
    assert rel.max() <= 1e-12


def _emulated_pipeline_frame(wave_kernel_emu, img, cam, seed, integrator, slots, grid, waves, form):
    out = np.zeros((cam.height, cam.width, 3))
    stats = np.zeros(64, dtype=np.uint64)
    launches = C.c_uint32(0)
    g, c = img.photons(0), img.photons(1)
    rc = wave_kernel_emu.wemu_render_pipeline(C.byref(img.scene), C.byref(g) if g is not None else None, C.byref(c) if c is not None else None,
                                              img.param("k_nearest_photons") or 50, int(img.param("direct_visualization") or 0), C.byref(cam), seed,
                                              integrator, slots, grid, waves, form, out.ctypes.data, stats.ctypes.data, C.byref(launches))
    return rc, out, stats, launches.value


# (pool slots, trace workgroups, waves per trace workgroup, trace kernel form)
PIPELINE_LAUNCHES = [(512, 2, 2, 3), (256, 1, 4, 3), (1024, 3, 1, 3), (768, 2, 2, 11), (512, 2, 2, 11), (256, 1, 4, 27), (1024, 3, 1, 27)]


@pytest.mark.parametrize("name", ["coffee_maker_qsah", "coffee_maker_bsah", "hexagon_room", "hexagon_room_dof", "quadric", "metals", "veach_mis", "ggx_test",
                                  "dragon_room", "shell_room"])
def test_wavefront_pipeline_on_the_host_gives_the_oracle_frame(pkg, wave_kernel_emu, oracle, manifest, name):
    """The wavefront pipeline as launchWavefront runs it - wfShadeKernel (one lane per pool slot: NEE finish, shading, regeneration, rays
    appended to the queue with wave-aggregated atomics under divergent control flow), wfTraceKernel<PoolRays> in every form, launch after
    launch until a shade launch queues nothing, then sampleResolveKernel - on emulated workgroups, the slot pool starting as garbage
    like device memory: the oracle's frame, bit for bit, for several pool sizes and launch shapes. (Its ray count may fall short of the
    oracle's by the shadow rays whose BSDF term is zero: the pipeline does not trace them.)"""
    case = manifest["cases"].get(name)
    if case is None:
        pytest.skip("no such golden case")
    from conftest import camera_for
    img = pkg.SceneImage(golden_path(case["image"]))
    cam = camera_for(img, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 24, 14, 2
    want, info = oracle.render(img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER)
    for slots, grid, waves, form in PIPELINE_LAUNCHES:
        rc, out, stats, launches = _emulated_pipeline_frame(wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, slots, grid, waves, form)
        if rc == -201 or (rc == -204 and form == 27):
            continue  # (no eight-wide nodes for this tree / a node with more than four children)
        what = "%s: %d slots, trace %d x %d waves, form %d" % (name, slots, grid, waves, form)
        assert rc == 0, what
        assert int(stats[0]) == cam.width * cam.height * 4 and 0 <= info["rays"] - int(stats[1]) <= 0.03 * info["rays"], what
        assert launches > 6
        np.testing.assert_array_equal(out, want, err_msg=what)


def test_photon_mapped_pipeline_on_the_host(pkg, wave_kernel_emu, oracle, manifest):
    """... and the photon-mapped pipeline: estimate requests staged by the shade launch, served by wfKnnKernel<eval> (one request per
    wave), read back by the next shade launch."""
    from conftest import camera_for
    case = manifest["cases"]["hexagon_room_pm"]
    img = pkg.SceneImage(golden_path(case["image"]))
    cam = camera_for(img, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 20, 12, 2
    want, info = oracle.render(img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER)
    rc, out, stats, launches = _emulated_pipeline_frame(wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER, 512, 2, 2, 3)
    assert rc == 0 and int(stats[4]) > 0
    rel = np.abs(out - want) / np.maximum(np.abs(want), 1e-3)
    print("hexagon_room_pm through the pipeline on the host: max rel %.3e, %d searches, %d launches" % (rel.max(), int(stats[4]), launches))
    assert rel.max() <= 1e-12


@pytest.mark.parametrize("name", ["hexagon_room_pm", "coffee_maker_qsah"])
def test_emission_kernel_on_the_host_gives_the_oracle_photons(pkg, wave_kernel_emu, oracle, manifest, name):
    """emitKernel on emulated workgroups (photon paths regenerated from a counter, photons appended with wave-aggregated atomics): the
    oracle's photon lists, record for record by (light, emission, bounce) key - and the sizing pilot (every 64th path, capacity 0)
    counts what it should: within a few per cent of a 64th of the lists."""
    from conftest import sort_by_key
    case = manifest["cases"][name]
    img = pkg.SceneImage(golden_path(case["image"]))
    emissions, factor = 300, 10.0
    want = oracle.emit_photons(img, emissions, factor, manifest["seed"])
    cap = 1 << 16
    g, gk = np.zeros((cap, 8), dtype=np.float32), np.zeros(cap, dtype=np.uint64)
    c, ck = np.zeros((cap, 8), dtype=np.float32), np.zeros(cap, dtype=np.uint64)
    counts = np.zeros(4, dtype=np.uint64)
    rc = wave_kernel_emu.wemu_emit(C.byref(img.scene), float(emissions), factor, manifest["seed"], 1, 2, cap, g.ctypes.data, gk.ctypes.data, c.ctypes.data,
                                   ck.ctypes.data, counts.ctypes.data)
    assert rc == 0
    assert int(counts[2]) == want["paths"] and int(counts[3]) == want["rays"]
    for (ph, keys, n), (wph, wkeys) in (((g, gk, int(counts[0])), want["global_"]), ((c, ck, int(counts[1])), want["caustic"])):
        assert n == len(wkeys)
        a, ak = sort_by_key(ph[:n], keys[:n])
        np.testing.assert_array_equal(ak, wkeys)
        np.testing.assert_array_equal(a.view(np.uint32), wph.view(np.uint32))
    pilot = np.zeros(4, dtype=np.uint64)
    rc = wave_kernel_emu.wemu_emit(C.byref(img.scene), float(emissions), factor, manifest["seed"], 8, 1, 0, None, None, None, None, pilot.ctypes.data)
    assert rc == 0 and int(pilot[2]) == -(-want["paths"] // 8)
    total, sample = int(counts[0]) + int(counts[1]), (int(pilot[0]) + int(pilot[1])) * 8
    assert abs(sample - total) <= 0.25 * total


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_frames_do_not_depend_on_the_order_the_waves_run_in(pkg, wave_kernel_emu, oracle, manifest, seed):
    """The waves of an emulated workgroup normally take turns; here they are visited in a random order that changes from pass to pass,
    a wave sitting a pass out now and then - arbitration as arbitrary as the hardware's. Work units, queue entries and photon slots
    are then handed out in other orders; frames (flat megakernel, lane state machine, pipeline, photon mapper) and photon sets are not
    allowed to notice."""
    from conftest import camera_for, sort_by_key
    try:
        wave_kernel_emu.wemu_set_shuffle(seed)
        for name, integ in (("hexagon_room", pkg.INTEGRATOR_PATH_TRACER), ("coffee_maker_qsah", pkg.INTEGRATOR_PATH_TRACER),
                            ("hexagon_room_pm", pkg.INTEGRATOR_PHOTON_MAPPER)):
            case = manifest["cases"][name]
            img = pkg.SceneImage(golden_path(case["image"]))
            cam = camera_for(img, case["renders"][0])
            cam.width, cam.height, cam.sqrtspp = 20, 12, 2
            want, info = oracle.render(img, cam, manifest["seed"], integ)
            rc, out, stats, kid = _emulated_frame(pkg, wave_kernel_emu, img, cam, manifest["seed"], integ, 0, 2)
            assert rc == 0
            rc2, pipe, stats2, _ = _emulated_pipeline_frame(wave_kernel_emu, img, cam, manifest["seed"], integ, 512, 2, 3, 3)
            assert rc2 == 0
            if integ == pkg.INTEGRATOR_PATH_TRACER:
                np.testing.assert_array_equal(out, want, err_msg=name)
                np.testing.assert_array_equal(pipe, want, err_msg=name + " (pipeline)")
            else:
                assert (np.abs(out - want) / np.maximum(np.abs(want), 1e-3)).max() <= 1e-12
                assert (np.abs(pipe - want) / np.maximum(np.abs(want), 1e-3)).max() <= 1e-12
    finally:
        wave_kernel_emu.wemu_set_shuffle(0)


@pytest.mark.parametrize("name", ["c3", "c5"])
def test_large_scene_kernels_on_the_host(pkg, wave_kernel_emu, oracle, name):
    """The kernels of the scaled BASELINE configurations on their own trees, without a GPU: C3 (metal_bunnies stand-in, 491 592 triangles:
    lane state machine and the wavefront pipeline) and C5 (water_caustics stand-in, 6 898 815 triangles, photon-mapped: renderKernelPM's
    instance for trees in memory - per-lane stacks partly in LDS, shared-leaf walks, the spill list's state in LDS - and the photon-
    mapped pipeline) render a small frame of the config's camera on emulated workgroups: the oracle's frame (bit for bit path-traced;
    1e-12 photon-mapped: sum order). The images are made by integration/large_scenes/make_large.py (skipped where they are not)."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "integration", "large_scenes"))
    import make_large
    p = make_large.ensure_image(name)
    if p is None:
        pytest.skip("oracle/_ref (reference binary + scene copies) not on this machine")
    img = pkg.SceneImage(p)
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = 20, 12, 1
    photon = bool(make_large.CONFIGS[name]["photon"])
    integ = pkg.INTEGRATOR_PHOTON_MAPPER if photon else pkg.INTEGRATOR_PATH_TRACER
    want, info = oracle.render(img, cam, 0x12345678, integ)
    rc, out, stats, kid = _emulated_frame(pkg, wave_kernel_emu, img, cam, 0x12345678, integ, 0, 1)
    assert rc == 0 and kid == (5 if photon else 3) and int(stats[1]) == info["rays"]
    # (the pipeline with the trace form the device runs on THIS tree: C3 is quaternary -> the lean visit, one block per node; C5's
    # octree hierarchy has nodes of up to eight children -> the lean visit with the block loop)
    rc2, pipe, stats2, launches = _emulated_pipeline_frame(wave_kernel_emu, img, cam, 0x12345678, integ, 256, 2, 2, 27 if name == "c3" else 11)
    assert rc2 == 0 and 0 <= info["rays"] - int(stats2[1]) <= 0.03 * info["rays"] + 1
    if photon:
        for got in (out, pipe):
            assert (np.abs(got - want) / np.maximum(np.abs(want), 1e-3)).max() <= 1e-12
    else:
        np.testing.assert_array_equal(out, want)
        np.testing.assert_array_equal(pipe, want)


@pytest.mark.parametrize("name", ["hexagon_room", "hexagon_room_dof", "ior_test", "coffee_maker_qsah", "coffee_maker_bsah"])
def test_lean_kernel_instances_on_the_host_give_the_oracle_frame(pkg, wave_kernel_emu_lean, oracle, manifest, name):
    """csrc/mcrt_hip_lean.hip compiles the default path's kernels WITHOUT the rough-diffuse, rough-specular and conductor branches
    (MCRT_MAT_FEATURES_OFF, csrc/mcrt_shade.hpp), for scenes none of whose materials carries one of those flags. The same kernels built
    that way for the host: the megakernel launchRender picks, the flat megakernel with its records as a kernel argument, and the wavefront
    pipeline render such scenes to the oracle's frame, bit for bit. (On the GPU: tests/test_gpu_lean_kernels.py.)"""
    case = manifest["cases"].get(name)
    if case is None:
        pytest.skip("no such golden case")
    from conftest import camera_for
    img = pkg.SceneImage(golden_path(case["image"]))
    s = img.scene
    assert not any(s.materials[i].flags & 67 for i in range(s.num_materials)), "the lean instances are not for this scene"
    cam = camera_for(img, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 24, 14, 2
    want, info = oracle.render(img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER)
    for force, grid in ((0, 1), (6, 2)):
        rc, out, stats, kid = _emulated_frame(pkg, wave_kernel_emu_lean, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, force, grid)
        if force == 6 and (rc == -206 or kid != 16):
            continue
        assert rc == 0 and int(stats[1]) == info["rays"]
        np.testing.assert_array_equal(out, want, err_msg="%s: lean %s is not the oracle's frame" % (name, KERNEL_NAMES.get(kid)))
    rc, out, stats, launches = _emulated_pipeline_frame(wave_kernel_emu_lean, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, 512, 2, 2, 11)
    assert rc == 0
    np.testing.assert_array_equal(out, want, err_msg="%s: lean pipeline" % name)


def test_lean_photon_mapping_kernel_on_the_host(pkg, wave_kernel_emu, wave_kernel_emu_lean, manifest):
    """... and renderKernelPM: the lean instance's hexagon_room_pm frame is the full instance's, bit for bit."""
    from conftest import camera_for
    case = manifest["cases"]["hexagon_room_pm"]
    img = pkg.SceneImage(golden_path(case["image"]))
    cam = camera_for(img, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 20, 10, 2
    rc0, full, st0, kid0 = _emulated_frame(pkg, wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER)
    rc1, lean, st1, kid1 = _emulated_frame(pkg, wave_kernel_emu_lean, img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER)
    assert rc0 == 0 and rc1 == 0 and kid0 == kid1 == 5 and int(st0[4]) == int(st1[4]) > 0
    np.testing.assert_array_equal(lean, full)


@pytest.mark.parametrize("name,photon,force", [("hexagon_room", False, 0), ("hexagon_room", False, 6), ("hexagon_room_ggx", False, 6), ("veach_mis", False, 0),
                                               ("coffee_maker_qsah", False, 0), ("quadric", False, 0), ("dragon_room", False, 0),
                                               ("hexagon_room_pm", True, 0)])
def test_emulated_frames_run_the_instance_the_host_selects(pkg, wave_kernel_emu, manifest, name, photon, force):
    """wemu_render asks the host's own selectKernel (csrc/mcrt_select.hpp) with SceneFacts derived by the host's sceneFacts
    (csrc/mcrt_launch.hpp). Here the same question is put to selectKernel from outside - the scene's facts, the frame, and the call
    written as the options a user would set - and the emulated frame must have run the instance, workgroup size and stack depth it names."""
    from conftest import camera_for
    case = manifest["cases"][name]
    img = pkg.SceneImage(golden_path(case["image"]))
    cam = camera_for(img, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 16, 8, 1
    integ = pkg.INTEGRATOR_PHOTON_MAPPER if photon else pkg.INTEGRATOR_PATH_TRACER
    facts = (C.c_uint64 * 26)()
    assert wave_kernel_emu.wemu_scene_facts(C.byref(img.scene), facts) == 0
    k = img.param("k_nearest_photons") or 50
    frame = (C.c_uint64 * 8)(int(photon), cam.width * cam.height, 0, 0, k, facts[25], 0, 0)
    options = {"MCRT_LEAN_KERNELS": "0"}  # (the full library)
    if not facts[0]:
        options["MCRT_KERNEL"] = "sm"
    elif force == 0:
        options["MCRT_FLAT_KARG"] = "0"
    keys = (C.c_char_p * len(options))(*[k_.encode() for k_ in options])
    values = (C.c_char_p * len(options))(*[v.encode() for v in options.values()])
    choice, msg = (C.c_uint64 * 9)(), C.create_string_buffer(256)
    assert wave_kernel_emu.emu_select_kernel(facts, frame, len(options), keys, values, choice, msg, 256) == 0, msg.value
    rc, out, stats, kid = _emulated_frame(pkg, wave_kernel_emu, img, cam, manifest["seed"], integ, force, 1)
    assert rc == 0
    launch = (C.c_uint64 * 4)()
    wave_kernel_emu.wemu_last_launch(launch)
    form, instance, block, stack_depth = int(choice[0]), int(choice[1]), int(choice[5]), int(choice[6])
    print("%s: form %d instance %d, %d lanes, %d stack entries in LDS, %d bytes of LDS" % (name, form, instance, block, stack_depth, launch[3]))
    assert (int(launch[0]), int(launch[1]), int(launch[2])) == (instance, block, stack_depth)
    assert kid == (16 if force == 6 and form == 1 else form)
    if force == 6 and form == 1:
        assert block == 768  # the full instance with its records as an argument: the shape the host launches


# ---- the counting instances (MCRT_COUNT_TESTS), the per-lane and the wide photon-mapping kernels, the raw kNN launch --------------------
# RenderInstance of csrc/mcrt_select.hpp by value (instanceName gives the same words: test_instance_names_follow_the_enumeration)
INSTANCE_NAMES = ["PT", "PT_All", "PT_Count", "PT_CountAll", "PT_Prof", "PT_ProfAll", "PMLane", "PMLane_All", "PMLane_Count", "PMLane_CountAll",
                  "Flat512", "FlatK512", "FlatK768", "SM", "SM_All", "SM_Count", "SM_CountAll", "SM_Prof", "SM_ProfAll",
                  "PM512", "PM512_All", "PM512_Count", "PM512_CountAll", "PM1024", "PM1024_All", "PM1024_Count", "PM1024_CountAll",
                  "PMWide", "PMWide_All", "PMWide_Count", "PMWide_CountAll", "ShadePT", "ShadePM", "Trace", "Trace_Count", "TraceLean", "TraceLeanSingle",
                  "KnnEval", "KnnEvalWide", "KnnRaw", "KnnRawWide", "Emit", "Emit_All"]


def test_instance_names_follow_the_enumeration():
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc", "mcrt_select.hpp")).read()
    body = re.sub(r"//[^\n]*", "", text[text.index("enum RenderInstance"):text.index("kInstCount\n")])
    enum = [m for m in re.findall(r"kInst(\w+)", body) if m != "None"]
    assert enum == INSTANCE_NAMES
    names = re.findall(r'"([A-Za-z0-9_]+)"', text[text.index("inline const char* instanceName"):text.index("static_assert(sizeof(names)")])
    assert names == INSTANCE_NAMES


class SceneWithMaps:
    """A SceneImage's scene with photon maps of the test's own making (oracle_lib and the emulation read .scene, .photons() and .param())."""

    def __init__(self, img, maps, k):
        self.img, self.maps, self.k, self.scene = img, maps, k, img.scene

    def photons(self, which):
        return self.maps[which].desc

    def param(self, key):
        return self.k if key == "k_nearest_photons" else 0


def coffee_maker_with_photons(pkg, oracle, manifest, k=50):
    """coffee_maker_qsah - a tree that stays in memory - with maps from the oracle's own emission pass: the scene of the photon-mapping
    instances for trees in memory (golden photon-mapped scenes are all LDS-resident)."""
    img = pkg.SceneImage(golden_path(manifest["cases"]["coffee_maker_qsah"]["image"]))
    em = oracle.emit_photons(img, 4000, 10.0, manifest["seed"])
    assert len(em["global_"][1]) > 1000 and len(em["caustic"][1]) > 100
    s = img.scene
    maps = [pkg.PhotonMap(em[key][0], s.bb_min[:], s.bb_max[:], 200) for key in ("global_", "caustic")]
    return SceneWithMaps(img, maps, k)


class emu_options:
    """MCRT_COUNT_TESTS / MCRT_WF_PM_EVAL / MCRT_FLAT_MAX of the emulated frames inside the block (wave_kernel_emu.cpp's switches)."""

    def __init__(self, lib, count=None, pm_eval=1, flat_max=64):
        self.lib, self.values = lib, (-1 if count is None else int(count), int(pm_eval), int(flat_max))
        for f, t in ((lib.wemu_set_count_tests, C.c_int), (lib.wemu_set_pm_eval, C.c_int), (lib.wemu_set_flat_max, C.c_uint32)):
            f.argtypes, f.restype = [t], None
        lib.wemu_last_launch.argtypes, lib.wemu_last_launch.restype = [C.c_void_p], None

    def _set(self, count, pm_eval, flat_max):
        self.lib.wemu_set_count_tests(count)
        self.lib.wemu_set_pm_eval(pm_eval)
        self.lib.wemu_set_flat_max(flat_max)

    def __enter__(self):
        self._set(*self.values)

    def __exit__(self, *exc):
        self._set(-1, 1, 64)


def emulated_megakernel_frame(pkg, lib, img, cam, seed, integrator, count, legacy=False, flat_max=64, k=None, grid=1):
    """-> (frame, stats words, the RenderInstance name wemu_render ran)"""
    out = np.zeros((cam.height, cam.width, 3))
    stats = np.zeros(64, dtype=np.uint64)
    kid = C.c_int(0)
    g, c = img.photons(0), img.photons(1)
    with emu_options(lib, count=count, flat_max=flat_max):
        rc = lib.wemu_render(C.byref(img.scene), C.byref(g) if g is not None else None, C.byref(c) if c is not None else None,
                             k or img.param("k_nearest_photons") or 50, 0, C.byref(cam), seed, integrator, 2 if legacy else 0, grid, out.ctypes.data,
                             stats.ctypes.data, C.byref(kid))
    launch = (C.c_uint64 * 4)()
    lib.wemu_last_launch(launch)
    assert rc == 0, "wemu_render: %d (instance %s)" % (rc, INSTANCE_NAMES[int(launch[0])])
    return out, [int(x) for x in stats[:20]], INSTANCE_NAMES[int(launch[0])]


def emulated_pipeline_frame(lib, img, cam, seed, integrator, count, pm_eval=1, k=None, slots=512, grid=2, waves=2):
    """... through the pipeline with the trace kernel's earlier visit (form 3: Trace / Trace_Count) -> (frame, stats words)"""
    out = np.zeros((cam.height, cam.width, 3))
    stats = np.zeros(64, dtype=np.uint64)
    launches = C.c_uint32(0)
    g, c = img.photons(0), img.photons(1)
    with emu_options(lib, count=count, pm_eval=pm_eval):
        rc = lib.wemu_render_pipeline(C.byref(img.scene), C.byref(g) if g is not None else None, C.byref(c) if c is not None else None,
                                      k or img.param("k_nearest_photons") or 50, 0, C.byref(cam), seed, integrator, slots, grid, waves, 3, out.ctypes.data,
                                      stats.ctypes.data, C.byref(launches))
    assert rc == 0, "wemu_render_pipeline: %d" % rc
    return out, [int(x) for x in stats[:20]]


def check_counter_bounds(img, stats, frame, flat):
    """What include/mcrt.h says of node_tests / prim_tests, as far as it can be said without walking the tree again: a flat scene tests no
    node and at most every primitive per ray - with cull records what the FP32 cull leaves (the bound of test_device_code_host_emulation.py) -
    a tree tests at least its root per ray that is walked; and a ray that hit something passed at least one primitive test. Rays that hit
    are not counted by any kernel: at least one per pixel that is not black."""
    paths, rays, node_tests, prim_tests = stats[:4]
    ns = img.scene.num_surfaces
    assert prim_tests > 0 and prim_tests >= int((frame != 0).any(axis=2).sum())
    if flat:
        assert node_tests == 0 and prim_tests <= ns * rays
        assert prim_tests < (0.15 if ns >= 20 else 0.6) * ns * rays
    else:
        assert node_tests > 0 and node_tests >= paths


FRAME = (70, 21, 2)       # ragged against the 8 x 8 tiles in both directions, four samples per pixel
SMALL_FRAME = (22, 9, 1)  # ... for the wave-cooperative searches, whose emulation takes 4 ms each

# (scene, photon-mapped, MCRT_KERNEL=legacy, MCRT_FLAT_MAX, k, frame, the instance without / with MCRT_COUNT_TESTS, counters are sums of per-ray quantities)
COUNTING_CASES = [
    ("hexagon_room_diffuse", False, False, 64, None, FRAME, "Flat512", "PT_CountAll", True),
    ("hexagon_room_diffuse", False, True, 64, None, FRAME, "PT_All", "PT_CountAll", True),
    ("hexagon_room_diffuse", False, False, 0, None, FRAME, "SM_All", "SM_CountAll", True),
    ("hexagon_room_diffuse", False, True, 0, None, FRAME, "PT_All", "PT_CountAll", True),
    ("coffee_maker_qsah", False, False, 64, None, FRAME, "SM", "SM_Count", True),
    ("coffee_maker_qsah", False, True, 64, None, FRAME, "PT", "PT_Count", True),
    ("quadric", False, False, 64, None, FRAME, "SM", "SM_Count", True),
    ("quadric", False, True, 64, None, FRAME, "PT", "PT_Count", True),
    ("hexagon_room_pm", True, False, 64, None, SMALL_FRAME, "PM1024_All", "PM1024_CountAll", True),
    ("hexagon_room_pm", True, True, 64, None, FRAME, "PMLane_All", "PMLane_CountAll", True),
    ("hexagon_room_pm", True, False, 64, 129, SMALL_FRAME, "PMWide_All", "PMWide_CountAll", True),
    ("coffee_maker_qsah+photons", True, False, 64, None, SMALL_FRAME, "PM1024", "PM1024_Count", False),
    ("coffee_maker_qsah+photons", True, True, 64, None, SMALL_FRAME, "PMLane", "PMLane_Count", True),
    ("coffee_maker_qsah+photons", True, False, 64, 129, SMALL_FRAME, "PMWide", "PMWide_Count", False),
]


def diagnostic_scene(pkg, oracle, manifest, name):
    if name == "coffee_maker_qsah+photons":
        img = coffee_maker_with_photons(pkg, oracle, manifest)
        return img, pkg.SceneImage(golden_path(manifest["cases"]["coffee_maker_qsah"]["image"])).camera.copy()
    from conftest import camera_for
    case = manifest["cases"][name]
    img = pkg.SceneImage(golden_path(case["image"]))
    return img, camera_for(img, case["renders"][0])


@pytest.mark.parametrize("name,photon,legacy,flat_max,k,frame,plain,counting,per_ray", COUNTING_CASES)
def test_counting_instances_on_the_host_render_the_plain_instances_bits(pkg, wave_kernel_emu, oracle, manifest, name, photon, legacy, flat_max, k, frame, plain,
                                                                         counting, per_ray):
    """MCRT_COUNT_TESTS selects another kernel instance (csrc/mcrt_select.hpp) - for a flat scene another FORM, the wave-synchronous kernel -
    and every decision of DESIGN.md that quotes node or primitive tests per ray was measured on such a frame: it has to be the frame that
    was being studied. Each counting instance on emulated workgroups against the instance the same call runs without the option: the same
    bits, paths, rays and searches (the ray count the oracle's, as in the cases above); words 2 and 3 zero without the option and within
    the bounds of check_counter_bounds with it; and, for the instances whose counters are sums of per-ray quantities (per_ray: every walk but
    the shared leaf step of trees in memory, whose deferred leaves are tested when OTHER lanes of the wave are ready), the same counters from
    one workgroup and from two whose waves are visited in a shuffled order."""
    img, cam = diagnostic_scene(pkg, oracle, manifest, name)
    cam.width, cam.height, cam.sqrtspp = frame
    integ = pkg.INTEGRATOR_PHOTON_MAPPER if photon else pkg.INTEGRATOR_PATH_TRACER
    seed = manifest["seed"]
    out0, st0, inst0 = emulated_megakernel_frame(pkg, wave_kernel_emu, img, cam, seed, integ, False, legacy, flat_max, k)
    out1, st1, inst1 = emulated_megakernel_frame(pkg, wave_kernel_emu, img, cam, seed, integ, True, legacy, flat_max, k)
    assert (inst0, inst1) == (plain, counting)
    np.testing.assert_array_equal(out1, out0)
    assert st1[0] == st0[0] == cam.width * cam.height * cam.sqrtspp ** 2 and st1[1] == st0[1] and st1[4] == st0[4] and (st0[4] > 0) == photon
    assert st0[2] == st0[3] == 0
    _, info = oracle.render(img, cam, seed, integ, k=k)
    if counting.startswith("SM"):  # (shadow rays whose BSDF term is zero are not traced by the state machine)
        assert 0 <= info["rays"] - st1[1] <= 0.03 * info["rays"]
    else:
        assert st1[1] == info["rays"]
    flat = name.startswith("hexagon_room") and flat_max != 0
    check_counter_bounds(img, st1, out1, flat)
    print("%s: %s = the bits of %s; %d rays, %.2f node and %.2f primitive tests per ray" % (name, inst1, inst0, st1[1], st1[2] / st1[1], st1[3] / st1[1]))
    if per_ray:
        try:
            wave_kernel_emu.wemu_set_shuffle(5)
            out2, st2, _ = emulated_megakernel_frame(pkg, wave_kernel_emu, img, cam, seed, integ, True, legacy, flat_max, k, grid=2)
        finally:
            wave_kernel_emu.wemu_set_shuffle(0)
        np.testing.assert_array_equal(out2, out0)
        assert st2[:5] == st1[:5]


def test_photon_mapping_instances_count_the_same_tests_per_ray_on_the_host(pkg, wave_kernel_emu, manifest):
    """The photon-mapping kernels of an LDS-resident scene - wave-cooperative at 1024 lanes, with the wide candidate buffer, per lane - trace
    the same rays through the same sceneIntersect: words 1 to 4 of the three counting instances are the same numbers."""
    img, cam = diagnostic_scene(pkg, None, manifest, "hexagon_room_pm")
    cam.width, cam.height, cam.sqrtspp = SMALL_FRAME
    seen = {}
    for legacy, k in ((False, None), (True, None), (False, 129), (True, 129)):
        _, st, inst = emulated_megakernel_frame(pkg, wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER, True, legacy, 64, k)
        seen[inst] = st[1:5]
    assert set(seen) == {"PM1024_CountAll", "PMLane_CountAll", "PMWide_CountAll"}
    assert len(set(map(tuple, seen.values()))) == 1, seen


@pytest.mark.parametrize("name", ["coffee_maker_qsah", "quadric"])
def test_counting_trace_kernel_on_the_host_renders_the_plain_kernels_bits(pkg, wave_kernel_emu, oracle, manifest, name):
    """Trace_Count (wfTraceKernel<PoolRays, true>: what MCRT_COUNT_TESTS runs in the pipeline) against Trace (MCRT_WF_LEAN=0): the oracle's
    frame from both, the same rays; the counters only from the first, with the step counters of the [mcrt trace] line consistent among
    themselves (an iteration holds at most 64 rays, steps at most one per iteration, lane steps at most 64 per step)."""
    img, cam = diagnostic_scene(pkg, oracle, manifest, name)
    cam.width, cam.height, cam.sqrtspp = FRAME
    want, info = oracle.render(img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER)
    out0, st0 = emulated_pipeline_frame(wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, False)
    out1, st1 = emulated_pipeline_frame(wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, True)
    np.testing.assert_array_equal(out0, want)
    np.testing.assert_array_equal(out1, want)
    assert st0[:2] == st1[:2] and 0 <= info["rays"] - st1[1] <= 0.03 * info["rays"]
    assert st0[2] == st0[3] == 0 and not any(st0[8:20])
    check_counter_bounds(img, st1, out1, False)
    iters, have, in_steps, in_lanes, lf_steps, lf_lanes = st1[8:14]
    assert 0 < in_steps <= iters and 0 < lf_steps <= iters and in_steps <= in_lanes <= 64 * in_steps and lf_steps <= lf_lanes <= 64 * lf_steps
    assert in_lanes <= have <= 64 * iters
    # an inner lane step tests the children of one node: between one and eight boxes
    assert in_lanes <= st1[2] <= 8 * in_lanes + st1[1]


@pytest.mark.parametrize("k", [50, 129])
def test_raw_knn_launch_on_the_host(pkg, wave_kernel_emu, oracle, manifest, k):
    """MCRT_WF_PM_EVAL=0: wfKnnKernel<false> (k = 129: with the wide candidate buffer) hands the k photons of a search back and the next
    shade launch sums them per lane (wfPhotonEstimate) - in the order of the candidate buffer, one after the other, where the evaluating
    launch adds them by a wave reduction: the same photons, another order of the FP64 sum, so the oracle's frame to 1e-12 and not the
    evaluating launch's bits. (Until the raw branch met its lanes at MCRT_LOCKSTEP before reading the compacted result this frame was off by
    per cent here: nothing in the memory model ordered those LDS reads behind the other lanes' writes.)"""
    img, cam = diagnostic_scene(pkg, oracle, manifest, "hexagon_room_pm")
    cam.width, cam.height, cam.sqrtspp = SMALL_FRAME
    want, info = oracle.render(img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER, k=k)
    ev, st_ev = emulated_pipeline_frame(wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER, None, 1, k)
    raw, st_raw = emulated_pipeline_frame(wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER, None, 0, k)
    assert st_raw[:2] == st_ev[:2] and st_raw[4] == st_ev[4] > 0
    rel_raw, rel_ev = np.abs(raw - want) / np.maximum(np.abs(want), 1e-3), np.abs(ev - want) / np.maximum(np.abs(want), 1e-3)
    print("k = %d: max rel %.3e raw, %.3e evaluating" % (k, rel_raw.max(), rel_ev.max()))
    assert rel_raw.max() <= 1e-12 and rel_ev.max() <= 1e-12


def test_both_walks_of_a_staged_tree_test_the_same_boxes_on_the_host(pkg, wave_kernel_emu, oracle, manifest):
    """Two implementations of one walk: sceneIntersect (csrc/mcrt_scene.hpp, the wave-synchronous kernel) and the state machine's steps
    (csrc/mcrt_lanesm.hpp) both go depth first over the exact boxes of an LDS-resident tree, the nearest child first, a leaf tested whole
    before the next node, and drop a pending node that starts behind the closest hit so far. In a scene without specular materials they
    trace the same rays (no shadow ray is skipped for a zero BSDF term), so they test the same boxes: PT_CountAll and SM_CountAll agree on
    node_tests to the last one - each counted in its own source file. (Primitive tests differ: the state machine tests a leaf two
    primitives at a time.)"""
    img, cam = diagnostic_scene(pkg, oracle, manifest, "hexagon_room_diffuse")
    cam.width, cam.height, cam.sqrtspp = FRAME
    _, sm, inst_sm = emulated_megakernel_frame(pkg, wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, True, False, 0)
    _, pt, inst_pt = emulated_megakernel_frame(pkg, wave_kernel_emu, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, True, True, 0)
    assert (inst_sm, inst_pt) == ("SM_CountAll", "PT_CountAll")
    assert sm[:2] == pt[:2]
    assert sm[2] == pt[2] > 0, "node tests: state machine %d, wave-synchronous kernel %d" % (sm[2], pt[2])
    assert 0 < pt[3] <= sm[3] <= 2 * pt[3]
