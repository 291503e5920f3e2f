"""Kernel selection and the render-again decision (csrc/mcrt_select.hpp: selectKernel, nextRender), checked without a GPU through
tests/emu, as tests/test_work_units.py checks the work-unit planning. The cases are the ones DESIGN.md and the bench line stand on;
the GPU tests' kernel_id assertions (test_gpu_parity.py, test_gpu_large_scene.py, ...) witness the same rules on the device."""
import ctypes as C
import itertools
import math

import pytest

NONE, FLAT, WAVESYNC, LANE_SM, WAVEFRONT, PM_WAVE, PM_LANE, WAVEFRONT_PM = range(8)  # include/mcrt.h MCRT_KERNEL_*
ERR_INVALID, ERR_UNSUPPORTED = -1, -7                                              # include/mcrt.h MCRT_ERR_*
PIPELINE = (WAVEFRONT, WAVEFRONT_PM)
MAT_ROUGH_SPECULAR = 2  # include/mcrt.h: a GGX material

# The dynamic LDS a shading kernel may ask for on the MI355X: the device's 160 KiB per workgroup minus the 3 520 bytes of static LDS
# the shading kernels hold (kShadeStaticLds, csrc/mcrt_libm.hpp). Confirmed on the device: hipDeviceAttributeMaxSharedMemoryPerBlock
# reports 163 840 there.
MAX_LDS = 160 * 1024 - 3520

DONE, ERROR, AGAIN = 0, 1, 2


@pytest.fixture(scope="module")
def sel(emu):
    vp = C.c_void_p
    emu.emu_select_kernel.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int]
    emu.emu_select_kernel.restype = C.c_int
    emu.emu_next_render.argtypes = [vp, vp, vp, vp, vp, C.c_int]
    emu.emu_next_render.restype = C.c_int
    emu.emu_select_constants.argtypes = [vp]
    emu.emu_select_constants.restype = None
    emu.emu_instance_ids.argtypes = [vp]
    emu.emu_instance_ids.restype = None
    ids = (C.c_int * len(INSTANCES))()
    emu.emu_instance_ids(ids)
    ID.update(zip(INSTANCES, (int(i) for i in ids)))
    assert len(set(ID.values())) == len(INSTANCES)
    return emu


# RenderInstance ids (csrc/mcrt_select.hpp), by the names this file uses; ID is filled from the library by the fixture
INSTANCES = ["Flat512", "FlatK512", "FlatK768", "SM", "SM_Count", "PT", "PT_Prof", "PMLane", "PM1024", "PM1024_All", "PMWide", "ShadePT", "ShadePM",
             "KnnEval", "KnnEvalWide", "Trace_Count", "TraceLean", "TraceLeanSingle"]
ID = {}


def scene(flat=0, cull=0, cull_floats=0, stage_all=0, num_nodes=0, q_nodes=0, q_single=1, material_flags=0, stage_nodes=0, image_bytes=0):
    """The scene facts selectKernel takes. The LDS totals of the photon-mapping kernel's plans are the caller's (planLds, csrc/mcrt_kernels.hpp);
    here they are made from what such a plan holds: the 24 KiB Sobol table, 8-byte stack entries (none for a flat scene) and 8-byte
    refraction-history entries per lane, then the staged image - the whole scene, or at most 128 top-of-tree nodes of 56 bytes."""
    up = lambda x: (x + 15) // 16 * 16
    image = image_bytes if stage_all else up(min(stage_nodes, 128) * 56)
    plan = lambda block, depth, iors: up(24576 + (0 if flat else depth * block * 8) + iors * block * 8) + image
    return [flat, cull, cull_floats, stage_all, num_nodes, q_nodes, q_single, material_flags, plan(512, 16, 8)] + \
           [plan(block, depth, 2) for block in (512, 1024) for depth in range(2, 17, 2)]


# 44 triangles, no rough / conductor material, whole scene in LDS, 22 cull-record pairs of 32 floats: the argument block holds 704
ROOM = dict(flat=1, cull=1, cull_floats=704, stage_all=1, num_nodes=15, q_nodes=15, stage_nodes=0, image_bytes=12 * 1024)
COCKPIT = dict(num_nodes=23000, q_nodes=23000, stage_nodes=512)     # tree in memory, below MCRT_WF_MIN_NODES
HULLS = dict(num_nodes=65536, q_nodes=65536, stage_nodes=512)       # at MCRT_WF_MIN_NODES
CAUSTICS = dict(num_nodes=40000, q_nodes=40000, stage_nodes=512)    # photon-mapped, lean materials, tree in memory


def select(sel, scn, photon=0, paths=2_000_000, filtered=0, film_out=0, k=50, max_lds=MAX_LDS, force_wf=0, force_pm_lane=0, **options):
    s = (C.c_uint64 * 25)(*scene(**scn))
    f = (C.c_uint64 * 8)(photon, paths, filtered, film_out, k, max_lds, force_wf, force_pm_lane)
    keys = (C.c_char_p * max(len(options), 1))(*[k_.encode() for k_ in options])
    vals = (C.c_char_p * max(len(options), 1))(*[str(v).encode() for v in options.values()])
    out = (C.c_uint64 * 9)()
    msg = C.create_string_buffer(512)
    err = sel.emu_select_kernel(s, f, len(options), keys, vals, out, msg, 512)
    names = ("form", "instance", "knn_instance", "lean", "knn_lean", "block", "stack_depth", "trace_visit", "trace_instance")
    r = dict(zip(names, (int(v) for v in out)))
    r["err"], r["message"] = err, msg.value.decode()
    return r


def expect(r, form, block=None, lean=None, instance=None, knn=None, knn_lean=None, stack=None, trace=None):
    assert r["err"] == 0, r
    assert r["form"] == form, r
    if block is not None:
        assert r["block"] == block, r
    if lean is not None:
        assert r["lean"] == int(lean), r
    if instance is not None:
        assert r["instance"] == ID[instance], r
    if knn is not None:
        assert r["knn_instance"] == ID[knn] and r["knn_lean"] == int(knn_lean), r
    if stack is not None:
        assert r["stack_depth"] == stack, r
    if trace is not None:
        assert r["trace_instance"] == ID[trace], r


def test_flat_scene_lean_512_lanes_and_ggx_768_full(sel):
    expect(select(sel, ROOM), FLAT, block=512, lean=True, instance="FlatK512")
    expect(select(sel, dict(ROOM, material_flags=MAT_ROUGH_SPECULAR)), FLAT, block=768, lean=False, instance="FlatK768")
    # records that do not fit the argument block (or MCRT_FLAT_KARG=0): the 512-lane instance that reads them from LDS
    expect(select(sel, dict(ROOM, cull_floats=0, material_flags=MAT_ROUGH_SPECULAR)), FLAT, block=512, lean=False, instance="Flat512")
    expect(select(sel, dict(ROOM, material_flags=MAT_ROUGH_SPECULAR), MCRT_FLAT_KARG=0), FLAT, block=512, lean=False, instance="Flat512")
    expect(select(sel, ROOM, MCRT_FLAT_KARG=0), FLAT, block=512, lean=True, instance="Flat512")
    expect(select(sel, ROOM, MCRT_LEAN_KERNELS=0), FLAT, block=768, lean=False, instance="FlatK768")


def test_tree_in_memory_megakernel_until_the_frame_or_the_tree_is_large(sel):
    expect(select(sel, COCKPIT, paths=2_000_000), LANE_SM, block=512, lean=True, instance="SM", stack=16)
    expect(select(sel, COCKPIT, paths=33_000_000), WAVEFRONT, block=256, lean=True, instance="ShadePT", trace="TraceLeanSingle")
    for paths in (1, 2_000_000, 33_000_000, 10**10):
        expect(select(sel, HULLS, paths=paths), WAVEFRONT, block=256, lean=True, instance="ShadePT", trace="TraceLeanSingle")
    expect(select(sel, dict(HULLS, material_flags=MAT_ROUGH_SPECULAR, q_single=0)), WAVEFRONT, block=256, lean=False, instance="ShadePT", trace="TraceLean")
    expect(select(sel, dict(COCKPIT, material_flags=MAT_ROUGH_SPECULAR)), LANE_SM, block=512, lean=False, instance="SM", stack=16)
    # the counting and the profiling instances: full kernels only
    expect(select(sel, COCKPIT, MCRT_COUNT_TESTS=1), LANE_SM, block=512, lean=False, instance="SM_Count")
    expect(select(sel, HULLS, MCRT_COUNT_TESTS=1), WAVEFRONT, block=256, lean=False, instance="ShadePT", trace="Trace_Count")
    expect(select(sel, COCKPIT, MCRT_KERNEL="legacy", MCRT_PROFILE_PHASES=1), WAVESYNC, block=512, lean=False, instance="PT_Prof")


def test_photon_mapped_frames(sel):
    expect(select(sel, CAUSTICS, photon=1, k=50, paths=32_000_000), WAVEFRONT_PM, block=256, lean=True, instance="ShadePM", knn="KnnEval", knn_lean=True,
           trace="TraceLeanSingle")
    # below the rule: 1024 lanes; of the 160 320 bytes, table + two history entries + 128 nodes + 16 waves' candidate buffers take 105 728,
    # which leaves 6 stack entries per lane (8 KiB each step); the tree-in-memory instance keeps its full form
    expect(select(sel, CAUSTICS, photon=1, k=50, paths=31_999_999), PM_WAVE, block=1024, lean=False, instance="PM1024", stack=6)
    # the wide rows (k > 128): 512 lanes, 8 waves' buffers of 12 816 bytes leave 4 entries per lane; never through the pipeline by themselves
    for paths in (2_000_000, 64_000_000):
        expect(select(sel, CAUSTICS, photon=1, k=200, paths=paths), PM_WAVE, block=512, lean=False, instance="PMWide", stack=4)
        expect(select(sel, CAUSTICS, photon=1, k=1000, paths=paths), PM_LANE, block=512, lean=False, instance="PMLane", stack=16)
    # a scene with rough materials has no lean kNN launch: the megakernel at any size
    expect(select(sel, dict(CAUSTICS, material_flags=MAT_ROUGH_SPECULAR), photon=1, k=50, paths=64_000_000), PM_WAVE, block=1024, lean=False, instance="PM1024", stack=6)
    # LDS-resident scenes: the lean 1024-lane instance, no traversal stack to shorten
    expect(select(sel, ROOM, photon=1, k=50, paths=64_000_000), PM_WAVE, block=1024, lean=True, instance="PM1024_All", stack=16)
    # MCRT_PROFILE_PHASES leaves the form alone and runs the full kernels
    expect(select(sel, CAUSTICS, photon=1, k=50, paths=32_000_000, MCRT_PROFILE_PHASES=1), WAVEFRONT_PM, block=256, lean=False, instance="ShadePM",
           knn="KnnEval", knn_lean=False)
    expect(select(sel, CAUSTICS, photon=1, k=200, paths=2_000_000, MCRT_KERNEL="wf"), WAVEFRONT_PM, block=256, lean=True, instance="ShadePM",
           knn="KnnEvalWide", knn_lean=False)


@pytest.mark.parametrize("kernel,room,cockpit_small,cockpit_large,hulls,pm50_small,pm50_large,pm200,pm1000", [
    ("wf", WAVEFRONT, WAVEFRONT, WAVEFRONT, WAVEFRONT, WAVEFRONT_PM, WAVEFRONT_PM, WAVEFRONT_PM, PM_LANE),
    ("sm", FLAT, LANE_SM, LANE_SM, LANE_SM, PM_WAVE, PM_WAVE, PM_WAVE, PM_LANE),
    ("legacy", FLAT, WAVESYNC, WAVESYNC, WAVESYNC, PM_LANE, PM_LANE, PM_LANE, PM_LANE),
])
def test_mcrt_kernel_option(sel, kernel, room, cockpit_small, cockpit_large, hulls, pm50_small, pm50_large, pm200, pm1000):
    o = dict(MCRT_KERNEL=kernel)
    # every scene here has lean materials: the pipeline, the state machine and the flat loop run lean, the wave-synchronous kernels and
    # the photon-mapping kernel of a tree in memory have no lean twin
    shape = {FLAT: (512, True), LANE_SM: (512, True), WAVESYNC: (512, False), WAVEFRONT: (256, True), WAVEFRONT_PM: (256, True), PM_LANE: (512, False)}
    def check(r, form, pm_block=None):
        block, lean = (pm_block, False) if form == PM_WAVE else shape[form]
        expect(r, form, block=block, lean=lean)
    check(select(sel, ROOM, **o), room)
    check(select(sel, COCKPIT, paths=2_000_000, **o), cockpit_small)
    check(select(sel, COCKPIT, paths=33_000_000, **o), cockpit_large)
    check(select(sel, HULLS, **o), hulls)
    check(select(sel, CAUSTICS, photon=1, k=50, paths=2_000_000, **o), pm50_small, 1024)
    check(select(sel, CAUSTICS, photon=1, k=50, paths=32_000_000, **o), pm50_large, 1024)
    check(select(sel, CAUSTICS, photon=1, k=200, **o), pm200, 512)
    check(select(sel, CAUSTICS, photon=1, k=1000, **o), pm1000)


def test_refusals(sel):
    r = select(sel, dict(ROOM, q_nodes=0), filtered=1)
    assert r["err"] == ERR_UNSUPPORTED and "reconstruction filters need the wavefront pipeline" in r["message"]
    r = select(sel, CAUSTICS, photon=1, k=769, filtered=1)
    assert r["err"] == ERR_UNSUPPORTED and "k_nearest_photons <= 768" in r["message"]
    expect(select(sel, CAUSTICS, photon=1, k=768, filtered=1), WAVEFRONT_PM)
    expect(select(sel, ROOM, filtered=1), WAVEFRONT)
    r = select(sel, COCKPIT, film_out=1)
    assert r["err"] == ERR_INVALID and "splatted frames" in r["message"]


def test_trace_visit(sel):
    assert select(sel, HULLS)["trace_visit"] == 3
    assert select(sel, dict(HULLS, q_single=0))["trace_visit"] == 1
    assert select(sel, HULLS, MCRT_WF_LEAN=2)["trace_visit"] == 1
    assert select(sel, HULLS, MCRT_WF_LEAN=0)["trace_visit"] == 0
    assert select(sel, HULLS, MCRT_COUNT_TESTS=1)["trace_visit"] == 0


GRID_SCENES = [dict(s, material_flags=m) for s in (ROOM, dict(ROOM, cull_floats=0), dict(ROOM, flat=0, cull=0, cull_floats=0, image_bytes=8 * 1024), COCKPIT, HULLS, CAUSTICS,
                                                    dict(COCKPIT, q_nodes=0, num_nodes=0), dict(COCKPIT, q_single=0))
               for m in (0, MAT_ROUGH_SPECULAR)]
GRID_OPTIONS = [dict(), dict(MCRT_KERNEL="wf"), dict(MCRT_KERNEL="sm"), dict(MCRT_KERNEL="legacy"), dict(MCRT_COUNT_TESTS=1), dict(MCRT_PROFILE_PHASES=1),
                dict(MCRT_COUNT_TESTS=1, MCRT_KERNEL="wf"), dict(MCRT_PROFILE_PHASES=1, MCRT_KERNEL="wf"), dict(MCRT_LEAN_KERNELS=0),
                dict(MCRT_WF_MIN_PATHS=1000), dict(MCRT_WF_PM_MIN_PATHS=1000), dict(MCRT_WF_MIN_NODES=1000), dict(MCRT_FLAT_KARG=0)]
GRID_FRAMES = [dict(photon=p, k=k, force_wf=fw, force_pm_lane=fl) for p, k in ((0, 50), (1, 50), (1, 128), (1, 129), (1, 768), (1, 769))
               for fw in (0, 1) for fl in (0, 1)]
GRID_PATHS = [1, 1000, 2_000_000, 31_999_999, 32_000_000, 133_000_000, 10**11]


def test_properties_over_a_grid(sel):
    n = 0
    for scn, opt, frame in itertools.product(GRID_SCENES, GRID_OPTIONS, GRID_FRAMES):
        was_pipeline = False
        for paths in GRID_PATHS:
            r = select(sel, scn, paths=paths, **frame, **opt)
            assert r["err"] == 0, (scn, opt, frame, r)
            # raising the frame's path samples never moves a frame from the pipeline back to a megakernel
            assert not (was_pipeline and r["form"] not in PIPELINE), (scn, opt, frame, paths, r)
            was_pipeline = r["form"] in PIPELINE
            # the counting and the profiling instances have no lean twin
            if "MCRT_COUNT_TESTS" in opt or "MCRT_PROFILE_PHASES" in opt or "MCRT_LEAN_KERNELS" in opt or scn["material_flags"]:
                assert not r["lean"] and not r["knn_lean"], (scn, opt, frame, paths, r)
            if frame["force_pm_lane"]:
                assert r["form"] not in (PM_WAVE, WAVEFRONT_PM), (scn, opt, frame, paths, r)
            if frame["force_wf"] and scn["q_nodes"] and not frame["photon"]:
                assert r["form"] == WAVEFRONT
            assert r["block"] in (256, 512, 768, 1024) and 2 <= r["stack_depth"] <= 16
            n += 1
    assert n == len(GRID_SCENES) * len(GRID_OPTIONS) * len(GRID_FRAMES) * len(GRID_PATHS)


def _next(sel, state, kernel_id, h5, h7, splats, can_pipeline):
    st = (C.c_uint64 * 4)(*state)
    oc = (C.c_uint64 * 5)(kernel_id, h5, h7, splats, can_pipeline)
    nxt = (C.c_uint64 * 4)()
    err = C.c_int(0)
    msg = C.create_string_buffer(512)
    action = sel.emu_next_render(st, oc, nxt, C.byref(err), msg, 512)
    return action, err.value, msg.value.decode(), [int(v) for v in nxt]


def test_every_render_again_chain_ends(sel):
    """select -> the same flags come back -> next state, until "done" or "error". Each step that renders again either raises a flag that was
    down (force_pm_lane, force_wf: two steps), grows the per-lane frontier eightfold (from 160 towards its limit) or the refraction-history
    rows fourfold (from 32 towards theirs); one more step reports the end. A frame rendered again is never rendered the way it just was:
    the form changes or a capacity grows. (Before this decision was one function, the chain {photon mapper, force_pm_lane, word 7} did
    not end: the per-lane kernel's frame was rendered again by the per-lane kernel, with nothing changed.)"""
    k = (C.c_uint64 * 6)()
    sel.emu_select_constants(k)
    visit0, visit_limit, iors0, iors_limit, knn_flag, _ = (int(v) for v in k)
    bound = math.ceil(math.log(visit_limit / visit0, 8)) + math.ceil(math.log(iors_limit / iors0, 4)) + 3
    chains = 0
    for photon, force_wf, force_pm_lane, visit, iors, h5, h7, splats, pipeline_possible in itertools.product(
            (0, 1), (0, 1), (0, 1), (visit0, visit_limit), (iors0, iors_limit), (0, 3, knn_flag), (0, 1), (0, 1), (0, 1)):
        scn = CAUSTICS if pipeline_possible else dict(CAUSTICS, q_nodes=0)
        for first_form in (None, FLAT, WAVESYNC, LANE_SM, WAVEFRONT, PM_WAVE, PM_LANE, WAVEFRONT_PM):
            state = [force_wf, force_pm_lane, visit, iors]
            steps, form = 0, first_form
            while True:
                if form is None:  # what selectKernel gives for this state (a splatted frame is a filtered one)
                    r = select(sel, scn, photon=photon, k=50, filtered=splats, force_wf=state[0], force_pm_lane=state[1])
                    if r["err"]:
                        break
                    form = r["form"]
                action, err, msg, nxt = _next(sel, state, form, h5, h7, splats, pipeline_possible)
                steps += 1
                assert steps <= bound, (photon, force_wf, force_pm_lane, visit, iors, h5, h7, splats, pipeline_possible, first_form)
                if action == DONE:
                    assert not h5 and not h7
                    break
                if action == ERROR:
                    assert err == ERR_UNSUPPORTED and msg
                    if splats and h5 >= knn_flag:
                        assert "splatted" in msg
                    break
                assert action == AGAIN and (h5 or h7)
                r = select(sel, scn, photon=photon, k=50, filtered=splats, force_wf=nxt[0], force_pm_lane=nxt[1])
                grown = nxt[2] > state[2] or nxt[3] > state[3]
                assert grown or r["err"] or r["form"] != form, ("rendered again the way it just was", state, nxt, form)
                state, form = nxt, None
            chains += 1
    assert chains == 2 ** 8 * 3 * 8


def test_per_lane_frame_that_nests_too_deep_is_refused(sel):
    """The frame of the per-lane kernel that stands in for overflowed wave-cooperative searches (force_pm_lane) and then reports a
    refraction history deeper than its 8 entries: MCRT_ERR_UNSUPPORTED, not another frame."""
    action, err, msg, _ = _next(sel, [0, 1, 2048, 32], PM_LANE, 0, 1, 0, 1)
    assert action == ERROR and err == ERR_UNSUPPORTED and "nested dielectric media" in msg
    # without the flag the same frame goes to the pipeline, as before
    action, _, _, nxt = _next(sel, [0, 0, 160, 32], PM_LANE, 0, 1, 0, 1)
    assert action == AGAIN and nxt == [1, 0, 160, 32]


def test_recovery_steps_keep_their_factors(sel):
    flag = 0x10000
    assert _next(sel, [0, 0, 160, 32], PM_WAVE, flag, 0, 0, 1)[3] == [0, 1, 2048, 32]
    assert _next(sel, [0, 1, 2048, 32], PM_LANE, flag, 0, 0, 1)[3] == [0, 1, 16384, 32]
    assert _next(sel, [0, 1, 16384, 32], PM_LANE, flag, 0, 0, 1)[3] == [0, 1, 32768, 32]
    assert _next(sel, [0, 1, 32768, 32], PM_LANE, flag, 0, 0, 1)[0] == ERROR
    assert _next(sel, [0, 0, 160, 32], LANE_SM, 0, 1, 0, 1)[3] == [1, 0, 160, 32]
    assert _next(sel, [1, 0, 160, 32], WAVEFRONT, 0, 1, 0, 1)[3] == [1, 0, 160, 128]
    assert _next(sel, [1, 0, 160, 32768], WAVEFRONT, 0, 1, 0, 1)[0] == ERROR
    assert _next(sel, [0, 0, 160, 32], LANE_SM, 0, 1, 0, 0)[0] == ERROR      # a scene the pipeline cannot take
    assert _next(sel, [0, 0, 160, 32], WAVEFRONT_PM, flag, 0, 1, 1)[0] == ERROR  # only the pipeline splats
    assert _next(sel, [0, 0, 160, 32], LANE_SM, 3, 0, 0, 1)[0] == ERROR      # traversal-stack overflow: internal error
    assert _next(sel, [0, 0, 160, 32], LANE_SM, 0, 0, 0, 1)[0] == DONE
