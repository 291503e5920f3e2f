"""The kernel instances behind the diagnostic options, on the GPU: MCRT_COUNT_TESTS (PT_Count*, PMLane_Count*, SM_Count*, PM1024_Count*,
PMWide_Count*, Trace_Count), MCRT_PROFILE_PHASES (PT_Prof*, SM_Prof*) and MCRT_WF_PM_EVAL=0 (KnnRaw, KnnRawWide). They are separate
code objects with their own register and LDS budgets, a flat scene even changes its kernel FORM as soon as counting is on, and every
number in DESIGN.md and profiles/ about tests per ray, phases and lane utilisation comes out of them - so here they are held to

  1. the frame: the bits, paths, rays and searches of the instance the same call runs without the option (whose frame the other GPU
     tests hold to the reference's), by one pass and three, by one chunk per pixel and four, and as two row shards;
  2. the counters: zero without the option (on dirty memory: conftest's autouse fixture), within what include/mcrt.h says of them with
     it, and - where they are sums of per-ray quantities - the same number from every one of those schedules and from the host emulation
     of the same instance (tests/emu/wave_kernel_emu.cpp);
  3. the readouts on stderr: well-formed, and only of what the instance that ran measured.

Every case pins the instances that ran through the read-only option MCRT_INSTANCES_USED ("frame,trace,knn" by RenderInstance name,
csrc/mcrt_select.hpp): a silent fallback to another instance fails. profiles/NOTES_diagnostic_kernels.md maps instance to test and
records what was measured for the counters that depend on the schedule."""
import math
import os
import re

import numpy as np
import pytest

from conftest import golden_path, load_radiance, rel_error
from test_wave_emulation import (FRAME, SMALL_FRAME, check_counter_bounds, diagnostic_scene, emulated_megakernel_frame, emulated_pipeline_frame)

pytestmark = pytest.mark.gpu

SMOOTH_TOL = 1e-12  # tests/test_gpu_parity.py: photon-mapped frames, sums in another order
OPTIONS = ("MCRT_KERNEL", "MCRT_COUNT_TESTS", "MCRT_PROFILE_PHASES", "MCRT_WF_PM_EVAL", "MCRT_CHUNKS", "MCRT_SAMPLE_STORE_GB", "MCRT_FLAT_MAX", "MCRT_WF_LEAN",
           "MCRT_LEAN_KERNELS")


@pytest.fixture
def env():
    old = {k: os.environ.get(k) for k in OPTIONS}
    for k in OPTIONS:
        os.environ.pop(k, None)
    yield os.environ
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


class Rendering:
    """One scene on one context; render(**options) sets the MCRT_* options for that frame only."""

    def __init__(self, pkg, env, img, photon, flat_max=None, k=None):
        self.pkg, self.env, self.img = pkg, env, img
        self.integ = pkg.INTEGRATOR_PHOTON_MAPPER if photon else pkg.INTEGRATOR_PATH_TRACER
        if flat_max is not None:
            env["MCRT_FLAT_MAX"] = str(flat_max)  # (read when the scene is uploaded)
        self.ctx = pkg.Context(0)
        self.ctx.upload_scene(img.scene)
        if photon:
            self.ctx.upload_photons(img.photons(0), img.photons(1), k or img.param("k_nearest_photons") or 50, False)
        env.pop("MCRT_FLAT_MAX", None)

    def render(self, cam, seed, **options):
        for key, value in options.items():
            self.env["MCRT_" + key] = str(value)
        try:
            out, st = self.ctx.sample_image(cam, seed, self.integ)
        finally:
            for key in options:
                self.env.pop("MCRT_" + key, None)
        st["instances"] = [w.split("/")[0] for w in self.ctx.get_option("MCRT_INSTANCES_USED").split(",")]
        return out, st

    def close(self):
        self.ctx.close()


def _schedules(r, cam, seed, **options):
    """The frame by three passes, by one and by four chunks per pixel, and as two shards of eight-row groups -> [(what, frame, stats)];
    the shards' frames and counters added up (a shard's frame is zero outside its rows)."""
    runs = []
    out, st = r.render(cam, seed, SAMPLE_STORE_GB="1e-6", **options)
    runs.append(("three passes", out, st))
    for chunks in (1, 4):
        out, st = r.render(cam, seed, CHUNKS=chunks, **options)
        runs.append(("%d chunk(s) per pixel" % chunks, out, st))
    parts = []
    for index in (0, 1):
        shard = cam.copy()
        shard.shard_rows, shard.shard_count, shard.shard_index = 8, 2, index
        parts.append(r.render(shard, seed, **options))
    total = dict(parts[0][1])
    for key in ("paths", "rays", "node_tests", "prim_tests", "knn_searches"):
        total[key] = parts[0][1][key] + parts[1][1][key]
    assert parts[0][1]["instances"] == parts[1][1]["instances"]
    runs.append(("two row shards", parts[0][0] + parts[1][0], total))
    return runs


# Counters that depend on the schedule: the shared leaf step (csrc/mcrt_sharedleaf.hpp) defers a lane's leaf until enough lanes of ITS wave
# wait at one, and meanwhile the lane walks on with the hit it has - so which rays share a wave, and when, decides how many boxes and
# primitives are tested for them. Relative spread allowed around the emulation's value (one workgroup, waves taking turns): what the
# MI355X showed over the schedules of _schedules, and a margin - profiles/NOTES_diagnostic_kernels.md has the numbers.
SCHEDULE_DEPENDENT_REL = {"PM1024_Count": 5e-3, "PMWide_Count": 5e-3, "Trace_Count": 5e-3}

# (scene, photon-mapped, MCRT_KERNEL, MCRT_FLAT_MAX, k, form without / with MCRT_COUNT_TESTS, instances "frame,trace,knn" with it,
#  what the emulation runs for the comparison: "same", "lane" = the per-lane instance of the same scene (the LDS-resident photon-mapping
#  kernels trace the same rays through the same sceneIntersect: test_photon_mapping_instances_count_the_same_tests_per_ray_on_the_host),
#  "small" = the same instance at SMALL_FRAME (a wave-cooperative search takes the emulation 4 ms), None = not emulated)
COUNTING = [
    ("hexagon_room_diffuse", False, None, None, None, "FLAT", "WAVESYNC", "PT_CountAll,-,-", "same"),
    ("hexagon_room_diffuse", False, None, 0, None, "LANE_SM", "LANE_SM", "SM_CountAll,-,-", "same"),
    ("hexagon_room_diffuse", False, "legacy", 0, None, "WAVESYNC", "WAVESYNC", "PT_CountAll,-,-", "same"),
    ("coffee_maker_qsah", False, None, None, None, "LANE_SM", "LANE_SM", "SM_Count,-,-", "same"),
    ("coffee_maker_qsah", False, "legacy", None, None, "WAVESYNC", "WAVESYNC", "PT_Count,-,-", "same"),
    ("coffee_maker_qsah", False, "wf", None, None, "WAVEFRONT", "WAVEFRONT", "ShadePT,Trace_Count,-", "same"),
    ("quadric", False, "wf", None, None, "WAVEFRONT", "WAVEFRONT", "ShadePT,Trace_Count,-", "same"),
    ("hexagon_room_pm", True, None, None, None, "PM_WAVE", "PM_WAVE", "PM1024_CountAll,-,-", "lane"),
    ("hexagon_room_pm", True, "legacy", None, None, "PM_LANE", "PM_LANE", "PMLane_CountAll,-,-", "same"),
    ("hexagon_room_pm", True, None, None, 129, "PM_WAVE", "PM_WAVE", "PMWide_CountAll,-,-", "lane"),
    ("hexagon_room_pm", True, "wf", None, None, "WAVEFRONT_PM", "WAVEFRONT_PM", "ShadePM,Trace_Count,KnnEval", None),
    ("coffee_maker_qsah+photons", True, None, None, None, "PM_WAVE", "PM_WAVE", "PM1024_Count,-,-", "small"),
    ("coffee_maker_qsah+photons", True, "legacy", None, None, "PM_LANE", "PM_LANE", "PMLane_Count,-,-", "same"),
    ("coffee_maker_qsah+photons", True, None, None, 129, "PM_WAVE", "PM_WAVE", "PMWide_Count,-,-", "small"),
]


@pytest.mark.parametrize("name,photon,kernel,flat_max,k,form,form_counting,instances,emulate", COUNTING)
def test_counting_instance_renders_the_frame_and_counts_what_the_header_says(pkg, wave_kernel_emu, oracle, manifest, env, name, photon, kernel, flat_max, k,
                                                                              form, form_counting, instances, emulate):
    """(module docstring, 1 and 2.) Schedule-independent are the counters of every walk in which a lane counts what ITS ray tests and nothing
    decides that but the ray: sceneIntersect (wave-synchronous kernel, flat loop behind the cull, per-lane and LDS-resident photon-mapping
    kernels) and the state machine's steps (csrc/mcrt_lanesm.hpp). Not so the shared leaf step (SCHEDULE_DEPENDENT_REL)."""
    img, cam = diagnostic_scene(pkg, oracle, manifest, name)
    cam.width, cam.height, cam.sqrtspp = FRAME
    seed = manifest["seed"]
    options = {"KERNEL": kernel} if kernel else {}
    r = Rendering(pkg, env, img, photon, flat_max, k)
    try:
        plain, st0 = r.render(cam, seed, **options)
        assert st0["kernel_id"] == getattr(pkg, "KERNEL_" + form)
        assert st0["node_tests"] == st0["prim_tests"] == 0
        out, st = r.render(cam, seed, COUNT_TESTS=1, **options)
        assert st["kernel_id"] == getattr(pkg, "KERNEL_" + form_counting) and ",".join(st["instances"]) == instances
        np.testing.assert_array_equal(out, plain)
        assert st["paths"] == st0["paths"] == cam.width * cam.height * cam.sqrtspp ** 2 and st["rays"] == st0["rays"]
        assert st["knn_searches"] == st0["knn_searches"] and (st["knn_searches"] > 0) == photon
        flat = name.startswith("hexagon_room") and flat_max is None and kernel != "wf"
        words = [st["paths"], st["rays"], st["node_tests"], st["prim_tests"]]
        check_counter_bounds(img, words, out, flat)
        counted = instances.split(",")[1] if kernel == "wf" else instances.split(",")[0]
        per_ray = counted not in SCHEDULE_DEPENDENT_REL
        runs = _schedules(r, cam, seed, COUNT_TESTS=1, **options)
        values = [(st["node_tests"], st["prim_tests"])]
        for what, frame, s in runs:
            assert ",".join(s["instances"]) == instances, what
            np.testing.assert_array_equal(frame, plain, err_msg=what)
            assert (s["paths"], s["rays"], s["knn_searches"]) == (st["paths"], st["rays"], st["knn_searches"]), what
            if what == "three passes":  # (... and the counters are the sum over the passes: each pass alone has fewer rays)
                assert s["kernel_launches"] > st["kernel_launches"]
            values.append((s["node_tests"], s["prim_tests"]))
            if per_ray:
                assert values[-1] == values[0], "%s: %s counts %s, one pass %s" % (counted, what, values[-1], values[0])
        if emulate is None:
            return
        small = emulate == "small"
        if small:
            cam.width, cam.height, cam.sqrtspp = SMALL_FRAME
            out_s, st_s = r.render(cam, seed, COUNT_TESTS=1, **options)
            values = [(st_s["node_tests"], st_s["prim_tests"])] + [(s["node_tests"], s["prim_tests"]) for _, _, s in _schedules(r, cam, seed, COUNT_TESTS=1, **options)]
        if kernel == "wf":
            _, emu = emulated_pipeline_frame(wave_kernel_emu, img, cam, seed, r.integ, True)
        else:
            _, emu, ran = emulated_megakernel_frame(pkg, wave_kernel_emu, img, cam, seed, r.integ, True, kernel == "legacy" or emulate == "lane",
                                                    64 if flat_max is None else flat_max, k)
            assert ran == (counted if emulate != "lane" else "PMLane_CountAll")
        print("%s: node / primitive tests %s over the schedules, emulation %s" % (counted, sorted(set(values)), (emu[2], emu[3])))
        if per_ray:
            assert values[0] == (emu[2], emu[3])
        else:
            tol = SCHEDULE_DEPENDENT_REL[counted]
            for v in values:
                for got, want in zip(v, (emu[2], emu[3])):
                    assert abs(got - want) <= tol * want, "%s: %d against the emulation's %d" % (counted, got, want)
    finally:
        r.close()


PHASES = ["regen", "trav/inner", "shade", "shadow/leaf", "sample", "loop"]
# the readouts' lines (tests/test_stats_words.py matches hand-made words with the same expressions, without a GPU)
PHASE_LINE = r"^\[mcrt phase\] (\S+)\s+wave-cycles\s+([0-9.naif-]+)%\s+lane utilisation\s+([0-9.naif-]+)%$"
TRACE_PER_RAY = r"per ray: ([0-9.]+) inner steps, ([0-9.]+) leaf steps \((\d+) inner and (\d+) leaf lane steps of (\d+) rays\)"
PM_LINE = r"^\[mcrt pm\] wave cycles inside the radiance estimates: ([0-9.]+)% of the kernel \((\d+) searches, ([0-9.]+) octants per search\)$"


def _phase_lines(err):
    rows = re.findall(PHASE_LINE, err, re.M)
    return [(n, float(a), float(b)) for n, a, b in rows]


def _no_nan(err):
    assert not re.search(r"\b(nan|inf)\b", err, re.I), err


@pytest.mark.parametrize("name,kernel,flat_max,form,instance", [
    ("hexagon_room_diffuse", None, None, "WAVESYNC", "PT_ProfAll"), ("hexagon_room_diffuse", None, 0, "LANE_SM", "SM_ProfAll"),
    ("hexagon_room_diffuse", "legacy", 0, "WAVESYNC", "PT_ProfAll"), ("coffee_maker_qsah", None, None, "LANE_SM", "SM_Prof"),
    ("coffee_maker_qsah", "legacy", None, "WAVESYNC", "PT_Prof")])
def test_profiling_instance_renders_the_frame_and_prints_its_phases(pkg, oracle, manifest, env, capfd, name, kernel, flat_max, form, instance):
    """MCRT_PROFILE_PHASES: the plain instance's bits and rays, no test counters, and on stderr one [mcrt phase] line per phase - wave-cycle
    shares that add up to 100 % within the rounding of six numbers printed to 0.01, lane utilisations in [0, 100], cycles in the shade
    phase and in a traversal phase - once per frame, also for three passes (the phase words add up like the counters). (The wave-synchronous
    instances read 122 to 167 % in the loop phase while every lane charged its own cycles, waiting included: PhaseProf::mark,
    csrc/mcrt_integrator.hpp.)"""
    img, cam = diagnostic_scene(pkg, oracle, manifest, name)
    cam.width, cam.height, cam.sqrtspp = FRAME
    options = {"KERNEL": kernel} if kernel else {}
    r = Rendering(pkg, env, img, False, flat_max)
    try:
        plain, st0 = r.render(cam, manifest["seed"], **options)
        capfd.readouterr()
        for more in ({}, {"SAMPLE_STORE_GB": "1e-6"}, {"COUNT_TESTS": 1}):  # (with both options the profiling instance runs: it has no counters)
            out, st = r.render(cam, manifest["seed"], PROFILE_PHASES=1, **options, **more)
            err = capfd.readouterr().err
            assert st["kernel_id"] == getattr(pkg, "KERNEL_" + form) and st["instances"] == [instance, "-", "-"]
            np.testing.assert_array_equal(out, plain)
            assert (st["paths"], st["rays"]) == (st0["paths"], st0["rays"]) and st["node_tests"] == st["prim_tests"] == 0
            rows = _phase_lines(err)
            print("%s%s:\n%s" % (instance, " " + str(more) if more else "", err.rstrip()))
            assert [n for n, _, _ in rows] == PHASES, err
            _no_nan(err)
            assert "[mcrt trace]" not in err and "[mcrt pm]" not in err
            assert abs(sum(a for _, a, _ in rows) - 100.0) <= 6 * 0.005 + 1e-9
            assert all(0.0 <= a <= 100.0 and 0.0 <= b <= 100.0 for _, a, b in rows)
            share = {n: a for n, a, _ in rows}
            assert share["shade"] > 0.0 and (share["trav/inner"] > 0.0 or share["shadow/leaf"] > 0.0)
    finally:
        r.close()


def _numbers(line):
    return [float(x) for x in re.findall(r"(?<![\w.])-?\d+(?:\.\d+)?(?![\w.])", line)]


@pytest.mark.parametrize("name", ["coffee_maker_qsah", "quadric"])
def test_trace_readout_is_well_formed(pkg, oracle, manifest, env, capfd, name):
    """[mcrt trace] of a pipeline frame under MCRT_COUNT_TESTS: every number finite, percentages in [0, 100], lanes per step in [0, 64], and
    the per-ray steps it prints are the lane steps it prints divided by the rays it prints - which are the frame's (mcrt_stats.rays); an
    inner lane step tests the children of one node, one to eight boxes, so node_tests lies between the inner lane steps and eight times
    them plus a root test per ray. With MCRT_PROFILE_PHASES on top nothing else appears: the pipeline has no profiling instance, and the
    phase readout used to print the trace kernel's words 8 to 19 as phases."""
    img, cam = diagnostic_scene(pkg, oracle, manifest, name)
    cam.width, cam.height, cam.sqrtspp = FRAME
    r = Rendering(pkg, env, img, False)
    try:
        for more in ({}, {"PROFILE_PHASES": 1}):
            capfd.readouterr()
            out, st = r.render(cam, manifest["seed"], KERNEL="wf", COUNT_TESTS=1, **more)
            err = capfd.readouterr().err
            assert st["instances"] == ["ShadePT", "Trace_Count", "-"]
            _no_nan(err)
            assert "[mcrt phase]" not in err and "[mcrt pm]" not in err
            lines = [l for l in err.splitlines() if l.startswith("[mcrt trace]")]
            assert len(lines) == 1, err
            line = lines[0]
            print(line)
            assert all(0.0 <= float(p) <= 100.0 for p in re.findall(r"(-?[0-9.]+)%", line)) and len(re.findall(r"%", line)) == 7
            assert all(0.0 <= float(x) <= 64.0 for x in re.findall(r"(-?[0-9.]+) (?:leaf )?lanes", line))
            m = re.search(TRACE_PER_RAY, line)
            assert m, line
            inner_per_ray, leaf_per_ray, inner, leaf, rays = float(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))
            assert rays == st["rays"] and inner > 0 and leaf > 0
            assert abs(inner_per_ray - inner / rays) <= 0.005 + 1e-9 and abs(leaf_per_ray - leaf / rays) <= 0.005 + 1e-9
            assert inner <= st["node_tests"] <= 8 * inner + rays
            assert all(math.isfinite(x) for x in _numbers(line))
    finally:
        r.close()


def test_photon_mapping_readout_is_well_formed(pkg, oracle, manifest, env, capfd):
    """[mcrt pm] of the wave-cooperative photon-mapping kernel under MCRT_COUNT_TESTS: a share in [0, 100] of a non-zero clock, the frame's
    searches; no phase line with MCRT_PROFILE_PHASES on top (the photon kernels have no profiling instance), and nothing at all with
    MCRT_PROFILE_PHASES alone - by the megakernel or by the pipeline - whose frame is the plain frame."""
    img, cam = diagnostic_scene(pkg, oracle, manifest, "hexagon_room_pm")
    cam.width, cam.height, cam.sqrtspp = FRAME
    r = Rendering(pkg, env, img, True)
    try:
        plain, st0 = r.render(cam, manifest["seed"])
        for more in ({}, {"PROFILE_PHASES": 1}):
            capfd.readouterr()
            out, st = r.render(cam, manifest["seed"], COUNT_TESTS=1, **more)
            err = capfd.readouterr().err
            assert st["instances"] == ["PM1024_CountAll", "-", "-"]
            _no_nan(err)
            assert "[mcrt phase]" not in err and "[mcrt trace]" not in err
            m = re.findall(PM_LINE, err, re.M)
            assert len(m) == 1, err
            print(err.rstrip())
            assert 0.0 < float(m[0][0]) <= 100.0 and int(m[0][1]) == st["knn_searches"] and float(m[0][2]) >= 1.0
        for kernel in (None, "wf", "legacy"):
            capfd.readouterr()
            out, st = r.render(cam, manifest["seed"], PROFILE_PHASES=1, **({"KERNEL": kernel} if kernel else {}))
            err = capfd.readouterr().err
            assert "[mcrt" not in err, err
            assert rel_error(out, plain).max() <= SMOOTH_TOL and st["node_tests"] == st["prim_tests"] == 0
            if kernel is None:
                np.testing.assert_array_equal(out, plain)
    finally:
        r.close()


def test_nothing_is_read_out_of_a_frame_that_measured_nothing(pkg, oracle, manifest, env, capfd):
    """A shard that owns no row launches nothing: with every diagnostic option set the readouts have no clock to divide by. Nothing is
    printed - no line of zeros, no nan - and the statistics are zero. The same call on a shard that owns rows prints its line."""
    img, cam = diagnostic_scene(pkg, oracle, manifest, "coffee_maker_qsah")
    cam.width, cam.height, cam.sqrtspp = FRAME
    cam.shard_rows, cam.shard_count = 8, 4  # rows 0-7, 8-15, 16-20 and none
    r = Rendering(pkg, env, img, False)
    try:
        for kernel, tag in (("wf", "[mcrt trace]"), ("sm", "[mcrt phase]")):
            for index in (3, 2):
                cam.shard_index = index
                capfd.readouterr()
                out, st = r.render(cam, manifest["seed"], KERNEL=kernel, COUNT_TESTS=1, PROFILE_PHASES=1)
                err = capfd.readouterr().err
                _no_nan(err)
                if index == 3:
                    assert "[mcrt" not in err, err
                    assert st["kernel_id"] == pkg.KERNEL_NONE and st["instances"] == ["-", "-", "-"]
                    assert st["paths"] == st["rays"] == st["node_tests"] == st["prim_tests"] == 0 and not out.any()
                else:
                    assert tag in err and st["paths"] == cam.width * 5 * cam.sqrtspp ** 2
    finally:
        r.close()


@pytest.mark.parametrize("k,instance", [(None, "KnnRaw"), (129, "KnnRawWide")])
def test_raw_knn_launch_renders_the_reference_frame(pkg, oracle, manifest, env, k, instance):
    """MCRT_WF_PM_EVAL=0: the kNN launch hands the k photons of a search back (wfKnnKernel<false>; k = 129: with the wide candidate buffer)
    and the shade launch sums them per lane (wfPhotonEstimate, csrc/mcrt_wavefront.hpp) - one after the other in the order of the candidate
    buffer, where the evaluating launch adds the same contributions by a wave reduction (waveEvalPhotons). Same photons, another order of the
    FP64 sum: the reference's golden frame to the bar of photon-mapped frames (1e-12), NOT the default pipeline's bits. k = 129 has no golden
    frame: the oracle's, which is the reference's for every k the goldens have, at the ragged frame."""
    case = manifest["cases"]["hexagon_room_pm"]
    img, cam = diagnostic_scene(pkg, oracle, manifest, "hexagon_room_pm")
    if k is None:
        want = load_radiance(case["renders"][0])
    else:
        cam.width, cam.height, cam.sqrtspp = FRAME
        want, _ = oracle.render(img, cam, manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER, k=k)
    r = Rendering(pkg, env, img, True, None, k)
    try:
        ev, st_ev = r.render(cam, manifest["seed"], KERNEL="wf")
        raw, st = r.render(cam, manifest["seed"], KERNEL="wf", WF_PM_EVAL=0)
        assert st["kernel_id"] == pkg.KERNEL_WAVEFRONT_PM and st["instances"][0] == "ShadePM" and st["instances"][2] == instance
        assert st_ev["instances"][2] == ("KnnEval" if k is None else "KnnEvalWide")
        assert (st["paths"], st["rays"], st["knn_searches"]) == (st_ev["paths"], st_ev["rays"], st_ev["knn_searches"]) and st["knn_searches"] > 0
        rel = rel_error(raw, want)
        print("%s: max rel %.3e against the reference, %.3e against the evaluating launch" % (instance, rel.max(), rel_error(raw, ev).max()))
        assert rel.max() <= SMOOTH_TOL
        assert rel_error(ev, want).max() <= SMOOTH_TOL
    finally:
        r.close()
