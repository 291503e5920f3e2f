"""The statistics words of a render, without a GPU: csrc/mcrt_stats_words.hpp names the 20 words every kernel reports through and
csrc/mcrt_stats_readout.hpp turns them into mcrt_stats' counters, the readouts on stderr and what the retry decision reads. Here

  1. the numbering is the one the tests index by (tests/test_wave_emulation.py: words 0 to 4 and 7 of an emulated frame;
     tests/test_gpu_diagnostic_kernels.py: the words 8 to 19 behind the readouts) - the header says it is frozen, this holds it to that;
  2. hand-made words go through the readout function mcrt_render_finish prints with (exported by tests/emu/wave_kernel_emu.cpp) and the
     lines are matched with the very expressions of tests/test_gpu_diagnostic_kernels.py - hand-made because the emulation's clock64() is 0,
     so an emulated frame has no clock words - plus the three cases in which nothing may be printed;
  3. the words of one emulated counting frame give the counters and an outcome without overflow."""
import ctypes as C
import re

import numpy as np
import pytest

from test_gpu_diagnostic_kernels import PHASES, PM_LINE, TRACE_PER_RAY, _no_nan, _numbers, _phase_lines
from test_wave_emulation import FRAME, INSTANCE_NAMES, diagnostic_scene, emulated_megakernel_frame

LAYOUT = ["paths", "rays", "node_tests", "prim_tests", "knn_searches", "overflow", "knn_octants", "iors_overflow",
          "overlay", "phase_wave", "phase_lane", "phases",
          "trace_iters", "trace_have", "trace_inner_steps", "trace_inner_lanes", "trace_leaf_steps", "trace_leaf_lanes", "trace_leaf_wait",
          "trace_inner_cycles", "trace_leaf_cycles", "trace_kernel_cycles", "trace_refill_cycles", "trace_pop_cycles",
          "pm_estimate_cycles", "pm_kernel_cycles", "words",
          "emit_work", "emit_global", "emit_caustic", "emit_paths", "emit_rays", "emit_overflow", "emit_iors_overflow", "emit_words",
          "knn_overflow_bit", "knn_overflow_unit"]


@pytest.fixture(scope="module")
def words_lib(wave_kernel_emu):
    L = wave_kernel_emu
    L.wemu_stats_layout.argtypes, L.wemu_stats_layout.restype = [C.c_void_p], C.c_int
    L.wemu_stats_readout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_uint32]
    L.wemu_stats_readout.restype = C.c_int
    L.wemu_stats_outcome.argtypes, L.wemu_stats_outcome.restype = [C.c_void_p, C.c_uint32, C.c_void_p], None
    return L


@pytest.fixture(scope="module")
def layout(words_lib):
    assert words_lib.wemu_stats_layout(None) == len(LAYOUT)
    v = np.zeros(len(LAYOUT), dtype=np.uint64)
    words_lib.wemu_stats_layout(v.ctypes.data)
    return {name: int(x) for name, x in zip(LAYOUT, v)}


def test_the_numbering_is_what_the_tests_index(layout):
    w = layout
    # words 0 to 4 and 7 (test_wave_emulation.py: st[0] paths, st[1] rays, st[2] / st[3] tests, st[4] searches; wave_kernel_emu.cpp: -100 / -101)
    assert [w[k] for k in LAYOUT[:8]] == list(range(8))
    # words 8 to 19: three overlays on one base
    assert w["overlay"] == 8 and w["phases"] == len(PHASES) == 6
    assert (w["phase_wave"], w["phase_lane"]) == (8, 8 + w["phases"])
    assert [w[k] for k in LAYOUT[12:24]] == list(range(8, 20))
    assert (w["pm_estimate_cycles"], w["pm_kernel_cycles"]) == (8, 9)
    assert w["words"] == 20 == max(w["phase_lane"] + w["phases"], w["trace_pop_cycles"] + 1, w["pm_kernel_cycles"] + 1)  # (emulated_*_frame: stats[:20])
    # the emission counters (mcrt_emit_photons*, wemu_emit)
    assert [w[k] for k in LAYOUT[27:34]] == list(range(7)) and w["emit_words"] == 8
    assert w["knn_overflow_bit"] == 0x10000 and w["knn_overflow_unit"] == 1 << 32


def _readout(lib, words, instance, trace, kernel_id):
    a = np.zeros(20, dtype=np.uint64)
    for i, x in words.items():
        a[i] = x
    ids = [INSTANCE_NAMES.index(n) if n != "-" else -1 for n in (instance, trace)]
    buf = C.create_string_buffer(4096)
    n = lib.wemu_stats_readout(a.ctypes.data, ids[0], ids[1], kernel_id, buf, len(buf))
    text = buf.value.decode()
    assert n == len(text) < len(buf) - 1
    return text


# one set of words per readout (word number: value)
COMMON = {0: 5880, 1: 1000, 2: 52000, 3: 9000, 4: 500, 6: 6000}
PHASE_WORDS = {**COMMON, 8: 100, 9: 400, 10: 200, 11: 300, 12: 0, 13: 1000,
               14: 64 * 100, 15: 32 * 400, 16: 16 * 200, 17: 48 * 300, 18: 0, 19: 16 * 1000}
TRACE_WORDS = {**COMMON, 8: 200, 9: 8000, 10: 150, 11: 4800, 12: 50, 13: 800, 14: 400, 15: 5000, 16: 2000, 17: 10000, 18: 1000, 19: 500}
PM_WORDS = {**COMMON, 8: 7500, 9: 10000}
TRACE_FORMAT = ("[mcrt trace] per wave iteration: %.1f lanes hold a ray; inner step in %.1f%% of the iterations with %.1f lanes, leaf step in %.1f%% with %.1f lanes, "
                "%.1f leaf lanes wait; wave cycles: inner %.1f%%, leaf %.1f%%, rest %.1f%% (of the kernel: refills %.1f%%, pop site %.1f%%); per ray: %.2f inner steps, %.2f leaf steps "
                "(%d inner and %d leaf lane steps of %d rays)\n")


def test_phase_readout_of_hand_made_words(pkg, words_lib):
    for instance, form in (("PT_Prof", pkg.KERNEL_WAVESYNC), ("PT_ProfAll", pkg.KERNEL_WAVESYNC), ("SM_Prof", pkg.KERNEL_LANE_SM), ("SM_ProfAll", pkg.KERNEL_LANE_SM)):
        err = _readout(words_lib, PHASE_WORDS, instance, "-", form)
        _no_nan(err)
        rows = _phase_lines(err)
        assert [n for n, _, _ in rows] == PHASES and len(err.splitlines()) == len(PHASES), err
        assert [a for _, a, _ in rows] == [5.0, 20.0, 10.0, 15.0, 0.0, 50.0]
        assert [b for _, _, b in rows] == [100.0, 50.0, 25.0, 75.0, 0.0, 25.0]  # (the phase without a cycle: 0, not 0 / 0)
        assert "[mcrt trace]" not in err and "[mcrt pm]" not in err
        assert err.splitlines(True)[0] == "[mcrt phase] regen     wave-cycles   5.00%  lane utilisation 100.0%\n"
        assert err.splitlines(True)[1] == "[mcrt phase] trav/inner wave-cycles  20.00%  lane utilisation  50.0%\n"


def test_trace_readout_of_hand_made_words(pkg, words_lib):
    err = _readout(words_lib, TRACE_WORDS, "ShadePT", "Trace_Count", pkg.KERNEL_WAVEFRONT)
    _no_nan(err)
    assert err == TRACE_FORMAT % (40.0, 75.0, 32.0, 25.0, 16.0, 2.0, 50.0, 20.0, 30.0, 10.0, 5.0, 4.8, 0.8, 4800, 800, 1000)
    lines = [l for l in err.splitlines() if l.startswith("[mcrt trace]")]
    assert len(lines) == 1 and "[mcrt phase]" not in err and "[mcrt pm]" not in err
    line = lines[0]
    assert all(0.0 <= float(p) <= 100.0 for p in re.findall(r"(-?[0-9.]+)%", line)) and len(re.findall(r"%", line)) == 7
    assert all(0.0 <= float(x) <= 64.0 for x in re.findall(r"(-?[0-9.]+) (?:leaf )?lanes", line))
    m = re.search(TRACE_PER_RAY, line)
    assert m and [float(g) for g in m.groups()] == [4.8, 0.8, 4800, 800, 1000]
    assert all(np.isfinite(x) for x in _numbers(line))
    # step clocks that add up to more than the kernel's (they are read on other lanes' behalf): the rest is 0 %, never negative; and
    # iterations without a step, a frame without rays: no zero divisor
    odd = {**TRACE_WORDS, 1: 0, 10: 0, 11: 0, 12: 0, 13: 0, 15: 9000, 16: 2000}
    err = _readout(words_lib, odd, "ShadePT", "Trace_Count", pkg.KERNEL_WAVEFRONT)
    _no_nan(err)
    assert err == TRACE_FORMAT % (40.0, 0.0, 0.0, 0.0, 0.0, 2.0, 90.0, 20.0, 0.0, 10.0, 5.0, 0.0, 0.0, 0, 0, 0)


def test_photon_mapping_readout_of_hand_made_words(pkg, words_lib):
    for instance in ("PM512_Count", "PM512_CountAll", "PM1024_Count", "PM1024_CountAll", "PMWide_Count", "PMWide_CountAll"):
        err = _readout(words_lib, PM_WORDS, instance, "-", pkg.KERNEL_PM_WAVE)
        _no_nan(err)
        assert err == "[mcrt pm] wave cycles inside the radiance estimates: 75.0% of the kernel (500 searches, 12.0 octants per search)\n"
        m = re.findall(PM_LINE, err, re.M)
        assert len(m) == 1 and (float(m[0][0]), int(m[0][1]), float(m[0][2])) == (75.0, 500, 12.0)
        assert "[mcrt phase]" not in err and "[mcrt trace]" not in err
    # an estimate clock beyond the kernel's reads 100 %; no search: no zero divisor
    err = _readout(words_lib, {**PM_WORDS, 4: 0, 8: 10001}, "PM1024_CountAll", "-", pkg.KERNEL_PM_WAVE)
    assert err == "[mcrt pm] wave cycles inside the radiance estimates: 100.0% of the kernel (0 searches, 0.0 octants per search)\n"


def test_nothing_is_read_out_of_words_nobody_measured(pkg, words_lib):
    """The three refusals of the readout: all clocks zero (a frame whose launches found no work), profiling words under an instance that
    does not profile (the option alone prints nothing), and the photon-mapping kernel's words under another kernel id."""
    ran = [("PT_Prof", "-", pkg.KERNEL_WAVESYNC), ("SM_ProfAll", "-", pkg.KERNEL_LANE_SM), ("ShadePT", "Trace_Count", pkg.KERNEL_WAVEFRONT),
           ("PM1024_CountAll", "-", pkg.KERNEL_PM_WAVE)]
    for instance, trace, form in ran:
        assert _readout(words_lib, COMMON, instance, trace, form) == ""
        assert _readout(words_lib, {}, instance, trace, form) == ""
    assert _readout(words_lib, {**TRACE_WORDS, 17: 0}, "ShadePT", "Trace_Count", pkg.KERNEL_WAVEFRONT) == ""  # (iterations, but no kernel clock)
    assert _readout(words_lib, {**TRACE_WORDS, 8: 0}, "ShadePT", "Trace_Count", pkg.KERNEL_WAVEFRONT) == ""
    assert _readout(words_lib, {**PM_WORDS, 9: 0}, "PM1024_CountAll", "-", pkg.KERNEL_PM_WAVE) == ""
    for words in (PHASE_WORDS, TRACE_WORDS, PM_WORDS):
        for instance, trace, form in (("PT_CountAll", "-", pkg.KERNEL_WAVESYNC), ("SM_Count", "-", pkg.KERNEL_LANE_SM), ("Flat512", "-", pkg.KERNEL_FLAT),
                                      ("ShadePT", "Trace", pkg.KERNEL_WAVEFRONT), ("ShadePT", "TraceLean", pkg.KERNEL_WAVEFRONT),
                                      ("PM1024_All", "-", pkg.KERNEL_PM_WAVE), ("PMLane_CountAll", "-", pkg.KERNEL_PM_LANE), ("-", "-", pkg.KERNEL_NONE)):
            assert _readout(words_lib, words, instance, trace, form) == "", (instance, trace)
    for form in (pkg.KERNEL_PM_LANE, pkg.KERNEL_WAVEFRONT_PM, pkg.KERNEL_WAVEFRONT, pkg.KERNEL_WAVESYNC, pkg.KERNEL_NONE):
        assert _readout(words_lib, PM_WORDS, "PM1024_CountAll", "-", form) == ""
    # ... and the counting trace kernel's words under a photon-mapped pipeline frame, as before
    assert _readout(words_lib, TRACE_WORDS, "ShadePM", "Trace_Count", pkg.KERNEL_WAVEFRONT_PM) == ""


def _outcome(lib, words, kernel_id):
    a = np.array(list(words) + [0] * (20 - len(words)), dtype=np.uint64)
    out = np.zeros(8, dtype=np.uint64)
    lib.wemu_stats_outcome(a.ctypes.data, kernel_id, out.ctypes.data)
    return [int(x) for x in out]


def test_words_of_an_emulated_counting_frame_give_the_counters_and_no_overflow(pkg, words_lib, layout, manifest):
    """hexagon_room_diffuse at the ragged frame through SM_CountAll (COUNTING_CASES, tests/test_wave_emulation.py): the words the kernel's
    epilogue wrote, read the way mcrt_render_finish reads them."""
    img, cam = diagnostic_scene(pkg, None, manifest, "hexagon_room_diffuse")
    cam.width, cam.height, cam.sqrtspp = FRAME
    _, st, ran = emulated_megakernel_frame(pkg, words_lib, img, cam, manifest["seed"], pkg.INTEGRATOR_PATH_TRACER, True, False, 0)
    assert ran == "SM_CountAll"
    paths, rays, node_tests, prim_tests, searches, overflow, iors_overflow, action = _outcome(words_lib, st, pkg.KERNEL_LANE_SM)
    assert paths == st[layout["paths"]] == cam.width * cam.height * cam.sqrtspp ** 2
    assert rays == st[layout["rays"]] > paths
    assert node_tests == st[layout["node_tests"]] >= paths and prim_tests == st[layout["prim_tests"]] > 0
    assert searches == st[layout["knn_searches"]] == 0
    assert overflow == st[layout["overflow"]] == 0 and iors_overflow == st[layout["iors_overflow"]] == 0
    assert action == 0  # kRetryDone: the frame is delivered
    assert st[layout["overlay"]:] == [0] * 12  # (no clock in the emulation, and a counting instance has no phase words)
    assert _readout(words_lib, dict(enumerate(st)), ran, "-", pkg.KERNEL_LANE_SM) == ""
    # the two meanings of the overflow word, as the retry decision reads them: a stack overflow is refused, a kNN overflow of a
    # wave-cooperative frame is rendered again
    st_stack = list(st)
    st_stack[layout["overflow"]] = 3
    assert _outcome(words_lib, st_stack, pkg.KERNEL_LANE_SM)[5:] == [3, 0, 1]
    for word in (layout["knn_overflow_bit"], layout["knn_overflow_unit"], 2 * layout["knn_overflow_unit"] + 1):
        st_knn = list(st)
        st_knn[layout["overflow"]] = word
        assert _outcome(words_lib, st_knn, pkg.KERNEL_PM_WAVE)[5:] == [word, 0, 2]
