"""The photon searches of the product on crowded maps, on the HOST: every map, query and k of tests/knn_crowds.py - equal distances by
the dozen and by the thousand, queries on photons, on box faces, outside the box and so far away that all distances share their
leading bits - through the device source unchanged:

  * waveKnnSearch (csrc/mcrt_waveknn.hpp) on an emulated wavefront, both widths of the candidate buffer, the spill list's state in
    registers and in LDS (wemu_knn, tests/emu/wave_knn_emu.cpp);
  * knnGroupKernel itself - four queries per wave (csrc/mcrt_groupknn.hpp), a row that gives up repeated by the whole wave
    (wemu_knn_group, tests/emu/wave_kernel_emu.cpp);
  * knnSearch per lane (emu_knn / emu_knn_cap, tests/emu/mcrt_emu.cpp);
  * the estimates of a crowded map pair, per lane against the emulated wave (wemu_estimate).

Every answer goes through knn_crowds.check: brute-force distances bit for bit, distinct indices, each at the distance reported for it,
ties by index. One test shows with gcov that these cases TAKE the branches that are there for crowds (BRANCH_SITES).

A case goes to the GPU tier (tests/test_gpu_knn_crowds.py) only when it passes here."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import knn_crowds as kc
from conftest import TESTS, golden_path

UPLOAD_K = 50  # what the record lists are built for (mcrt_upload_photons' k_nearest_photons), as in the GPU tier


def wave_search(lib, desc, pts, k, rows, spill_mode, upload_k=UPLOAD_K):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(pts)
    cnt, idx, d2 = np.zeros(n, dtype=np.uint32), np.zeros((n, k), dtype=np.uint32), np.zeros((n, k))
    overflow = np.zeros(1, dtype=np.uint32)
    rc = lib.wemu_knn(C.byref(desc), upload_k, n, pts.ctypes.data, k, rows, spill_mode, cnt.ctypes.data, idx.ctypes.data, d2.ctypes.data, overflow.ctypes.data)
    assert rc == 0, rc
    return cnt, idx, d2, int(overflow[0])


def lane_search(lib, desc, pts, k, cap=None):
    """-> (count, index, distance2, rc); cap: the frontier's entries per lane (None: mcrt_knn's growing loop)"""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(pts)
    cnt, idx, d2 = np.zeros(n, dtype=np.uint32), np.zeros((n, k), dtype=np.uint32), np.zeros((n, k))
    outs = (cnt.ctypes.data, idx.ctypes.data, d2.ctypes.data)
    if cap is None:
        rc = lib.emu_knn(C.byref(desc), n, pts.ctypes.data, k, *outs)
    else:
        rc = lib.emu_knn_cap(C.byref(desc), n, pts.ctypes.data, k, cap, *outs)
    return cnt, idx, d2, rc


def group_search(lib, desc, pts, k, upload_k=UPLOAD_K, grid=2):
    """-> (count, index, distance2, the kernel's overflow word)"""
    lib.wemu_knn_group.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wemu_knn_group.restype = C.c_int
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(pts)
    cnt, idx, d2 = np.full(n, 0xDEAD, dtype=np.uint32), np.full((n, k), 0xDEAD, dtype=np.uint32), np.full((n, k), np.nan)
    flags = C.c_uint64(0)
    rc = lib.wemu_knn_group(C.byref(desc), upload_k, n, pts.ctypes.data, k, grid, cnt.ctypes.data, idx.ctypes.data, d2.ctypes.data, C.byref(flags))
    assert rc == 0, rc
    return cnt, idx, d2, int(flags.value)


@pytest.mark.parametrize("name", kc.MAP_NAMES)
def test_the_maps_are_what_they_are_for(pkg, name):
    """The predicates of the cases, before anything is searched: positions that are float32 values, ties where the map is there for
    ties, and a far query under which every distance has the same 20 leading bits."""
    c = kc.crowd(pkg, name)
    assert c.photons.dtype == np.float32 and len(c.pts) <= 64
    far = c.labels.index("far_all")
    assert kc.prefixes_agree(c.d2_all[far]), "far_all: the distances of %s spread over more than one 20-bit prefix" % name
    assert not kc.prefixes_agree(c.d2_all[c.labels.index("outside by 70")]) or name in ("point_and_one", "one_stack")
    stack = c.labels.index("on a stack")
    runs = {"lattice": 6, "stacks60": 60, "stacks150": 150, "stacks300": 300, "stacks1200": 1200, "point_and_one": 179, "one_stack": 62}
    if name in runs:
        d = c.d2_sorted[stack]
        first = 1 if name == "lattice" else 0  # (the lattice's query sits on a node: the photon there, then its six neighbours)
        assert (d[first:first + runs[name]] == d[first]).all() and (name == "one_stack" or d[first + runs[name]] > d[first])
    if name == "tight":
        d = c.d2_sorted[c.labels.index("near a stack")]
        assert d[1499] / d[0] < 1.004  # a whole cluster inside 0.4 % in distance2: one coarse prefix, or two
    if name == "plane":
        assert (c.pos[:, 2] == 1.0).all()


@pytest.mark.parametrize("spill_mode", [1, 2])
@pytest.mark.parametrize("name", kc.MAP_NAMES)
def test_wave_search_on_crowded_maps(pkg, wave_emu, name, spill_mode):
    c = kc.crowd(pkg, name)
    for rows, ks in ((4, c.ks(("narrow",))), (16, c.ks(("wide",)) + [50, 128])):
        for k in ks:
            cnt, idx, d2, overflow = wave_search(wave_emu, c.desc, c.pts, k, rows, spill_mode)
            assert overflow == 0
            c.check(cnt, idx, d2, k, "wave search, %d rows, spill mode %d" % (rows, spill_mode))


@pytest.mark.parametrize("name", kc.MAP_NAMES)
def test_wave_search_with_lists_built_for_the_k_asked(pkg, wave_emu, name):
    """... and with the record lists built for the k of the search (the render path's case: octants of up to k photons are scanned
    whole), the k around the stacks' heights."""
    c = kc.crowd(pkg, name)
    for k, rows in ((1, 4), (64, 4), (128, 4), (300, 16), (768, 16)):
        cnt, idx, d2, overflow = wave_search(wave_emu, c.desc, c.pts, k, rows, 1, upload_k=k)
        assert overflow == 0
        c.check(cnt, idx, d2, k, "wave search, lists for k")


@pytest.mark.parametrize("name", kc.MAP_NAMES)
def test_group_kernel_on_crowded_maps(pkg, wave_kernel_emu, wave_emu, name):
    """knnGroupKernel on two emulated workgroups (the last wave's rows partly without a query): check(), no overflow word, and the wave
    search's answer wherever the k-set is unique."""
    c = kc.crowd(pkg, name)
    for k in c.ks(("group",)):
        cnt, idx, d2, flags = group_search(wave_kernel_emu, c.desc, c.pts, k)
        assert flags == 0
        c.check(cnt, idx, d2, k, "group kernel")
        w = wave_search(wave_emu, c.desc, c.pts, k, 4, 1)
        kc.assert_same_answers((cnt, idx, d2), w[:3], c.tied_at_cut(k), "%s k = %d: group kernel against wave search" % (name, k))


def test_group_kernel_with_a_full_frontier(pkg, wave_kernel_emu):
    """Leaves far smaller than k, and record lists built for the leaves' size: more than the 64 octants a row's frontier holds lie within
    the bound at once; the row gives up and the wave repeats its query (that this happens: the branch-evidence test below)."""
    for name, leaf, k in FULL_FRONTIER_CASES:
        c = kc.crowd(pkg, name, leaf=leaf)
        cnt, idx, d2, flags = group_search(wave_kernel_emu, c.desc, c.pts, k, upload_k=leaf)
        assert flags == 0
        c.check(cnt, idx, d2, k, "group kernel, leaves of %d" % leaf)


@pytest.mark.parametrize("name", kc.MAP_NAMES)
def test_per_lane_search_on_crowded_maps(pkg, emu, wave_emu, name):
    """knnSearch per lane at EVERY k of the map - the narrow and the wide buffer's as well as its own beyond 768, and n - 1, n, n + 1: the
    device runs it at any k (MCRT_KERNEL=legacy, and behind a frontier overflow of the wave search). check(), and the wave search's
    answer at the k the wave search serves, wherever the k-set is unique."""
    c = kc.crowd(pkg, name)
    for k in c.ks(("narrow", "wide", "lane")):
        cnt, idx, d2, rc = lane_search(emu, c.desc, c.pts, k)
        assert rc == 0
        c.check(cnt, idx, d2, k, "per-lane search")
        if k <= 768:
            w = wave_search(wave_emu, c.desc, c.pts, k, 4 if k <= 128 else 16, 1)
            kc.assert_same_answers((cnt, idx, d2), w[:3], c.tied_at_cut(k), "%s k = %d: per-lane against wave search" % (name, k))


def test_per_lane_search_with_a_small_frontier_on_a_lattice(pkg, emu):
    """Leaves of three photons on the lattice: shells of equal distance keep dozens of octants inside the bound. Six entries per lane
    are reported as too few; the library's growing loop returns the brute-force answer."""
    c = kc.crowd(pkg, "lattice", leaf=3)
    assert lane_search(emu, c.desc, c.pts, 50, cap=6)[3] == 1
    cnt, idx, d2, rc = lane_search(emu, c.desc, c.pts, 50)
    assert rc == 0
    c.check(cnt, idx, d2, 50, "per-lane search, leaves of 3")


@pytest.fixture(scope="module")
def crowded_room(pkg, manifest):
    img = pkg.SceneImage(golden_path(manifest["cases"]["hexagon_room_pm"]["image"]))
    return kc.CrowdedRoom(pkg, img)


@pytest.mark.parametrize("k,rows", [(50, 4), (200, 16)])
def test_estimates_on_a_crowded_map_pair(pkg, wave_walk_emu, manifest, crowded_room, k, rows):
    """The estimates at the first hits of a small frame on hexagon_room_pm's maps snapped to a 2^-3 grid, constant flux and direction:
    per lane against the emulated wave, the bar of test_wave_radiance_estimate_on_the_host (the order of the FP64 sum: 1e-12). With
    stacks at the k-th distance the two searches may keep different photons of a stack; the payload makes those the same terms."""
    from conftest import camera_for
    room = crowded_room
    assert min(room.stacked) > 1000  # the maps are crowded: thousands of photons share a position with another
    cam = camera_for(room.img, manifest["cases"]["hexagon_room_pm"]["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 24, 14, 1
    n = cam.width * cam.height
    lane, wave = np.zeros((n, 6)), np.zeros((n, 6))
    valid = np.zeros(n, dtype=np.uint8)
    rc = wave_walk_emu.wemu_estimate(C.byref(room.scene), C.byref(room.photons(0)), C.byref(room.photons(1)), k, rows, C.byref(cam), manifest["seed"], n,
                                     lane.ctypes.data, wave.ctypes.data, valid.ctypes.data)
    assert rc == 0
    v = valid != 0
    assert v.sum() > n // 2 and (lane[v] != 0).any(axis=1).sum() > v.sum() // 4
    rel = np.abs(wave[v] - lane[v]) / np.maximum(np.abs(lane[v]), 1e-3)
    print("crowded estimates at %d hits, k = %d: max rel %.3e between the wave's and the lane's sums" % (v.sum(), k, rel.max()))
    assert rel.max() <= 1e-12


@pytest.mark.parametrize("k", [50, 200])
def test_frames_on_a_crowded_map_pair_on_the_host(pkg, wave_kernel_emu, oracle, manifest, crowded_room, k):
    """What tests/test_gpu_knn_crowds.py renders on the device, first on emulated workgroups: a small frame of the crowded room by the
    wave-cooperative megakernel, the per-lane one, and the pipeline with the evaluating and the raw kNN launch, each against the
    oracle's eye pass on the same maps (the order of an estimate's FP64 sum: 1e-12, the bar of the host's photon-mapped frames)."""
    from conftest import camera_for
    from test_wave_emulation import SMALL_FRAME, emulated_megakernel_frame, emulated_pipeline_frame
    cam = camera_for(crowded_room.img, manifest["cases"]["hexagon_room_pm"]["renders"][0])
    cam.width, cam.height, cam.sqrtspp = SMALL_FRAME
    seed, pm = manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER
    want, info = oracle.render(crowded_room, cam, seed, pm, k=k)
    bare, _ = oracle.render(kc.EmptyMaps(crowded_room.img), cam, seed, pm, k=k)
    assert (want != bare).any(axis=2).mean() >= 0.25
    frames = {}
    for legacy in (False, True):
        out, st, inst = emulated_megakernel_frame(pkg, wave_kernel_emu, crowded_room, cam, seed, pm, None, legacy=legacy, k=k)
        frames[inst] = out
        assert st[1] == info["rays"] and st[4] > 0
    assert set(frames) == {"PMLane_All", "PM1024_All" if k <= 128 else "PMWide_All"}
    for pm_eval in (1, 0):
        frames["pipeline, MCRT_WF_PM_EVAL=%d" % pm_eval] = emulated_pipeline_frame(wave_kernel_emu, crowded_room, cam, seed, pm, None, pm_eval, k)[0]
    for form, out in frames.items():
        rel = (np.abs(out - want) / np.maximum(np.abs(want), 1e-3)).max()
        print("crowded room, k = %d, %s: max rel %.3e" % (k, form, rel))
        assert rel <= 1e-12, form


# ---- branch evidence ------------------------------------------------------------------------------------------------------------------
# The sites that are there for crowds, found by their source text (never by line number; the statement alone, so that a reworded comment
# behind it does not lose the site): (name, file, function, text, what must hold).
# "both": every branch gcov lists on the line was taken and every call on it returned (a condition that was true AND false, and the
# statement behind it); "run": the line was executed. `function`: a substring of the demangled instance the line must have run in.
BRANCH_SITES = [
    ("waveSelectK: equal keys compacted, and the tie cut (eq_rank >= eq_left in some lane)", "mcrt_waveknn.hpp", "waveSelectK<4>",
     "const bool keep_eq = eq && eq_rank < eq_left;", "both"),
    ("waveSelectK: ... in the wide buffer", "mcrt_waveknn.hpp", "waveSelectK<16>", "const bool keep_eq = eq && eq_rank < eq_left;", "both"),
    ("waveKnnSearch: the crowd fall-back of a buffer reduction, 4 rows", "mcrt_waveknn.hpp", "waveKnnSearch<4,",
     "if (count > waveCand(R) - 64u) count = waveSelectK<R>(W, count, k, bound);", "both"),
    ("waveKnnSearch: the crowd fall-back of a buffer reduction, 16 rows", "mcrt_waveknn.hpp", "waveKnnSearch<16,",
     "if (count > waveCand(R) - 64u) count = waveSelectK<R>(W, count, k, bound);", "both"),
    ("histSelectK: both early returns (have > 64u, have - need > 6u)", "mcrt_waveknn.hpp", "histSelectK<4>",
     "if (have > 64u || have - need > 6u) return 0u;", "both"),
    ("histSelectK: the drop loop", "mcrt_waveknn.hpp", "histSelectK<", "while (n > need) {", "both"),
    ("waveTrimToK: the drop loop", "mcrt_waveknn.hpp", "waveTrimToK", "while (n > k) {", "both"),
    ("groupTrimToK: the drop loop", "mcrt_groupknn.hpp", "groupTrimToK", "const uint32_t s_drop = (mine - 1u) >> 4;", "run"),
    ("groupKnnSearch: redo set by the full frontier", "mcrt_groupknn.hpp", "groupKnnSearch", "if (has && !placed) redo = true;", "both"),
    ("groupKnnSearch: redo set by the crowded buffer", "mcrt_groupknn.hpp", "groupKnnSearch", "if (count > kGrpCand - 16u) {", "both"),
    ("groupKnnSearch: redo set by count > k + 6u", "mcrt_groupknn.hpp", "groupKnnSearch", "if (on && !redo && count > k + 6u) redo = true;", "both"),
    ("knnGroupKernel: the wave repeats a row's query", "mcrt_kernels.hpp", "knnGroupKernel", "const uint32_t cc = waveKnnSearch(map, qp, k, W, rr, overflow, visits);",
     "run"),
]
# With ONLY stacks60 and one_stack searched (stacks of 60 / 62 coincident photons and nothing else) whatever a drop loop drops first, it
# drops among 60 equal keys: these sites taken in that run are "the drop loop with equal keys" / "with `owners` holding more than one lane".
EQUAL_KEY_SITES = ("histSelectK: the drop loop", "waveTrimToK: the drop loop", "groupTrimToK: the drop loop")
EVIDENCE_NARROW_K, EVIDENCE_WIDE_K = (2, 50, 56, 58, 64, 65, 128), (129, 300, 768)


def _load_for_evidence(wave_lib, kernel_lib):
    import importlib
    pkg = importlib.import_module("monte-carlo-ray-tracer_amd")
    pkg.lib()
    W, K = C.CDLL(wave_lib), C.CDLL(kernel_lib)
    W.wemu_knn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    W.wemu_knn.restype = C.c_int
    return pkg, W, K


def run_evidence_cases(wave_lib, kernel_lib, phase):
    """What the child process of the branch-evidence test runs, on libraries built with --coverage: phase "equal" = stacks60 and one_stack alone,
    phase "all" = every map (a subset of the k: the sites, not the matrix, are the point). Every answer still goes through check()."""
    pkg, W, K = _load_for_evidence(wave_lib, kernel_lib)
    for name in (("stacks60", "one_stack") if phase == "equal" else kc.MAP_NAMES):
        c = kc.crowd(pkg, name)
        for k in [k for k in EVIDENCE_NARROW_K + (c.n - 1,) if 0 < k <= 128]:
            for upload_k in (UPLOAD_K, k):
                cnt, idx, d2, overflow = wave_search(W, c.desc, c.pts, k, 4, 1, upload_k=upload_k)
                assert overflow == 0
                c.check(cnt, idx, d2, k, "wave search (coverage build)")
            if k <= kc.GROUP_MAX_K:
                cnt, idx, d2, flags = group_search(K, c.desc, c.pts, k)
                assert flags == 0
                c.check(cnt, idx, d2, k, "group kernel (coverage build)")
        if phase == "all":
            for k in EVIDENCE_WIDE_K:
                cnt, idx, d2, overflow = wave_search(W, c.desc, c.pts, k, 16, 2)
                assert overflow == 0
                c.check(cnt, idx, d2, k, "wave search, 16 rows (coverage build)")
    if phase == "all":
        for name, leaf, k in FULL_FRONTIER_CASES:
            c = kc.crowd(pkg, name, leaf=leaf)
            cnt, idx, d2, flags = group_search(K, c.desc, c.pts, k, upload_k=leaf)
            assert flags == 0
            c.check(cnt, idx, d2, k, "group kernel, leaves of %d (coverage build)" % leaf)


def parse_gcov(path):
    """A .gcov file of `gcov -b -m` -> {source line text (stripped): [(function, executions, [branch counts], [call counts])]}: one entry
    for the line itself and one per template instance (the blocks gcov prints between rows of dashes, headed by the instance's name)."""
    out, function, last = {}, "", None
    dashes = False
    for raw in open(path, errors="replace"):
        line = raw.rstrip("\n")
        if line.startswith("------------------"):
            dashes, function = True, ""
            continue
        m = re.match(r"\s*([0-9]+\*?|-|#####|=====):\s*([0-9]+):(.*)$", line)
        if m:
            dashes = False
            count = m.group(1).rstrip("*")
            last = [function, int(count) if count.isdigit() else 0, [], []]
            out.setdefault(m.group(3).strip(), []).append(last)
            continue
        if dashes and line.endswith(":"):  # the name of the instance whose lines follow
            function, dashes = line[:-1], False
            continue
        m = re.match(r"function (.*) called [0-9]+ returned", line)
        if m:
            function, dashes = m.group(1), False
            continue
        m = re.match(r"branch\s+[0-9]+ (never executed|taken ([0-9]+))(.*)$", line)
        if m and last is not None:
            if "(throw)" not in m.group(3):
                last[2].append(int(m.group(2) or 0))
            continue
        m = re.match(r"call\s+[0-9]+ (never executed|returned ([0-9]+))", line)
        if m and last is not None:
            last[3].append(int(m.group(2) or 0))
    return out


def sites_taken(gcov_dir, sites=None):
    """-> {site name: True / False / None (the text was not found in the file's report)}"""
    reports, result = {}, {}
    for name, file, function, text, rule in (sites or BRANCH_SITES):
        if file not in reports:
            merged = {}
            for f in os.listdir(gcov_dir):
                if f.endswith(file + ".gcov"):
                    for key, rows in parse_gcov(os.path.join(gcov_dir, f)).items():
                        merged.setdefault(key, []).extend(rows)
            reports[file] = merged
        rows = [r for key, rs in reports[file].items() if key.startswith(text) for r in rs if function.replace(" ", "") in r[0].replace(" ", "")]
        if not rows:
            result[name] = None
        elif rule == "run":
            result[name] = any(r[1] > 0 for r in rows)
        else:
            result[name] = any(r[1] > 0 and r[2] and all(b > 0 for b in r[2]) and all(c > 0 for c in r[3]) for r in rows)
    return result


# (map, leaf capacity = the k the record lists are built for, k): more octants within the bound at once than a row's 64 frontier entries,
# not more than the 128 of the wave that repeats the query
FULL_FRONTIER_CASES = [("plane", 2, 64), ("lattice", 8, 16)]


def build_for_evidence(build_dir):
    import emu_build
    flags = ("--coverage", "-fno-inline")
    return [emu_build.build_emu(src, flags=flags, opt="-O0", build_dir=str(build_dir)) for src in ("wave_knn_emu.cpp", "wave_kernel_emu.cpp")]


def gcov_report(build_dir, phase):
    """Runs the cases of `phase` in a child process on the libraries of build_dir, then gcov -b; -> the directory of the .gcov files"""
    libs = [os.path.join(str(build_dir), f) for f in ("libwave_knn_emu.so", "libwave_kernel_emu.so")]
    subprocess.check_call([sys.executable, os.path.abspath(__file__), libs[0], libs[1], phase], cwd=TESTS)
    out = os.path.join(str(build_dir), "gcov_" + phase)
    os.makedirs(out, exist_ok=True)
    notes = [os.path.join(str(build_dir), f) for f in os.listdir(str(build_dir)) if f.endswith(".gcda")]
    assert len(notes) == 2, notes
    subprocess.check_call(["gcov", "-b", "-c", "-m", "-p"] + notes, cwd=out, stdout=subprocess.DEVNULL)
    return out


def test_crowd_cases_take_the_branches_that_are_there_for_crowds(tmp_path):
    """wave_knn_emu.cpp and wave_kernel_emu.cpp (the group entry's source) built with --coverage, the crowd cases run in a child
    process, gcov -b: every site of BRANCH_SITES was taken, and the drop loops already by stacks60 and one_stack alone - there, among equal keys."""
    if shutil.which("gcov") is None:
        pytest.skip("no gcov on this machine: the branch evidence needs it")
    build_for_evidence(tmp_path)
    equal = sites_taken(gcov_report(tmp_path, "equal"))
    for name in EQUAL_KEY_SITES:
        assert equal[name], "%s: not taken by stacks60 and one_stack alone (%r)" % (name, equal[name])
    taken = sites_taken(gcov_report(tmp_path, "all"))  # (the counts add up: the second report covers both runs)
    for name, hit in taken.items():
        print("%-90s %s" % (name, "taken" if hit else "NOT TAKEN" if hit is not None else "text not found"))
    assert all(taken.values()), [name for name, hit in taken.items() if not hit]


if __name__ == "__main__":
    run_evidence_cases(sys.argv[1], sys.argv[2], sys.argv[3])
