"""The photon searches on crowded maps, on the device: the maps, queries and k of tests/knn_crowds.py through every form mcrt_knn has -
the wave-cooperative kernel at both buffer widths, four queries per wave (MCRT_KNN_GROUPS=1), the per-lane kernel (MCRT_KERNEL=legacy,
and k > 768) and the per-lane branch behind MCRT_TEST_KNN_OVERFLOW - and through photon-mapped frames on maps whose photons sit in
stacks, against the oracle on the very same maps.

A case is here only after it passed on the CPU tier (tests/test_knn_crowds_emulation.py): the same source runs there on emulated
wavefronts, and a search that loops or overruns its buffer on some input has to show up on the host, not on a shared machine. So: add a
map, a query or a k to knn_crowds.py, see the CPU tier green, then run this.

Shapes are the smallest that still reach the crowd branches: n <= 5000 photons, 26 queries per call, one context for the module."""
import numpy as np
import pytest

import knn_crowds as kc
from conftest import camera_for, golden_path, rel_error

pytestmark = pytest.mark.gpu

UPLOAD_K = 50


@pytest.fixture(scope="module")
def room(pkg, manifest):
    return pkg.SceneImage(golden_path(manifest["cases"]["hexagon_room_pm"]["image"]))


@pytest.fixture(scope="module")
def ctx(pkg, room):
    c = pkg.Context(0)
    c.upload_image(room)
    yield c
    c.close()


class options:
    """Options of the context inside the block, the defaults after it."""

    def __init__(self, ctx, **values):
        self.ctx, self.values = ctx, values

    def __enter__(self):
        for key, value in self.values.items():
            self.ctx.set_option(key, value)

    def __exit__(self, *exc):
        for key in self.values:
            self.ctx.set_option(key, None)


# form -> (options, which k of a map it serves)
FORMS = {
    "wave": ({}, ("narrow", "wide")),
    "groups": ({"MCRT_KNN_GROUPS": 1}, ("group",)),
    "per lane (legacy)": ({"MCRT_KERNEL": "legacy"}, (1, 50, 64, 65, 128, 300)),
    "per lane (k > 768)": ({}, ("lane",)),
    "per lane (overflow branch)": ({"MCRT_TEST_KNN_OVERFLOW": 1}, (2, 50, 129, 768)),
}


@pytest.mark.parametrize("name", kc.MAP_NAMES)
def test_gpu_knn_on_crowded_maps(pkg, ctx, name):
    """Every form on every (map, queries, k) it serves: knn_crowds.check, and the same answer from all forms - counts and distances
    always, indices wherever the k-th distance is not tied across the cut. Which of the photons tied there a form returns is its own
    business (include/mcrt.h); how often the forms agree on it is printed."""
    c = kc.crowd(pkg, name)
    ctx.upload_photons(c.desc, c.desc, UPLOAD_K, False)
    answers = {}
    for form, (opts, kinds) in FORMS.items():
        ks = c.ks(kinds) if isinstance(kinds[0], str) else list(kinds)
        with options(ctx, **opts):
            for k in ks:
                got = ctx.knn(0, c.pts, k)
                c.check(*got, k, form)
                answers.setdefault(k, {})[form] = got
    same, tied_queries = 0, 0
    for k, by_form in answers.items():
        forms = list(by_form)
        tied = c.tied_at_cut(k)
        for other in forms[1:]:
            kc.assert_same_answers(by_form[forms[0]], by_form[other], tied, "%s k = %d: %s against %s" % (name, k, forms[0], other))
            a, b = kc.same_choice_among_ties(by_form[forms[0]], by_form[other], tied)
            same, tied_queries = same + a, tied_queries + b
    assert {f for by_form in answers.values() for f in by_form} == set(FORMS)
    print("%s: %d k, %d (query, k, pair of forms) with the k-th distance tied across the cut, the same photons chosen in %d" % (name, len(answers), tied_queries, same))


def test_gpu_knn_on_a_map_whose_frontier_outgrows_a_row(pkg, ctx):
    """The four-queries-per-wave kernel on leaves far smaller than k: a row's 64 frontier entries do not hold the octants within the
    bound, the wave repeats the query (the CPU tier shows with gcov that this branch is the one taken)."""
    with options(ctx, MCRT_KNN_GROUPS=1):
        for name, leaf, k in (("plane", 2, 64), ("lattice", 8, 16)):
            c = kc.crowd(pkg, name, leaf=leaf)
            ctx.upload_photons(c.desc, c.desc, leaf, False)
            c.check(*ctx.knn(0, c.pts, k), k, "groups, leaves of %d" % leaf)


@pytest.fixture(scope="module")
def crowded_room(pkg, room):
    return kc.CrowdedRoom(pkg, room)


def test_gpu_frames_on_crowded_maps(pkg, ctx, oracle, manifest, room, crowded_room):
    """hexagon_room_pm at 96 x 54, one sample, on its golden maps snapped to a 2^-3 grid with one flux and one direction for every photon,
    k = 50 and then k = 200 on the same context: the wave-cooperative megakernel, the per-lane one, and the pipeline with the evaluating
    and the raw kNN launch, each against the oracle's eye pass on the same maps - the bar of photon-mapped frames against the oracle
    (tests/test_knn_large_k.py: 1e-10, the order of an estimate's FP64 sum) - and the pipeline's frame the megakernel's, bit for bit.
    The maps matter: the oracle's frame without them differs in more than a quarter of the pixels.
    (The order of the renders is part of the case: a raw launch, an evaluating launch with a larger k, a raw launch with that k. Until
    the pipeline sized each of its kNN buffers by itself, the last of them wrote its k photons per search into the buffers of the
    first - an illegal memory access on the device.)"""
    case = manifest["cases"]["hexagon_room_pm"]
    cam = camera_for(room, case["renders"][0])
    cam.width, cam.height, cam.sqrtspp = 96, 54, 1
    seed, pm = manifest["seed"], pkg.INTEGRATOR_PHOTON_MAPPER
    bare, _ = oracle.render(kc.EmptyMaps(room), cam, seed, pm)
    try:
        for k in (50, 200):
            want, _ = oracle.render(crowded_room, cam, seed, pm, k=k)
            lit = (want != bare).any(axis=2).mean()
            print("k = %d: the crowded maps change %.1f %% of the oracle's pixels; %d / %d photons share a position" % (k, 100 * lit, *crowded_room.stacked))
            assert lit >= 0.25
            ctx.upload_photons(crowded_room.photons(0), crowded_room.photons(1), k, False)
            frames = {}
            for form, opts, kernel in (("wave megakernel", {}, pkg.KERNEL_PM_WAVE), ("per-lane megakernel", {"MCRT_KERNEL": "legacy"}, pkg.KERNEL_PM_LANE),
                                       ("pipeline, evaluating", {"MCRT_KERNEL": "wf", "MCRT_WF_PM_EVAL": 1}, pkg.KERNEL_WAVEFRONT_PM),
                                       ("pipeline, raw", {"MCRT_KERNEL": "wf", "MCRT_WF_PM_EVAL": 0}, pkg.KERNEL_WAVEFRONT_PM)):
                with options(ctx, **opts):
                    out, st = ctx.sample_image(cam, seed, pm)
                assert st["kernel_id"] == kernel, "%s ran %s" % (form, pkg.KERNEL_NAMES.get(st["kernel_id"]))
                assert st["knn_searches"] > 0
                rel = rel_error(out, want).max()
                print("k = %d, %s: max rel %.3e vs the oracle on the same maps, %d searches" % (k, form, rel, st["knn_searches"]))
                assert rel <= 1e-10, form
                frames[form] = (out, st)
            assert frames["pipeline, evaluating"][1]["knn_searches"] == frames["wave megakernel"][1]["knn_searches"]
            np.testing.assert_array_equal(frames["pipeline, evaluating"][0], frames["wave megakernel"][0])
    finally:
        ctx.upload_photons(room.photons(0), room.photons(1), room.param("k_nearest_photons") or 50, False)  # (the golden maps again)
