"""The hierarchy builders on inputs they have trouble with (tests/awkward_scenes.py), host tier, compared as BYTES - a box
coordinate -0.0 is not +0.0 here, unlike np.testing.assert_array_equal:

  * the fixtures the reference itself made of those scenes (tests/golden/awkward/, made by tests/golden/make_awkward.py):
    building the scene must give the image's LinearNode arrays and the image's surface order - recursive builder on one thread
    and on all, level-synchronous host loop, octree host path;
  * every family and the concatenation at 2, 3, 5 and 16 bins per axis under both SAH rules: the level-synchronous host loop
    against the recursive builder, after the family's predicate has shown on the recursive tree that the input reaches the rule
    it is there for (coincident centroids, one usable axis, empty quadrants, splits refused by cost, the 1e-9 extent test, zeros
    of both signs, three surface kinds, open nodes smaller than a wave, the smallest scenes);
  * the octree host path against the octree built plainly (serial insertion), and its refusal of more than 8 centroids in one
    finest cell.
The GPU paths on the same inputs: tests/test_gpu_bvh_awkward.py."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import awkward_scenes as A
from conftest import GOLDEN

AWKWARD, BINS, MCRT_ERR_UNSUPPORTED = A.AWKWARD, A.BINS, A.MCRT_ERR_UNSUPPORTED
FIXTURES = A.fixtures()
scene_of, scene_of_without_overlapping, image_arrays, same_tree_and_order = A.scene_of, A.scene_of_without_overlapping, A.image_arrays, A.same_tree_and_order
SAH_SCENES = list(A.SAH_FAMILIES) + ["sah_concatenation"]

def fixture_builds(fx):
    """(label, keyword arguments of pkg.Bvh) of every host execution that must rebuild the fixture."""
    if fx["bvh"] == "octree":
        return [("octree host path", dict(kind="octree"))]
    kw = dict(kind=fx["bvh"], bins_per_axis=fx["bins_per_axis"])
    return [("recursive, 1 thread", dict(kw, threads=1)), ("recursive, all threads", dict(kw, threads=0)), ("level-synchronous host loop", dict(kw, levels=True))]


# Why the SAH fixtures are rebuilt from the SCENE FILE's order and not from the image's surfaces: the reference's own output order is
# no fixed point of its SAH builders on these scenes. arbitrarySplit deals surface i of a node to part i % N, so dealing the dealt
# order again gives other parts (coincident_256, overlapping_300); and the sign of a zero box coordinate is the first surface's in
# node order, which the image's order changes (signed_zero). The reference itself would not reproduce its arrays from its image.
# What is demanded instead is the same and more: the image's nodes, and the image's surface ORDER out of the input order. The
# octree BVH lists a leaf's surfaces in input order and merges octants in octant order, so it is rebuilt from its own image too.


@pytest.mark.parametrize("fx", FIXTURES, ids=[f["name"] for f in FIXTURES])
def test_rebuilds_the_reference_tree_of_an_awkward_scene(pkg, fx):
    """From the scene in the scene file's order (what the reference's builder was given): the image's nodes, and the image's surface
    order. The octree BVH also from the image's own surfaces, which must then stay in place."""
    path = os.path.join(AWKWARD, fx["image"])
    assert os.path.getsize(path) < os.path.getsize(os.path.join(GOLDEN, "coffee_maker_qsah.mcrt"))
    img = pkg.SceneImage(path)
    sc = scene_of(pkg, fx["scene"])
    assert img.scene.num_nodes == fx["nodes"] > 0 and img.scene.num_surfaces == fx["surfaces"] == sc.n
    for label, kw in fixture_builds(fx):
        bvh = pkg.Bvh(sc.desc, **kw)
        same_tree_and_order(bvh.arrays(), sc.desc, img, "%s, %s:" % (fx["name"], label))
        bvh.close()
        if fx["bvh"] == "octree":
            bvh = pkg.Bvh(img.scene, **kw)
            A.same_bytes(bvh.arrays(), image_arrays(img), "%s from its own image, %s:" % (fx["name"], label))
            bvh.close()
    img.close()


@pytest.mark.parametrize("fx", [f for f in FIXTURES if f["scene"] == "signed_zero"], ids=lambda f: f["name"])
def test_signed_zero_fixture_holds_zeros_of_both_signs(pkg, fx):
    """The reference's loader kept the -0.0 of the scene file, and its tree has box coordinates of both zero signs: the fixture
    can tell a builder that orders -0.0 below +0.0 from one that keeps the first surface's zero."""
    img = pkg.SceneImage(os.path.join(AWKWARD, fx["image"]))
    s = img.scene
    v = np.ctypeslib.as_array(s.surf_v, shape=(s.num_surfaces * 9,)).view(np.uint64)
    assert (v == 0x8000000000000000).sum() > 50 and (v == 0).sum() > 50
    b = image_arrays(img)["bounds"][1:].view(np.uint64)  # (node 0 of a SAH tree is the scene box)
    assert (b == 0x8000000000000000).any() and (b == 0).any()
    img.close()


def test_fixture_inputs_are_the_generated_scenes(pkg):
    """The committed scene files (gzip'd JSON) hold the scenes this module generates today, surface by surface in order: triangles and spheres bit for
    bit (Python writes the shortest decimal that reads back as the same double, -0.0 included); quadrics by position (their records
    are compared with the image's in test_rebuilds_the_reference_tree_of_an_awkward_scene)."""
    for name in sorted({f["scene"] for f in FIXTURES}):
        sc = scene_of(pkg, name)
        j = json.load(gzip.open(os.path.join(AWKWARD, name + ".json.gz"), "rt"))
        kind, v = [], []
        for s in j["surfaces"]:
            if s["type"] == "object":
                vs = np.array(j["vertices"][s["vertex_set"]], np.float64)
                for t in s["triangles"]:
                    kind.append(A.TRI)
                    v.append(vs[t].reshape(9))
            elif s["type"] == "sphere":
                kind.append(A.SPHERE)
                v.append(np.array(s["position"] + [s["radius"]] + [0.0] * 5))
            else:
                assert s["type"] == "quadric"
                kind.append(A.QUADRIC)
                v.append(np.zeros(9))
        mine = sc.v.copy()
        mine[sc.kind == A.QUADRIC, 0] = 0.0
        assert np.array(kind, np.uint8).tobytes() == sc.kind.tobytes(), name
        assert np.array(v).tobytes() == mine.tobytes(), name


@pytest.mark.parametrize("kind", A.SAH_KINDS)
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("name", SAH_SCENES)
def test_level_synchronous_host_loop_equals_recursive(pkg, name, bins, kind):
    sc = scene_of(pkg, name)
    a = pkg.Bvh(sc.desc, kind=kind, bins_per_axis=bins, threads=1)
    want = a.arrays()
    A.check(sc, kind, bins, want)  # the input does its job - or the test fails here
    b = pkg.Bvh(sc.desc, kind=kind, bins_per_axis=bins, levels=True)
    A.same_bytes(b.arrays(), want, "%s %s %d bins: level-synchronous host loop against recursive:" % (name, kind, bins))
    c = pkg.Bvh(sc.desc, kind=kind, bins_per_axis=bins, threads=0)
    A.same_bytes(c.arrays(), want, "%s %s %d bins: all threads against one:" % (name, kind, bins))
    for x in (a, b, c):
        x.close()


@pytest.mark.parametrize("kind", A.SAH_KINDS)
def test_concatenation_predicates_hold_at_the_default_bins(pkg, kind):
    """... where the fixtures were made (bins_per_axis 0: 8 x 8 / 16)."""
    sc = scene_of(pkg, "sah_concatenation")
    assert 0 in A.CONCATENATION_PREDICATE_BINS and sc.n <= 2000
    a = pkg.Bvh(sc.desc, kind=kind, threads=1)
    A.check(sc, kind, 0, a.arrays())
    a.close()


@pytest.mark.parametrize("name", [n for n in A.OCTREE_FAMILIES if n not in A.OCTREE_REFUSED] + ["octree_concatenation"])
def test_octree_host_path_equals_plain_insertion(pkg, name):
    sc = scene_of(pkg, name)
    bvh = pkg.Bvh(sc.desc)
    got = bvh.arrays()
    A.check(sc, "octree", 0, got)
    A.same_bytes(got, A.plain_octree_bvh(sc), "%s: octree host path against serial insertion:" % name)
    bvh.close()


def test_octree_host_path_refuses_nine_coincident_centroids(pkg):
    """More than 8 centroids inside one finest cell: MCRT_ERR_UNSUPPORTED, no handle, nothing kept (the builder deletes its
    half-made tree: the process's memory does not grow over many refusals), and the next scene builds."""
    import resource
    sc = scene_of(pkg, "nine_coincident")
    with pytest.raises(RecursionError):
        A.plain_octree_bvh(sc)
    L = pkg.lib()

    def refuse():
        h = C.c_void_p()
        assert L.mcrt_bvh_build_octree(None, C.byref(sc.desc), C.byref(h)) == MCRT_ERR_UNSUPPORTED
        assert not h.value
    for _ in range(200):  # warm the allocator
        refuse()
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    for _ in range(20000):
        refuse()
    grown_kib = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before
    # a leaked tree of this scene is more than 1 KiB (11 surfaces: order, boxes, nodes); 20 000 of them more than 20 MiB
    assert grown_kib < 4096, "peak resident set grew by %d KiB over 20 000 refusals" % grown_kib
    ok = scene_of(pkg, "on_planes")
    bvh = pkg.Bvh(ok.desc)
    A.same_bytes(bvh.arrays(), A.plain_octree_bvh(ok), "after the refusals:")
    bvh.close()


@pytest.mark.parametrize("at_surfaces", [False, True], ids=["at_box", "at_surfaces"])
@pytest.mark.parametrize("kind", A.SAH_KINDS)
def test_rays_of_the_traversal_check_have_no_more_ties_than_allowed(pkg, oracle, emu, kind, at_surfaces):
    """The ray set of the GPU traversal check (tests/test_gpu_bvh_awkward.py), on the host: the oracle through the rebuilt tree
    (255-surface leaf included) against the oracle's loop over all surfaces of the untouched scene - same t bits, same misses,
    same surfaces up to the allowance for exact-t ties. (Without the overlapping_* families: their triangles all overlap.)"""
    sc = scene_of_without_overlapping(pkg)
    bvh = pkg.Bvh(sc.desc, kind=kind, threads=1)
    order = bvh.arrays()["order"]
    assert 255 in bvh.arrays()["count"]
    rebuilt = bvh.apply(sc.desc)
    start, direction = A.ordinary_rays(sc, 2000, at_surfaces)

    class Rebuilt:
        scene = rebuilt.desc

    class Flat:  # no nodes: Scene::intersect loops over the surfaces (scene.cpp:159-172)
        scene = sc.desc
    t, surf, _, _ = oracle.intersect(Rebuilt, start, direction)
    t0, surf0, _, _ = oracle.intersect(Flat, start, direction)
    named = np.where(surf == A.MISS, A.MISS, order[np.minimum(surf, sc.n - 1)])  # position in the rebuilt scene -> input index
    hits, ties = A.same_hits(t, named, t0, surf0, "%s:" % kind)
    print("%s, %s: %d of 2000 rays hit, %d exact-t ties" % (kind, "at surfaces" if at_surfaces else "at the box", hits, ties))
    # (the families stand far apart: rays aimed at the scene box mostly pass between them and check the misses; the second set, aimed
    # at surfaces, is there for the hits)
    assert hits >= (1000 if at_surfaces else 1)
    # ... and the device's own walk compiled for the host (tests/emu/mcrt_emu.cpp), before the GPU sees its first 255-surface leaf
    for stage in (0, 1, 3):
        te, se, uve = np.empty(2000), np.empty(2000, dtype=np.uint32), np.empty((2000, 2))
        assert emu.emu_intersect(C.byref(rebuilt.desc), 2000, start.ctypes.data, direction.ctypes.data, stage, te.ctypes.data, se.ctypes.data, uve.ctypes.data) == 0
        A.same_hits(te, se, t, surf, "%s, emulated device walk, stage %d:" % (kind, stage))
    rebuilt.close()
    bvh.close()

