"""The GPU paths of the hierarchy builders (csrc/mcrt_sah_gpu.hip, bvhOctreeGpu in csrc/mcrt_octree_gpu.hip) on the awkward
scenes of tests/awkward_scenes.py, compared as BYTES with the recursive host builder, the octree host path and the fixtures the
reference made (tests/golden/awkward/). What each family is for, and the host tier of the same comparisons:
tests/test_bvh_awkward.py. One context for the whole module; every case is at most a few thousand surfaces."""
import ctypes as C
import os

import numpy as np
import pytest

import awkward_scenes as A
AWKWARD, BINS, MCRT_ERR_UNSUPPORTED, FIXTURES = A.AWKWARD, A.BINS, A.MCRT_ERR_UNSUPPORTED, A.fixtures()
SAH_SCENES = list(A.SAH_FAMILIES) + ["sah_concatenation"]
scene_of, scene_of_without_overlapping, image_arrays, same_tree_and_order = A.scene_of, A.scene_of_without_overlapping, A.image_arrays, A.same_tree_and_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind", A.SAH_KINDS)
@pytest.mark.parametrize("name", SAH_SCENES)
def test_gpu_sah_equals_recursive(pkg, ctx, name, kind):
    """All five arrays of the level-synchronous GPU build against the recursive builder's, at 2, 3, 5 and 16 bins per axis."""
    sc = scene_of(pkg, name)
    for bins in BINS:
        a = pkg.Bvh(sc.desc, kind=kind, bins_per_axis=bins, threads=1)
        want = a.arrays()
        A.check(sc, kind, bins, want)
        g = pkg.Bvh(sc.desc, ctx=ctx, kind=kind, bins_per_axis=bins)
        A.same_bytes(g.arrays(), want, "%s %s %d bins: GPU against recursive:" % (name, kind, bins))
        a.close()
        g.close()


@pytest.mark.parametrize("fx", FIXTURES, ids=[f["name"] for f in FIXTURES])
def test_gpu_rebuilds_the_reference_tree_of_an_awkward_scene(pkg, ctx, fx):
    """Through the GPU path: the nodes of the reference's image and its surface order (from the scene file's order; the octree BVH
    from the image's own surfaces as well - see tests/test_bvh_awkward.py for why not the SAH ones)."""
    img = pkg.SceneImage(os.path.join(AWKWARD, fx["image"]))
    sc = scene_of(pkg, fx["scene"])
    kw = dict(kind=fx["bvh"]) if fx["bvh"] == "octree" else dict(kind=fx["bvh"], bins_per_axis=fx["bins_per_axis"])
    bvh = pkg.Bvh(sc.desc, ctx=ctx, **kw)
    same_tree_and_order(bvh.arrays(), sc.desc, img, "%s, GPU path:" % fx["name"])
    bvh.close()
    if fx["bvh"] == "octree":
        bvh = pkg.Bvh(img.scene, ctx=ctx, **kw)
        A.same_bytes(bvh.arrays(), image_arrays(img), "%s from its own image, GPU path:" % fx["name"])
        bvh.close()
    img.close()


@pytest.mark.parametrize("kind", A.SAH_KINDS)
def test_gpu_entry_point_hands_17_bins_to_the_recursive_builder(pkg, ctx, kind):
    """bins_per_axis = 17 is one more than the level loop's bin tables hold: with a context too the entry point builds through the
    recursive builder - same bytes as asking it directly, and another tree than with 16 bins."""
    sc = scene_of(pkg, "sah_concatenation")
    direct = pkg.Bvh(sc.desc, kind=kind, bins_per_axis=17, threads=1)
    via = pkg.Bvh(sc.desc, ctx=ctx, kind=kind, bins_per_axis=17)
    A.same_bytes(via.arrays(), direct.arrays(), "%s 17 bins with a context:" % kind)
    coarse = pkg.Bvh(sc.desc, ctx=ctx, kind=kind, bins_per_axis=16)
    assert coarse.arrays()["bounds"].tobytes() != direct.arrays()["bounds"].tobytes()
    for x in (direct, via, coarse):
        x.close()


@pytest.mark.parametrize("name", [n for n in A.OCTREE_FAMILIES if n not in A.OCTREE_REFUSED] + ["octree_concatenation"])
def test_gpu_octree_equals_host_path(pkg, ctx, name):
    sc = scene_of(pkg, name)
    host = pkg.Bvh(sc.desc)
    want = host.arrays()
    A.check(sc, "octree", 0, want)
    gpu = pkg.Bvh(sc.desc, ctx=ctx)
    A.same_bytes(gpu.arrays(), want, "%s: bvhOctreeGpu against the host path:" % name)
    host.close()
    gpu.close()


def test_gpu_octree_refuses_nine_coincident_centroids(pkg, ctx):
    """The same refusal as the host path's (code and, with a context, the message); the refusal comes from the host assembly of
    ordinarily sized arrays, nothing oversized is launched; and the context builds the next scene correctly afterwards."""
    sc = scene_of(pkg, "nine_coincident")
    L = pkg.lib()
    h = C.c_void_p()
    assert L.mcrt_bvh_build_octree(None, C.byref(sc.desc), C.byref(h)) == MCRT_ERR_UNSUPPORTED
    h = C.c_void_p()
    assert L.mcrt_bvh_build_octree(ctx._h, C.byref(sc.desc), C.byref(h)) == MCRT_ERR_UNSUPPORTED
    assert not h.value
    assert L.mcrt_last_error(ctx._h).decode() == "more than 8 surface centroids inside one 2^-21 cell of the scene cube"
    with pytest.raises(pkg.McrtError, match="more than 8 surface centroids inside one 2\\^-21 cell"):
        pkg.Bvh(sc.desc, ctx=ctx)
    for name, kind in (("on_planes", "octree"), ("signed_zero", "octree"), ("cloud", "quaternary_sah")):
        ok = scene_of(pkg, name)
        host = pkg.Bvh(ok.desc, kind=kind, threads=1)
        gpu = pkg.Bvh(ok.desc, ctx=ctx, kind=kind)
        A.same_bytes(gpu.arrays(), host.arrays(), "%s after the refusal:" % name)
        host.close()
        gpu.close()


@pytest.mark.parametrize("kind", A.SAH_KINDS)
def test_gpu_traversal_of_the_awkward_tree_equals_oracle(pkg, ctx, oracle, kind):
    """The tree built on the GPU (a 255-surface leaf in it), applied, uploaded and traversed by the device against the oracle on
    the same rebuilt scene: t bits and miss sets equal, surfaces equal except at most 5 exact-t ties. 2 000 ordinary rays aimed
    at the scene box, and 2 000 more aimed at surfaces (the families stand far apart: the first set mostly checks misses).
    Without the overlapping_* families, whose triangles all overlap."""
    sc = scene_of_without_overlapping(pkg)
    bvh = pkg.Bvh(sc.desc, ctx=ctx, kind=kind)
    assert 255 in bvh.arrays()["count"]
    rebuilt = bvh.apply(sc.desc)
    ctx.upload_scene(rebuilt.desc)

    class Rebuilt:
        scene = rebuilt.desc
    for at_surfaces in (False, True):
        start, direction = A.ordinary_rays(sc, 2000, at_surfaces)
        t, surf, _ = ctx.intersect(start, direction)
        t0, surf0, _, _ = oracle.intersect(Rebuilt, start, direction)
        hits, ties = A.same_hits(t, surf, t0, surf0, "%s, %s:" % (kind, "at surfaces" if at_surfaces else "at the box"))
        print("%s, %s: %d of 2000 rays hit, %d exact-t ties" % (kind, "at surfaces" if at_surfaces else "at the box", hits, ties))
        assert hits >= (1000 if at_surfaces else 1)
    rebuilt.close()
    bvh.close()
