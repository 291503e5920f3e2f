"""Small scenes the hierarchy builders have trouble with, for tests/test_bvh_awkward.py and tests/test_gpu_bvh_awkward.py
(a plain helper module: no fixtures, no pytest hooks).

Every family is a deterministic list of surfaces (fixed seed) together with a PREDICATE on the tree the recursive builder
(mcrt_bvh_build_sah / the octree host path) makes of it, which proves that the family reaches the rule it is there for:
a test asserts the predicate before it compares anything, so an input that stopped doing its job fails on the CPU instead
of passing silently. The predicates read the LinearNode arrays only (Bvh.arrays()) plus the family's own input.

    scene = awkward_scenes.scene(pkg, "coincident_256")      # one family
    scene = awkward_scenes.sah_concatenation(pkg)            # all SAH families side by side, < 2 000 surfaces
    scene.desc                                                # the SceneDesc (its numpy buffers live in `scene`)
    awkward_scenes.check(scene, "quaternary_sah", 8, arrays)  # the predicate(s); raises AssertionError

Surfaces are records (kind, v[9]); triangles get their edges and normal like the scene flattener writes them, spheres are
(centre, radius), quadrics are the records of tests/golden/quadric.mcrt (real coefficients and boxes)."""
import ctypes as C
import importlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20261020
TRI, SPHERE, QUADRIC = 0, 1, 2
LEAF, MAX_LEAF = 8, 255
EPS = 1e-9  # the centroid-extent test of the split rules (bvh.cpp:187,314)

SAH_KINDS = ("quaternary_sah", "binary_sah")


def _rng(name):
    return np.random.default_rng([SEED] + [ord(ch) for ch in name])


# ------------------------------------------------------------------------------------------------
# surfaces
# ------------------------------------------------------------------------------------------------
class Surfaces:
    """A list of surfaces: kind[n], v[n][9], and the quadric records [q][22] that kind-2 surfaces name in v[:, 0]."""

    def __init__(self, kind=None, v=None, quadrics=None):
        self.kind = np.zeros(0, np.uint8) if kind is None else np.asarray(kind, np.uint8)
        self.v = np.zeros((0, 9)) if v is None else np.ascontiguousarray(v, np.float64).reshape(-1, 9)
        self.quadrics = np.zeros((0, 22)) if quadrics is None else np.ascontiguousarray(quadrics, np.float64).reshape(-1, 22)

    @classmethod
    def triangles(cls, tris):
        v = np.ascontiguousarray(tris, np.float64).reshape(-1, 9)
        return cls(np.zeros(len(v), np.uint8), v)

    @classmethod
    def spheres(cls, centres, radii):
        c = np.asarray(centres, np.float64).reshape(-1, 3)
        v = np.zeros((len(c), 9))
        v[:, :3] = c
        v[:, 3] = radii
        return cls(np.full(len(c), SPHERE, np.uint8), v)

    @classmethod
    def quadric_records(cls, records):
        q = np.ascontiguousarray(records, np.float64).reshape(-1, 22)
        v = np.zeros((len(q), 9))
        v[:, 0] = np.arange(len(q))
        return cls(np.full(len(q), QUADRIC, np.uint8), v, q)

    def __len__(self):
        return len(self.kind)

    def __add__(self, other):
        ov = other.v.copy()
        ov[other.kind == QUADRIC, 0] += len(self.quadrics)
        return Surfaces(np.concatenate([self.kind, other.kind]), np.concatenate([self.v, ov]), np.concatenate([self.quadrics, other.quadrics]))

    def moved(self, offset):
        """Translated (triangles and spheres only: a quadric record is not moved by adding to its box)."""
        assert not (self.kind == QUADRIC).any()
        v = self.v.copy()
        off = np.asarray(offset, np.float64)
        t = self.kind == TRI
        v[t] = (v[t].reshape(-1, 3, 3) + off).reshape(-1, 9)
        s = self.kind == SPHERE
        v[s, :3] += off
        return Surfaces(self.kind, v)

    def take(self, idx):
        idx = np.asarray(idx)
        v = self.v[idx].copy()
        q = self.kind[idx] == QUADRIC
        used = v[q, 0].astype(int)
        v[q, 0] = np.arange(len(used))
        return Surfaces(self.kind[idx], v, self.quadrics[used])

    def boxes(self):
        """Surface::BB() as the builders compute it: [n][6] = min[3], max[3]; a triangle's box keeps the first vertex that
        attains the extreme (bounding-box.cpp:65-72), which decides the sign of a zero."""
        n = len(self)
        bb = np.zeros((n, 6))
        for i in range(n):
            k, v = self.kind[i], self.v[i]
            if k == SPHERE:
                bb[i, :3] = v[:3] - v[3]
                bb[i, 3:] = v[:3] + v[3]
            elif k == QUADRIC:
                bb[i] = self.quadrics[int(v[0]), 16:22]
            else:
                p = v.reshape(3, 3)
                for c in range(3):
                    mn = mx = p[0, c]
                    for j in (1, 2):
                        if mn > p[j, c]:
                            mn = p[j, c]
                        if mx < p[j, c]:
                            mx = p[j, c]
                    bb[i, c], bb[i, 3 + c] = mn, mx
        return bb

    def centroids(self):
        bb = self.boxes()
        return (bb[:, 3:] + bb[:, :3]) / 2.0


def first_seen_box(bb):
    """BoundingBox::merge over boxes in order (bounding-box.cpp:56-63): the first box that attains an extreme keeps its bits."""
    out = np.array([np.inf] * 3 + [-np.inf] * 3)
    for b in bb:
        for c in range(3):
            if out[c] > b[c]:
                out[c] = b[c]
            if out[3 + c] < b[3 + c]:
                out[3 + c] = b[3 + c]
    return out


class Scene:
    """A SceneDesc and everything it points into."""

    def __init__(self, pkg, surfaces, name, parts=None, scene_box=None):
        self.name = name
        self.surfaces = surfaces
        self.parts = parts or {name: (0, len(surfaces))}  # family -> (first surface, count)
        n = len(surfaces)
        self.n = n
        self.kind = np.ascontiguousarray(surfaces.kind)
        self.v = np.ascontiguousarray(surfaces.v)
        self.e = np.zeros((n, 9))
        t = self.kind == TRI
        e1, e2 = self.v[t, 3:6] - self.v[t, 0:3], self.v[t, 6:9] - self.v[t, 0:3]
        nrm = np.cross(e1, e2)
        self.area = np.ones(n)
        self.area[t] = np.linalg.norm(nrm, axis=1) / 2.0
        self.e[t, 0:3], self.e[t, 3:6] = e1, e2
        self.e[t, 6:9] = nrm / np.maximum(np.linalg.norm(nrm, axis=1), 1e-300)[:, None]
        self.interp = np.zeros(n, np.uint8)
        self.mat = np.zeros(n, np.uint32)
        self.quadrics = np.ascontiguousarray(surfaces.quadrics)
        self.material = pkg.Material()
        self.bb = surfaces.boxes()
        box = first_seen_box(self.bb) if scene_box is None else np.asarray(scene_box, np.float64)  # Scene::computeBoundingBox
        self.box = box
        d = pkg.SceneDesc()
        d.abi_version = 2
        d.num_surfaces = n
        d.surf_kind = self.kind.ctypes.data_as(C.POINTER(C.c_uint8))
        d.surf_interpolate = self.interp.ctypes.data_as(C.POINTER(C.c_uint8))
        d.surf_material = self.mat.ctypes.data_as(C.POINTER(C.c_uint32))
        d.surf_area = self.area.ctypes.data_as(C.POINTER(C.c_double))
        d.surf_v = self.v.ctypes.data_as(C.POINTER(C.c_double))
        d.surf_e = self.e.ctypes.data_as(C.POINTER(C.c_double))
        d.num_materials = 1
        d.materials = C.pointer(self.material)
        d.scene_ior = 1.0
        d.bb_min[:] = box[:3].tolist()
        d.bb_max[:] = box[3:].tolist()
        if len(self.quadrics):
            d.num_quadrics = len(self.quadrics)
            d.quadrics = self.quadrics.ctypes.data_as(C.POINTER(C.c_double))
        self.desc = d


# ------------------------------------------------------------------------------------------------
# the tree, read from the LinearNode arrays
# ------------------------------------------------------------------------------------------------
class Tree:
    def __init__(self, arrays):
        self.a = arrays
        self.n = len(arrays["start"])
        self.children = [[] for _ in range(self.n)]
        self.parent = np.full(self.n, -1)
        cnt, nxt = arrays["count"], arrays["next"]
        self.end = np.zeros(self.n, np.int64)  # one past the node's subtree in depth-first numbering

        def walk(i, after):  # iterative: trees over coincident centroids get deep
            stack = [(i, after)]
            while stack:
                i, after = stack.pop()
                self.end[i] = after
                if cnt[i]:
                    continue
                c = i + 1
                kids = []
                while c != 0:
                    kids.append(c)
                    c = int(nxt[c])
                for k, c in enumerate(kids):
                    self.parent[c] = i
                    stack.append((c, kids[k + 1] if k + 1 < len(kids) else after))
                self.children[i] = kids
        if self.n:
            walk(0, self.n)
        # surfaces below a node: positions [first, last) of `order`
        self.first = np.asarray(arrays["start"], np.int64).copy()
        self.last = np.zeros(self.n, np.int64)
        total = len(arrays["order"])
        for i in range(self.n):
            e = int(self.end[i])
            self.last[i] = int(arrays["start"][e]) if e < self.n else total
        for i in range(self.n):
            if cnt[i]:
                assert self.last[i] - self.first[i] == cnt[i], "leaf %d: %d surfaces listed, next node starts %d later" % (i, cnt[i], self.last[i] - self.first[i])

    def size(self, i):
        return int(self.last[i] - self.first[i])

    def surfaces(self, i):
        return self.a["order"][self.first[i]:self.last[i]]

    def leaves(self):
        return [i for i in range(self.n) if self.a["count"][i]]

    def inner(self):
        return [i for i in range(self.n) if not self.a["count"][i]]

    def node_of_exactly(self, surfaces):
        """The node whose surfaces are exactly this set, or None."""
        want = np.sort(np.asarray(surfaces))
        for i in range(self.n):
            if self.size(i) == len(want) and np.array_equal(np.sort(self.surfaces(i)), want):
                return i
        return None

    def below(self, i):
        return range(i, int(self.end[i]))


def _centroid_dims(scene, surfaces):
    c = (scene.bb[surfaces, 3:] + scene.bb[surfaces, :3]) / 2.0
    return c.max(axis=0) - c.min(axis=0)


# ------------------------------------------------------------------------------------------------
# SAH families: name -> Surfaces; predicates: name -> f(scene, tree, part = (first, count), kind, bins)
# ------------------------------------------------------------------------------------------------
def _tilted_coincident(name, count, centre=(0.0, 0.0, 0.0)):
    """`count` triangles whose BOXES share one centroid exactly (box = centre -/+ (a, b, h) with dyadic a, b, h) and whose planes
    all differ: triangle i is (-a, -b, -h), (a, -b, h), (s, b, w) with its own a, b, h, s, w - the third vertex's x and z lie strictly
    inside the box, so they move the plane and not the box."""
    rng = _rng(name)
    tris = []
    for i in range(count):
        a, b, h = (8 + i) / 64.0, (8 + (i * 7) % 97) / 64.0, (1 + (i * 5) % 31) / 128.0
        s, w = (rng.random() - 0.5) * a, (rng.random() - 0.5) * h
        tris.append([[-a, -b, -h], [a, -b, h], [s, b, w]])
    return Surfaces.triangles(tris).moved(centre)


def _line(name, count=150):
    rng = _rng(name)
    xs = np.round(rng.random(count) * 4096.0) / 64.0  # dyadic, so that every box centroid has y and z exactly 1 and 5
    tris = [[[x - 0.5, 0.75, 4.5], [x + 0.5, 0.75, 5.5], [x + (rng.random() - 0.5) * 0.5, 1.25, 5.0 + (rng.random() - 0.5) * 0.5]] for x in xs]
    return Surfaces.triangles(tris)


def _diagonal(name, count=150):
    rng = _rng(name)
    ds = np.round(rng.random(count) * 4096.0) / 64.0
    tris = []
    for d in ds:  # box = d -/+ 1/4 on every axis: centroid exactly (d, d, d)
        tris.append([[d - 0.25, d - 0.25, d - 0.25], [d + 0.25, d - 0.25, d + 0.25], [d + (rng.random() - 0.5) * 0.25, d + 0.25, d + (rng.random() - 0.5) * 0.25]])
    return Surfaces.triangles(tris)


def _overlapping(name, count):
    """Triangles that each span (nearly) the unit cube: every bin's box is (nearly) the node's, every split costs 1 + size. The
    vertices are jittered by 1e-6, so the centroids differ by about that much on every axis (far above 1e-9)."""
    rng = _rng(name)
    tris = []
    for i in range(count):
        j = rng.random((3, 3)) * 2e-6
        tris.append((np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]]) + j).tolist())
    return Surfaces.triangles(tris)


THRESHOLD_CLUSTER = 40


def _threshold(name):
    """Two clusters of 40 tiny triangles (1e-10 across) at x = 1 and x = 3; the box centroids of the first spread over 0.9e-9 along
    x, those of the second over 1.1e-9: either side of the 1e-9 test."""
    rng = _rng(name)
    tris = []
    for base, spread in ((1.0, 0.9e-9), (3.0, 1.1e-9)):
        for i in range(THRESHOLD_CLUSTER):
            x = base + spread * i / (THRESHOLD_CLUSTER - 1)
            h = 0.5e-10
            tris.append([[x - h, 2.0 - h, 2.0 - h], [x + h, 2.0 - h, 2.0 + h], [x + (rng.random() - 0.5) * h, 2.0 + h, 2.0 + (rng.random() - 0.5) * h]])
    return Surfaces.triangles(tris)


def _signed_zero(name, per_octant=12):
    """In each octant triangles that touch the three coordinate planes: on every axis one vertex coordinate is a zero, stored as
    -0.0 or +0.0 at random, and the others lie on the octant's side. Plus one sphere per positive-side plane pair that touches
    the planes (centre = radius). Boxes of nodes inside one octant then have zeros that came from both signs."""
    rng = _rng(name)
    tris = []
    for octant in range(8):
        sgn = np.array([1.0 if octant & (1 << c) else -1.0 for c in range(3)])
        for _ in range(per_octant):
            p = (0.25 + rng.random((3, 3)) * 2.0) * sgn  # three vertices inside the octant
            for c in range(3):
                p[rng.integers(3), c] = -0.0 if rng.random() < 0.5 else 0.0
            tris.append(p.tolist())
    out = Surfaces.triangles(tris)
    order = rng.permutation(len(out))  # octants interleaved: a node's first zero is not always the same octant's
    out = out.take(order)
    return out + Surfaces.spheres([[0.5, 0.5, 0.5], [1.25, 0.75, 0.75]], [0.5, 0.75])


def _quadric_records():
    """The small quadrics of the `quadric` golden image (its seven large slabs left out): (Q[16], box[6]) records."""
    pkg = importlib.import_module("monte-carlo-ray-tracer_amd")
    img = pkg.SceneImage(os.path.join(GOLDEN, "quadric.mcrt"))
    s = img.scene
    q = np.ctypeslib.as_array(s.quadrics, shape=(s.num_quadrics, 22)).copy()
    img.close()
    small = (q[:, 19:22] - q[:, 16:19]).max(axis=1) < 2.0
    q = q[small]
    return q[np.lexsort(q[:, 16:22].T[::-1])]  # an order of their own (by box), not the image's


def _mixed_kinds(name):
    rng = _rng(name)
    q = Surfaces.quadric_records(_quadric_records())
    assert len(q) >= 2
    c = rng.random((14, 3)) * 2.0 - 1.0
    sph = Surfaces.spheres(c, 0.05 + rng.random(14) * 0.2)
    tc = rng.random((24, 3)) * 2.0 - 1.0
    tri = Surfaces.triangles(tc[:, None, :] + rng.normal(scale=0.15, size=(24, 3, 3)))
    allof = tri + sph + q
    return allof.take(rng.permutation(len(allof)))


def _cloud(name, count=300):
    rng = _rng("cloud")  # (cloud_1, cloud_8, ... are prefixes of the same cloud)
    c = rng.random((300, 3)) * 8.0 - 4.0
    tris = c[:, None, :] + rng.normal(scale=0.08, size=(300, 3, 3))
    return Surfaces.triangles(tris[:count])


SAH_FAMILIES = {
    "coincident_255": lambda n: _tilted_coincident(n, 255),
    "coincident_256": lambda n: _tilted_coincident(n, 256),
    "line": _line,
    "diagonal": _diagonal,
    "overlapping_300": lambda n: _overlapping(n, 300),
    "overlapping_100": lambda n: _overlapping(n, 100),
    "threshold": _threshold,
    "signed_zero": _signed_zero,
    "mixed_kinds": _mixed_kinds,
    "cloud": _cloud,
    "cloud_1": lambda n: _cloud(n, 1),
    "cloud_8": lambda n: _cloud(n, 8),
    "cloud_9": lambda n: _cloud(n, 9),
    "cloud_10": lambda n: _cloud(n, 10),
}

# where a family sits in the concatenation (far apart: the top splits separate them); mixed_kinds holds quadrics and stays put
SAH_CONCATENATION = [("mixed_kinds", None), ("coincident_255", (40.0, 0.0, 0.0)), ("coincident_256", (0.0, 40.0, 0.0)), ("line", (-90.0, -40.0, 30.0)),
                     ("diagonal", (60.0, 60.0, 60.0)), ("overlapping_300", (-40.0, 0.0, -40.0)), ("overlapping_100", (0.0, -40.0, -40.0)),
                     ("threshold", (-40.0, 40.0, 0.0)), ("signed_zero", None), ("cloud", (40.0, -40.0, 40.0))]
OVERLAPPING = ("overlapping_300", "overlapping_100")


def _node_of_part(scene, tree, part):
    first, count = part
    node = tree.node_of_exactly(np.arange(first, first + count))
    assert node is not None, "%s: no node holds exactly the family's %d surfaces" % (scene.name, count)
    return node


def _p_coincident_255(scene, tree, part, kind, bins):
    node = _node_of_part(scene, tree, part)
    assert tree.a["count"][node] == 255, "255 coincident centroids must stay ONE leaf (count %d)" % tree.a["count"][node]
    assert (_centroid_dims(scene, np.arange(part[0], part[0] + part[1])) < EPS).all()


def _p_coincident_256(scene, tree, part, kind, bins):
    node = _node_of_part(scene, tree, part)
    kids = tree.children[node]
    assert len(kids) == 2 and [tree.a["count"][k] for k in kids] == [128, 128], "256 coincident centroids: dealt into 128 + 128"
    for k, child in enumerate(kids):  # positions i = k (mod 2) of the node's run (the node's run is in input order)
        np.testing.assert_array_equal(tree.surfaces(child), part[0] + np.arange(k, 256, 2))


def _p_line(scene, tree, part, kind, bins):
    node = _node_of_part(scene, tree, part)
    d = _centroid_dims(scene, np.arange(part[0], part[0] + part[1]))
    assert d[0] > 1.0 and d[1] == 0.0 and d[2] == 0.0
    assert not tree.a["count"][node] and tree.size(node) > LEAF
    assert max(len(tree.children[i]) for i in tree.below(node)) == 2, "one usable axis: binary rule for the whole subtree"
    assert max(tree.a["count"][i] for i in tree.below(node)) <= LEAF


def _p_diagonal(scene, tree, part, kind, bins):
    node = _node_of_part(scene, tree, part)
    d = _centroid_dims(scene, np.arange(part[0], part[0] + part[1]))
    assert (d > 1.0).all()
    if kind == "quaternary_sah":  # two usable axes, so the node is split by the quaternary rule - and two quadrants stay empty
        assert 2 <= len(tree.children[node]) < 4, "diagonal: quaternary node with %d children" % len(tree.children[node])
    else:
        assert len(tree.children[node]) == 2


def _p_overlapping_300(scene, tree, part, kind, bins):
    node = _node_of_part(scene, tree, part)
    d = _centroid_dims(scene, np.arange(part[0], part[0] + part[1]))
    assert np.sort(d)[1] >= EPS, "two usable axes: the split is refused by COST, not by extent"
    parts = 4 if kind == "quaternary_sah" else 2
    kids = tree.children[node]
    assert len(kids) == parts, "300 overlapping: %d children" % len(kids)
    for k, child in enumerate(kids):
        np.testing.assert_array_equal(tree.surfaces(child), part[0] + np.arange(k, 300, parts))
        if kind == "quaternary_sah":
            assert tree.a["count"][child] == 75, "a part of 75 overlapping triangles stays a leaf (child rule 4: cost again)"


def _p_overlapping_100(scene, tree, part, kind, bins):
    node = _node_of_part(scene, tree, part)
    assert np.sort(_centroid_dims(scene, np.arange(part[0], part[0] + part[1])))[1] >= EPS
    assert tree.a["count"][node] == 100, "100 overlapping triangles: no split is cheaper than the leaf"


def _p_threshold(scene, tree, part, kind, bins):
    first = part[0]
    a, b = np.arange(first, first + THRESHOLD_CLUSTER), np.arange(first + THRESHOLD_CLUSTER, first + 2 * THRESHOLD_CLUSTER)
    da, db = _centroid_dims(scene, a), _centroid_dims(scene, b)
    assert 0.5e-9 < da[0] < EPS < db[0] < 1.5e-9 and da[1] == da[2] == db[1] == db[2] == 0.0, (da, db)
    na, nb = tree.node_of_exactly(a), tree.node_of_exactly(b)
    assert na is not None and nb is not None, "the two clusters must be nodes of their own"
    assert tree.a["count"][na] == THRESHOLD_CLUSTER, "extent 0.9e-9 < 1e-9: the cluster stays a leaf of 40"
    # extent 1.1e-9: split by the binary rule (one usable axis) - into halves whose own extent is below 1e-9, which stay leaves
    assert not tree.a["count"][nb] and len(tree.children[nb]) == 2, "extent 1.1e-9 >= 1e-9: the cluster is split"
    assert all(LEAF < tree.a["count"][k] < THRESHOLD_CLUSTER for k in tree.children[nb])


def zero_sign_cases(scene, tree):
    """Nodes (other than the root, whose box is the scene's) with a box coordinate 0 that surfaces of BOTH zero signs attain:
    list of (node, coordinate, sign bit of the first such surface in node order = input order, sign bit stored in the tree)."""
    out = []
    bits = scene.bb.view(np.uint64)
    for i in range(1, tree.n):
        s = np.sort(tree.surfaces(i))
        for c in range(6):
            if tree.a["bounds"][i, c] != 0.0:
                continue
            at = s[scene.bb[s, c] == 0.0]
            signs = bits[at, c] >> 63
            if len(at) and signs.min() != signs.max():
                out.append((i, c, int(signs[0]), int(tree.a["bounds"][i].view(np.uint64)[c] >> 63)))
    return out


def _p_signed_zero(scene, tree, part, kind, bins):
    first, count = part
    mine = set(range(first, first + count))
    cases = [x for x in zero_sign_cases(scene, tree) if set(tree.surfaces(x[0]).tolist()) <= mine]
    firsts = {x[2] for x in cases}
    assert firsts == {0, 1}, "signed_zero: mixed-sign zero coordinates with each sign first are needed, got %d cases, first signs %s" % (len(cases), firsts)
    # ... in minima and in maxima
    assert {x[1] < 3 for x in cases} == {True, False}
    for node, c, first_sign, stored in cases:  # bounding-box.cpp:56-63: the first surface that attains the extreme keeps its bits
        assert stored == first_sign, "node %d coordinate %d: sign of zero %d, first contributor has %d" % (node, c, stored, first_sign)


def _p_mixed_kinds(scene, tree, part, kind, bins):
    k = scene.kind[part[0]:part[0] + part[1]]
    assert (k == QUADRIC).sum() >= 2 and (k == SPHERE).sum() >= 2 and (k == TRI).sum() >= 2
    assert len(scene.quadrics) >= 2 and np.abs(scene.quadrics[:, :16]).max() > 0
    leaf_kinds = set()
    for l in tree.leaves():
        s = tree.surfaces(l)
        s = s[(s >= part[0]) & (s < part[0] + part[1])]
        leaf_kinds |= set(scene.kind[s].tolist())
    assert leaf_kinds == {TRI, SPHERE, QUADRIC}


def _p_cloud(scene, tree, part, kind, bins):
    mine = lambda i: part[0] <= tree.surfaces(i).min() and tree.surfaces(i).max() < part[0] + part[1]
    small = [i for i in tree.inner() if tree.size(i) < 64 and mine(i)]
    assert len(small) >= 8, "cloud: %d open nodes smaller than a wave" % len(small)
    v = scene.v[part[0]:part[0] + part[1]]
    assert (v < 0).any() and (v > 0).any()


def _p_cloud_n(n):
    def p(scene, tree, part, kind, bins):
        assert scene.n == n
        if n <= LEAF:
            assert tree.n == 1 and tree.a["count"][0] == n, "root leaf"
        else:
            assert not tree.a["count"][0] and tree.n >= 3, "smallest open root"
    return p


SAH_PREDICATES = {
    "coincident_255": _p_coincident_255, "coincident_256": _p_coincident_256, "line": _p_line, "diagonal": _p_diagonal,
    "overlapping_300": _p_overlapping_300, "overlapping_100": _p_overlapping_100, "threshold": _p_threshold, "signed_zero": _p_signed_zero,
    "mixed_kinds": _p_mixed_kinds, "cloud": _p_cloud, "cloud_1": _p_cloud_n(1), "cloud_8": _p_cloud_n(8), "cloud_9": _p_cloud_n(9),
    "cloud_10": _p_cloud_n(10),
}


# ------------------------------------------------------------------------------------------------
# octree families
# ------------------------------------------------------------------------------------------------
def _box_triangle(c, h, rng):
    """A triangle whose box is exactly c -/+ h (h dyadic): centroid exactly c."""
    c = np.asarray(c, np.float64)
    return [[c[0] - h, c[1] - h, c[2] - h], [c[0] + h, c[1] - h, c[2] + h], [c[0] + (rng.random() - 0.5) * h, c[1] + h, c[2] + (rng.random() - 0.5) * h]]


def _corner_triangles():
    """Two triangles that make the scene box exactly [-4, 4]^3."""
    return [[[-4.0, -4.0, -4.0], [-3.5, -4.0, -3.5], [-3.75, -3.5, -3.75]], [[4.0, 4.0, 4.0], [3.5, 4.0, 3.5], [3.75, 3.5, 3.75]]]


def _on_planes(name):
    rng = _rng(name)
    tris = _corner_triangles()
    grid = [0.0, 1.0, -1.0, 2.0, -2.0]
    for x in grid:
        for y in grid:
            for z in grid:
                tris.append(_box_triangle((x, y, z), 0.125, rng))
    return Surfaces.triangles(tris)


def _far_face(name):
    """The scene box is [-4, 4]^3 and so is the root cube; one triangle lies IN the plane x = 4 (its box has no extent along x), one
    in y = 4, one in z = 4: their centroids sit on the cube's maximum faces. Plus a few ordinary ones."""
    rng = _rng(name)
    tris = _corner_triangles()
    tris.append([[4.0, 1.0, 1.0], [4.0, 2.0, 1.5], [4.0, 1.5, 2.5]])
    tris.append([[1.0, 4.0, -1.0], [2.0, 4.0, -1.5], [1.5, 4.0, -2.5]])
    tris.append([[-1.0, -1.0, 4.0], [-2.0, -1.5, 4.0], [-1.5, -2.5, 4.0]])
    tris.append([[4.0, 4.0, 4.0], [4.0, 3.0, 4.0], [4.0, 4.0, 3.0]])  # and one in the far corner: centroid (4, 3.5, 3.5)
    for _ in range(20):
        tris.append(_box_triangle(rng.random(3) * 6.0 - 3.0, 0.125, rng))
    return Surfaces.triangles(tris)


def _nine_coincident(name):
    rng = _rng(name)
    tris = _corner_triangles()
    for i in range(9):
        h = (1 + i) / 16.0
        tris.append(_box_triangle((1.0, 1.0, 1.0), h, rng))
    return Surfaces.triangles(tris)


OCTREE_FAMILIES = {
    "on_planes": _on_planes, "far_face": _far_face, "mixed_kinds": _mixed_kinds, "nine_coincident": _nine_coincident, "signed_zero": _signed_zero,
    "cloud_1": lambda n: _cloud(n, 1), "cloud_8": lambda n: _cloud(n, 8), "cloud_9": lambda n: _cloud(n, 9),
}
OCTREE_REFUSED = ("nine_coincident",)


def _root_cube(scene):
    dims = scene.box[3:] - scene.box[:3]
    half = dims.max() / 2.0
    mid = (scene.box[3:] + scene.box[:3]) / 2.0
    return mid - half, mid + half


def _po_on_planes(scene, tree):
    mn, mx = _root_cube(scene)
    assert (mn == -4.0).all() and (mx == 4.0).all()
    c = (scene.bb[2:, 3:] + scene.bb[2:, :3]) / 2.0
    assert set(np.unique(c).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}, "centroids on the mid-planes of levels 0 (0), 1 (-/+2) and 2 (-/+1)"
    assert tree.n > 9 and max(tree.a["count"]) <= LEAF


def _po_far_face(scene, tree):
    mn, mx = _root_cube(scene)
    assert (mn == -4.0).all() and (mx == 4.0).all()
    c = (scene.bb[:, 3:] + scene.bb[:, :3]) / 2.0
    for axis in range(3):
        assert (c[:, axis] == mx[axis]).any(), "a centroid exactly on the cube's maximum face %d" % axis
    assert tree.n > 1


def _po_mixed(scene, tree):
    _p_mixed_kinds(scene, tree, (0, scene.n), "octree", 0)


def _po_cloud_n(n):
    def p(scene, tree):
        assert scene.n == n
        if n <= LEAF:
            assert tree.n == 1 and tree.a["count"][0] == n
        else:
            assert not tree.a["count"][0] and tree.n >= 3
    return p


def _po_signed_zero(scene, tree):
    cases = zero_sign_cases(scene, tree)
    assert {x[2] for x in cases} == {0, 1}, "octree signed_zero: nodes whose zero coordinates come from both signs, each sign first somewhere"


OCTREE_PREDICATES = {"signed_zero": _po_signed_zero, "on_planes": _po_on_planes, "far_face": _po_far_face, "mixed_kinds": _po_mixed, "cloud_1": _po_cloud_n(1), "cloud_8": _po_cloud_n(8),
                     "cloud_9": _po_cloud_n(9)}


# ------------------------------------------------------------------------------------------------
# entry points
# ------------------------------------------------------------------------------------------------
def surfaces_of(name):
    f = SAH_FAMILIES.get(name) or OCTREE_FAMILIES[name]
    return f(name)


def scene(pkg, name):
    return Scene(pkg, surfaces_of(name), name)


def sah_concatenation(pkg, without=()):
    """All SAH families side by side in one scene; `without`: families to leave out (the traversal checks drop the overlapping ones)."""
    allof, parts = Surfaces(), {}
    for name, offset in SAH_CONCATENATION:
        if name in without:
            continue
        s = surfaces_of(name)
        if offset is not None:
            s = s.moved(offset)
        parts[name] = (len(allof), len(s))
        allof = allof + s
    assert len(allof) <= 2000
    return Scene(pkg, allof, "sah_concatenation" + ("_without_" + "_".join(without) if without else ""), parts)


def octree_concatenation(pkg):
    """The octree families that fit one [-4, 4]^3 cube together (at most 8 centroids in any finest cell)."""
    allof, parts = Surfaces(), {}
    for name in ("on_planes", "far_face", "mixed_kinds"):
        s = surfaces_of(name)
        parts[name] = (len(allof), len(s))
        allof = allof + s
    return Scene(pkg, allof, "octree_concatenation", parts)


# Bin counts at which the top splits of the concatenation set every family apart as a node of its own, so that each family's
# predicate also holds inside it (0 = the rule's default, 8 or 16). With 2 or 3 bins per axis the top splits are too coarse for
# that (families share nodes for a few levels); there the concatenation is compared without its predicates, and the families
# alone carry them.
CONCATENATION_PREDICATE_BINS = (0, 5, 8, 16)


def check(scene_, kind, bins, arrays):
    """Asserts the predicate of every family in the scene on a tree of the RECURSIVE builder; returns the Tree."""
    tree = Tree(arrays)
    np.testing.assert_array_equal(np.sort(arrays["order"]), np.arange(scene_.n, dtype=np.uint32), err_msg="order is not a permutation")
    if kind == "octree":
        if scene_.name in OCTREE_PREDICATES:
            OCTREE_PREDICATES[scene_.name](scene_, tree)
        else:  # the octree concatenation: what still holds with the three families in one cube
            _po_far_face(scene_, tree)
            _p_mixed_kinds(scene_, tree, scene_.parts["mixed_kinds"], kind, 0)
        return tree
    if len(scene_.parts) > 1 and bins not in CONCATENATION_PREDICATE_BINS:
        return tree
    for name, part in scene_.parts.items():
        SAH_PREDICATES[name](scene_, tree, part, kind, bins)
    return tree


def same_bytes(got, want, what="", keys=("bounds", "start", "count", "next", "order")):
    """Two Bvh.arrays() dicts hold the same BYTES (-0.0 is not +0.0). On a difference in the bounds: which nodes and coordinates."""
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, "%s %s: shape %s %s against %s %s" % (what, k, a.shape, a.dtype, b.shape, b.dtype)
        if a.tobytes() == b.tobytes():
            continue
        if k == "bounds":
            ua, ub = a.view(np.uint64), b.view(np.uint64)
            bad = np.argwhere(ua != ub)
            lines = ["node %d coordinate %d: %r (0x%016x) against %r (0x%016x)" % (i, c, a[i, c], ua[i, c], b[i, c], ub[i, c]) for i, c in bad[:12]]
            raise AssertionError("%s bounds differ in %d places:\n  %s" % (what, len(bad), "\n  ".join(lines)))
        bad = np.nonzero(a.ravel() != b.ravel())[0]
        raise AssertionError("%s %s differs at %d places, first %d: %r against %r" % (what, k, len(bad), bad[0], a.ravel()[bad[0]], b.ravel()[bad[0]]))


# ------------------------------------------------------------------------------------------------
# the octree BVH, plainly: serial insertion into an octree of leaves of 8, then one node per non-empty octant
# ------------------------------------------------------------------------------------------------
class _Octant:
    def __init__(self, mn, mx):
        self.mn, self.mx = mn, mx  # float lists
        self.data = []             # surface indices, insertion order
        self.octants = None

    def centroid(self):
        return [(self.mx[c] + self.mn[c]) / 2.0 for c in range(3)]

    def insert(self, i, pos, depth=0):
        if depth > 64:
            raise RecursionError("more than 8 centroids that no subdivision separates")
        if self.octants is None:
            if len(self.data) < LEAF:
                self.data.append(i)
                return
            old, self.data = self.data, []
            mid = self.centroid()
            half = [(self.mx[c] - self.mn[c]) / 2.0 for c in range(3)]
            self.octants = []
            for o in range(8):
                origin = [mid[c] + half[c] * (0.5 if o & (4 >> c) else -0.5) for c in range(3)]
                h = [half[c] * 0.5 for c in range(3)]
                self.octants.append(_Octant([origin[c] - h[c] for c in range(3)], [origin[c] + h[c] for c in range(3)]))
            for d in old:
                self._into_octant(d, pos, depth)
        self._into_octant(i, pos, depth)

    def _into_octant(self, i, pos, depth):
        mid = self.centroid()
        o = 0
        for c in range(3):
            if pos[i][c] >= mid[c]:  # a centroid ON a mid-plane goes to the upper octant
                o |= 4 >> c
        self.octants[o].insert(i, pos, depth + 1)


def plain_octree_bvh(scene_):
    """The octree BVH of a Scene built the slow way, as a dict like Bvh.arrays(): the independent statement that the sorted-code
    builders (host and GPU) are compared with. Boxes are merged first-seen (leaves: surfaces in insertion order; inner nodes:
    children in octant order), so zero signs are defined too. Raises RecursionError where no subdivision can separate the
    centroids (the builders refuse such input)."""
    mn, mx = _root_cube(scene_)
    root = _Octant(mn.tolist(), mx.tolist())
    pos = ((scene_.bb[:, 3:] + scene_.bb[:, :3]) / 2.0).tolist()
    for i in range(scene_.n):
        root.insert(i, pos)
    bounds, start, count, nxt, order = [], [], [], [], []

    def build(o):
        """-> (box, node index); appends the subtree depth-first."""
        me = len(start)
        bounds.append(None)
        start.append(len(order))
        nxt.append(0)
        if o.octants is None:
            count.append(len(o.data))
            order.extend(o.data)
            box = first_seen_box(scene_.bb[o.data])
        else:
            count.append(0)
            boxes, prev = [], None
            for ch in o.octants:
                if ch.octants is None and not ch.data:
                    continue
                if prev is not None:
                    nxt[prev] = len(start)
                b, prev = build(ch)
                boxes.append(b)
            box = first_seen_box(boxes)
        bounds[me] = box
        return box, me
    build(root)
    return dict(bounds=np.array(bounds, np.float64).reshape(-1, 6), start=np.array(start, np.uint32), count=np.array(count, np.uint32),
                next=np.array(nxt, np.uint32), order=np.array(order, np.uint32))


def ordinary_rays(scene_, count=2000, at_surfaces=False):
    """Ordinary rays for a traversal check: origins on a sphere around the scene, aimed at random points of the scene box (or,
    at_surfaces: of the boxes of randomly chosen surfaces, so that most of them hit something). Nothing adversarial: no
    axis-parallel directions, no rays through vertices. -> start[count][3], direction[count][3] (unit)."""
    rng = _rng("rays" + scene_.name + ("s" if at_surfaces else ""))
    lo, hi = scene_.box[:3], scene_.box[3:]
    centre, radius = (lo + hi) / 2.0, np.linalg.norm(hi - lo)  # twice the box's circumscribed radius
    d = rng.normal(size=(count, 3))
    start = centre + radius * d / np.linalg.norm(d, axis=1)[:, None]
    if at_surfaces:
        pick = rng.integers(scene_.n, size=count)
        tlo, thi = scene_.bb[pick, :3], scene_.bb[pick, 3:]
    else:
        tlo, thi = lo, hi
    target = tlo + rng.random((count, 3)) * (thi - tlo)
    direction = target - start
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    assert (np.abs(direction) > 1e-6).all()
    return np.ascontiguousarray(start), np.ascontiguousarray(direction)


MISS = 0xFFFFFFFF
TIES_ALLOWED = 5  # exact-t ties between two surfaces, as in tests/test_bvh_build.py::test_shuffled_surfaces_give_the_same_hits


def same_hits(t, surf, t_ref, surf_ref, what=""):
    """t bits equal, miss sets equal, surface ids (both in the SAME numbering) equal except at most TIES_ALLOWED exact-t ties.
    -> (hits, ties)."""
    t, t_ref = np.asarray(t), np.asarray(t_ref)
    assert t.view(np.uint64).tobytes() == t_ref.view(np.uint64).tobytes(), "%s t differs at %d rays" % (what, (t.view(np.uint64) != t_ref.view(np.uint64)).sum())
    miss, miss_ref = surf == MISS, surf_ref == MISS
    assert np.array_equal(miss, miss_ref), "%s miss sets differ" % what
    ties = int((surf[~miss] != surf_ref[~miss]).sum())
    assert ties <= TIES_ALLOWED, "%s %d rays name another surface" % (what, ties)
    return int((~miss).sum()), ties


# ------------------------------------------------------------------------------------------------
# shared by the host and the GPU test modules
# ------------------------------------------------------------------------------------------------
AWKWARD = os.path.join(GOLDEN, "awkward")  # the reference-made fixtures (tests/golden/make_awkward.py)
BINS = (2, 3, 5, 16)
MCRT_ERR_UNSUPPORTED = -7


def fixtures():
    import json
    return json.load(open(os.path.join(AWKWARD, "index.json")))["fixtures"]


_scenes = {}


def scene_of(pkg, name):
    """The scenes are made once per session and never modified."""
    if name not in _scenes:
        if name == "sah_concatenation":
            _scenes[name] = sah_concatenation(pkg)
        elif name == "octree_concatenation":
            _scenes[name] = octree_concatenation(pkg)
        else:
            _scenes[name] = scene(pkg, name)
    return _scenes[name]


def image_arrays(img):
    s = img.scene
    n = s.num_nodes
    g = lambda p, c, t: np.ctypeslib.as_array(p, shape=(c,)).astype(t, copy=True)
    return dict(bounds=g(s.node_bounds, n * 6, np.float64).reshape(n, 6), start=g(s.node_start_surface, n, np.uint32),
                count=g(s.node_num_surfaces, n, np.uint32), next=g(s.node_next_sibling, n, np.uint32),
                order=np.arange(s.num_surfaces, dtype=np.uint32))  # the image's surfaces are in the reference's order already


def scene_of_without_overlapping(pkg):
    if "no_overlap" not in _scenes:
        _scenes["no_overlap"] = sah_concatenation(pkg, without=OVERLAPPING)
    return _scenes["no_overlap"]


def image_surfaces(img):
    """kind[n], v[n][9] with a quadric's index replaced by nothing (0), and the quadric record of every surface ([n][22], zeros elsewhere)."""
    s = img.scene if hasattr(img, "scene") else img
    n = s.num_surfaces
    kind = np.ctypeslib.as_array(s.surf_kind, shape=(n,)).copy()
    v = np.ctypeslib.as_array(s.surf_v, shape=(n, 9)).copy()
    rec = np.zeros((n, 22))
    if s.num_quadrics:
        q = np.ctypeslib.as_array(s.quadrics, shape=(s.num_quadrics, 22))
        isq = kind == QUADRIC
        rec[isq] = q[v[isq, 0].astype(int)]
        v[isq, 0] = 0.0
    return kind, v, rec


def same_tree_and_order(got, scene_desc, img, what):
    """The nodes are the image's, byte for byte, and the input's surfaces taken in the built order are the image's surfaces."""
    ref = image_arrays(img)
    same_bytes(got, ref, what, keys=("bounds", "start", "count", "next"))
    np.testing.assert_array_equal(np.sort(got["order"]), np.arange(len(got["order"]), dtype=np.uint32))
    kind, v, rec = image_surfaces(scene_desc)
    rkind, rv, rrec = image_surfaces(img)
    o = got["order"]
    assert kind[o].tobytes() == rkind.tobytes() and v[o].tobytes() == rv.tobytes() and rec[o].tobytes() == rrec.tobytes(), what + " surface order differs from the reference's"
