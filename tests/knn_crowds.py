"""Photon maps on which many photons share a distance, the queries and k that go with them, and the checks - for
tests/test_knn_crowds_emulation.py and tests/test_gpu_knn_crowds.py (a plain helper module: no fixtures, no pytest hooks).

The selection code of the photon searches (csrc/mcrt_waveknn.hpp, csrc/mcrt_groupknn.hpp, knnSearch per lane) is mostly there for equal
and nearly equal distances; caustic maps are tight clusters. Every map here is a seeded photon array [n][8] whose positions are float32
values (the array IS float32), a box and a leaf capacity:

    lattice        photons on a 0.5 grid: a query at a node or a cell centre has 6, 8, 12, 24 ... photons at one distance
    stacks60       stacks of 60 coincident photons and nothing else: whatever a search drops, it drops among equal keys first
    stacks150      stacks of 150 coincident photons plus loose ones: a stack does not fit what the 4-row buffer keeps after a reduction
    stacks300      stacks of 300: more than the 192 entries at which the 4-row buffer is reduced
    stacks1200     stacks of 1200: more than the 960 entries at which the 16-row buffer is reduced
    tight          clusters with sigma = 1e-5: thousands of distances inside 0.4 % of one another
    plane          photons on z = 1 (octant boxes of zero thickness)
    line           photons on a segment parallel to x, on a 2^-6 grid (stacks of a few)
    point_and_one  n - 1 coincident photons and one far away
    one_stack      62 coincident photons and nothing else: one leaf, every distance of a query equal

The reference is brute force with the reference's own expression on the float positions widened to double, (dx*dx + dy*dy) + dz*dz
(glm::distance2 as the other kNN tests write it), over the photons in the MAP's order, sorted. check() needs no tolerance.

Which of several photons at the k-th distance a search returns is not part of check(): the reference decides it by insertion order
(linear-octree.cpp:58-77), the searches here by the order of their buffers; include/mcrt.h says what is guaranteed."""
import numpy as np

SEED = 20261021
LO, HI = np.array([-2.0, -2.0, -1.0]), np.array([4.5, 4.0, 4.5])
NARROW_K = (1, 2, 49, 50, 51, 63, 64, 65, 127, 128)  # the 4-row candidate buffer (k <= 128)
WIDE_K = (129, 300, 767, 768)                        # the 16-row buffer (k <= 768)
LANE_K = (769, 1000)                                 # beyond: the per-lane search
GROUP_MAX_K = 64                                     # four queries per wave (kGrpMaxK)
# A query this far from the box sees every photon of every map here under ONE 20-bit prefix of the distance's bits (sign, exponent and
# 8 mantissa bits: what waveSelectBound / groupSelectBound search): d2 = 2.1e11 .. 2.1e11 (1 + 1e-4), and the next prefix boundary above
# 2^37 * 1.52734375 is 2^37 * 1.53125. prefixes_agree() is the predicate; the CPU tier asserts it for every map.
FAR_ALL = np.array([3.0e5, 2.5e5, 2.4e5])

MAP_NAMES = ("lattice", "stacks60", "stacks150", "stacks300", "stacks1200", "tight", "plane", "line", "point_and_one", "one_stack")


def _rng(name):
    return np.random.default_rng([SEED] + [ord(ch) for ch in name])


def _photons(pos, rng):
    """[n][8] records in a shuffled order (so that the index order says nothing about the position): unit flux, direction angles 0."""
    pos = np.asarray(pos, dtype=np.float32)
    pos = pos[rng.permutation(len(pos))]
    ph = np.zeros((len(pos), 8), dtype=np.float32)
    ph[:, 0:3] = 1.0
    ph[:, 3:6] = pos
    return ph


def _loose(rng, n):
    return (LO + rng.random((n, 3)) * (HI - LO)).astype(np.float32)


def _stacks(rng, stacks, height, loose):
    at = (LO + (0.1 + 0.8 * rng.random((stacks, 3))) * (HI - LO)).astype(np.float32)
    parts = [np.repeat(at, height, axis=0)]
    if loose:
        parts.append(_loose(rng, loose))
    return np.concatenate(parts), at


def photon_list(name):
    """-> (photons [n][8] float32, leaf capacity, positions worth asking at: stacks / cluster centres)"""
    rng = _rng(name)
    if name == "lattice":
        g = np.stack(np.meshgrid(np.arange(-1.5, 4.01, 0.5), np.arange(-1.5, 3.51, 0.5), np.arange(-0.5, 4.01, 0.5), indexing="ij"), axis=-1).reshape(-1, 3)
        return _photons(g, rng), 200, np.array([[1.0, 1.0, 2.0]])
    if name in ("stacks60", "stacks150", "stacks300", "stacks1200"):
        stacks, height, loose, leaf = {"stacks60": (8, 60, 0, 200), "stacks150": (9, 150, 600, 200), "stacks300": (5, 300, 500, 400),
                                       "stacks1200": (3, 1200, 600, 2000)}[name]
        pos, at = _stacks(rng, stacks, height, loose)
        return _photons(pos, rng), leaf, at
    if name == "tight":
        centres = LO + (0.2 + 0.6 * rng.random((3, 3))) * (HI - LO)
        pos = np.concatenate([c + 1e-5 * rng.normal(size=(1500, 3)) for c in centres] + [_loose(rng, 500)])
        return _photons(pos, rng), 2000, centres.astype(np.float32)
    if name == "plane":
        pos = _loose(rng, 3000)
        pos[:, 2] = 1.0
        return _photons(pos, rng), 200, pos[:2].copy()
    if name == "line":
        x = np.round((LO[0] + rng.random(1000) * (HI[0] - LO[0])) * 64.0) / 64.0
        pos = np.stack([x, np.full(1000, 0.5), np.full(1000, 1.25)], axis=1)
        return _photons(pos, rng), 200, pos[:2].astype(np.float32)
    if name == "point_and_one":
        at = np.array([[0.75, -0.5, 2.0]], dtype=np.float32)
        pos = np.concatenate([np.repeat(at, 179, axis=0), np.array([[4.0, 3.5, -0.5]], dtype=np.float32)])
        return _photons(pos, rng), 200, at
    if name == "one_stack":
        at = np.array([[2.25, 1.5, 0.375]], dtype=np.float32)
        return _photons(np.repeat(at, 62, axis=0), rng), 200, at
    raise KeyError(name)


def queries(name, positions, special):
    """-> (points [q][3] float64, a label per point). At most 64 per map."""
    rng = _rng(name + "/queries")
    pts, labels = [], []

    def add(label, p):
        for row in np.atleast_2d(np.asarray(p, dtype=np.float64)):
            pts.append(row)
            labels.append(label)
    add("inside", LO + rng.random((6, 3)) * (HI - LO))
    add("on a photon", positions[rng.integers(0, len(positions), 3)])   # float positions, widened: distance 0 to at least one photon
    add("on a stack", special[:2])
    add("near a stack", np.asarray(special[:2], dtype=np.float64) + np.array([0.03125, -0.0625, 0.015625]))
    add("lattice cell centre", [[1.25, 0.75, 1.75]])
    add("lattice node", [[1.0, 1.0, 2.0], [0.5, 2.0, 0.0]])
    add("lattice edge midpoint", [[1.25, 1.0, 2.0]])
    add("on a face", [[LO[0], 0.5, 1.0], [1.0, HI[1], 2.0], [HI[0], HI[1], HI[2]]])
    add("outside by 3", [[HI[0] + 3.0, 1.0, 1.5]])
    add("outside by 70", [[-40.0, -42.0, 38.0]])
    add("far_all", [FAR_ALL])
    return np.ascontiguousarray(np.array(pts)), labels


def distance2_all(pts, pos):
    """The reference's expression, photons in the order given: [q][n] float64."""
    d = np.asarray(pts, dtype=np.float64)[:, None, :] - np.asarray(pos, dtype=np.float64)[None, :, :]
    return (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]


def prefixes_agree(d2_row, bits=20):
    """All distances of one query share their top `bits` bits (kCoarseBits of csrc/mcrt_waveknn.hpp)."""
    hi = np.ascontiguousarray(d2_row, dtype=np.float64).view(np.uint64) >> np.uint64(64 - bits)
    return bool((hi == hi[0]).all())


class Crowd:
    """One map, built by the host builder (the reference's tree), with its queries and the brute-force answer - computed once."""

    def __init__(self, pkg, name, leaf=None):
        self.name = name
        ph, default_leaf, special = photon_list(name)
        self.leaf = leaf or default_leaf
        self.map = pkg.PhotonMap(ph, LO.tolist(), HI.tolist(), self.leaf)
        self.desc = self.map.desc
        self.n = int(self.desc.num_photons)
        assert self.n == len(ph)
        self.photons = np.ctypeslib.as_array(self.desc.photons, (self.n, 8))  # in the MAP's order: what the indices of a search mean
        self.pos = self.photons[:, 3:6].astype(np.float64)
        self.pts, self.labels = queries(name, self.pos, special)
        self.d2_all = distance2_all(self.pts, self.pos)
        self.d2_sorted = np.sort(self.d2_all, axis=1)
        for a in (self.pts, self.d2_all, self.d2_sorted):
            a.setflags(write=False)

    def ks(self, kinds):
        """The k of the forms named in `kinds` ("narrow", "wide", "lane", "group"), with n - 1, n, n + 1 where they fit one."""
        around = [k for k in (self.n - 1, self.n, self.n + 1) if k >= 1]
        out = []
        if "group" in kinds:
            out += [k for k in NARROW_K + tuple(around) if k <= GROUP_MAX_K]
        if "narrow" in kinds:
            out += [k for k in NARROW_K + tuple(around) if k <= 128]
        if "wide" in kinds:
            out += [k for k in WIDE_K + tuple(around) if 128 < k <= 768]
        if "lane" in kinds:
            out += [k for k in LANE_K + tuple(around) if k > 768]
        return sorted(set(out))

    def tied_at_cut(self, k):
        """Per query: more photons share the k-th distance than the answer has room for (which of them come back is the search's choice)."""
        if k >= self.n:
            return np.zeros(len(self.pts), dtype=bool)
        return self.d2_sorted[:, k - 1] == self.d2_sorted[:, k]

    def check(self, cnt, idx, d2, k, what=""):
        check(cnt, idx, d2, self.d2_all, k, what="%s %s" % (self.name, what), d2_sorted=self.d2_sorted, labels=self.labels)


_BUILT = {}


def crowd(pkg, name, leaf=None):
    key = (name, leaf)
    if key not in _BUILT:
        _BUILT[key] = Crowd(pkg, name, leaf)
    return _BUILT[key]


ROOM_GRID = 8.0                  # the golden maps' positions snapped to multiples of 2^-3: stacks on the surfaces
ROOM_PAYLOAD = (0.02, 0.7, 2.2)  # one flux (all channels) and one direction (phi, theta) for every photon of a map


class CrowdedRoom:
    """A golden photon-mapped scene with its two maps made crowded: positions snapped to a 2^-3 grid (clipped to the scene's box), one
    constant flux and direction. Whichever of several photons at the k-th distance a search keeps, the terms of an estimate are then
    the same numbers. Quacks like a SceneImage for oracle_lib and the emulation (.scene, .photons(which), .param(key))."""

    def __init__(self, pkg, img, k=50):
        self.img, self.scene, self.k = img, img.scene, k
        lo, hi = np.array(img.scene.bb_min[:]), np.array(img.scene.bb_max[:])
        lo32 = np.nextafter(lo.astype(np.float32), np.float32(np.inf))  # float32 values inside the box
        hi32 = np.nextafter(hi.astype(np.float32), np.float32(-np.inf))
        self.maps, self.stacked = [], []
        for which in (0, 1):
            d = img.photons(which)
            n = int(d.num_photons)
            ph = np.ctypeslib.as_array(d.photons, (n, 8)).copy()
            ph[:, 3:6] = np.clip(np.round(ph[:, 3:6] * np.float32(ROOM_GRID)) / np.float32(ROOM_GRID), lo32, hi32)
            ph[:, 0:3] = ROOM_PAYLOAD[0]
            ph[:, 6], ph[:, 7] = ROOM_PAYLOAD[1], ROOM_PAYLOAD[2]
            heights = np.unique(ph[:, 3:6], axis=0, return_counts=True)[1]
            self.stacked.append(int(heights[heights > 1].sum()))  # photons that share their position with another
            # (a leaf cannot split a stack: the reference's 200 per leaf unless a grid point holds more)
            self.maps.append(pkg.PhotonMap(ph, lo.tolist(), hi.tolist(), max(200, 2 * int(heights.max()))))

    def photons(self, which):
        return self.maps[which].desc

    def param(self, key):
        return {"k_nearest_photons": self.k, "direct_visualization": 0}.get(key, 0)


class EmptyMaps:
    """... and with no photons at all: what the frames of CrowdedRoom are compared with to show that its maps matter."""

    def __init__(self, img, k=50):
        self.img, self.scene, self.k = img, img.scene, k

    def photons(self, which):
        return None

    def param(self, key):
        return {"k_nearest_photons": self.k, "direct_visualization": 0}.get(key, 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(cnt, idx, d2, d2_all, k, what="", d2_sorted=None, labels=None):
    """What every search owes on any map, ties or none - all of it exact:
    the count is min(k, n); the distances are the sorted brute-force prefix, bit for bit; unused slots are +inf / 0xFFFFFFFF; every index
    is a photon's, the indices of a query are pairwise distinct, and each names a photon at exactly the distance reported with it; within a
    run of equal distances the indices ascend ("ties by index", include/mcrt.h)."""
    nq, n = d2_all.shape
    c = min(k, n)
    cnt, idx, d2 = np.asarray(cnt), np.asarray(idx), np.asarray(d2)
    assert idx.shape == (nq, k) and d2.shape == (nq, k) and cnt.shape == (nq,), what

    def where(bad):  # the first offending query, by its label
        q = int(np.nonzero(bad)[0][0])
        return "%s k = %d: query %d (%s)" % (what, k, q, labels[q] if labels else "?")
    assert (cnt == c).all(), where(cnt != c) + ": count %s, not %d" % (cnt[cnt != c][:4], c)
    want = (np.sort(d2_all, axis=1) if d2_sorted is None else d2_sorted)[:, :c]
    bad = (_bits(d2[:, :c]) != _bits(want)).any(axis=1)
    assert not bad.any(), where(bad) + ": distances are not the brute-force prefix"
    bad = (~np.isposinf(d2[:, c:])).any(axis=1) | (idx[:, c:] != 0xFFFFFFFF).any(axis=1)
    assert not bad.any(), where(bad) + ": unused slots are not +inf / 0xFFFFFFFF"
    got = idx[:, :c].astype(np.int64)
    bad = (got >= n).any(axis=1)
    assert not bad.any(), where(bad) + ": an index is no photon's"
    s = np.sort(got, axis=1)
    bad = (s[:, 1:] == s[:, :-1]).any(axis=1)
    assert not bad.any(), where(bad) + ": a photon is returned twice"
    bad = (_bits(d2_all[np.arange(nq)[:, None], got]) != _bits(d2[:, :c])).any(axis=1)
    assert not bad.any(), where(bad) + ": an index names a photon at another distance"
    bad = ((d2[:, 1:c] == d2[:, :c - 1]) & (got[:, 1:] <= got[:, :-1])).any(axis=1)
    assert not bad.any(), where(bad) + ": equal distances are not in ascending index order"


def assert_same_answers(a, b, tied, what=""):
    """Two forms on the same (map, queries, k): the same counts and distances, and the same indices wherever the k-th distance is not tied
    across the cut (there the k-set is unique, and both order it by (distance, index))."""
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]), err_msg=what)
    np.testing.assert_array_equal(np.asarray(a[1])[~tied], np.asarray(b[1])[~tied], err_msg=what)


def same_choice_among_ties(a, b, tied):
    """-> how many of the queries whose k-th distance IS tied across the cut got the same indices from both forms, and how many there are"""
    ia, ib = np.asarray(a[1])[tied], np.asarray(b[1])[tied]
    return int((ia == ib).all(axis=1).sum()), int(tied.sum())
