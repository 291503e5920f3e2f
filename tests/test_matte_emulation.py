"""ID mattes, CPU tier: csrc/mcrt_matte.hpp - the text the two kernels of csrc/mcrt_matte.hip run - on emulated wavefronts
(tests/emu/matte_emu.cpp, tests/emu/wave_emu.hpp) against the definition of include/mcrt.h ("ID mattes") restated HERE in numpy, compared
with ==: the feature is integer work and one exact FP64 division, there is no tolerance anywhere.

Synthetic keys: 70 pixels (no multiple of 64, of the 4 wavefronts of a workgroup or of a tile), spp in {1, 9, 64, 65, 81, 200} (one
sample; less than a wavefront; exactly one row of 64 samples; one more; a square; four rows, the last ragged), ranks in {2, 6, 16}, both forms.
Scene keys: the four scene images and 70 x 13 frames of test_aov_emulation at sqrtspp 1, 3 and 9, the hits the AOV emulation's, all
three key modes. test_gpu_matte.py imports the definition and the synthetic cases from here."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import test_aov_emulation as aov
from emu_build import build_emu

NO_KEY = 0xFFFFFFFF
PIXELS = 70
SPPS = (1, 9, 64, 65, 81, 200)
RANKS = (2, 6, 16)
FORM_TILE, FORM_MEMORY = 1, 2
SMALL_KEYS = 512  # the synthetic keys of synthetic_keys(spp, small=True) are below this: a code table can cover them
# the named pixels of synthetic_keys
P_MISSES, P_ONE_KEY, P_ALL_DISTINCT, P_FIRST_DECIDES, P_STRADDLE, P_EXTREME_KEYS, P_LAST_SAMPLE, P_RANDOM = range(8)
HASH_VECTORS = {"": 0, "hello": 0x248bfa47, "The quick brown fox jumps over the lazy dog": 0x2e4ff723, "material0": 0x66933a1b, "CryptoMaterial": 0xbe359d67}


def load_matte_emu():
    """Host build of the ranking (tests/emu/matte_emu.cpp = wave_emu.hpp + csrc/mcrt_matte.hpp), the way the other emulations are built."""
    L = C.CDLL(build_emu("matte_emu.cpp"))
    vp = C.c_void_p
    L.matte_emu_rank.argtypes = [C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_int, C.c_uint64]
    L.matte_emu_tile_pixels.argtypes = [C.c_uint32]
    L.matte_emu_tile_pixels.restype = C.c_uint32
    L.matte_emu_tile_lds_words.argtypes = [C.c_uint32]
    L.matte_emu_tile_lds_words.restype = C.c_uint32
    return L


@functools.lru_cache(maxsize=None)
def _emu():
    return load_matte_emu()


def _pkg():
    import importlib
    return importlib.import_module("monte-carlo-ray-tracer_amd")


# ------------------------------------------------------------------ the definition (include/mcrt.h "ID mattes"), in numpy
def rank_definition(keys, ranks, codes=None):
    """keys [S, P] uint32 (NO_KEY = none) -> dict id [P, ranks], coverage, distinct [P] and, with codes, layer [P, ranks, 2]."""
    keys = np.asarray(keys, dtype=np.uint32)
    n, pixels = keys.shape
    out = dict(id=np.full((pixels, ranks), NO_KEY, dtype=np.uint32), coverage=np.zeros((pixels, ranks)), distinct=np.zeros(pixels, dtype=np.uint32))
    if codes is not None:
        out["layer"] = np.zeros((pixels, ranks, 2))
    for p in range(pixels):
        col = keys[:, p]
        at = np.nonzero(col != NO_KEY)[0]
        k, first, c = np.unique(col[at], return_index=True, return_counts=True)
        f = at[first]                                    # f_k = min{i : key_i = k}
        order = np.lexsort((f, -c.astype(np.int64)))     # c descending, then f ascending
        out["distinct"][p] = len(k)
        for r, j in enumerate(order[:ranks]):
            out["id"][p, r] = k[j]
            out["coverage"][p, r] = float(c[j]) / float(n)
            if codes is not None:
                out["layer"][p, r] = (float(np.array([codes[k[j]]], dtype=np.uint32).view(np.float32)[0]), out["coverage"][p, r])
    return out


def murmur3_32(data):
    """MurmurHash3_x86_32 with seed 0, from its public description."""
    m = 0xFFFFFFFF
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & m
    h = 0
    for b in range(len(data) // 4):
        k = int.from_bytes(data[4 * b:4 * b + 4], "little")
        k = rotl(k * 0xcc9e2d51 & m, 15) * 0x1b873593 & m
        h = (rotl(h ^ k, 13) * 5 + 0xe6546b64) & m
    tail = data[len(data) // 4 * 4:]
    if tail:
        k = int.from_bytes(tail, "little")
        h ^= rotl(k * 0xcc9e2d51 & m, 15) * 0x1b873593 & m
    h ^= len(data)
    h ^= h >> 16
    h = h * 0x85ebca6b & m
    h ^= h >> 13
    h = h * 0xc2b2ae35 & m
    h ^= h >> 16
    return h


def code_definition(name):
    h = murmur3_32(name if isinstance(name, bytes) else name.encode("ascii"))
    return h ^ (1 << 23) if (h >> 23) & 255 in (0, 255) else h


@functools.lru_cache(maxsize=None)
def small_codes():
    return np.array([code_definition("key%d" % k) for k in range(SMALL_KEYS)], dtype=np.uint32)


# ------------------------------------------------------------------ synthetic keys
@functools.lru_cache(maxsize=None)
def synthetic_keys(spp, small=False):
    """[spp, PIXELS] uint32. The first pixels are the named cases (P_*), the others random: a few keys with misses, then ever more keys up
    to as many as samples. small: the same with 0xFFFFFFFE replaced by SMALL_KEYS - 1, every key then below SMALL_KEYS."""
    rng = np.random.RandomState(1000 + spp)
    k = np.full((spp, PIXELS), NO_KEY, dtype=np.uint32)
    k[:, P_ONE_KEY] = 7
    k[:, P_ALL_DISTINCT] = 100 + np.arange(spp)
    half = spp // 2                                      # 3 and 5 cover half samples each, 5 appears first; an odd last sample misses
    k[:2 * half, P_FIRST_DECIDES] = np.where(np.isin(np.arange(2 * half) % 4, (0, 3)), 5, 3)   # 5 3 3 5 5 3 3 5 ...
    if spp >= 65:                                        # 11 first at sample 63 (lane 63), 12 first at sample 64 (lane 0), equal counts
        k[63, P_STRADDLE], k[64, P_STRADDLE] = 11, 12
        rest = (spp - 65) // 2
        k[65:65 + 2 * rest, P_STRADDLE] = [12, 11] * rest
    else:
        k[:, P_STRADDLE] = np.where(np.arange(spp) % 3 == 0, 11, NO_KEY)
    k[:, P_EXTREME_KEYS] = np.where(np.arange(spp) % 3 == 1, 0, 0xFFFFFFFE)   # 0xFFFFFFFE first and more often (or as often), then 0
    k[spp - 1, P_LAST_SAMPLE] = 9                        # every other sample misses: the winner is the last sample's
    for p in range(P_RANDOM, PIXELS):
        alphabet = max(1, min(spp, [2, 3, 6, 7, 16, 17, 40, spp][(p - P_RANDOM) % 8]))
        col = 20 + rng.randint(0, alphabet, size=spp).astype(np.uint32)
        col[rng.rand(spp) < (0.0, 0.1, 0.5)[p % 3]] = NO_KEY
        k[:, p] = col
    if small:
        k = np.where(k == 0xFFFFFFFE, SMALL_KEYS - 1, k).astype(np.uint32)
        assert k[k != NO_KEY].max() < SMALL_KEYS
    k.setflags(write=False)
    return k


def emu_rank(keys, ranks, codes=None, form=FORM_TILE, chunk_pixels=0, surface_map=None):
    """The emulation's ranking of keys [S, P] -> dict like rank_definition's (arrays prefilled with a pattern: what is not written shows)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    n, pixels = keys.shape
    out = dict(id=np.empty((pixels, ranks), dtype=np.uint32), coverage=np.empty((pixels, ranks)), distinct=np.empty(pixels, dtype=np.uint32))
    if codes is not None:
        out["layer"] = np.empty((pixels, ranks, 2))
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
    bufs = _pkg().MatteBuffers()
    for name, a in out.items():
        a.view(np.uint8).fill(0xAB)
        setattr(bufs, name, a.ctypes.data)
    if surface_map is not None:
        surface_map = np.ascontiguousarray(surface_map, dtype=np.uint32)
    rc = _emu().matte_emu_rank(pixels, n, keys.ctypes.data, surface_map.ctypes.data if surface_map is not None else None, ranks,
                               codes.ctypes.data if codes is not None else None, C.byref(bufs), form, chunk_pixels)
    assert rc == 0, "matte_emu_rank: %d" % rc
    return out


def assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name)
        assert got[name].tobytes() == want[name].tobytes(), "%s: %s differs at pixels %s" % (
            what, name, np.nonzero((got[name].reshape(len(want[name]), -1) != want[name].reshape(len(want[name]), -1)).any(axis=1))[0][:8])


# ------------------------------------------------------------------ synthetic keys through the rank entry
def test_synthetic_input_holds_the_cases_it_is_here_for():
    for spp in SPPS:
        k = synthetic_keys(spp)
        d = rank_definition(k, 16)
        assert (k[:, P_MISSES] == NO_KEY).all() and d["distinct"][P_MISSES] == 0
        assert d["distinct"][P_ONE_KEY] == 1 and d["coverage"][P_ONE_KEY, 0] == 1.0
        assert d["distinct"][P_ALL_DISTINCT] == spp and (spp <= 16 or d["distinct"][P_ALL_DISTINCT] > 16)
        assert d["id"][P_LAST_SAMPLE, 0] == 9 and d["coverage"][P_LAST_SAMPLE, 0] == 1.0 / spp and (k[:spp - 1, P_LAST_SAMPLE] == NO_KEY).all()
        if spp >= 2:
            assert list(d["id"][P_FIRST_DECIDES, :2]) == [5, 3] and d["coverage"][P_FIRST_DECIDES, 0] == d["coverage"][P_FIRST_DECIDES, 1]
            assert set(np.unique(k[:, P_EXTREME_KEYS])) == {0, 0xFFFFFFFE} and d["id"][P_EXTREME_KEYS, 0] == 0xFFFFFFFE and d["id"][P_EXTREME_KEYS, 1] == 0
        if spp >= 65:
            col = k[:, P_STRADDLE]
            assert np.nonzero(col == 11)[0][0] == 63 and np.nonzero(col == 12)[0][0] == 64 and (col == 11).sum() == (col == 12).sum()
            assert list(d["id"][P_STRADDLE, :2]) == [11, 12]
        rand = d["distinct"][P_RANDOM:]
        assert (rand > 16).any() == (spp > 16) and (rand <= 2).any()
        assert synthetic_keys(spp, small=True)[synthetic_keys(spp, small=True) != NO_KEY].max() < SMALL_KEYS
    assert PIXELS % 64 and PIXELS % 4 and all(PIXELS % _emu().matte_emu_tile_pixels(s) for s in SPPS if _emu().matte_emu_tile_pixels(s) > 1)


@pytest.mark.parametrize("form", [FORM_TILE, FORM_MEMORY])
@pytest.mark.parametrize("ranks", RANKS)
@pytest.mark.parametrize("spp", SPPS)
def test_emulated_ranking_of_synthetic_keys_equals_the_definition(spp, ranks, form):
    assert_same(emu_rank(synthetic_keys(spp), ranks, form=form), rank_definition(synthetic_keys(spp), ranks), "spp %d ranks %d form %d" % (spp, ranks, form))
    small = synthetic_keys(spp, small=True)
    assert_same(emu_rank(small, ranks, codes=small_codes(), form=form), rank_definition(small, ranks, small_codes()), "small keys with codes")


def test_tile_sizes_and_the_spp_where_the_forms_change():
    """A tile's keys and the four wavefronts' count arrays fit 64 KiB; past 2048 samples per pixel the tile form does not run. One pixel at
    2048 and at 2049 samples (the memory form's only), every sample a key of its own but two: exact whatever the number of distinct keys."""
    L = _emu()
    for spp, tile in ((1, 16), (256, 16), (819, 16), (820, 12), (1024, 12), (1025, 8), (1365, 8), (1366, 4), (2048, 4), (2049, 0), (100000, 0)):
        assert L.matte_emu_tile_pixels(spp) == tile, spp
        assert L.matte_emu_tile_lds_words(spp) * 4 <= 65536 and L.matte_emu_tile_lds_words(spp) == (tile + 4) * spp * (tile > 0)
    for spp, forms in ((2048, (FORM_TILE, FORM_MEMORY)), (2049, (FORM_MEMORY,))):
        keys = (1000 + np.arange(spp, dtype=np.uint32)).reshape(spp, 1).repeat(5, axis=1)
        keys[spp - 1], keys[spp - 2] = 1000 + 77, 1000 + 300          # two keys twice each: ranks 0 and 1 by first appearance, then the first sample's
        want = rank_definition(keys, 6)
        assert list(want["id"][0, :3]) == [1077, 1300, 1000] and want["distinct"][0] == spp - 2
        for form in forms:
            assert_same(emu_rank(keys, 6, form=form), want, "spp %d form %d" % (spp, form))


# ------------------------------------------------------------------ scene keys
KEY_MODES = ("material", "surface", "custom")
CUSTOM_KEYS = 5


def surface_map(scene, key):
    """surface -> key of the three modes (None: the identity) and the number of keys."""
    material = aov.scene_arrays(scene)["material"]
    if key == "material":
        return material, int(aov._image(scene).scene.num_materials)
    if key == "surface":
        return None, len(material)
    return (np.arange(len(material), dtype=np.uint32) * 7 % CUSTOM_KEYS).astype(np.uint32), CUSTOM_KEYS


def keys_of(surf, smap):
    """Per-sample surfaces [P, S] -> keys [S, P] by the definition: key_i = map[s_i], a miss has none."""
    s = np.ascontiguousarray(surf.T)
    if smap is None:
        return s
    return np.where(s == NO_KEY, NO_KEY, smap[np.where(s == NO_KEY, 0, s)]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def scene_frame(scene, sqrtspp):
    """The AOV emulation's frame and per-sample surfaces [P, S] of a 70 x 13 frame."""
    frame, _, surf, _ = aov.emu_frame(scene, sqrtspp)
    return frame, surf


@pytest.mark.parametrize("sqrtspp", [1, 3, 9])
@pytest.mark.parametrize("scene", list(aov.SCENES))
def test_emulated_ranking_of_scene_keys_equals_the_definition(scene, sqrtspp):
    frame, surf = scene_frame(scene, sqrtspp)
    n = sqrtspp * sqrtspp
    hits = (surf != NO_KEY).sum(axis=1)
    for key in KEY_MODES:
        smap, num_keys = surface_map(scene, key)
        codes = np.array([code_definition(_pkg().MATTE_DEFAULT_NAMES[key].replace("%u", "%d") % k) for k in range(num_keys)], dtype=np.uint32)
        want = rank_definition(keys_of(surf, smap), 6, codes)
        # the kernel maps as it loads: it is given the surfaces and the map
        got = emu_rank(np.ascontiguousarray(surf.T), 6, codes=codes, form=FORM_TILE, surface_map=smap)
        assert_same(got, want, "%s sqrtspp %d key %s" % (scene, sqrtspp, key))
        assert_same(emu_rank(np.ascontiguousarray(surf.T), 6, codes=codes, form=FORM_MEMORY, surface_map=smap), want, "memory form")
        # invariants: where no rank was cut off, the ranks' counts add up to the pixel's hits, and to the AOV pass's coverage
        counts = np.rint(got["coverage"] * n)
        assert (got["coverage"] == counts / float(n)).all()
        whole = got["distinct"] <= 6
        assert (counts.sum(axis=1)[whole] == hits[whole]).all() and (key != "material" or whole.any())
        assert (frame["coverage"][whole] == counts.sum(axis=1)[whole] / float(n)).all()
        assert (got["distinct"] == np.array([len(set(c[c != NO_KEY])) for c in keys_of(surf, smap).T])).all()
        if sqrtspp == 1 and key != "custom":
            assert (got["id"][:, 0] == frame[key]).all() and (got["id"][:, 1:] == NO_KEY).all()
    print("%s sqrtspp %d: up to %d distinct surfaces in a pixel" % (scene, sqrtspp, rank_definition(keys_of(surf, None), 2)["distinct"].max()))


def test_scene_frames_reach_cut_off_ranks_and_misses():
    surf = scene_frame("coffee_maker_qsah", 9)[1]
    assert rank_definition(keys_of(surf, None), 2)["distinct"].max() > 6   # more surfaces in a pixel than the scene tests' ranks (the synthetic keys pass 16)
    assert (scene_frame("quadric", 3)[1] == NO_KEY).any()


def test_emulated_ranking_does_not_depend_on_chunks_or_shards():
    """Chunks of 64 pixels (15 of them, the last ragged) and of one pixel; three shards of 5-row groups (the last group ragged)."""
    scene = "coffee_maker_qsah"
    surf = scene_frame(scene, 3)[1]
    smap, _ = surface_map(scene, "material")
    whole = emu_rank(np.ascontiguousarray(surf.T), 6, surface_map=smap)
    for chunk_pixels in (64, 1):
        for form in (FORM_TILE, FORM_MEMORY):
            assert_same(emu_rank(np.ascontiguousarray(surf.T), 6, surface_map=smap, chunk_pixels=chunk_pixels, form=form), whole, "chunks of %d" % chunk_pixels)
    seen = 0
    for index in range(3):
        rows = _pkg().shard_rows(aov.camera(scene, 3, (index, 3, 5)))
        part = emu_rank(np.ascontiguousarray(aov.emu_frame(scene, 3, shard=(index, 3, 5))[2].T), 6, surface_map=smap)
        for name in whole:
            full = whole[name].reshape((aov.HEIGHT, aov.WIDTH) + whole[name].shape[1:])
            assert full[rows].tobytes() == part[name].tobytes(), "shard %d: %s" % (index, name)
        seen += len(rows)
    assert seen == aov.HEIGHT


# ------------------------------------------------------------------ codes, manifest, refusals without a device
def test_matte_code_against_the_vectors_and_a_python_murmur(pkg):
    for text, h in HASH_VECTORS.items():
        assert murmur3_32(text.encode()) == h, text
        assert pkg.matte_code(text) == code_definition(text) == (h ^ (1 << 23) if (h >> 23) & 255 in (0, 255) else h), text
    assert pkg.matte_code("") == 0x00800000
    rng = np.random.RandomState(7)
    seen_fixed = 0
    for i in range(4000):
        name = bytes(rng.randint(0x20, 0x7f, size=rng.randint(0, 40)).astype(np.uint8))
        code = pkg.matte_code(name)
        assert code == code_definition(name), name
        assert (code >> 23) & 255 not in (0, 255)
        seen_fixed += code != murmur3_32(name)
    assert seen_fixed > 0   # (1 name in 128 has an exponent the rule changes)


def test_manifest_is_json_in_key_order(pkg):
    names = ["floor", 'say "hi"', "back\\slash", "a b,c:{d}", "x" * 255]
    text = pkg.matte_manifest("custom", names=names)
    parsed = json.loads(text)
    assert list(parsed) == names and all(parsed[n] == "%08x" % code_definition(n) for n in names)
    assert json.loads(pkg.matte_manifest("material", 3)) == {"material%d" % k: "%08x" % code_definition("material%d" % k) for k in range(3)}
    assert list(json.loads(pkg.matte_manifest("surface", 2))) == ["surface0", "surface1"] and pkg.matte_manifest("custom", 0) == "{}"
    assert list(json.loads(pkg.matte_manifest("custom", 2))) == ["key0", "key1"]
    # the size without a buffer, a buffer one byte short (not overrun), bad names
    L = pkg.lib()
    par = pkg.MatteParams()
    need = L.mcrt_matte_manifest(C.byref(par), 3, None, 0)
    buf = C.create_string_buffer(b"\xAB" * (need + 8), need + 8)
    assert L.mcrt_matte_manifest(C.byref(par), 3, buf, need - 1) == need and buf.raw[need - 1:] == b"\xAB" * 9
    assert L.mcrt_matte_manifest(None, 3, buf, need) == need and buf.value.decode() == pkg.matte_manifest("material", 3)
    for bad in (["ok", "tab\there"], ["ok", ""], ["x" * 256], ["caf\xe9"]):
        with pytest.raises(pkg.McrtError):
            pkg.matte_manifest("custom", names=bad)


def test_null_context_is_refused(pkg):
    L = pkg.lib()
    cam, bufs = pkg.CameraDesc(), pkg.MatteBuffers()
    assert L.mcrt_render_matte(None, C.byref(cam), 1, None, C.byref(bufs), None, None) == -1      # MCRT_ERR_INVALID
    assert L.mcrt_render_matte_device(None, C.byref(cam), 1, None, C.byref(bufs), None, None) == -1
    assert L.mcrt_matte_rank_device(None, 1, 1, None, 6, None, C.byref(bufs), None) == -1
    assert L.mcrt_abi_version() == 2
