"""OpenEXR input (mcrt_exr_open .. mcrt_exr_load*), CPU tier: csrc/mcrt_exr_read.hpp - the text the kernels of csrc/mcrt_exr_read.hip run -
driven on the host (tests/emu/exr_read_emu.cpp: the scan's three kernels on the emulated workgroup of tests/emu/wave_emu.hpp, the gather as
a loop over its lanes, all in the launches' geometry) together with csrc/mcrt_exr_read_file.hpp, against files of the Python WRITER that
tests/test_exr_emulation.py keeps, and of a second small writer here for the variants that one cannot produce.

Every comparison is assert_array_equal on bits or bytes; nothing is a tolerance. Expected values never come from the code under test:
they are file_values.astype(np.float64) - exact widening - for the patterns that are no NaN, and the header's NaN formula in numpy
integer operations."""
import ctypes as C
import functools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import test_exr_emulation as ex
from conftest import TESTS
from emu_build import build_emu

OK, ERR_INVALID, ERR_IO, ERR_UNSUPPORTED = 0, ex.ERR_INVALID, ex.ERR_IO, ex.ERR_UNSUPPORTED
NONE, ZIPS, ZIP = 0, 2, 3
UINT, HALF, FLOAT = ex.UINT, ex.HALF, ex.FLOAT
DEST_F64, DEST_U32 = 0, 1
SENTINEL_F64, SENTINEL_U32 = 0x7FF4DEADBEEF0001, 0xC0FFEE01


class Target(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dest_type", C.c_uint32), ("stride", C.c_uint32), ("offset", C.c_uint32), ("reserved", C.c_uint32)]


class LoadParams(C.Structure):
    _fields_ = [("threads", C.c_uint32), ("flags", C.c_uint32)]


class LoadResult(C.Structure):
    _fields_ = [("file_bytes", C.c_uint64), ("payload_bytes", C.c_uint64), ("chunks", C.c_uint32), ("raw_chunks", C.c_uint32)]


class Info(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("data_window", C.c_int32 * 4), ("display_window", C.c_int32 * 4), ("channels", C.c_uint32),
                ("attributes", C.c_uint32), ("compression", C.c_uint32), ("line_order", C.c_uint32), ("lines_per_chunk", C.c_uint32), ("chunks", C.c_uint32),
                ("file_bytes", C.c_uint64)]


def load_read_emu(libz=None):
    # (fp_contract=None: these builds have never carried -ffp-contract=off. -fno-gnu-unique: the two builds keep their own
    # "zlib loaded?" state in one process)
    L = C.CDLL(build_emu("exr_read_emu.cpp", "libexr_read_emu%s.so" % ("" if libz is None else "_nolibz"), fp_contract=None,
                         flags=["-pthread", "-fno-gnu-unique"] + ([] if libz is None else ['-DMCRT_EXR_LIBZ="%s"' % libz]), link=["-ldl"]))
    vp = C.c_void_p
    L.exr_read_half_emu.argtypes = [vp, C.c_uint64, vp]
    L.exr_read_half_emu.restype = None
    L.exr_read_float_emu.argtypes = [vp, C.c_uint64, vp]
    L.exr_read_float_emu.restype = None
    L.exr_read_tile_bytes_emu.restype = C.c_uint32
    L.exr_read_open_emu.argtypes = [C.c_char_p, C.POINTER(vp), C.c_char_p]
    L.exr_read_close_emu.argtypes = [vp]
    L.exr_read_close_emu.restype = None
    L.exr_read_info_emu.argtypes = [vp, C.POINTER(Info)]
    L.exr_read_info_emu.restype = None
    L.exr_read_channel_emu.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
    L.exr_read_channel_emu.restype = C.c_char_p
    L.exr_read_attribute_emu.argtypes = [vp, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(C.c_uint32)]
    L.exr_read_attribute_emu.restype = C.c_char_p
    L.exr_read_load_emu.argtypes = [vp, C.POINTER(Target), C.c_uint32, C.POINTER(LoadParams), C.POINTER(LoadResult), C.c_char_p]
    return L


@functools.lru_cache(maxsize=None)
def _emu():
    return load_read_emu()


# ---- the header's widening in numpy ----------------------------------------------------------------------------------------------------

def widen_half_bits(h):
    """uint16 patterns -> the binary64 bits of the header: astype is exact for every pattern that is no NaN; NaN by the formula."""
    h = np.asarray(h, dtype=np.uint16)
    with np.errstate(all="ignore"):
        exact = h.view(np.float16).astype(np.float64).view(np.uint64)
    f = (h & np.uint16(1023)).astype(np.uint64)
    nan = ((h & np.uint16(0x7c00)) == 0x7c00) & (f != 0)
    formula = ((h >> np.uint16(15)).astype(np.uint64) << np.uint64(63)) | np.uint64(0x7FF8000000000000) | (f << np.uint64(42))
    return np.where(nan, formula, exact)


def widen_float_bits(b):
    b = np.asarray(b, dtype=np.uint32)
    with np.errstate(all="ignore"):
        exact = b.view(np.float32).astype(np.float64).view(np.uint64)
    f = (b & np.uint32(0x7FFFFF)).astype(np.uint64)
    nan = ((b & np.uint32(0x7f800000)) == 0x7f800000) & (f != 0)
    formula = ((b >> np.uint32(31)).astype(np.uint64) << np.uint64(63)) | np.uint64(0x7FF8000000000000) | (f << np.uint64(29))
    return np.where(nan, formula, exact)


def widened(values, ptype):
    """A channel's file values [H,W] -> what a load gives: uint64 bits of the float64 frame, or the uint32 values."""
    if ptype == UINT:
        return np.ascontiguousarray(values).view(np.uint32)
    bits_ = np.ascontiguousarray(values).view(np.uint16 if ptype == HALF else np.uint32)
    return widen_half_bits(bits_) if ptype == HALF else widen_float_bits(bits_)


def test_the_numpy_side_widens_by_hand():
    """A few values of the header's table worked out here, so that the numpy side is not taken on trust either."""
    assert widen_half_bits([0x0001, 0x8200, 0x03ff, 0x3c00, 0x7bff, 0xfc00, 0x7e00, 0xfc01]).tolist() == [
        (999 + 0) << 52, (1 << 63) | (999 + 9) << 52, (999 + 9) << 52 | (0x1ff << (52 - 9)), 1023 << 52, (30 + 1008) << 52 | 1023 << 42,
        (1 << 63) | 0x7FF0000000000000, 0x7FF8000000000000 | 0x200 << 42, (1 << 63) | 0x7FF8000000000000 | 1 << 42]
    assert widen_float_bits([0x00000001, 0x00400001, 0x00800000, 0x7f800001, 0xffc00000]).tolist() == [
        874 << 52, (874 + 22) << 52 | 1 << (52 - 22), 897 << 52, 0x7FF8000000000000 | 1 << 29, (1 << 63) | 0x7FF8000000000000 | 0x400000 << 29]


# ---- a second writer: the variants ------------------------------------------------------------------------------------------------------

def _attr(name, typ, value):
    return name.encode("latin-1") + b"\0" + typ.encode("latin-1") + b"\0" + struct.pack("<i", len(value)) + value


def variant_file(width, height, file_chans, compression, origin=(0, 0), display=None, line_order=0, long_names=False, extra=(), physical=None, plinear=0,
                 version=None, sampling=(1, 1), zip_level=4, standard=True):
    """Single-part scan-line file -> (bytes, raw_chunks, header_bytes). origin: the data window's corner; physical: the order in which
    the chunks lie in the file (a permutation of their indices; the offset table always has entry k for the chunk of lines k * lines ..);
    extra: (name, type, bytes) attributes behind the standard ones."""
    x0, y0 = origin
    lines = 16 if compression == ZIP else 1
    chlist = b"".join(n.encode("latin-1") + b"\0" + struct.pack("<iB3xii", t, plinear, sampling[0], sampling[1]) for n, t, _ in file_chans) + b"\0"
    head = b"\x76\x2f\x31\x01" + struct.pack("<I", version if version is not None else (2 | (0x400 if long_names else 0)))
    head += _attr("channels", "chlist", chlist) + _attr("compression", "compression", bytes([compression]))
    head += _attr("dataWindow", "box2i", struct.pack("<4i", x0, y0, x0 + width - 1, y0 + height - 1))
    head += _attr("displayWindow", "box2i", struct.pack("<4i", *(display or (x0, y0, x0 + width - 1, y0 + height - 1))))
    head += _attr("lineOrder", "lineOrder", bytes([line_order]))
    if standard:
        head += _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
        head += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    for name, typ, value in extra:
        head += _attr(name, typ, value)
    head += b"\0"
    bodies, raws = [], 0
    for first in range(0, height, lines):
        raw = b"".join(v[y].tobytes() for y in range(first, min(first + lines, height)) for _, _, v in file_chans)
        data = raw
        if compression != NONE:
            data = zlib.compress(ex.zip_transform(raw), zip_level)
            if len(data) >= len(raw):
                data, raws = raw, raws + 1
        bodies.append(struct.pack("<ii", y0 + first, len(data)) + data)
    order = list(range(len(bodies))) if physical is None else list(physical)
    assert sorted(order) == list(range(len(bodies)))
    at, where = len(head) + 8 * len(bodies), {}
    for k in order:
        where[k] = at
        at += len(bodies[k])
    table = b"".join(struct.pack("<Q", where[k]) for k in range(len(bodies)))
    return head + table + b"".join(bodies[k] for k in order), raws, len(head)


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


# ---- the emulation --------------------------------------------------------------------------------------------------------------------

def view_target(name, a):
    """A Target of a [H,W] view: views of one buffer name that buffer, by stride and offset (as ex.c_channels does for a save)."""
    item = a.dtype.itemsize
    root = a
    while isinstance(root.base, np.ndarray):
        root = root.base
    step = (a.strides[1] if a.shape[1] > 1 else (a.strides[0] if a.shape[0] > 1 else item)) // item
    offset = ((a.ctypes.data - root.ctypes.data) // item) % step
    return Target(name.encode("latin-1") if isinstance(name, str) else name, a.ctypes.data - offset * item, DEST_U32 if a.dtype == np.uint32 else DEST_F64, step, offset, 0)


class Opened:
    def __init__(self, path, emu=None):
        self.emu = emu or _emu()
        self.h = C.c_void_p()
        msg = C.create_string_buffer(512)
        self.rc = self.emu.exr_read_open_emu(path.encode(), C.byref(self.h), msg)
        self.message = msg.value.decode("latin-1")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.h:
            self.emu.exr_read_close_emu(self.h)

    def info(self):
        i = Info()
        self.emu.exr_read_info_emu(self.h, C.byref(i))
        return i

    def channels(self):
        out = []
        for i in range(self.info().channels):
            t = C.c_uint32()
            out.append((self.emu.exr_read_channel_emu(self.h, i, C.byref(t)).decode("latin-1"), t.value))
        return out

    def attributes(self):
        out = []
        for i in range(self.info().attributes):
            typ, value, size = C.c_char_p(), C.c_void_p(), C.c_uint32()
            name = self.emu.exr_read_attribute_emu(self.h, i, C.byref(typ), C.byref(value), C.byref(size))
            out.append((name.decode("latin-1"), typ.value.decode("latin-1"), C.string_at(value.value, size.value) if size.value else b""))
        return out

    def load(self, targets, threads=0, count=None, flags=0, params=True):
        arr = (Target * max(len(targets), 1))(*targets) if targets is not None else None
        res, msg = LoadResult(), C.create_string_buffer(512)
        par = LoadParams(threads, flags)
        rc = self.emu.exr_read_load_emu(self.h, arr, len(targets) if count is None else count, C.byref(par) if params else None, C.byref(res), msg)
        return rc, res, msg.value.decode("latin-1")


def load_all(path, names=None, threads=0, emu=None):
    """Every channel (or `names`, in that order) into arrays of its own -> (dict name -> array, result, info, attributes)."""
    with Opened(path, emu) as f:
        assert f.rc == OK, (f.rc, f.message)
        info = f.info()
        types = dict(f.channels())
        wanted = [n for n, _ in f.channels()] if names is None else list(names)
        out = {n: np.full((info.height, info.width), SENTINEL_U32 if types[n] == UINT else 0, dtype=np.uint32 if types[n] == UINT else np.float64) for n in wanted}
        rc, res, msg = f.load([view_target(n, a) for n, a in out.items()], threads=threads)
        assert rc == OK, (rc, msg)
        return out, res, info, f.attributes()


def try_file(path, emu=None):
    """-> (status, message) of opening the file and loading all its channels."""
    with Opened(path, emu) as f:
        if f.rc != OK:
            assert not f.h
            return f.rc, f.message
        info, chans = f.info(), f.channels()
        out = [np.zeros((info.height, info.width), dtype=np.uint32 if t == UINT else np.float64) for _, t in chans]
        rc, _, msg = f.load([view_target(n, a) for (n, _), a in zip(chans, out)])
        return rc, msg


def assert_channels(got, file_chans):
    for n, t, v in file_chans:
        if n in got:
            np.testing.assert_array_equal(got[n].view(np.uint32 if t == UINT else np.uint64), widened(v, t), err_msg=n)


# ---- tests: the conversions -------------------------------------------------------------------------------------------------------------

def test_all_half_patterns_widen_to_the_definition_and_round_back():
    h = np.arange(1 << 16, dtype=np.uint16)
    got = np.empty(h.size, dtype=np.uint64)
    _emu().exr_read_half_emu(h.ctypes.data, h.size, got.ctypes.data)
    np.testing.assert_array_equal(got, widen_half_bits(h))
    nan = ((h & 0x7c00) == 0x7c00) & ((h & 1023) != 0)
    assert nan.sum() == 2046 and got[0x7c01] == 0x7FF8000000000000 | 1 << 42 and got[0x0001] == 999 << 52 and got[0x8000] == 1 << 63
    for keep_inf in (0, 1):  # the save's rounding gives every pattern that is no NaN back, and the NaN it writes itself
        back = np.empty(h.size, dtype=np.uint16)
        ex._emu().exr_half_emu(got.ctypes.data, got.size, keep_inf, back.ctypes.data)
        same = ~nan | (h == 0x7e00) | (h == 0xfe00)
        if not keep_inf:  # (without MCRT_EXR_HALF_INF only a FINITE input saturates: Inf stays Inf)
            assert back[0x7c00] == 0x7c00 and back[0xfc00] == 0xfc00
        np.testing.assert_array_equal(back[same], h[same])
        np.testing.assert_array_equal(back[nan], np.where(h[nan] & 0x8000, 0xfe00, 0x7e00).astype(np.uint16))


def test_float_widening_and_the_round_trip_back():
    with np.errstate(all="ignore"):
        listed = ex.conversion_list().astype(np.float32).view(np.uint32)
    edges = np.array([s | e << 23 | f for s in (0, 0x80000000) for e in (0, 1) for f in (0, 1, 0x7fffff)], dtype=np.uint32)
    subnormals = np.array([1 << k for k in range(23)] + [(1 << k) | 1 for k in range(1, 23)], dtype=np.uint32)
    rand = np.random.default_rng(99).integers(0, 1 << 32, size=100000, dtype=np.uint32)
    nans = np.array([0x7f800001, 0xff800001, 0x7fc00000, 0xffc12345, 0x7fbfffff, 0x7fffffff], dtype=np.uint32)
    b = np.concatenate([listed, edges, subnormals, rand, nans])
    got = np.empty(b.size, dtype=np.uint64)
    _emu().exr_read_float_emu(b.ctypes.data, b.size, got.ctypes.data)
    np.testing.assert_array_equal(got, widen_float_bits(b))
    back = np.empty(b.size, dtype=np.uint32)
    ex._emu().exr_float_emu(got.ctypes.data, got.size, back.ctypes.data)
    nan = ((b & 0x7f800000) == 0x7f800000) & ((b & 0x7fffff) != 0)
    quiet = nan & ((b & 0x400000) != 0)
    assert nan.sum() > 100 and quiet.sum() > 50 and (nan & ~quiet).sum() > 50 and ((b & 0x7f800000) == 0).sum() > 300
    np.testing.assert_array_equal(back[~nan | quiet], b[~nan | quiet])
    np.testing.assert_array_equal(back[nan & ~quiet], b[nan & ~quiet] | np.uint32(0x400000))  # (a signalling NaN comes back quiet, payload kept)


# ---- tests: whole files -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("compression", [NONE, ZIP], ids=["none", "zip"])
@pytest.mark.parametrize("which", ex.CHANNEL_SETS)
@pytest.mark.parametrize("height", ex.HEIGHTS)
@pytest.mark.parametrize("width", ex.WIDTHS)
def test_files_of_the_python_writer_load_bit_for_bit(tmp_path, width, height, which, compression):
    file_chans = ex.sorted_file_channels(ex.channel_set(which, width, height))
    data, raws = ex.py_exr_file(width, height, file_chans, compression, ex.ATTRIBUTES)
    path = write(tmp_path, "f.exr", data)
    got, res, info, attrs = load_all(path, threads=3)
    assert list(got) == [n for n, _, _ in file_chans]
    assert_channels(got, file_chans)
    lines = 16 if compression == ZIP else 1
    line_bytes = width * sum(ex.FILE_DTYPES[t].itemsize for _, t, _ in file_chans)
    assert (res.chunks, res.raw_chunks) == ((height + lines - 1) // lines, raws if compression == ZIP else height)
    assert res.payload_bytes == height * line_bytes and res.file_bytes == len(data)
    assert (info.width, info.height, info.compression, info.line_order, info.lines_per_chunk, info.chunks) == (width, height, compression, 0, lines, res.chunks)
    assert list(info.data_window) == list(info.display_window) == [0, 0, width - 1, height - 1]
    assert [(n, t, v) for n, t, v in attrs[8:]] == [(k, "string", v.encode()) for k, v in ex.ATTRIBUTES] and attrs[1] == ("compression", "compression", bytes([compression]))


def test_strided_destinations_keep_their_sentinels(tmp_path):
    """R, G, B into one [H,W,3]; the twelve tops channels into [H,W,4,3] of which the file holds... all twelve, so the sentinel sits in a
    wider [H,W,5,3] whose plane 4 no target names, and in a [H,W,4] of which only B's slot 2 is written."""
    w, h = 65, 17
    file_chans = ex.sorted_file_channels(ex.channel_set("strided_15", w, h))
    by = {n: (t, v) for n, t, v in file_chans}
    for compression in (NONE, ZIP):
        path = write(tmp_path, "s%d.exr" % compression, ex.py_exr_file(w, h, file_chans, compression)[0])
        rgb = np.full((h, w, 3), SENTINEL_F64, dtype=np.uint64).view(np.float64)
        tops = np.full((h, w, 5, 3), SENTINEL_F64, dtype=np.uint64).view(np.float64)
        lone = np.full((h, w, 4), SENTINEL_F64, dtype=np.uint64).view(np.float64)
        targets = [view_target("RGB"[c], rgb[..., c]) for c in (0, 1)] + [view_target("tops%d.%s" % (k, "RGB"[c]), tops[:, :, k, c]) for k in range(4) for c in range(3)]
        targets.append(view_target("B", lone[..., 2]))
        assert [(t.stride, t.offset) for t in targets[:3]] == [(3, 0), (3, 1), (15, 0)] and (targets[-1].stride, targets[-1].offset) == (4, 2)
        with Opened(path) as f:
            rc, res, msg = f.load(targets)
        assert rc == OK, msg
        for c in (0, 1):
            np.testing.assert_array_equal(rgb[..., c].view(np.uint64), widened(by["RGB"[c]][1], by["RGB"[c]][0]))
        assert (rgb[..., 2].view(np.uint64) == SENTINEL_F64).all()
        for k in range(4):
            for c in range(3):
                n = "tops%d.%s" % (k, "RGB"[c])
                np.testing.assert_array_equal(tops[:, :, k, c].view(np.uint64), widened(by[n][1], by[n][0]), err_msg=n)
        assert (tops[:, :, 4, :].view(np.uint64) == SENTINEL_F64).all()
        np.testing.assert_array_equal(lone[..., 2].view(np.uint64), widened(by["B"][1], by["B"][0]))
        assert (lone[..., [0, 1, 3]].view(np.uint64) == SENTINEL_F64).all()


def test_a_subset_in_another_order(tmp_path):
    w, h = 63, 33
    file_chans = ex.sorted_file_channels(ex.channel_set("mixed_unsorted", w, h))
    for compression in (NONE, ZIP):
        path = write(tmp_path, "m%d.exr" % compression, ex.py_exr_file(w, h, file_chans, compression)[0])
        got, res, _, _ = load_all(path, names=["surface.id", "B", "R"])
        assert list(got) == ["surface.id", "B", "R"] and got["surface.id"].dtype == np.uint32
        assert_channels(got, file_chans)
        assert res.payload_bytes == h * w * (4 + 2 + 4 + 2 + 4)   # (the channels not asked for ride along)


def smooth(shape, dtype=np.float64):
    n = int(np.prod(shape))
    return (np.arange(n, dtype=np.float64) / 1024.0).astype(dtype).reshape(shape)


def boundary_cases(tile):
    """-> [(label, file bytes, file channels, chunks, raw_chunks)]: chunks cut by the scan's tile of `tile` bytes - past two tiles and no
    multiple; exactly a tile and a byte pair, as one chunk and as ZIPS chunks, the later ones of which start off the payload buffer's
    words; more tiles than one trip of the chunk's scan takes; and a raw chunk between two transformed ones."""
    assert tile % 512 == 0
    out = []
    w = tile // 16 + 1                     # 16 lines of w HALF values: two tiles and 32 bytes
    chans = [("Y", HALF, ex.numpy_file_values(smooth((16, w)), HALF))]
    data, raws, _ = variant_file(w, 16, chans, ZIP)
    assert raws == 0 and 16 * w * 2 > 2 * tile and (16 * w * 2) % tile != 0
    out.append(("two_tiles_and_more", data, chans, 1, 0))
    w = (tile + 2) // 2                    # one line of it: a tile and a byte pair
    for compression, h in ((ZIP, 1), (ZIPS, 3)):
        chans = [("Y", HALF, ex.numpy_file_values(smooth((h, w)), HALF))]
        data, raws, _ = variant_file(w, h, chans, compression)
        assert raws == 0 and w * 2 == tile + 2
        out.append(("tile_and_a_pair_%d" % compression, data, chans, h, 0))
    w = (256 * tile) // 4 + 1025           # one line of w FLOAT values: more than 256 tiles
    chans = [("Z", FLOAT, ex.numpy_file_values(smooth((2, w)), FLOAT))]
    data, raws, _ = variant_file(w, 2, chans, ZIPS, zip_level=1)
    assert raws == 0 and w * 4 > 257 * tile
    out.append(("two_trips_of_tiles", data, chans, 2, 0))
    ids = np.zeros((48, 64), dtype=np.uint32) + np.arange(64, dtype=np.uint32)
    ids[16:32] = np.random.default_rng(11).integers(0, 1 << 32, size=(16, 64), dtype=np.uint32)
    chans = [("id", UINT, ids)]
    data, raws = ex.py_exr_file(64, 48, chans, 3)
    assert raws == 1
    out.append(("raw_between", data, chans, 3, 1))
    return out


def test_scan_boundaries(tmp_path):
    """The tile's size comes from the launch header through the emulation."""
    for label, data, chans, chunks, raws in boundary_cases(_emu().exr_read_tile_bytes_emu()):
        got, res, _, _ = load_all(write(tmp_path, label + ".exr", data))
        assert_channels(got, chans)
        assert (res.chunks, res.raw_chunks) == (chunks, raws), label


EXTRA = (("exposure", "float", struct.pack("<f", 1.5)), ("offset", "v2f", struct.pack("<2f", 0.25, -2.0)),
         ("chromaticities", "chromaticities", struct.pack("<8f", 0.64, 0.33, 0.3, 0.6, 0.15, 0.06, 0.3127, 0.329)),
         ("made.up", "a type nobody knows", b"\x00\x01\xfe\xff\x00"), ("empty", "another", b""), ("mcrt:spp", "string", b"16"))


VARIANTS = ["window", "decreasing", "shuffled", "zips", "long_names", "plinear", "attributes", "random_order"]
LONG_NAME = "a.channel.name.of.forty.bytes.in.all.xyz"


def variant_case(variant, w=65, h=40):
    """-> (file bytes, file channels, compression, raw_chunks, the writer's keywords)."""
    file_chans = ex.sorted_file_channels(ex.channel_set("mixed_unsorted", w, h))
    kw, compression = {}, ZIP
    if variant == "window":
        kw = dict(origin=(-7, 5), display=(0, 0, 1919, 1079))
    elif variant == "decreasing":
        kw = dict(line_order=1, physical=[2, 1, 0], origin=(0, 3))
    elif variant == "shuffled":
        kw = dict(physical=[1, 2, 0])
    elif variant == "zips":
        compression = ZIPS
    elif variant == "long_names":
        assert len(LONG_NAME) == 40
        file_chans = sorted(file_chans + [(LONG_NAME, FLOAT, file_chans[0][2].astype(np.float32))], key=lambda c: c[0].encode())
        kw = dict(long_names=True)
    elif variant == "plinear":
        kw = dict(plinear=1)
    elif variant == "attributes":
        kw = dict(extra=EXTRA)
    elif variant == "random_order":
        compression, kw = NONE, dict(line_order=2, physical=[int(k) for k in np.random.default_rng(3).permutation(h)])
    data, raws, _ = variant_file(w, h, file_chans, compression, **kw)
    return data, file_chans, compression, raws, kw


@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_files(tmp_path, variant):
    w, h = 65, 40
    data, file_chans, compression, raws, kw = variant_case(variant, w, h)
    got, res, info, attrs = load_all(write(tmp_path, variant + ".exr", data), threads=2)
    assert list(got) == [n for n, _, _ in file_chans]
    assert_channels(got, file_chans)
    lines = 16 if compression == ZIP else 1
    assert (res.chunks, res.raw_chunks) == ((h + lines - 1) // lines, raws if compression != NONE else h)
    assert (info.width, info.height, info.compression, info.line_order) == (w, h, compression, kw.get("line_order", 0))
    x0, y0 = kw.get("origin", (0, 0))
    assert list(info.data_window) == [x0, y0, x0 + w - 1, y0 + h - 1]
    assert list(info.display_window) == list(kw.get("display", info.data_window))
    assert [a[0] for a in attrs[:8]] == ["channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter", "screenWindowWidth"]
    assert attrs[8:] == list(kw.get("extra", ()))
    assert attrs[5] == ("pixelAspectRatio", "float", struct.pack("<f", 1.0)) and attrs[2][1:] == ("box2i", struct.pack("<4i", x0, y0, x0 + w - 1, y0 + h - 1))


@functools.lru_cache(maxsize=None)
def small_chans():
    """9 x 18, the five channels of the mixed set (16 bytes a pixel) with smooth values: both ZIP chunks deflate."""
    w, h = 9, 18
    ramp = np.arange(h * w, dtype=np.float64).reshape(h, w)
    chans = [("surface.id", (ramp // 7).astype(np.uint32), UINT), ("R", ramp / 64.0, HALF), ("depth.Z", 3.0 + ramp / 8.0, FLOAT), ("B", -ramp, FLOAT), ("G", ramp / 16.0, HALF)]
    return ex.sorted_file_channels(chans)


def small_file(compression=ZIP, **kw):
    return variant_file(9, 18, small_chans(), compression, **kw)


def test_unsupported_files_name_their_cause(tmp_path):
    cases = [(dict(version=2 | bit), word) for bit, word in ((0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part"))]
    cases += [(dict(version=1), "version"), (dict(version=3), "version"), (dict(version=2 | 0x2000), "version")]
    cases += [(dict(sampling=(2, 1)), "subsampled"), (dict(sampling=(1, 2)), "subsampled")]
    for kw, word in cases:
        rc, msg = try_file(write(tmp_path, "u.exr", small_file(**kw)[0]))
        assert rc == ERR_UNSUPPORTED and word in msg, (kw, rc, msg)
    for number in (1, 4, 5, 6, 7, 8, 9):
        data, _, _ = small_file(NONE)
        at = data.index(b"compression\0compression\0") + 24 + 4
        assert data[at] == 0
        rc, msg = try_file(write(tmp_path, "c.exr", data[:at] + bytes([number]) + data[at + 1:]))
        assert rc == ERR_UNSUPPORTED and "compression %d" % number in msg, (number, rc, msg)


def test_without_libz_uncompressed_files_and_raw_chunks_still_load(tmp_path):
    nolibz = load_read_emu(libz="libz-that-is-not-there.so.1")
    w, h = 65, 17
    file_chans = ex.sorted_file_channels(ex.channel_set("mixed_unsorted", w, h))
    got, _, _, _ = load_all(write(tmp_path, "none.exr", ex.py_exr_file(w, h, file_chans, 0)[0]), emu=nolibz)
    assert_channels(got, file_chans)
    noise = np.random.default_rng(5).integers(0, 1 << 32, size=(32, 64), dtype=np.uint32)
    data, raws = ex.py_exr_file(64, 32, [("noise", UINT, noise)], 3)
    assert raws == 2
    got, res, _, _ = load_all(write(tmp_path, "raw.exr", data), emu=nolibz)
    assert_channels(got, [("noise", UINT, noise)])
    assert res.raw_chunks == 2
    path = write(tmp_path, "zip.exr", ex.py_exr_file(w, h, file_chans, 3)[0])
    rc, msg = try_file(path, emu=nolibz)
    assert rc == ERR_UNSUPPORTED and "libz-that-is-not-there.so.1" in msg
    assert try_file(path)[0] == OK   # (the build that finds libz loads it, in the same process)


def _patch(data, at, new):
    return data[:at] + new + data[at + len(new):]


def test_malformed_files_are_io_errors(tmp_path):
    """One file per cause of the header's MCRT_ERR_IO list."""
    w, h = 9, 18
    file_chans = small_chans()
    good, raws, head = small_file()
    assert raws == 0 and try_file(write(tmp_path, "good.exr", good))[0] == OK
    none, _, none_head = small_file(NONE)
    table = lambda d, hb, k: struct.unpack_from("<Q", d, hb + 8 * k)[0]
    ch_at = good.index(b"channels\0chlist\0") + 16      # the channel list's size
    ch_size = struct.unpack_from("<i", good, ch_at)[0]
    dw_at = good.index(b"dataWindow\0box2i\0") + 17     # its size, then the box
    first = table(good, head, 0)
    size0 = struct.unpack_from("<i", good, first + 4)[0]
    cases = {
        "magic": _patch(good, 0, b"\x76\x2f\x31\x02"),
        "header cut in a name": good[:12],
        "header cut in a value": good[:ch_at + 4 + 10],
        "header without its end": good[:head - 1],
        "channel list cut short": _patch(good, ch_at, struct.pack("<i", ch_size - 5)),
        "channel list longer than it says": _patch(good, ch_at + 4 + ch_size - 1, b"\x01"),
        "attribute not ending where its size says": _patch(good, dw_at, struct.pack("<i", 12)),
        "negative attribute size": _patch(good, ch_at, struct.pack("<i", -8)),
        "oversized attribute size": _patch(good, ch_at, struct.pack("<i", 0x7fffffff)),
        "wrong type": good.replace(b"dataWindow\0box2i\0", b"dataWindow\0box2f\0"),
        "wrong size": _patch(good, good.index(b"lineOrder\0lineOrder\0") + 20, struct.pack("<i", 2)),
        "line order 3": _patch(good, good.index(b"lineOrder\0lineOrder\0") + 24, b"\x03"),
        "unknown pixel type": _patch(good, ch_at + 4 + 2, struct.pack("<i", 3)),
        "empty data window": _patch(good, dw_at + 4, struct.pack("<4i", 5, 0, 4, 17)),
        "offset table cut short": good[:head + 8],
        "offset outside the file": _patch(good, head + 8, struct.pack("<Q", len(good) + 100)),
        "offset into the header": _patch(good, head, struct.pack("<Q", 8)),
        "offset 2^63": _patch(good, head, struct.pack("<Q", 1 << 63)),
        "chunk with another y": _patch(good, first, struct.pack("<i", 16)),
        "chunks swapped in the table": _patch(good, head, good[head + 8:head + 16] + good[head:head + 8]),
        "negative chunk size": _patch(good, first + 4, struct.pack("<i", -1)),
        "chunk larger than raw": _patch(good, first + 4, struct.pack("<i", 16 * w * 16 + 1)),
        "chunk past the end": good[:len(good) - 1],
        "chunk that inflates to less": None,
        "chunk that inflates to more": None,
        "chunk that is no deflate stream": _patch(good, first + 8, b"\xff" * 8),
        "chunk too small to inflate to its size": _patch(good, first + 4, struct.pack("<i", 1)),
        "uncompressed chunk of another size": _patch(none, table(none, none_head, 3) + 4, struct.pack("<i", 10)),
    }
    for name in ("channels", "compression", "dataWindow", "displayWindow", "lineOrder"):
        at = good.index(name.encode() + b"\0")
        cases["no " + name] = _patch(good, at, b"x")
    # a chunk whose stream is sound but holds 2 bytes less / more than its lines do: the same file with another height claims so
    line_bytes = w * 16
    for word, lines in (("less", 15), ("more", 17)):
        raw = b"".join(v[y].tobytes() for y in range(lines) for _, _, v in file_chans)
        stream = zlib.compress(ex.zip_transform(raw), 4)
        body = good[:first + 4] + struct.pack("<i", len(stream)) + stream
        shift = len(stream) - size0
        body += good[first + 8 + size0:]
        body = _patch(body, head + 8, struct.pack("<Q", table(good, head, 1) + shift))
        assert len(stream) < 16 * line_bytes
        cases["chunk that inflates to " + word] = body
    # 65 537 channels (a header of its own: 1 x 1 pixels)
    many = [("c%05d" % i, UINT, np.zeros((1, 1), dtype=np.uint32)) for i in range(65537)]
    cases["too many channels"] = variant_file(1, 1, many, NONE)[0]
    with Opened(write(tmp_path, "many_ok.exr", variant_file(1, 1, many[:65536], NONE)[0])) as f:   # (65 536 open, and any of them loads)
        one = np.ones((1, 1), dtype=np.uint32)
        assert f.rc == OK and f.info().channels == 65536 and f.load([view_target("c65535", one)])[0] == OK and one[0, 0] == 0
    twice = [("a", HALF, np.zeros((2, 2), dtype=np.float16)), ("a", HALF, np.zeros((2, 2), dtype=np.float16))]
    cases["a channel name twice"] = variant_file(2, 2, twice, NONE)[0]
    cases["no channel"] = variant_file(2, 2, [], NONE)[0]
    for name, data in cases.items():
        assert data is not None, name
        rc, msg = try_file(write(tmp_path, "bad.exr", data))
        assert rc == ERR_IO and msg, (name, rc, msg)
    rc, msg = try_file(str(tmp_path / "not there.exr"))
    assert rc == ERR_IO and "not there.exr" in msg
    assert try_file(str(tmp_path))[0] == ERR_IO   # a directory
    assert try_file(write(tmp_path, "empty.exr", b""))[0] == ERR_IO


def test_what_a_load_refuses_as_invalid(tmp_path):
    w, h = 9, 18
    path = write(tmp_path, "good.exr", small_file()[0])
    f64 = lambda: np.zeros((h, w), dtype=np.float64)
    u32 = lambda: np.zeros((h, w), dtype=np.uint32)
    rgb = np.zeros((h, w, 3))
    with Opened(path) as f:
        assert f.rc == OK and dict(f.channels()) == {"B": FLOAT, "G": HALF, "R": HALF, "depth.Z": FLOAT, "surface.id": UINT}
        good = lambda: [view_target("R", rgb[..., 0]), view_target("surface.id", u32())]
        assert f.load(good())[0] == OK and f.load(good(), params=False)[0] == OK
        invalid = lambda targets, **kw: f.load(targets, **kw)
        assert invalid(None, count=1)[0] == ERR_INVALID                                        # NULL target array
        assert invalid(good(), count=0)[0] == ERR_INVALID
        assert invalid([view_target("R", f64())] * 1025)[0] == ERR_INVALID                     # more than MCRT_EXR_MAX_CHANNELS
        assert invalid(good(), flags=1)[0] == ERR_INVALID
        rc, _, msg = invalid([view_target("R", f64()), view_target("albedo.R", f64())])
        assert rc == ERR_INVALID and "albedo.R" in msg                                         # a name the file does not hold
        for field, value in (("name", None), ("data", None), ("stride", 0), ("offset", 3), ("offset", 7), ("reserved", 1)):
            t = good()
            setattr(t[0], field, value)
            assert invalid(t)[0] == ERR_INVALID, field
        assert invalid([view_target("R", u32())])[0] == ERR_INVALID                            # HALF -> U32
        assert invalid([view_target("B", u32())])[0] == ERR_INVALID                            # FLOAT -> U32
        assert invalid([view_target("surface.id", f64())])[0] == ERR_INVALID                   # UINT -> F64
        t = good()
        t[0].dest_type = 2
        assert invalid(t)[0] == ERR_INVALID
        one = f64()
        assert invalid([view_target("R", one), view_target("G", one)])[0] == ERR_INVALID       # two targets, one element
        assert invalid([view_target("R", rgb[..., 1]), view_target("G", rgb[..., 1])])[0] == ERR_INVALID
        assert invalid([view_target("R", rgb[..., 0]), view_target("G", rgb[:, :, 0:2][..., 0])])[0] == ERR_INVALID
        words = np.zeros((h, w, 2), dtype=np.uint32)                                           # a uint32 target inside a double's bytes
        assert invalid([view_target("R", words.view(np.float64)[..., 0]), view_target("surface.id", words[..., 1])])[0] == ERR_INVALID
        assert invalid([view_target("R", rgb[..., 0]), view_target("G", rgb[..., 1]), view_target("B", rgb[..., 2])])[0] == OK


def test_stand_alone_sanitizer_run(tmp_path):
    """tests/emu/exr_read_main.cpp, a program of its own, under AddressSanitizer and UndefinedBehaviorSanitizer: once, as a subprocess.
    Every truncation of two files, every byte of their headers and offset tables overwritten three ways, 2 000 byte flips in their chunks:
    the exit status is the number of loads that came back with anything but MCRT_OK, MCRT_ERR_IO or MCRT_ERR_UNSUPPORTED, or that took a
    truncated file for whole."""
    src = os.path.join(TESTS, "emu", "exr_read_main.cpp")
    exe = str(tmp_path / "exr_read_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-pthread", "-o", exe, src, "-ldl"])
    out = tmp_path / "files"
    out.mkdir()
    run = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = [l.split() for l in run.stdout.splitlines()]
    assert [l[0] for l in lines] == ["zip", "none"]
    for l in lines:
        fields = dict(zip(l[1::2], (int(v) for v in l[2::2])))
        assert fields["violations"] == 0 and fields["truncations"] == fields["bytes"] and fields["header_loads"] == 3 * fields["header_bytes"] and fields["flips"] == 2000
        assert fields["whole"] == 0 and fields["ok"] > 0 and fields["io"] > fields["bytes"], fields   # (the whole file loads; mutations are told apart)


def test_a_loaded_file_saves_as_the_same_bytes(tmp_path):
    """NONE file of the Python writer (no NaN payloads: the random patterns' NaNs are made the save's own) -> load -> save with the same
    types and attributes through the save emulation: the same bytes."""
    w, h = 65, 17
    chans = []
    for n, a, t in ex.channel_set("mixed_unsorted", w, h):
        chans.append((n, np.where(np.isnan(a), np.nan, a) if a.dtype == np.float64 else a, t))
    file_chans = ex.sorted_file_channels(chans)
    data, _ = ex.py_exr_file(w, h, file_chans, 0, ex.ATTRIBUTES)
    path = write(tmp_path, "first.exr", data)
    got, _, _, attrs = load_all(path)
    again = str(tmp_path / "again.exr")
    ex.emu_save(again, w, h, [(n, got[n], t) for n, t, _ in file_chans], ex.NONE, [(n, v.decode()) for n, _, v in attrs[8:]])
    assert open(again, "rb").read() == data
    assert any(np.isinf(v.astype(np.float64)).any() for _, t, v in file_chans if t == HALF)   # (an infinity that the file holds stays one)
