"""OpenEXR output (mcrt_exr_save*), CPU tier: csrc/mcrt_exr.hpp - the text the kernel of csrc/mcrt_exr.hip runs - driven on the host
(tests/emu/exr_emu.cpp: the kernel as a loop over its lanes in the launch's geometry) together with csrc/mcrt_exr_file.hpp, against the
text of include/mcrt.h ("OpenEXR output") written out HERE in numpy and struct.

Every comparison is assert_array_equal on bits or bytes; nothing is a tolerance. The numpy side does not see the code under test:
  conversions   astype(np.float16) / astype(np.float32) from float64 are single roundings to nearest even (test_numpy_rounds_once holds
                numpy to that: 1 + 2^-11 + 2^-30 -> 0x3c01); the saturation and the header's NaN patterns are np.where on top
  payloads      a chunk's raw bytes are tobytes() of the converted rows in sorted channel order, ZIP's transform two slices and a difference
  files         a writer of the layout (py_exr_file) kept here; ZIP files, whose deflate bytes depend on the zlib at hand, are read back
                by tools/exr_probe.py - which this module first holds to the Python writer's own ZIP files."""
import ctypes as C
import functools
import importlib.util
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, TESTS
from emu_build import build_emu

UINT, HALF, FLOAT = 0, 1, 2
SRC_F64, SRC_U32 = 0, 1
NONE, ZIP = 0x100 | 0, 0x100 | 3
HALF_INF = 1
ERR_INVALID, ERR_IO, ERR_UNSUPPORTED = -1, -6, -7
FILE_DTYPES = {UINT: np.dtype("<u4"), HALF: np.dtype("<f2"), FLOAT: np.dtype("<f4")}
WIDTHS = [1, 63, 64, 65, 257]   # a pixel, short of / at / past a wave of values, past a workgroup's
HEIGHTS = [1, 15, 16, 17, 33]   # a ZIP chunk short of, at and past 16 lines; two chunks and a last short one
CHANNEL_SETS = ("one_half", "mixed_unsorted", "strided_15")


class Channel(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("source_type", C.c_uint32), ("pixel_type", C.c_uint32), ("stride", C.c_uint32), ("offset", C.c_uint32)]


class Attribute(C.Structure):
    _fields_ = [("name", C.c_char_p), ("value", C.c_char_p)]


class Params(C.Structure):
    _fields_ = [("compression", C.c_uint32), ("zip_level", C.c_uint32), ("threads", C.c_uint32), ("flags", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("file_bytes", C.c_uint64), ("packed_bytes", C.c_uint64), ("chunks", C.c_uint32), ("raw_chunks", C.c_uint32)]


def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def probe():
    return tool("exr_probe")


def load_exr_emu(libz=None):
    # (fp_contract=None: these builds have never carried -ffp-contract=off. -fno-gnu-unique: the two builds keep their own
    # "zlib loaded?" state in one process)
    L = C.CDLL(build_emu("exr_emu.cpp", "libexr_emu%s.so" % ("" if libz is None else "_nolibz"), fp_contract=None,
                         flags=["-pthread", "-fno-gnu-unique"] + ([] if libz is None else ['-DMCRT_EXR_LIBZ="%s"' % libz]), link=["-ldl"]))
    vp = C.c_void_p
    L.exr_half_emu.argtypes = [vp, C.c_uint64, C.c_int, vp]
    L.exr_half_emu.restype = None
    L.exr_float_emu.argtypes = [vp, C.c_uint64, vp]
    L.exr_float_emu.restype = None
    L.exr_pack_emu.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(Channel), C.c_uint32, C.POINTER(Params), vp, vp, C.POINTER(C.c_uint64)]
    L.exr_save_emu.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(Channel), C.c_uint32, C.POINTER(Attribute), C.c_uint32, C.POINTER(Params),
                               C.POINTER(Result), C.c_char_p]
    return L


@functools.lru_cache(maxsize=None)
def _emu():
    return load_exr_emu()


# ---- the header's text in numpy -------------------------------------------------------------------------------------------------

def f64(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def numpy_half_bits(x, half_inf=False):
    """F64 -> HALF by the header: one rounding (astype), the saturation and the NaN pattern on top."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        h = x.astype(np.float16).view(np.uint16)
    sign = (x.view(np.uint64) >> np.uint64(48)).astype(np.uint16) & np.uint16(0x8000)
    if not half_inf:
        h = np.where(np.isfinite(x) & ((h & np.uint16(0x7fff)) == 0x7c00), sign | np.uint16(0x7bff), h)
    return np.where(np.isnan(x), sign | np.uint16(0x7e00), h).astype(np.uint16)


def numpy_float_bits(x):
    """F64 -> FLOAT by the header: one rounding (astype); NaN is sign | 0x7fc00000 | the fraction's top bits."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = x.astype(np.float32).view(np.uint32)
    b = x.view(np.uint64)
    nan = ((b >> np.uint64(32)).astype(np.uint32) & np.uint32(0x80000000)) | np.uint32(0x7fc00000) | ((b & np.uint64((1 << 52) - 1)) >> np.uint64(29)).astype(np.uint32)
    return np.where(np.isnan(x), nan, f).astype(np.uint32)


def numpy_file_values(a, ptype, half_inf=False):
    """A channel's values as the file holds them: an array of FILE_DTYPES[ptype] with the same shape."""
    if ptype == UINT:
        return np.ascontiguousarray(a, dtype=np.uint32).astype("<u4")
    bits_ = numpy_half_bits(a, half_inf) if ptype == HALF else numpy_float_bits(a)
    return np.ascontiguousarray(bits_).view(FILE_DTYPES[ptype])


def conversion_list():
    """The values of the issue's list, as float64."""
    up = lambda v: np.nextafter(v, np.inf)
    down = lambda v: np.nextafter(v, -np.inf)
    pos = [0.0, 2.0 ** -24, 2.0 ** -25, up(2.0 ** -25), down(2.0 ** -14), 2.0 ** -14, up(2.0 ** -14),
           1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -30, 65504.0, 65519.999, 65520.0, 1e300, np.inf, np.nan,
           # FLOAT: the smallest subnormal, the tie below it and the double just above, a value in the binary32 subnormal range, FLT_MAX and
           # the first double that rounds to Inf (FLT_MAX + half an ulp: a tie that goes to the even 2^128)
           2.0 ** -149, 2.0 ** -150, up(2.0 ** -150), 3.3 * 2.0 ** -140, float(np.finfo(np.float32).max), (2.0 - 2.0 ** -24) * 2.0 ** 127,
           down((2.0 - 2.0 ** -24) * 2.0 ** 127), 5e-324, 2.0 ** -1022]
    x = np.array(pos + [-v for v in pos], dtype=np.float64)
    assert np.signbit(x[len(pos)]) and np.signbit(x[len(pos) + 15]) and np.isnan(x[len(pos) + 15])
    return x


def random_doubles(n, seed):
    """Random bit patterns: every exponent, NaNs and infinities of both signs among them; half of them pulled into the range where
    half and float results are normal, subnormal or just overflow."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    near = rng.integers(1023 - 160, 1023 + 20, size=n, dtype=np.uint64) << np.uint64(52)
    b = np.where(rng.random(n) < 0.5, (b & ~np.uint64(0x7FF << 52)) | near, b)
    return b.view(np.float64)


def frame_data(shape, seed):
    x = random_doubles(int(np.prod(shape)), seed)
    special = conversion_list()
    k = min(x.size, special.size)
    x[:k] = special[:k]
    return np.array(x.reshape(shape))  # (a buffer of its own: the views of it name it)


@functools.lru_cache(maxsize=None)
def channel_set(which, width, height):
    """-> list of (name, view [H,W], pixel type) in the order GIVEN to the library, over buffers made once (read-only)."""
    seed = 1000 * width + height
    if which == "one_half":
        y = frame_data((height, width), seed)
        chans = [("Y", y, HALF)]
    elif which == "mixed_unsorted":
        rgb, depth = frame_data((height, width, 3), seed), frame_data((height, width), seed + 1)
        ids = np.random.default_rng(seed + 2).integers(0, 1 << 32, size=(height, width), dtype=np.uint32)
        chans = [("surface.id", ids, UINT), ("R", rgb[..., 0], HALF), ("depth.Z", depth, FLOAT), ("B", rgb[..., 2], FLOAT), ("G", rgb[..., 1], HALF)]
    else:
        tops, rgb = frame_data((height, width, 4, 3), seed), frame_data((height, width, 3), seed + 1)
        chans = [("tops%d.%s" % (k, "RGB"[c]), tops[:, :, k, c], FLOAT if (3 * k + c) % 2 else HALF) for k in range(4) for c in range(3)]
        chans += [("RGB"[c], rgb[..., c], HALF) for c in range(3)]
    for _, a, _ in chans:
        (a.base if a.base is not None else a).setflags(write=False)
    return chans


def sorted_file_channels(chans, half_inf=False):
    """-> [(name, pixel type, values [H,W] of the file's dtype)] sorted by name as bytes."""
    return [(n, t, numpy_file_values(a, t, half_inf)) for n, a, t in sorted(chans, key=lambda c: c[0].encode("ascii"))]


def zip_transform(raw):
    r = np.frombuffer(raw, dtype=np.uint8)
    t = np.concatenate([r[0::2], r[1::2]])
    u = t.copy()
    u[1:] = ((t[1:].astype(np.int32) - t[:-1].astype(np.int32) + 128) % 256).astype(np.uint8)
    return u.tobytes()


def numpy_chunks(file_chans, height, zipped):
    """-> [(y, raw bytes, payload as the packed buffer holds it)] per chunk."""
    lines = 16 if zipped else 1
    out = []
    for y0 in range(0, height, lines):
        raw = b"".join(v[y].tobytes() for y in range(y0, min(y0 + lines, height)) for _, _, v in file_chans)
        out.append((y0, raw, zip_transform(raw) if zipped else raw))
    return out


def py_exr_file(width, height, file_chans, compression, attributes=(), zip_level=4):
    """The file by the header's layout -> (bytes, raw_chunks)."""
    def attr(name, typ, value):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value
    zipped = compression == 3
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t, _ in file_chans) + b"\0"
    box = struct.pack("<4i", 0, 0, width - 1, height - 1)
    head = b"\x76\x2f\x31\x01\x02\x00\x00\x00" + attr("channels", "chlist", chlist) + attr("compression", "compression", bytes([compression]))
    head += attr("dataWindow", "box2i", box) + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0")
    head += attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
    head += attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    for k, v in attributes:
        head += attr(k, "string", v.encode())
    head += b"\0"
    body, raws = [], 0
    for y0, raw, payload in numpy_chunks(file_chans, height, zipped):
        data = raw
        if zipped:
            data = zlib.compress(payload, zip_level)
            if len(data) >= len(raw):
                data, raws = raw, raws + 1
        body.append(struct.pack("<ii", y0, len(data)) + data)
    at, table = len(head) + 8 * len(body), b""
    for b in body:
        table += struct.pack("<Q", at)
        at += len(b)
    return head + table + b"".join(body), raws


# ---- the emulation ---------------------------------------------------------------------------------------------------------------

def c_channels(chans):
    """The mcrt_exr_channel array of (name, view, pixel type): views of one buffer name that buffer, by stride and offset."""
    recs, keep = [], []
    for name, a, t in chans:
        item = a.dtype.itemsize
        root = a
        while isinstance(root.base, np.ndarray):
            root = root.base
        step = (a.strides[1] if a.shape[1] > 1 else (a.strides[0] if a.shape[0] > 1 else item)) // item
        offset = ((a.ctypes.data - root.ctypes.data) // item) % step
        recs.append(Channel(name.encode() if isinstance(name, str) else name, a.ctypes.data - offset * item, SRC_U32 if a.dtype == np.uint32 else SRC_F64, t, step, offset))
        keep.append(a)
    return (Channel * len(recs))(*recs), keep


def emu_pack(width, height, chans, compression, flags=0):
    arr, keep = c_channels(chans)
    size = sum(FILE_DTYPES[t].itemsize for _, _, t in chans) * width * height
    packed, by_byte = np.full((size + 3) // 4 * 4, 0xAB, dtype=np.uint8), np.full((size + 3) // 4 * 4, 0xCD, dtype=np.uint8)
    n = C.c_uint64()
    par = Params(compression, 0, 0, flags)
    assert _emu().exr_pack_emu(width, height, arr, len(chans), C.byref(par), packed.ctypes.data, by_byte.ctypes.data, C.byref(n)) == 0
    assert n.value == size
    return packed, by_byte, size


def emu_save(path, width, height, chans, compression=ZIP, attributes=(), expect=0, emu=None, **params):
    arr, keep = c_channels(chans) if chans is not None else (None, None)
    attrs = (Attribute * max(len(attributes), 1))(*[Attribute(k.encode() if k is not None else None, v.encode() if v is not None else None) for k, v in attributes])
    par, res, msg = Params(compression, params.get("zip_level", 0), params.get("threads", 0), params.get("flags", 0)), Result(), C.create_string_buffer(256)
    rc = (emu or _emu()).exr_save_emu(path.encode() if path is not None else None, width, height, arr, params.get("count", len(chans) if chans is not None else 1),
                                     attrs if attributes else None, len(attributes), C.byref(par), C.byref(res), msg)
    assert rc == expect, (rc, expect, msg.value)
    return res, msg.value.decode()


# ---- tests -----------------------------------------------------------------------------------------------------------------------

def test_numpy_rounds_once():
    x = np.array([1 + 2.0 ** -11 + 2.0 ** -30])
    assert x.astype(np.float16).view(np.uint16)[0] == 0x3c01 and x.astype(np.float32).astype(np.float16).view(np.uint16)[0] == 0x3c00
    assert numpy_half_bits(np.array([65520.0, -1e300, 65519.999]))[:].tolist() == [0x7bff, 0xfbff, 0x7bff]
    assert numpy_half_bits(np.array([65520.0, -1e300]), True).tolist() == [0x7c00, 0xfc00]
    assert numpy_half_bits(np.array([2.0 ** -25, np.nextafter(2.0 ** -25, 1.0), -0.0])).tolist() == [0, 1, 0x8000]


@pytest.mark.parametrize("half_inf", [False, True])
def test_half_is_one_rounding_from_binary64(half_inf):
    x = np.concatenate([conversion_list(), random_doubles(100000, 7)])
    got = np.empty(x.size, dtype=np.uint16)
    _emu().exr_half_emu(x.ctypes.data, x.size, int(half_inf), got.ctypes.data)
    want = numpy_half_bits(x, half_inf)
    np.testing.assert_array_equal(got, want)
    k = conversion_list().size // 2
    assert got[9] == 0x3c01 and got[k + 9] == 0xbc01                        # the double-rounding witness
    assert got[15] == 0x7e00 and got[k + 15] == 0xfe00                      # NaN keeps its sign
    assert got[k] == 0x8000 and got[1] == 1 and got[2] == 0 and got[3] == 1  # -0, the smallest subnormal, the tie and what is above it
    assert got[12] == (0x7c00 if half_inf else 0x7bff) and got[13] == got[12] and got[11] == 0x7bff and got[14] == 0x7c00
    assert (np.abs(x[np.isfinite(x)]) > 65520).sum() > 1000 and ((np.abs(x) < 2.0 ** -14) & (np.abs(x) > 2.0 ** -25)).sum() > 1000


def test_float_is_one_rounding_and_keeps_subnormals():
    x = np.concatenate([conversion_list(), random_doubles(100000, 8)])
    got = np.empty(x.size, dtype=np.uint32)
    _emu().exr_float_emu(x.ctypes.data, x.size, got.ctypes.data)
    np.testing.assert_array_equal(got, numpy_float_bits(x))
    assert got[16] == 1 and got[17] == 0 and got[18] == 1 and 0 < got[19] < 0x00800000   # 2^-149, the tie below it, above it, a subnormal
    assert got[20] == 0x7f7fffff and got[21] == 0x7f800000 and got[22] == 0x7f7fffff   # FLT_MAX, the first double that rounds to Inf, below it
    assert ((np.abs(x) < 2.0 ** -126) & (np.abs(x) > 2.0 ** -149)).sum() > 1000


@pytest.mark.parametrize("zipped", [False, True], ids=["file_order", "zip_order"])
@pytest.mark.parametrize("which", CHANNEL_SETS)
@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_chunk_payloads_are_the_header_in_numpy(width, height, which, zipped):
    chans = channel_set(which, width, height)
    packed, by_byte, size = emu_pack(width, height, chans, ZIP if zipped else NONE)
    want = b"".join(p for _, _, p in numpy_chunks(sorted_file_channels(chans), height, zipped))
    assert len(want) == size
    want = np.frombuffer(want, dtype=np.uint8)
    np.testing.assert_array_equal(packed[:size], want)    # the lanes' words
    np.testing.assert_array_equal(by_byte[:size], want)   # the per-byte map
    assert (packed[size:] == 0).all()                     # (the last word's padding)
    if zipped:  # the step across the half boundary, chunk by chunk
        at = 0
        for _, raw, payload in numpy_chunks(sorted_file_channels(chans), height, True):
            h = len(raw) // 2
            assert payload[h] == (raw[1] - raw[2 * (h - 1)] + 128) % 256 and packed[at + h] == payload[h] and packed[at + h - 1] == payload[h - 1]
            at += len(raw)


def test_half_inf_reaches_the_payload():
    chans = channel_set("mixed_unsorted", 65, 17)
    for flags in (0, HALF_INF):
        packed, _, size = emu_pack(65, 17, chans, NONE, flags)
        want = b"".join(p for _, _, p in numpy_chunks(sorted_file_channels(chans, flags == HALF_INF), 17, False))
        np.testing.assert_array_equal(packed[:size], np.frombuffer(want, dtype=np.uint8))
    r = channel_set("mixed_unsorted", 65, 17)[1][1]
    assert (np.isfinite(r) & (np.abs(r) >= 65520)).any()


ATTRIBUTES = (("mcrt:spp", "16"), ("mcrt:seed", "305419896"), ("mcrt:integrator", "path tracer"), ("mcrt:kernel", ""))


@pytest.mark.parametrize("which", CHANNEL_SETS)
@pytest.mark.parametrize("width,height", [(1, 1), (65, 17), (257, 33), (64, 16)])
def test_none_files_are_the_python_writers_bytes(tmp_path, width, height, which):
    chans = channel_set(which, width, height)
    path = str(tmp_path / "none.exr")
    res, _ = emu_save(path, width, height, chans, NONE, ATTRIBUTES)
    want, _ = py_exr_file(width, height, sorted_file_channels(chans), 0, ATTRIBUTES)
    got = open(path, "rb").read()
    assert got == want
    assert res.file_bytes == len(want) and res.chunks == height and res.raw_chunks == 0
    assert res.packed_bytes == sum(FILE_DTYPES[t].itemsize for _, _, t in chans) * width * height


def assert_reads_back(path, width, height, chans, compression, attributes=(), half_inf=False):
    got, attrs, info = probe().read(path)
    want = sorted_file_channels(chans, half_inf)
    assert list(got) == [n for n, _, _ in want]
    for n, t, v in want:
        assert got[n].dtype == FILE_DTYPES[t] and got[n].shape == (height, width), n
        np.testing.assert_array_equal(got[n].view("u%d" % v.dtype.itemsize), v.view("u%d" % v.dtype.itemsize), err_msg=n)
    assert (info["width"], info["height"], info["compression"]) == (width, height, compression)
    assert [(k, attrs[k]) for k in list(attrs)[8:]] == [(k, ("string", v)) for k, v in attributes]
    assert list(attrs)[:8] == ["channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter", "screenWindowWidth"]
    return info


def test_the_probe_reads_the_python_writers_files(tmp_path):
    """The reader against the independent writer, ZIP and raw chunks included, before it judges the library's files."""
    for which, (w, h) in (("mixed_unsorted", (65, 33)), ("strided_15", (63, 17))):
        chans = channel_set(which, w, h)
        for comp in (0, 3):
            data, _ = py_exr_file(w, h, sorted_file_channels(chans), comp, ATTRIBUTES)
            path = str(tmp_path / ("py_%s_%d.exr" % (which, comp)))
            open(path, "wb").write(data)
            assert_reads_back(path, w, h, chans, comp, ATTRIBUTES)
    noise = np.random.default_rng(5).integers(0, 1 << 32, size=(16, 64), dtype=np.uint32)
    data, raws = py_exr_file(64, 16, [("noise", UINT, noise)], 3)
    assert raws == 1
    open(str(tmp_path / "raw.exr"), "wb").write(data)
    assert assert_reads_back(str(tmp_path / "raw.exr"), 64, 16, [("noise", noise, UINT)], 3)["raw_chunks"] == 1


@pytest.mark.parametrize("which", CHANNEL_SETS)
@pytest.mark.parametrize("width,height", [(1, 1), (65, 17), (257, 33), (63, 15)])
def test_zip_files_read_back_bit_equal(tmp_path, width, height, which):
    chans = channel_set(which, width, height)
    path = str(tmp_path / "zip.exr")
    res, _ = emu_save(path, width, height, chans, ZIP, ATTRIBUTES, threads=3)
    info = assert_reads_back(path, width, height, chans, 3, ATTRIBUTES)
    assert res.chunks == (height + 15) // 16 == info["chunks"] and res.raw_chunks == info["raw_chunks"] and res.file_bytes == os.path.getsize(path)
    by_default, _ = emu_save(str(tmp_path / "default.exr"), width, height, chans, 0, ATTRIBUTES)   # compression 0: the default is ZIP
    assert assert_reads_back(str(tmp_path / "default.exr"), width, height, chans, 3, ATTRIBUTES)["chunks"] == res.chunks


def test_raw_chunk_rule(tmp_path):
    """Deflate of random bytes is longer than its input: every chunk of a random uint32 channel is stored raw; none of a smooth ramp is."""
    noise = np.random.default_rng(11).integers(0, 1 << 32, size=(48, 64), dtype=np.uint32)
    for h in (16, 48):
        path = str(tmp_path / ("noise%d.exr" % h))
        res, _ = emu_save(path, 64, h, [("noise", noise[:h], UINT)], ZIP, threads=2)
        assert res.chunks == h // 16 and res.raw_chunks == res.chunks
        assert res.file_bytes == os.path.getsize(path)
        assert assert_reads_back(path, 64, h, [("noise", noise[:h], UINT)], 3)["raw_chunks"] == res.chunks
    ramp = np.tile(np.arange(64, dtype=np.float64) / 64.0, (16, 1))
    path = str(tmp_path / "ramp.exr")
    res, _ = emu_save(path, 64, 16, [("Y", ramp, HALF)], ZIP)
    assert res.chunks == 1 and res.raw_chunks == 0 and res.file_bytes < 64 * 16 * 2
    assert_reads_back(path, 64, 16, [("Y", ramp, HALF)], 3)


def test_what_the_library_refuses_the_plain_cpp_path_refuses(tmp_path):
    w, h = 5, 3
    rgb = frame_data((h, w, 3), 3)
    ids = np.zeros((h, w), dtype=np.uint32)
    good = [("R", rgb[..., 0], HALF), ("id", ids, UINT)]
    path = str(tmp_path / "x.exr")
    emu_save(path, w, h, good)
    os.remove(path)
    bad = lambda chans, **kw: emu_save(path, kw.pop("w", w), kw.pop("h", h), chans, expect=ERR_INVALID, **kw)
    emu_save(None, w, h, good, expect=ERR_INVALID)                                   # NULL path
    bad(None)                                                                        # NULL channel array
    bad(good, count=0)
    many = [("c%04d" % i, ids, UINT) for i in range(1025)]
    bad(many)
    emu_save(path, w, h, many[:1024], NONE)                                          # (1024 are fine)
    bad(good, w=0)
    bad(good, h=0)
    bad(good, w=1 << 16, h=1 << 16)                                                  # 2^32 pixels: refused before anything is read
    for name in ("", "x" * 32, "a\tb", "caf\xe9".encode("latin-1"), "\x7f"):
        bad([(name, ids, UINT)])
    emu_save(path, w, h, [("x" * 31, ids, UINT), (" ~", ids, UINT)], NONE)           # (31 bytes and the ends of printable ASCII are fine)
    bad([("R", rgb[..., 0], HALF), ("R", rgb[..., 1], HALF)])                        # duplicate names
    arr, keep = c_channels(good)
    for field, value in (("data", None), ("stride", 0), ("offset", 3), ("offset", 7)):
        arr2, _ = c_channels(good)
        setattr(arr2[0], field, value)
        par, res = Params(), Result()
        assert _emu().exr_save_emu(path.encode(), w, h, arr2, 2, None, 0, C.byref(par), C.byref(res), None) == ERR_INVALID, field
    bad([("R", rgb[..., 0], UINT)])                                                   # F64 -> UINT
    bad([("id", ids, HALF)])                                                          # U32 -> HALF
    bad([("id", ids, FLOAT)])
    bad([("R", rgb[..., 0], 3)])                                                      # no such pixel type
    arr2, _ = c_channels(good)
    arr2[0].source_type = 2
    assert _emu().exr_save_emu(path.encode(), w, h, arr2, 2, None, 0, None, None, None) == ERR_INVALID
    bad(good, zip_level=10)
    emu_save(path, w, h, good, ZIP, zip_level=9)
    for comp in (3, 0x100 | 1, 0x100 | 2, 0x100 | 4, 1):
        bad(good, compression=comp)
    for name in ("channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter", "screenWindowWidth"):
        bad(good, attributes=((name, "x"),))
    bad(good, attributes=(("", "x"),))
    bad(good, attributes=(("a", None),))
    assert not os.path.exists(path) or os.remove(path) is None
    # MCRT_ERR_IO: a directory that is not there, and nothing is left behind
    missing = str(tmp_path / "no_such_dir" / "x.exr")
    _, msg = emu_save(missing, w, h, good, expect=ERR_IO)
    assert "no_such_dir" in msg and not os.path.exists(missing)
    if os.path.exists("/dev/full"):  # created but not writable to the end: the partial file is removed
        link = str(tmp_path / "full.exr")
        os.symlink("/dev/full", link)
        emu_save(link, w, h, good, expect=ERR_IO)
        assert not os.path.lexists(link)


def test_zip_without_libz_is_unsupported_and_none_still_works(tmp_path):
    nolibz = load_exr_emu(libz="libz-that-is-not-there.so.1")
    chans = channel_set("mixed_unsorted", 65, 17)
    path = str(tmp_path / "nolibz.exr")
    _, msg = emu_save(path, 65, 17, chans, ZIP, expect=ERR_UNSUPPORTED, emu=nolibz)
    assert "libz-that-is-not-there.so.1" in msg and not os.path.exists(path)
    emu_save(path, 65, 17, chans, NONE, emu=nolibz)
    assert open(path, "rb").read() == py_exr_file(65, 17, sorted_file_channels(chans), 0)[0]


def test_stand_alone_sanitizer_run(tmp_path):
    """tests/emu/exr_file_main.cpp, a program of its own, under AddressSanitizer and UndefinedBehaviorSanitizer: once, as a subprocess."""
    src = os.path.join(TESTS, "emu", "exr_file_main.cpp")
    exe = str(tmp_path / "exr_file_main")
    # (the sanitizers' runtimes linked statically: the program then runs the same whatever else the loader of the day brings in first)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-pthread", "-o", exe, src, "-ldl"])
    out = tmp_path / "files"
    out.mkdir()
    run = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, (run.returncode, run.stdout, run.stderr[-2000:])
    lines = [l.split() for l in run.stdout.splitlines()]
    assert [os.path.basename(l[0]) for l in lines] == ["mixed_none.exr", "mixed_zip.exr", "one_pixel.exr", "noise_zip.exr", "ramp_zip.exr"]
    assert all(l[1] == "0" for l in lines)
    by = {os.path.basename(l[0]): l for l in lines}
    assert by["noise_zip.exr"][4:6] == ["1", "1"] and by["ramp_zip.exr"][4:6] == ["1", "0"] and by["mixed_zip.exr"][4] == "3" and by["mixed_none.exr"][4] == "33"
    a, attrs, ia = probe().read(str(out / "mixed_none.exr"))
    b, _, ib = probe().read(str(out / "mixed_zip.exr"))
    assert len(a) == 16 and list(a) == sorted(a) and attrs["mcrt:spp"] == ("string", "16") and (ia["width"], ia["height"]) == (65, 33)
    for n in a:
        np.testing.assert_array_equal(a[n].view("u%d" % a[n].dtype.itemsize), b[n].view("u%d" % b[n].dtype.itemsize), err_msg=n)
    # rgb[5 .. 8] of the program: B of pixel 1 is Inf, pixel 2 is (R -NaN, G 1e300 as FLOAT, B -0)
    assert a["B"].view(np.uint16).ravel()[1] == 0x7c00 and a["R"].view(np.uint16).ravel()[2] == 0xfe00
    assert a["G"].view(np.uint32).ravel()[2] == 0x7f800000 and a["B"].view(np.uint16).ravel()[2] == 0x8000
