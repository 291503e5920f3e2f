#!/usr/bin/env python3
"""A reader of the OpenEXR files the library writes (include/mcrt.h "OpenEXR output"), written from the format's specification with
struct, numpy and the zlib module - no part of the library takes part, so tests read the library's files back with it.

Single-part scan-line files with short names, compression NONE or ZIP (raw chunks included), channels of type UINT, HALF and FLOAT
without subsampling; anything else raises ValueError.

    read(path) -> (channels, attributes, info)
        channels    dict name -> array [H][W] of uint32 / float16 / float32, in the file's (sorted) order
        attributes  dict name -> (type, value): strings decoded, the standard ones parsed, others as bytes
        info        width, height, compression, chunks, raw_chunks, offsets

As a command: the channel list and per channel min / max / NaN count.
    python tools/exr_probe.py FILE.exr
"""
import struct
import sys
import zlib

import numpy as np

PIXEL_DTYPES = {0: np.dtype("<u4"), 1: np.dtype("<f2"), 2: np.dtype("<f4")}
PIXEL_NAMES = {0: "UINT", 1: "HALF", 2: "FLOAT"}
NONE, ZIP = 0, 3


def _cstr(buf, at):
    end = buf.index(b"\0", at)
    return buf[at:end].decode("ascii"), end + 1


def zip_undo(u):
    """ZIP's pre-deflate transform backwards: the running sum of the deltas, then the two byte planes interleaved."""
    u = np.frombuffer(u, dtype=np.uint8).astype(np.int64)
    n = u.size
    d = u - 128
    d[0] = u[0]
    t = (np.cumsum(d) % 256).astype(np.uint8)
    h = (n + 1) // 2
    raw = np.empty(n, dtype=np.uint8)
    raw[0::2] = t[:h]
    raw[1::2] = t[h:]
    return raw.tobytes()


def read(path):
    buf = open(path, "rb").read()
    if buf[:4] != b"\x76\x2f\x31\x01":
        raise ValueError("not an OpenEXR file")
    version, = struct.unpack_from("<I", buf, 4)
    if version != 2:
        raise ValueError("version field %#x: only single-part scan-line files with short names" % version)
    at = 8
    attributes = {}
    while buf[at] != 0:
        name, at = _cstr(buf, at)
        typ, at = _cstr(buf, at)
        size, = struct.unpack_from("<i", buf, at)
        at += 4
        attributes[name] = (typ, buf[at:at + size])
        at += size
    at += 1
    chlist = attributes["channels"][1]
    channels_def = []
    p = 0
    while chlist[p] != 0:
        name, p = _cstr(chlist, p)
        ptype, plinear, xs, ys = struct.unpack_from("<iB3xii", chlist, p)
        p += 16
        if xs != 1 or ys != 1 or ptype not in PIXEL_DTYPES:
            raise ValueError("channel %s: subsampled or of unknown type" % name)
        channels_def.append((name, ptype))
    if p + 1 != len(chlist):
        raise ValueError("the channel list does not end where its size says")
    compression = attributes["compression"][1][0]
    if compression not in (NONE, ZIP):
        raise ValueError("compression %d" % compression)
    x0, y0, x1, y1 = struct.unpack("<4i", attributes["dataWindow"][1])
    if (x0, y0) != (0, 0) or attributes["lineOrder"][1] != b"\0":
        raise ValueError("a data window off the origin or a line order other than increasing y")
    width, height = x1 + 1, y1 + 1
    lines = 16 if compression == ZIP else 1
    chunks = (height + lines - 1) // lines
    offsets = struct.unpack_from("<%dQ" % chunks, buf, at)
    line_bytes = sum(PIXEL_DTYPES[t].itemsize for _, t in channels_def) * width
    out = {name: np.empty((height, width), dtype=PIXEL_DTYPES[t]) for name, t in channels_def}
    raw_chunks = 0
    for k, off in enumerate(offsets):
        y, size = struct.unpack_from("<ii", buf, off)
        if y != k * lines:
            raise ValueError("chunk %d starts at line %d" % (k, y))
        n_lines = min(lines, height - y)
        n = n_lines * line_bytes
        data = buf[off + 8:off + 8 + size]
        if len(data) != size:
            raise ValueError("chunk %d is cut short" % k)
        if compression == ZIP:
            if size < n:
                data = zip_undo(zlib.decompress(data))
            else:
                raw_chunks += 1
        if len(data) != n:
            raise ValueError("chunk %d holds %d bytes, not %d" % (k, len(data), n))
        p = 0
        for line in range(n_lines):
            for name, t in channels_def:
                dt = PIXEL_DTYPES[t]
                out[name][y + line] = np.frombuffer(data, dtype=dt, count=width, offset=p)
                p += width * dt.itemsize
    parsed = {}
    for name, (typ, value) in attributes.items():
        if typ == "string":
            value = value.decode("ascii", "replace")
        elif typ == "float":
            value = struct.unpack("<f", value)[0]
        elif typ == "v2f":
            value = struct.unpack("<2f", value)
        elif typ == "box2i":
            value = struct.unpack("<4i", value)
        elif typ in ("compression", "lineOrder"):
            value = value[0]
        elif typ == "chlist":
            value = [(n, PIXEL_NAMES[t]) for n, t in channels_def]
        parsed[name] = (typ, value)
    info = {"width": width, "height": height, "compression": compression, "chunks": chunks, "raw_chunks": raw_chunks, "offsets": list(offsets),
            "header_bytes": at, "file_bytes": len(buf)}
    return out, parsed, info


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    channels, attributes, info = read(argv[1])
    print("%s: %d x %d, compression %s, %d chunks (%d raw), %d bytes" % (argv[1], info["width"], info["height"], {NONE: "NONE", ZIP: "ZIP"}[info["compression"]],
                                                                       info["chunks"], info["raw_chunks"], info["file_bytes"]))
    for name, (typ, value) in attributes.items():
        if name != "channels":
            print("  attribute %-20s %-12s %r" % (name, typ, value))
    for name, a in channels.items():
        if a.dtype.kind == "f":
            f = a.astype(np.float64)
            nan = int(np.isnan(f).sum())
            ok = f[~np.isnan(f)]
            lo, hi = (ok.min(), ok.max()) if ok.size else (float("nan"), float("nan"))
            print("  %-28s %-5s min %.6g max %.6g NaN %d" % (name, {2: "HALF", 4: "FLOAT"}[a.dtype.itemsize], lo, hi, nan))
        else:
            print("  %-28s UINT  min %d max %d NaN 0" % (name, a.min(), a.max()))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
