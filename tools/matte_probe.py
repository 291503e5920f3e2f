#!/usr/bin/env python3
"""A decoder of the Cryptomatte layers in the OpenEXR files the library writes (include/mcrt.h "ID mattes"), built on tools/exr_probe.read
and the layout's public description - no part of the library takes part, so tests decode the library's files with it.

A layer is announced by the string attributes cryptomatte/<key>/name, /hash, /conversion and /manifest; its data are the FLOAT channels
NAME00.R/G/B/A, NAME01.*, ...: R and B hold ids (a name's 32-bit code as a float32's bits), G and A the coverage of the id before them.
The matte of a name is the sum of the coverages of the ranks whose id is the name's code.

    layers(path) -> dict layer name -> {"key", "hash", "conversion", "manifest": dict name -> code, "ids" [H][W][ranks] uint32,
                                         "coverage" [H][W][ranks] float32}
    matte(layer, name) -> [H][W] float64
    totals(layer) -> dict name -> total coverage in pixels

As a command: the layers, their manifests and the total coverage per name; with --extract, the matte of one name as a .npy file.
    python tools/matte_probe.py FILE.exr [--layer NAME] [--extract NAME OUT.npy]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exr_probe  # noqa: E402


def layers(path):
    channels, attributes, _ = exr_probe.read(path)
    found = {}
    for attr, (typ, value) in attributes.items():
        parts = attr.split("/")
        if len(parts) == 3 and parts[0] == "cryptomatte" and parts[2] == "name" and typ == "string":
            found[parts[1]] = value
    out = {}
    for key, name in found.items():
        get = lambda what: attributes.get("cryptomatte/%s/%s" % (key, what), (None, None))[1]
        manifest = get("manifest")
        ids, coverage = [], []
        level = 0
        while "%s%02d.R" % (name, level) in channels:
            for id_part, cov_part in (("R", "G"), ("B", "A")):
                a, c = channels["%s%02d.%s" % (name, level, id_part)], channels["%s%02d.%s" % (name, level, cov_part)]
                if a.dtype != np.dtype("<f4") or c.dtype != np.dtype("<f4"):
                    raise ValueError("layer %s: level %d is not FLOAT" % (name, level))
                ids.append(a.view(np.uint32))
                coverage.append(c)
            level += 1
        if not ids:
            raise ValueError("layer %s is announced but has no channels" % name)
        out[name] = {"key": key, "hash": get("hash"), "conversion": get("conversion"),
                     "manifest": {k: int(v, 16) for k, v in json.loads(manifest).items()} if manifest is not None else None,
                     "ids": np.stack(ids, axis=-1), "coverage": np.stack(coverage, axis=-1)}
    return out


def matte(layer, name):
    """The coverage of `name` per pixel: the sum over the ranks whose id is its code (ranks of coverage 0 are empty, whatever their id)."""
    code = layer["manifest"][name]
    cov = layer["coverage"].astype(np.float64)
    return np.where((layer["ids"] == np.uint32(code)) & (cov > 0), cov, 0.0).sum(axis=-1)


def totals(layer):
    return {name: float(matte(layer, name).sum()) for name in layer["manifest"]}


def main(argv):
    args = list(argv[1:])
    want_layer, extract = None, None
    if "--layer" in args:
        i = args.index("--layer")
        want_layer = args[i + 1]
        del args[i:i + 2]
    if "--extract" in args:
        i = args.index("--extract")
        extract = (args[i + 1], args[i + 2])
        del args[i:i + 3]
    if len(args) != 1:
        print(__doc__)
        return 2
    found = layers(args[0])
    if not found:
        print("%s: no Cryptomatte layer" % args[0])
        return 1
    for name, layer in found.items():
        if want_layer not in (None, name):
            continue
        h, w, ranks = layer["ids"].shape
        print("%s: layer %s (key %s, hash %s, conversion %s): %d x %d, %d ranks, %s" % (
            args[0], name, layer["key"], layer["hash"], layer["conversion"], w, h, ranks,
            "%d names" % len(layer["manifest"]) if layer["manifest"] is not None else "no manifest"))
        if layer["manifest"] is None:
            continue
        for key_name, total in sorted(totals(layer).items(), key=lambda kv: -kv[1]):
            print("  %08x  %12.3f px  %s" % (layer["manifest"][key_name], total, key_name))
        if extract:
            np.save(extract[1], matte(layer, extract[0]))
            print("  matte of %s -> %s" % (extract[0], extract[1]))
            extract = None
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
