#!/usr/bin/env python3
"""Regenerates tests/golden/awkward/ from the REFERENCE ITSELF, like make_golden.py (oracle/_ref/mcrt_ref = the reference's
translation units compiled in place + oracle/ref_main.cpp). Runs only in the build container; the outputs are committed.

The scenes are those of tests/awkward_scenes.py (inputs the hierarchy builders have trouble with). Each is written as a
scene file of its own in the format of the shipped scenes - "vertices" sets with "object" surfaces that list "triangles",
"sphere"s, "quadric"s - and flattened with the reference's own builders:

  <scene>.json.gz                   the input (data: the scene file the reference's loader read, gzip'd - the largest is 270 KB of
                                    numbers on one line)
  <scene>_<qsah|bsah|octree>[_binsN].mcrt   the scene image with the reference's LinearNode arrays and surface order
  index.json                        the list of fixtures: image, input, "bvh" type, bins_per_axis (0 = the type's default)

What the reference's loader can and cannot express:
  * -0.0: the JSON number "-0.0" is read as the double -0.0 and untransformed triangles keep their vertices as read, so
    `signed_zero` reaches the reference's builders with its signs (checked below on the flattened image).
  * quadrics: a scene file describes a quadric by its coefficients, bounds and transform, not by its 4 x 4 form and box. The
    `mixed_kinds` family takes the RECORDS of the six small quadrics of tests/golden/quadric.mcrt; here the same six come from
    their entries in the reference's quadric.json, and the flattened records are checked to be the family's, bit for bit.
"""
import gzip
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
OUT = os.path.join(HERE, "awkward")
REF = os.path.join(ROOT, "oracle", "_ref", "mcrt_ref")
QUADRIC_SCENE = "/root/reference/scenes/quadric.json"
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import awkward_scenes as A  # noqa: E402

# scene, builder, bins_per_axis (0: default)
FIXTURES = [
    ("sah_concatenation", "quaternary_sah", 0), ("sah_concatenation", "binary_sah", 0), ("sah_concatenation", "quaternary_sah", 5),
    ("signed_zero", "quaternary_sah", 0), ("signed_zero", "binary_sah", 0),
    ("octree_concatenation", "octree", 0), ("signed_zero", "octree", 0),
]
SHORT = {"quaternary_sah": "qsah", "binary_sah": "bsah", "octree": "octree"}
MAX_BYTES = 1 << 20  # also below tests/golden/coffee_maker_qsah.mcrt


def fixture_name(scene, kind, bins):
    return "%s_%s%s" % (scene, SHORT[kind], "_bins%d" % bins if bins else "")


def small_quadric_entries():
    """The entries of the reference's quadric.json whose records awkward_scenes._quadric_records() takes from the golden image."""
    surfaces = json.load(open(QUADRIC_SCENE))["surfaces"]
    out = []
    for s in surfaces:
        bd = s["bound_dimensions"]
        if (max(bd) if isinstance(bd, list) else bd) >= 2:  # the seven large slabs
            continue
        s = dict(s)
        s["material"] = "default"
        out.append(s)
    return out


def scene_json(scene):
    """The scene as a scene file: surfaces in the scene's order (runs of triangles become one "object" each)."""
    quadric_entries = small_quadric_entries() if len(scene.quadrics) else []
    j = {
        "num_render_threads": -1, "ior": 1.0,
        "cameras": [{"focal_length": 35, "sensor_width": 35, "eye": [0.0, 0.0, -300.0], "look_at": [0.0, 0.0, 0.0],
                     "image": {"width": 16, "height": 16}, "sqrtspp": 1, "savename": scene.name}],
        "bvh": {"type": "octree"},
        "materials": {"default": {"reflectance": 0.5}},
        "vertices": {}, "surfaces": [],
    }
    # a quadric's record is found by its box: the family orders the records by box, the scene file's entries come in file order
    entry_of_record = {}
    if quadric_entries:
        probe = dict(j, surfaces=quadric_entries)
        probe.pop("vertices")
        probe_path = os.path.join(OUT, "_probe.json")
        json.dump(probe, open(probe_path, "w"))
        img_path = os.path.join(OUT, "_probe.mcrt")
        run([REF, "flatten", "--scene", probe_path, "--bvh", "none", "--out", img_path])
        pkg = importlib.import_module("monte-carlo-ray-tracer_amd")
        img = pkg.SceneImage(img_path)
        s = img.scene
        assert s.num_quadrics == len(quadric_entries) == s.num_surfaces
        rec = np.ctypeslib.as_array(s.quadrics, shape=(s.num_quadrics, 22)).copy()
        which = np.ctypeslib.as_array(s.surf_v, shape=(s.num_surfaces, 9))[:, 0].astype(int)  # no BVH: surfaces in file order
        for entry, r in zip(quadric_entries, rec[which]):
            entry_of_record[r.tobytes()] = entry
        img.close()
        os.remove(probe_path)
        os.remove(img_path)
    i, n = 0, scene.n
    while i < n:
        k = scene.kind[i]
        if k == A.TRI:
            e = i
            while e < n and scene.kind[e] == A.TRI:
                e += 1
            name = "run%d" % i
            j["vertices"][name] = scene.v[i:e].reshape(-1, 3).tolist()
            j["surfaces"].append({"type": "object", "material": "default", "vertex_set": name,
                                  "triangles": [[3 * t, 3 * t + 1, 3 * t + 2] for t in range(e - i)]})
            i = e
            continue
        if k == A.SPHERE:
            j["surfaces"].append({"type": "sphere", "material": "default", "position": scene.v[i, :3].tolist(), "radius": float(scene.v[i, 3])})
        else:
            r = scene.quadrics[int(scene.v[i, 0])].tobytes()
            assert r in entry_of_record, "a quadric record of the family is not what the reference makes of quadric.json"
            j["surfaces"].append(entry_of_record[r])
        i += 1
    return j


def run(cmd):
    print("+", " ".join(cmd), flush=True)
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def same_surfaces(pkg, scene, image_path):
    """The flattened image holds the scene's surfaces, bit for bit (in the builder's order): vertices with their zero signs,
    sphere records, quadric records."""
    img = pkg.SceneImage(image_path)
    s = img.scene
    assert s.num_surfaces == scene.n, (s.num_surfaces, scene.n)
    v = np.ctypeslib.as_array(s.surf_v, shape=(scene.n, 9)).copy()
    kind = np.ctypeslib.as_array(s.surf_kind, shape=(scene.n,)).copy()
    mine = scene.v.copy()
    if s.num_quadrics:
        q = np.ctypeslib.as_array(s.quadrics, shape=(s.num_quadrics, 22))
        assert sorted(r.tobytes() for r in q) == sorted(r.tobytes() for r in scene.quadrics), "quadric records differ"
        rank = {r: i for i, r in enumerate(sorted(r.tobytes() for r in q))}  # name quadrics by their record rather than by their index
        v[kind == A.QUADRIC, 0] = [rank[q[int(x)].tobytes()] for x in v[kind == A.QUADRIC, 0]]
        mine[scene.kind == A.QUADRIC, 0] = [rank[scene.quadrics[int(x)].tobytes()] for x in mine[scene.kind == A.QUADRIC, 0]]
    assert sorted(r.tobytes() for r in v) == sorted(r.tobytes() for r in mine), "the image's surfaces are not the scene's"
    box = np.array(list(s.bb_min) + list(s.bb_max))
    assert box.tobytes() == scene.box.tobytes(), "scene box: %r against %r" % (box, scene.box)
    nodes = int(s.num_nodes)
    img.close()
    return nodes


def main():
    os.makedirs(OUT, exist_ok=True)
    pkg = importlib.import_module("monte-carlo-ray-tracer_amd")
    scenes = {"sah_concatenation": A.sah_concatenation(pkg), "signed_zero": A.scene(pkg, "signed_zero"), "octree_concatenation": A.octree_concatenation(pkg)}
    for name, scene in scenes.items():
        json.dump(scene_json(scene), open(os.path.join(OUT, name + ".json"), "w"), separators=(",", ":"))
    index = []
    for name, kind, bins in FIXTURES:
        image = fixture_name(name, kind, bins) + ".mcrt"
        cmd = [REF, "flatten", "--scene", os.path.join(OUT, name + ".json"), "--bvh", kind, "--out", os.path.join(OUT, image)]
        if bins:
            cmd += ["--bins", str(bins)]
        run(cmd)
        nodes = same_surfaces(pkg, scenes[name], os.path.join(OUT, image))
        size = os.path.getsize(os.path.join(OUT, image))
        assert size < MAX_BYTES, "%s: %d bytes" % (image, size)
        index.append(dict(name=fixture_name(name, kind, bins), scene=name, input=name + ".json.gz", image=image, bvh=kind, bins_per_axis=bins,
                          surfaces=scenes[name].n, nodes=nodes))
        print("%s: %d surfaces, %d nodes, %d bytes" % (image, scenes[name].n, nodes, size))
    for name in scenes:  # the inputs are kept compressed (mtime 0, no file name: the same bytes every time)
        plain = os.path.join(OUT, name + ".json")
        with open(plain, "rb") as f, open(plain + ".gz", "wb") as g, gzip.GzipFile(filename="", mode="wb", fileobj=g, mtime=0) as z:
            z.write(f.read())
        os.remove(plain)
    json.dump({"fixtures": index}, open(os.path.join(OUT, "index.json"), "w"), indent=1, sort_keys=True)
    print("wrote", os.path.join(OUT, "index.json"))


if __name__ == "__main__":
    main()
