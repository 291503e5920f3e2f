"""The row scatter of the sharded host-pointer forms (csrc/mcrt_rows.hpp: a shard's packed rows to their places in the caller's full
frame, behind mcrt_render_aov, mcrt_render_pixel_stats and mcrt_render_highlights) under the address and undefined-behaviour
sanitizers: tests/emu/row_scatter_main.cpp is built as a program of its own and run as a child process - nothing is loaded into this
interpreter - on 13 x 5 frames with the row indices mcrt_shard_rows gives for each camera; it compares every byte of the frame and of a
guard row on either side with the plain statement of what they must hold. Any report of a sanitizer ends the program with a non-zero
status (-fno-sanitize-recover=all)."""
import os
import subprocess

import numpy as np

from conftest import ROOT, TESTS

HEIGHT, WIDTH = 13, 5
SHARDS = {  # case -> (shard_index, shard_count, shard_rows)
    "whole": [(0, 1, 0)],
    "ragged groups of 5": [(0, 3, 5), (1, 3, 5), (2, 3, 5)],  # {0-4}, {5-9}, {10-12}: tests/test_gpu_aov.py's
    "default interleave": [(0, 3, 0), (1, 3, 0), (2, 3, 0)],  # shard_rows 0: whatever mcrt_shard_rows deals then
    "no rows": [(3, 4, 5), (13, 14, 0)],  # more shards than groups of rows
}
ELEMENTS = [(elem, per_pixel) for elem in (4, 8) for per_pixel in (1, 3, 12)]


def rows_of(pkg, shard):
    cam = pkg.CameraDesc()
    cam.width, cam.height, cam.sqrtspp = WIDTH, HEIGHT, 1
    cam.shard_index, cam.shard_count, cam.shard_rows = shard
    return pkg.shard_rows(cam)


def test_packed_rows_go_to_their_places_and_nowhere_else(pkg, tmp_path):
    rows = {case: [rows_of(pkg, s) for s in shards] for case, shards in SHARDS.items()}
    # the cameras are the ones meant: every row once per sharding, the ragged groups, and shards without rows
    assert rows["whole"][0].tolist() == list(range(HEIGHT))
    assert [r.tolist() for r in rows["ragged groups of 5"]] == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11, 12]]
    assert sorted(np.concatenate(rows["default interleave"]).tolist()) == list(range(HEIGHT)) and all(len(r) for r in rows["default interleave"])
    assert [len(r) for r in rows["no rows"]] == [0, 0]
    lines = ["%d %d %d %d %d %s" % (HEIGHT, WIDTH, elem, per_pixel, len(r), " ".join(str(i) for i in r))
             for shards in rows.values() for r in shards for elem, per_pixel in ELEMENTS]
    conf = tmp_path / "configurations.txt"
    conf.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "row_scatter")
    # (the sanitizers' runtimes linked statically: the program then runs the same whatever else the loader of the day brings in first)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-o", exe, os.path.join(TESTS, "emu", "row_scatter_main.cpp")], check=True, cwd=ROOT)
    run = subprocess.run([exe, str(conf)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stdout, run.stderr)
    assert run.stdout.strip() == "ok %d configurations" % len(lines)
