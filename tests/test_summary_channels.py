"""The one table of a render's per-sample summary, both statements of it: the binding's FRAME_SUMMARY_CHANNELS with the two tables derived
from it against the ctypes structs, and against the channel table of csrc/mcrt_summary_channels.hpp (whose static_asserts hold the C
structs of include/mcrt.h to the same order when the library is built). No GPU."""
import os
import re

import numpy as np

from conftest import ROOT


def fields(struct):
    return [name for name, _ in struct._fields_]


def test_the_structs_are_the_table(pkg):
    table = pkg.FRAME_SUMMARY_CHANNELS
    assert fields(pkg.FrameSummary) == list(table)
    assert isinstance(pkg.PIXEL_STATS_CHANNELS, tuple) and fields(pkg.PixelStatsBuffers) == list(pkg.PIXEL_STATS_CHANNELS) == list(table)[1:4]
    assert isinstance(pkg.HIGHLIGHT_CHANNELS, dict) and fields(pkg.HighlightBuffers) == list(pkg.HIGHLIGHT_CHANNELS) == list(table)[4:6]
    assert all(table[k] == (3,) for k in ("rgb",) + pkg.PIXEL_STATS_CHANNELS)
    assert pkg.HIGHLIGHT_CHANNELS == {"tops": (pkg.ROBUST_TOPS, 3), "level": ()} == {k: table[k] for k in pkg.HIGHLIGHT_CHANNELS}
    assert [k for group in pkg.FRAME_SUMMARY_GROUPS for k in group] == list(table)


def test_the_librarys_table_is_the_bindings(pkg):
    text = open(os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc", "mcrt_summary_channels.hpp")).read()
    rows = re.findall(r"\{&mcrt_frame_summary::(\w+), ([^}]+)\}", text)
    assert [name for name, _ in rows] == list(pkg.FRAME_SUMMARY_CHANNELS)
    for name, pixel_bytes in rows:
        assert eval(pixel_bytes, {"MCRT_ROBUST_TOPS": pkg.ROBUST_TOPS}) == 8 * int(np.prod(pkg.FRAME_SUMMARY_CHANNELS[name], dtype=np.int64)), name
