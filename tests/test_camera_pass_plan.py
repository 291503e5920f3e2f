"""The chunk plan of the passes that trace camera rays and its three defaults, CPU tier: the pure layer of csrc/mcrt_camera_pass.hpp - the
text the five host sides and the four emulations run - behind tests/emu/camera_pass_emu.cpp, against a truth table.

Every expected value is a literal worked out by hand from the expressions the host sides had before they shared this header:
chunk_slots = min(option > 0 ? option : default, 0xFFF00000), chunk_pixels = min(max(chunk_slots / per_pixel, 1), max(total_pixels, 1)),
a chunk's camera rays chunk_pixels * spp and slots chunk_pixels * per_pixel; the lighting passes' default
min(max(2^17 * per_pixel, 2^24), 2^26); the light groups' min(min(max(2^17 * per_pixel, 2^25), 2^26), 2^33 / sample_bytes * 2) with
sample_bytes = kLgStateBytes + 24 * planes + 2 * 76 + 8."""
import ctypes as C
import functools

import pytest

from emu_build import build_emu

LIMIT = 0xFFF00000  # 4293918720
FIXED = 1 << 24


@functools.lru_cache(maxsize=None)
def _emu():
    L = C.CDLL(build_emu("camera_pass_emu.cpp"))
    L.camera_pass_emu_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.camera_pass_emu_plan.restype = None
    for name, n in (("limit", 0), ("default", 0), ("lighting_default", 1), ("light_groups_default", 2), ("lg_state_bytes", 0)):
        f = getattr(L, "camera_pass_emu_" + name)
        f.argtypes = [C.c_uint64] * n
        f.restype = C.c_uint64
    return L


# (total_pixels, spp, per_pixel, wanted, default) -> (chunk_pixels, camera rays of a chunk, slots of a chunk, chunks, pixels of the last chunk)
PLANS = {
    "910 pixels, 4 samples, 256 wanted": ((910, 4, 4, 256, FIXED), (64, 256, 256, 15, 14)),  # 14 * 64 = 896, then 14
    "1 wanted": ((910, 4, 4, 1, FIXED), (1, 4, 4, 910, 1)),
    "unset, the fixed default": ((910, 4, 4, 0, FIXED), (910, 3640, 3640, 1, 910)),
    "wanted above the limit": ((0xFFFFFFFF, 1, 1, 1 << 33, FIXED), (4293918720, 4293918720, 4293918720, 2, 1048575)),  # 2^32 - 1 - 0xFFF00000
    "wanted above the limit, 4 slots a pixel": ((0xFFFFFFFF, 4, 4, 1 << 33, FIXED), (1073479680, 4293918720, 4293918720, 5, 1048575)),  # 4 * 1073479680 + 1048575
    "default above the limit": ((0xFFFFFFFF, 1, 1, 0, 1 << 40), (4293918720, 4293918720, 4293918720, 2, 1048575)),
    "per_pixel larger than wanted": ((910, 4, 256, 40, FIXED), (1, 4, 256, 910, 1)),  # 64 occlusion rays a sample
    "no pixel": ((0, 4, 4, 0, FIXED), (1, 4, 4, 0, 0)),
    "no pixel, 256 wanted": ((0, 4, 8, 256, FIXED), (1, 4, 8, 0, 0)),
    "occlusion, 3 rays a sample, 40 wanted": ((192, 4, 12, 40, FIXED), (3, 12, 36, 64, 3)),
    "lighting, 40 wanted": ((192, 4, 8, 40, FIXED), (5, 20, 40, 39, 2)),  # 38 * 5 = 190, then 2
    "aov, 40 wanted, 7 x 5": ((35, 4, 4, 40, FIXED), (10, 40, 40, 4, 5)),
}


@pytest.mark.parametrize("case", list(PLANS))
def test_chunk_plan(case):
    args, want = PLANS[case]
    out = (C.c_uint64 * 5)()
    _emu().camera_pass_emu_plan(*args, out)
    assert tuple(out) == want


def test_limit_and_fixed_default():
    assert _emu().camera_pass_emu_limit() == 4293918720 == 0xFFF00000
    assert _emu().camera_pass_emu_default() == 16777216  # 2^24: the AOV pass, the mattes, the occlusion pass


@pytest.mark.parametrize("spp, want", [(4, 16777216),      # 2^17 * 8 = 2^20: the least, 2^24
                                       (100, 26214400),    # 2^17 * 200
                                       (256, 67108864),    # 2^17 * 512 = 2^26
                                       (1024, 67108864)])  # 2^28: the most, 2^26
def test_lighting_default(spp, want):
    assert _emu().camera_pass_emu_lighting_default(2 * spp) == want


# 2 planes: 216 + 24 * 2 + 2 * 76 + 8 = 424 bytes a sample; 2^33 / 424 = 20259279 samples (424 * 20259279 = 8589934296, 296 short of 2^33)
# = 40518558 slots, between the bounds 2^25 = 33554432 and 2^26 = 67108864: the cut binds where 2^17 * per_pixel is more, from 155 samples on
@pytest.mark.parametrize("spp, want", [(4, 33554432),      # 2^20: the least, 2^25 - the cut does not bind
                                       (144, 37748736),    # 2^17 * 288 - the cut does not bind
                                       (256, 40518558),    # 2^26 cut to 8 GiB
                                       (1024, 40518558)])
def test_light_groups_default_with_two_planes(spp, want):
    assert _emu().camera_pass_emu_lg_state_bytes() == 216  # 76 + 16 + 24 + 16 + 20 + 8 * 8 (csrc/mcrt_light_groups.hpp)
    assert _emu().camera_pass_emu_light_groups_default(2 * spp, 424) == want


def test_light_groups_default_with_the_most_planes():
    # 16 planes (15 groups and the sky's): 216 + 384 + 152 + 8 = 760 bytes a sample; 2^33 / 760 = 11302545 samples (760 * 11302545 =
    # 8589934200, 392 short) = 22605090 slots: below 2^25, so the cut binds at every sample count
    assert _emu().camera_pass_emu_light_groups_default(8, 760) == 22605090
    assert _emu().camera_pass_emu_light_groups_default(512, 760) == 22605090
