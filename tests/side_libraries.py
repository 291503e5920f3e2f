"""What the side libraries may contain: one row per image pass, read by tests/test_side_libraries.py (the generic checks, once) and by
what stays in tests/test_*_library.py (struct layouts, refusals, presets: whatever only one pass has).

Every pass of monte-carlo-ray-tracer_amd/build.py's PASSES ships its kernels as a code object of its own, lib<stem>.so, so that the gfx950
functions of libmcrt_hip.so stay the render path's (tests/golden/device_code_hashes.json). The invariant behind the rows: every kernel
lives in exactly one library. A plain helper module like oracle_lib.py and kat_bits.py - no fixtures, no hooks."""
import atexit
import importlib.util
import os
import re
import subprocess

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(TESTS, ".."))
CSRC = os.path.join(ROOT, "monte-carlo-ray-tracer_amd", "csrc")
MAIN_LIBS = ("libmcrt_hip.so", "libmcrt_hip_tol.so")  # (the second only where built: MCRT_SKIP_TOLERANCE_BUILD=1 leaves it out)

_tools, _kernels, _dynamic = {}, {}, {}
extractions = 0  # code objects taken out of a library and read (tools/kernel_spill_table.py kernels_of): once per library and process


def tool(name):
    """tools/<name>.py as a module, executed once per process."""
    if name not in _tools:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        _tools[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_tools[name])
    return _tools[name]


def _key(path):
    st = os.stat(path)
    return (os.path.abspath(path), st.st_mtime_ns, st.st_size)


def _report():
    if extractions:
        print("side_libraries: %d code-object extractions" % extractions)


atexit.register(_report)


def kernels_of(path):
    """tools/kernel_spill_table.py's kernels_of(path), kept per (path, mtime, size): a library is copied, taken apart and read once."""
    global extractions
    key = _key(path)
    if key not in _kernels:
        extractions += 1
        _kernels[key] = tool("kernel_spill_table").kernels_of(path)
    return _kernels[key]


def dynamic_section(path):
    """`readelf -d` of a library, kept the same way."""
    key = _key(path)
    if key not in _dynamic:
        _dynamic[key] = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
    return _dynamic[key]


def libraries_on_disk():
    """Every libmcrt_*.so in csrc/, the main libraries included."""
    return sorted(f for f in os.listdir(CSRC) if f.startswith("libmcrt_") and f.endswith(".so"))


def recorded_resources(notes_file, kernel_regex):
    """The resource table of profiles/<notes_file>: kernel -> dict of vgpr, vgpr_spill, sgpr_spill, scratch, lds (upper bounds)."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", notes_file)):
        m = re.match(r"\|\s*`(" + kernel_regex + r")`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", line)
        if m:
            rows[m.group(1)] = dict(zip(("vgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds"), (int(x) for x in m.groups()[1:])))
    return rows


def c_values(tmp_path, c_expressions, fmt, parse=int):
    """What a small C program prints for expressions over include/mcrt.h (sizeof, offsetof, constants): fmt holds one printf
    conversion per expression, separated by blanks; the integers by default."""
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcrt.h"\nint main(void){printf("%s\\n",%s);return 0;}\n' % (fmt, ",".join(c_expressions)))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    return [parse(x) for x in subprocess.check_output([str(exe)]).decode().split()]


def foreign(rules, name, kernels=()):
    """Does a kernel name found in ANOTHER library fall under a pass's foreign-kernel rule? A rule is a list of
    ("substring", lower-case text) | ("prefix", text) | ("regex", pattern) | ("names",) - the last: the pass's own kernel names, whole."""
    for kind, *text in rules:
        if (kind == "substring" and text[0] in name.lower()) or (kind == "prefix" and name.startswith(text[0])) \
                or (kind == "regex" and re.search(text[0], name)) or (kind == "names" and name in kernels):
            return True
    return False


# LDS of the kernels that shade (light groups, path classes, adaptive sampling): the Sobol byte tables, the sine / cosine table and
# 8 history entries for each of 256 lanes
SOBOL_LDS = 6 * 4 * 256 * 4
SHADING_LDS = SOBOL_LDS + 440 * 8 + 8 * 256 * 8


def _row(kernels, foreign, lds=None, max_wg=None, sgpr_spill_allowed=(), notes=None, calls=(), attributes=(), methods=(), no_libz=False, skip=None):
    return dict(kernels=kernels, foreign=foreign, lds=lds, max_wg=max_wg or {}, sgpr_spill_allowed=tuple(sgpr_spill_allowed), notes=notes, calls=tuple(calls),
                attributes=tuple(attributes), methods=tuple(methods), no_libz=no_libz, skip=skip or {})


# One row per pass, in build.py's order.
#   kernels:    the exact sorted list of the library's kernels. All of them: no scratch, no spilled VGPR.
#   foreign:    the names no OTHER library on disk may hold (foreign() above; skip: {library: why it is not searched}).
#   lds:        static LDS bytes per kernel (a kernel not named: 0); None: the pass states none.
#   max_wg:     the launch bound per kernel, where the pass states one.
#   sgpr_spill_allowed: the kernels that may spill SGPRs (to lanes of a VGPR, not to memory); every other kernel spills none.
#   notes:      (file under profiles/, regex of its kernels): the file's resource table lists exactly the kernels, as upper bounds.
#   calls / attributes / methods: the exported C calls, the binding's module attributes, the Context methods.
#   no_libz:    neither the main libraries nor this one list libz under NEEDED (zlib is looked up when a ZIP file is first used).
TABLE = {
    "mcrt_aov": _row(["aovRayKernel", "aovResolveKernel"], [("substring", "aov")]),
    "mcrt_denoise": _row(
        ["denoisePlainKernel", "denoisePrepKernel", "denoiseTileKernel"],
        # was the substring "denoise", searched in libmcrt_hip.so and libmcrt_aov.so only; over every library it can only speak of the
        # names that are not the variance-guided or the dual-buffer filter's (those libraries' own rows hold denoiseVar* and denoiseDual*)
        [("regex", r"(?i)denoise(?!var|dual)")],
        lds={"denoiseTileKernel": 13 * 20 * 20 * 8},  # the 16 x 16 tile with its halo, 13 doubles per record
        calls=("mcrt_denoise", "mcrt_denoise_device")),
    "mcrt_pixel_stats": _row(
        ["frameNoiseKernel", "pixelStatsKernel"], [("substring", "pixelstats"), ("substring", "framenoise")],
        lds={"frameNoiseKernel": 2 * 256 * 8},  # the two sums' blocks
        calls=("mcrt_render_pixel_stats", "mcrt_render_pixel_stats_device", "mcrt_frame_noise", "mcrt_frame_noise_device")),
    "mcrt_robust": _row(
        ["robustHighlightsKernel", "robustResolveKernel"], [("substring", "robust"), ("substring", "highlights")],
        lds={},  # the K-list of the highlights kernel stays in registers
        calls=("mcrt_render_highlights", "mcrt_render_highlights_device", "mcrt_robust_resolve", "mcrt_robust_resolve_device")),
    "mcrt_denoise_var": _row(
        ["denoiseVarPlainKernel", "denoiseVarPrepKernel", "denoiseVarTileKernel"], [("substring", "denoisevar")],
        # the 16 x 16 tile with its halo, 16 doubles per record: kDenoiseVarTileLdsBytes (tests/test_denoise_var_library.py asks the header)
        lds={"denoiseVarTileKernel": 16 * 20 * 20 * 8},
        calls=("mcrt_denoise_variance", "mcrt_denoise_variance_device")),
    "mcrt_accumulate": _row(
        ["frameMergeKernel"], [("substring", "framemerge"), ("substring", "accumulate")],
        lds={},  # the eight-entry merge of the highlights stays in registers
        calls=("mcrt_frame_merge", "mcrt_frame_merge_device", "mcrt_render_converged", "mcrt_render_converged_device"),
        attributes=("ConvergeParams", "ConvergeResult"), methods=("frame_merge",)),
    "mcrt_denoise_dual": _row(
        ["denoiseDualPlainKernel", "denoiseDualPrepKernel", "denoiseDualTileKernel"], [("substring", "denoisedual")],
        lds={},  # the tile kernel's is dynamic
        max_wg={"denoiseDualPlainKernel": 256, "denoiseDualPrepKernel": 256, "denoiseDualTileKernel": 1024},  # the tile form: up to 16 waves on one tile
        calls=("mcrt_denoise_dual", "mcrt_denoise_dual_device")),
    "mcrt_exr": _row(
        ["exrPackKernel"], [("substring", "exr")],
        skip={"libmcrt_exr_read.so": "the kernels of the OpenEXR input are named exrRead*: the substring cannot tell them from a pack kernel"},
        calls=("mcrt_exr_save", "mcrt_exr_save_device"), attributes=("ExrChannel", "ExrParams", "ExrResult", "exr_layers"), methods=("exr_save",),
        no_libz=True),
    "mcrt_matte": _row(
        ["matteRankKernel", "matteRankMemoryKernel"], [("substring", "matte")],
        calls=("mcrt_render_matte", "mcrt_render_matte_device", "mcrt_matte_rank_device", "mcrt_matte_code", "mcrt_matte_manifest"),
        attributes=("MatteParams", "MatteBuffers", "matte_code", "matte_manifest", "matte_attributes", "exr_layers"),
        methods=("render_matte", "render_matte_device", "matte_rank", "matte_rank_device")),
    "mcrt_compare": _row(
        ["compareLevelKernel", "comparePixelsKernel", "compareSsimKernel"], [("prefix", "compare"), ("substring", "ssim")],
        lds={"comparePixelsKernel": 2 * 3 * 256 * 8,                       # the two frames' words of a block; the tree reuses them
             "compareLevelKernel": 9 * 256 * 8,                            # four sums, the maximum's values and indices, three counts
             "compareSsimKernel": 2 * 42 * 26 * 8 + 5 * 26 * 32 * 8},      # (three workgroups per CU: tests/test_compare_library.py)
        calls=("mcrt_frame_compare", "mcrt_frame_compare_device"),
        attributes=("CompareParams", "CompareMaps", "CompareResult", "COMPARE_MAPS", "exr_layers"), methods=("frame_compare", "frame_compare_device")),
    "mcrt_occlusion": _row(
        ["occlusionRayKernel", "occlusionResolveKernel"], [("substring", "occlusion")],
        lds={"occlusionRayKernel": SOBOL_LDS},  # (the Sobol byte tables)
        calls=("mcrt_render_occlusion", "mcrt_render_occlusion_device"),
        attributes=("OcclusionParams", "OcclusionBuffers", "OCCLUSION_CHANNELS", "OCCLUSION_GEOMETRIC", "exr_layers"),
        methods=("render_occlusion", "render_occlusion_device")),
    "mcrt_lighting": _row(
        ["lightingRayKernel", "lightingResolveKernel"], [("names",)],  # whole names: robustHighlightsKernel contains "light"
        lds={"lightingRayKernel": SOBOL_LDS + 440 * 8, "lightingResolveKernel": SOBOL_LDS + 440 * 8},  # the Sobol byte tables and the sine / cosine table
        sgpr_spill_allowed=("lightingRayKernel", "lightingResolveKernel"), notes=("NOTES_lighting.md", r"lighting\w+Kernel"),
        calls=("mcrt_render_lighting", "mcrt_render_lighting_device"), attributes=("LightingBuffers", "LIGHTING_CHANNELS"),
        methods=("render_lighting", "render_lighting_device")),
    "mcrt_light_groups": _row(
        ["lightGroupsBeginKernel", "lightGroupsRayKernel", "lightGroupsResolveKernel", "lightGroupsStepKernel"], [("names",)],
        lds={"lightGroupsRayKernel": SHADING_LDS, "lightGroupsStepKernel": SHADING_LDS},
        sgpr_spill_allowed=("lightGroupsBeginKernel", "lightGroupsRayKernel", "lightGroupsResolveKernel", "lightGroupsStepKernel"),
        notes=("NOTES_light_groups.md", r"lightGroups\w+Kernel"),
        calls=("mcrt_render_light_groups", "mcrt_render_light_groups_device", "mcrt_light_group_planes"),
        attributes=("LightGroupParams", "LIGHT_GROUPS_MAX", "LIGHT_GROUPS_SKY_PLANE", "light_group_map"),
        methods=("render_light_groups", "render_light_groups_device")),
    "mcrt_path_classes": _row(
        ["pathClassesBeginKernel", "pathClassesRayKernel", "pathClassesResolveKernel", "pathClassesStepKernel"], [("names",)],
        lds={"pathClassesRayKernel": SHADING_LDS, "pathClassesStepKernel": SHADING_LDS},
        max_wg={k: 256 for k in ("pathClassesBeginKernel", "pathClassesRayKernel", "pathClassesResolveKernel", "pathClassesStepKernel")},
        sgpr_spill_allowed=("pathClassesBeginKernel", "pathClassesRayKernel", "pathClassesResolveKernel", "pathClassesStepKernel"),
        notes=("NOTES_path_classes.md", r"pathClasses\w+Kernel"),
        calls=("mcrt_render_path_classes", "mcrt_render_path_classes_device", "mcrt_path_class_planes"),
        attributes=("PathClassParams", "PATH_CLASSES", "PATH_CLASSES_MAP", "PATH_CLASS_NAMES", "path_class_map"),
        methods=("render_path_classes", "render_path_classes_device")),
    "mcrt_adaptive": _row(
        ["adaptiveBeginKernel", "adaptiveCameraRayKernel", "adaptiveCountKernel", "adaptiveFlagKernel", "adaptiveMergeKernel", "adaptiveRayKernel",
         "adaptiveResolveKernel", "adaptiveScanKernel", "adaptiveScatterKernel", "adaptiveStepKernel"], [("names",), ("prefix", "adaptive")],
        # the shading kernels as above; the camera rays the Sobol tables; the list's kernels four wave sums, the scan two rows of 256 lane sums
        lds={"adaptiveRayKernel": SHADING_LDS, "adaptiveStepKernel": SHADING_LDS, "adaptiveCameraRayKernel": SOBOL_LDS, "adaptiveCountKernel": 16,
             "adaptiveScatterKernel": 16, "adaptiveScanKernel": 2 * 256 * 4},
        max_wg={k: 256 for k in ("adaptiveBeginKernel", "adaptiveCameraRayKernel", "adaptiveCountKernel", "adaptiveFlagKernel", "adaptiveMergeKernel",
                                 "adaptiveRayKernel", "adaptiveResolveKernel", "adaptiveScanKernel", "adaptiveScatterKernel", "adaptiveStepKernel")},
        # the shading kernels only; the rule, the list, the camera rays, begin, resolve and merge: no spill of any kind
        sgpr_spill_allowed=("adaptiveRayKernel", "adaptiveStepKernel"), notes=("NOTES_adaptive.md", r"adaptive\w+Kernel"),
        calls=("mcrt_render_adaptive", "mcrt_render_adaptive_device", "mcrt_adaptive_list"),
        attributes=("AdaptiveParams", "AdaptiveResult", "ADAPTIVE_WINDOW_NONE"), methods=("render_adaptive", "render_adaptive_device", "adaptive_list")),
    "mcrt_exr_read": _row(
        ["exrReadGatherKernel", "exrReadScanKernel", "exrReadSumKernel", "exrReadUndoKernel"], [("prefix", "exrRead")],
        # a word per wave of the workgroup's scan; the gather's table of requested channels is dynamic LDS, sized per launch
        lds={"exrReadScanKernel": 256 // 64 * 4, "exrReadSumKernel": 256 // 64 * 4, "exrReadUndoKernel": 256 // 64 * 4},
        calls=("mcrt_exr_open", "mcrt_exr_close", "mcrt_exr_file_info", "mcrt_exr_file_channel", "mcrt_exr_file_attribute", "mcrt_exr_load", "mcrt_exr_load_device"),
        attributes=("ExrInfo", "ExrTarget", "ExrLoadParams", "ExrLoadResult", "exr_unlayer"), methods=("exr_load",), no_libz=True),
}
