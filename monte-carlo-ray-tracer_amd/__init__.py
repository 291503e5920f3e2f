"""Host-side Python binding of libmcrt_hip.so (the C ABI in include/mcrt.h).

The reference (linusmossberg/monte-carlo-ray-tracer) is a C++ program whose render seam is
``Camera::sampleImage()`` (source/camera/camera.cpp:101-145); the product is the HIP library behind
the C ABI, and the C++ host driver lives in ``host/``. This module is the thin ctypes layer the
tests and bench.py use to reach the same entry points; it contains no rendering logic and no CPU
fallback: if the shared library (built in-tree by ``build.py`` / ``__graft_entry__.build()``) is
missing, importing :func:`lib` raises.

Import with ``importlib.import_module("monte-carlo-ray-tracer_amd")`` (the directory name is not a
Python identifier).
"""
import ctypes as C
import math
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MCRT_TOLERANCE_BUILD=1 in the environment at import: the opt-in tolerance library (build.py LIB_TOL: FP64 contraction + the platform's
# libm; frames within BASELINE.json's 1e-4 relative bar instead of the reference's bits). Default: the exact library.
TOLERANCE_BUILD = os.environ.get("MCRT_TOLERANCE_BUILD") == "1"
LIB_PATH = os.path.join(_HERE, "csrc", "libmcrt_hip_tol.so" if TOLERANCE_BUILD else "libmcrt_hip.so")
ABI_VERSION = 2

FILM_FILTERS = {"box": 0, "mitchell-netravali": 1, "catmull-rom": 2, "b-spline": 3, "hermite": 4, "gaussian": 5, "lanczos": 6}
INTEGRATOR_PATH_TRACER = 0
INTEGRATOR_PHOTON_MAPPER = 1
LIBM_SINCOS, LIBM_SIN, LIBM_COS, LIBM_ASIN, LIBM_ATAN2, LIBM_SINCOSF, LIBM_POW = range(7)  # mcrt_libm function selectors (include/mcrt.h MCRT_LIBM_*)
# mcrt_stats.kernel_id (include/mcrt.h MCRT_KERNEL_*)
KERNEL_NONE, KERNEL_FLAT, KERNEL_WAVESYNC, KERNEL_LANE_SM, KERNEL_WAVEFRONT, KERNEL_PM_WAVE, KERNEL_PM_LANE, KERNEL_WAVEFRONT_PM = range(8)
KERNEL_NAMES = {KERNEL_NONE: "none", KERNEL_FLAT: "renderKernelFlatK (flat loop; renderKernel<path_tracer, flat> when the cull records do not fit the argument block)", KERNEL_WAVESYNC: "renderKernel<path_tracer>",
                KERNEL_LANE_SM: "renderKernelSM", KERNEL_WAVEFRONT: "wfTraceKernel + wfShadeKernel", KERNEL_PM_WAVE: "renderKernelPM",
                KERNEL_PM_LANE: "renderKernel<photon_mapper>", KERNEL_WAVEFRONT_PM: "wfTraceKernel + wfKnnKernel + wfShadeKernel"}
SURF_TRIANGLE, SURF_SPHERE = 0, 1
NO_SURFACE = 0xFFFFFFFF

_dp = C.POINTER(C.c_double)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)
_fp = C.POINTER(C.c_float)


class Material(C.Structure):
    """mcrt_material — one record per reference Material (material/material.hpp:9-55)."""
    _fields_ = [
        ("reflectance", C.c_double * 3), ("specular_reflectance", C.c_double * 3),
        ("transmittance", C.c_double * 3), ("emittance", C.c_double * 3),
        ("roughness", C.c_double), ("specular_roughness", C.c_double), ("ior", C.c_double),
        ("transparency", C.c_double), ("A", C.c_double), ("B", C.c_double), ("a", C.c_double * 2),
        ("ior_real", C.c_double * 3), ("ior_imag", C.c_double * 3),
        ("flags", C.c_uint32), ("reserved", C.c_uint32),
    ]


class SceneDesc(C.Structure):
    """mcrt_scene_desc."""
    _fields_ = [
        ("abi_version", C.c_uint32), ("num_nodes", C.c_uint32),
        ("node_bounds", _dp), ("node_start_surface", _u32p), ("node_num_surfaces", _u32p),
        ("node_next_sibling", _u32p),
        ("num_surfaces", C.c_uint32),
        ("surf_kind", _u8p), ("surf_interpolate", _u8p), ("surf_material", _u32p),
        ("surf_area", _dp), ("surf_v", _dp), ("surf_e", _dp), ("surf_vn", _dp),
        ("num_materials", C.c_uint32), ("materials", C.POINTER(Material)),
        ("num_lights", C.c_uint32), ("light_surface", _u32p), ("light_cdf", _dp),
        ("scene_ior", C.c_double), ("bb_min", C.c_double * 3), ("bb_max", C.c_double * 3),
        ("num_quadrics", C.c_uint32), ("quadrics", _dp),
    ]


class BvhDesc(C.Structure):
    """mcrt_bvh_desc."""
    _fields_ = [
        ("num_nodes", C.c_uint32), ("node_bounds", _dp), ("node_start_surface", _u32p), ("node_num_surfaces", _u32p),
        ("node_next_sibling", _u32p), ("num_surfaces", C.c_uint32), ("order", _u32p),
    ]


class PhotonMapDesc(C.Structure):
    """mcrt_photon_map_desc."""
    _fields_ = [
        ("num_octants", C.c_uint32), ("octant_bounds", _dp), ("octant_start_data", _u64p),
        ("octant_contained_data", _u64p), ("octant_next_sibling", _u32p), ("octant_leaf", _u8p),
        ("num_photons", C.c_uint64), ("photons", _fp),
    ]


class CameraDesc(C.Structure):
    """mcrt_camera_desc — the Camera fields read by samplePixel (camera/camera.cpp:66-99)."""
    _fields_ = [
        ("eye", C.c_double * 3), ("forward", C.c_double * 3), ("left", C.c_double * 3),
        ("up", C.c_double * 3),
        ("focal_length", C.c_double), ("sensor_width", C.c_double),
        ("aperture_radius", C.c_double), ("focus_distance", C.c_double),
        ("thin_lens", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("sqrtspp", C.c_uint32),
        ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("shard_rows", C.c_uint32),
        ("film_filter", C.c_uint32), ("film_radius", C.c_double), ("film_cache_size", C.c_uint32), ("reserved", C.c_uint32),
    ]

    def copy(self):
        c = CameraDesc()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(CameraDesc))
        return c


class Stats(C.Structure):
    """mcrt_stats."""
    _fields_ = [
        ("paths", C.c_uint64), ("rays", C.c_uint64), ("node_tests", C.c_uint64),
        ("prim_tests", C.c_uint64), ("knn_searches", C.c_uint64),
        ("kernel_ms", C.c_double), ("total_ms", C.c_double),
        ("kernel_launches", C.c_uint32), ("kernel_id", C.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


TONEMAP_HABLE, TONEMAP_ACES = 0, 1
TONEMAPPERS = {"HABLE": TONEMAP_HABLE, "ACES": TONEMAP_ACES}


class ImageDesc(C.Structure):
    """mcrt_image_desc — the camera's "image" object (camera/image.cpp:10-35)."""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("tonemapper", C.c_uint32), ("plain", C.c_uint32),
        ("exposure_compensation", C.c_double), ("gain_compensation", C.c_double),
    ]

    @classmethod
    def make(cls, width, height, tonemapper="HABLE", plain=False, exposure_compensation=0.0, gain_compensation=0.0):
        # image.cpp:25-34: the name is upper-cased; "ACES" selects filmicACES, anything else filmicHable
        tm = tonemapper if isinstance(tonemapper, int) else TONEMAPPERS.get(str(tonemapper).upper(), TONEMAP_HABLE)
        return cls(int(width), int(height), tm, int(bool(plain)), float(exposure_compensation), float(gain_compensation))


class PhotonEmission(C.Structure):
    """mcrt_photon_emission."""
    _fields_ = [
        ("global_count", C.c_uint64), ("caustic_count", C.c_uint64),
        ("global_photons", _fp), ("caustic_photons", _fp),
        ("global_keys", _u64p), ("caustic_keys", _u64p),
        ("emission_paths", C.c_uint64), ("rays", C.c_uint64), ("kernel_ms", C.c_double),
    ]


class PhotonPassStats(C.Structure):
    _fields_ = [("global_count", C.c_uint64), ("caustic_count", C.c_uint64), ("global_octants", C.c_uint64), ("caustic_octants", C.c_uint64),
                ("emission_paths", C.c_uint64), ("rays", C.c_uint64), ("emission_ms", C.c_double), ("sort_ms", C.c_double),
                ("octant_ms", C.c_double), ("finish_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AovBuffers(C.Structure):
    """mcrt_aov_buffers: one pointer per channel of the first-hit AOV pass, NULL = channel not wanted."""
    _fields_ = [("depth", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("shading_normal", C.c_void_p),
                ("albedo", C.c_void_p), ("coverage", C.c_void_p), ("surface", C.c_void_p), ("material", C.c_void_p)]


# channel -> (dtype, values per pixel), in mcrt_aov_buffers order
AOV_CHANNELS = {"depth": (np.float64, 1), "position": (np.float64, 3), "normal": (np.float64, 3), "shading_normal": (np.float64, 3),
                "albedo": (np.float64, 3), "coverage": (np.float64, 1), "surface": (np.uint32, 1), "material": (np.uint32, 1)}


class OcclusionParams(C.Structure):
    """mcrt_occlusion_params: rays per camera sample that hits (0 = 1), MCRT_OCCLUSION_* flags, max_distance (0 = unbounded)."""
    _fields_ = [("rays", C.c_uint32), ("flags", C.c_uint32), ("max_distance", C.c_double)]


class OcclusionBuffers(C.Structure):
    """mcrt_occlusion_buffers: one pointer per channel of the occlusion pass, NULL = channel not wanted."""
    _fields_ = [("ao", C.c_void_p), ("sky", C.c_void_p), ("bent_normal", C.c_void_p)]


OCCLUSION_GEOMETRIC = 1
OCCLUSION_MAX_RAYS = 64
# channel -> (dtype, values per pixel), in mcrt_occlusion_buffers order
OCCLUSION_CHANNELS = {"ao": (np.float64, 1), "sky": (np.float64, 1), "bent_normal": (np.float64, 3)}


class LightingBuffers(C.Structure):
    """mcrt_lighting_buffers: one pointer per channel of the lighting passes, NULL = channel not wanted."""
    _fields_ = [("emission", C.c_void_p), ("sky", C.c_void_p), ("direct", C.c_void_p), ("light", C.c_void_p), ("unoccluded", C.c_void_p)]


# channel -> (dtype, values per pixel), in mcrt_lighting_buffers order
LIGHTING_CHANNELS = {"emission": (np.float64, 3), "sky": (np.float64, 3), "direct": (np.float64, 3), "light": (np.float64, 3), "unoccluded": (np.float64, 3)}


class LightGroupParams(C.Structure):
    """mcrt_light_group_params: num_groups (0 = 1), MCRT_LIGHT_GROUPS_* flags, sky_plane (read with LIGHT_GROUPS_SKY_PLANE), max_depth
    (0 = the whole path), surface_group (host uint32 per surface, NULL = every emitter in group 0)."""
    _fields_ = [("num_groups", C.c_uint32), ("flags", C.c_uint32), ("sky_plane", C.c_uint32), ("max_depth", C.c_uint32), ("surface_group", C.c_void_p)]


LIGHT_GROUPS_MAX = 15
LIGHT_GROUPS_SKY_PLANE = 1
LIGHT_GROUPS_FILM = 2        # the planes through the camera's film (include/mcrt.h "Filtered planes")
LIGHT_GROUPS_FILM_CLAMP = 4  # with LIGHT_GROUPS_FILM: max(., 0) on every word
MAT_EMISSIVE = 1 << 3


def light_group_map(scene, by="material"):
    """surface_group and plane names for Context.render_light_groups from a scene descriptor (SceneDesc): -> (groups [num_surfaces]
    uint32, names). by="material": one group per emissive material, in the order of the materials, named "material%u" by the material's
    index; by="light": one group per emitter surface, in the order of the surfaces, named "light%u" by the surface's index; by="one":
    every emitter in group 0, named "lights". names ends with "sky", the plane the sky takes by default. More than LIGHT_GROUPS_MAX
    groups are a ValueError."""
    n = int(scene.num_surfaces)
    material = np.ctypeslib.as_array(scene.surf_material, shape=(n,)) if n else np.zeros(0, dtype=np.uint32)
    emissive = np.array([bool(scene.materials[i].flags & MAT_EMISSIVE) for i in range(int(scene.num_materials))], dtype=bool)
    emitter = emissive[material] if n else np.zeros(0, dtype=bool)
    groups = np.zeros(n, dtype=np.uint32)
    if by == "material":
        ids = [int(m) for m in np.nonzero(emissive)[0] if (material[emitter] == m).any()]
        for g, m in enumerate(ids):
            groups[emitter & (material == m)] = g
        names = ["material%u" % m for m in ids]
    elif by == "light":
        ids = [int(i) for i in np.nonzero(emitter)[0]]
        groups[ids] = np.arange(len(ids), dtype=np.uint32)
        names = ["light%u" % i for i in ids]
    elif by == "one":
        names = ["lights"]
    else:
        raise ValueError("light_group_map: by must be \"material\", \"light\" or \"one\", not %r" % (by,))
    if not names:
        names = ["lights"]  # (a scene without emitters: one empty group)
    if len(names) > LIGHT_GROUPS_MAX:
        raise ValueError("light_group_map: %d groups by %s, at most %d can be rendered" % (len(names), by, LIGHT_GROUPS_MAX))
    return groups, names + ["sky"]


class PathClassParams(C.Structure):
    """mcrt_path_class_params: MCRT_PATH_CLASSES_* flags, max_depth (0 = the whole path), class_plane (read with PATH_CLASSES_MAP: the
    output plane of each of the eight classes, in the order of PATH_CLASS_NAMES)."""
    _fields_ = [("flags", C.c_uint32), ("max_depth", C.c_uint32), ("class_plane", C.c_uint8 * 8)]


PATH_CLASSES = 8
PATH_CLASSES_MAP = 1
PATH_CLASSES_FILM = 2        # the planes through the camera's film (include/mcrt.h "Filtered planes")
PATH_CLASSES_FILM_CLAMP = 4  # with PATH_CLASSES_FILM: max(., 0) on every word
PATH_CLASS_NAMES = ("emission", "background", "diffuse_direct", "diffuse_indirect", "glossy_direct", "glossy_indirect", "transmission_direct",
                    "transmission_indirect")


def path_class_map(merge="all"):
    """class_plane and plane names for Context.render_path_classes: -> (class_plane [8] uint8, names). merge="all": the eight classes in
    planes of their own, named by PATH_CLASS_NAMES; "lobes": direct and indirect of a lobe in one plane - emission, background, diffuse,
    glossy, transmission; "one": everything in plane 0, named "beauty" (mcrt_render's frame bit for bit)."""
    if merge == "all":
        names = list(PATH_CLASS_NAMES)
    elif merge == "lobes":
        names = ["emission", "background", "diffuse", "glossy", "transmission"]
    elif merge == "one":
        names = ["beauty"]
    else:
        raise ValueError("path_class_map: merge must be \"all\", \"lobes\" or \"one\", not %r" % (merge,))
    plane = {"all": lambda c: c, "lobes": lambda c: c if c < 2 else 2 + (c - 2) // 2, "one": lambda c: 0}[merge]
    return np.array([plane(c) for c in range(PATH_CLASSES)], dtype=np.uint8), names


class LensDesc(C.Structure):
    """mcrt_lens_desc: model (LENS_*), flags (0), width_world (ORTHOGRAPHIC), fov_x and fov_y in radians (0 = the model's default),
    reserved (0). include/mcrt.h "Camera models" defines every model operation by operation."""
    _fields_ = [("model", C.c_uint32), ("flags", C.c_uint32), ("width_world", C.c_double), ("fov_x", C.c_double), ("fov_y", C.c_double),
                ("reserved", C.c_double * 3)]

    def as_dict(self):
        return {"model": LENS_NAMES.get(int(self.model), int(self.model)), "width_world": self.width_world, "fov_x": self.fov_x, "fov_y": self.fov_y}


LENS_NONE, LENS_PERSPECTIVE, LENS_ORTHOGRAPHIC, LENS_EQUIRECTANGULAR, LENS_FISHEYE = range(5)
LENS_NAMES = {LENS_NONE: "none", LENS_PERSPECTIVE: "perspective", LENS_ORTHOGRAPHIC: "orthographic", LENS_EQUIRECTANGULAR: "equirectangular",
              LENS_FISHEYE: "fisheye"}


def lens(model, width_world=0.0, fov_x=0.0, fov_y=0.0):
    """A LensDesc for Context.set_lens. model: a LENS_* number or its name ("orthographic", "equirectangular", "fisheye", "perspective",
    "none"); width_world: the orthographic frame's width in world units; fov_x, fov_y: radians, 0 = the model's default (equirectangular
    2 pi by pi; fisheye fov_x = the full angle, pi)."""
    if isinstance(model, str):
        by_name = {v: k for k, v in LENS_NAMES.items()}
        if model not in by_name:
            raise ValueError("lens: model must be one of %s, not %r" % (", ".join(sorted(by_name)), model))
        model = by_name[model]
    return LensDesc(int(model), 0, float(width_world), float(fov_x), float(fov_y))


class RaySourceDesc(C.Structure):
    """mcrt_ray_source_desc: kind (RAY_SOURCE_*), flags (RAY_SOURCE_PER_PIXEL), pixels (packed pixels the arrays were made for), spp
    (RAYS with per-sample arrays), first / second (device pointers: start / direction or position / normal), offset (SURFACE),
    reserved (0). include/mcrt.h "Ray sources" defines both kinds operation by operation."""
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("pixels", C.c_uint64), ("spp", C.c_uint32), ("reserved0", C.c_uint32),
                ("first", C.c_void_p), ("second", C.c_void_p), ("offset", C.c_double), ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        return {"kind": RAY_SOURCE_NAMES.get(int(self.kind), int(self.kind)), "per_pixel": bool(self.flags & RAY_SOURCE_PER_PIXEL), "pixels": int(self.pixels),
                "spp": int(self.spp), "first": self.first or 0, "second": self.second or 0, "offset": self.offset}


RAY_SOURCE_NONE, RAY_SOURCE_RAYS, RAY_SOURCE_SURFACE = range(3)
RAY_SOURCE_PER_PIXEL = 1
RAY_SOURCE_NAMES = {RAY_SOURCE_NONE: "none", RAY_SOURCE_RAYS: "rays", RAY_SOURCE_SURFACE: "surface"}
RAY_SOURCE_DEFAULT_OFFSET = 1e-9  # kEpsilon of csrc/mcrt_math.hpp


class ProbeParams(C.Structure):
    """mcrt_probe_params: groups (a LightGroupParams, as in render_light_groups), order (L = 0, 1, 2: K = (L + 1)^2 coefficients), flags
    (0), positions (pointer to [pixels][3] doubles or NULL: the context's camera, lens or ray source), weight (pointer to [spp][pixels]
    doubles or NULL), reserved (0). include/mcrt.h "Light probes" defines the call operation by operation."""
    _fields_ = [("groups", LightGroupParams), ("order", C.c_uint32), ("flags", C.c_uint32), ("positions", C.c_void_p), ("weight", C.c_void_p),
                ("reserved", C.c_uint64 * 2)]


PROBE_ORDER_MAX = 2
# MCRT_PROBE_SH_N*: Y_k = PROBE_SH_NORM[k] * b_k, the real spherical harmonics over the un-normalised basis the probe calls project on
PROBE_SH_NORM = np.array([0.5 * math.sqrt(1.0 / math.pi)] + [0.5 * math.sqrt(3.0 / math.pi)] * 3 +
                         [0.5 * math.sqrt(15.0 / math.pi), 0.5 * math.sqrt(15.0 / math.pi), 0.25 * math.sqrt(5.0 / math.pi), 0.5 * math.sqrt(15.0 / math.pi),
                          0.25 * math.sqrt(15.0 / math.pi)])
PROBE_SH_BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])                      # l of coefficient k
PROBE_IRRADIANCE_BAND = np.array([math.pi, 2.0 * math.pi / 3.0, math.pi / 4.0])  # A_l: the clamped cosine's zonal factors


def probe_basis(directions):
    """The un-normalised basis b_0 .. b_8 of unit directions [..., 3] -> [9, ...] (include/mcrt.h "Light probes")."""
    d = np.asarray(directions, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.ones_like(x), y, z, x, x * y, y * z, 3.0 * (z * z) - 1.0, x * z, (x * x) - (y * y)])


def probe_sh(coefficients):
    """The raw coefficients of render_probes / bake_probes, [..., K, H, W, 3] (K = 1, 4 or 9), as coefficients L_lm of the real
    spherical harmonics: times 4 pi N_k - the mean over uniform directions estimates the integral over the sphere divided by 4 pi."""
    c = np.asarray(coefficients, dtype=np.float64)
    k = c.shape[-4]
    if k not in (1, 4, 9):
        raise ValueError("probe_sh: [..., K, H, W, 3] with K = 1, 4 or 9, not %r" % (c.shape,))
    return c * (4.0 * math.pi * PROBE_SH_NORM[:k])[:, None, None, None]


def probe_irradiance(sh, normals):
    """The irradiance at unit normals [H, W, 3] from probe_sh's coefficients [..., K, H, W, 3] -> [..., H, W, 3]:
    sum_k A_l(k) L_k Y_k(n) with A = pi, 2 pi / 3, pi / 4 (bands past the order given are taken as zero)."""
    sh = np.asarray(sh, dtype=np.float64)
    k = sh.shape[-4]
    y = probe_basis(normals)[:k] * PROBE_SH_NORM[:k, None, None]            # [K, H, W]
    factor = PROBE_IRRADIANCE_BAND[PROBE_SH_BAND[:k]][:, None, None] * y    # [K, H, W]
    return (sh * factor[..., None]).sum(axis=-4)


class DenoiseParams(C.Structure):
    """mcrt_denoise_params: a zero field = the default (include/mcrt.h)."""
    _fields_ = [("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_color", C.c_double), ("sigma_plane", C.c_double),
                ("albedo_floor", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


DENOISE_NO_ALBEDO = 1
# the guide channels mcrt_denoise reads (albedo not with DENOISE_NO_ALBEDO)
DENOISE_GUIDES = ("shading_normal", "normal", "position", "coverage", "albedo")


class DenoiseVarianceParams(C.Structure):
    """mcrt_denoise_variance_params: a zero field = the default (include/mcrt.h)."""
    _fields_ = [("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_variance", C.c_double), ("sigma_floor", C.c_double),
                ("sigma_plane", C.c_double), ("albedo_floor", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class DenoiseDualParams(C.Structure):
    """mcrt_denoise_dual_params: a zero field = the default (include/mcrt.h)."""
    _fields_ = [("window_radius", C.c_uint32), ("patch_radius", C.c_uint32), ("k", C.c_double), ("alpha", C.c_double), ("epsilon", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class DenoiseDualBuffers(C.Structure):
    """mcrt_denoise_dual_buffers: a null pointer = not wanted (rgb is required)."""
    _fields_ = [("rgb", C.c_void_p), ("variance", C.c_void_p), ("half_a", C.c_void_p), ("half_b", C.c_void_p)]


DENOISE_DUAL_OUTPUTS = tuple(k for k, _ in DenoiseDualBuffers._fields_)
ROBUST_TOPS = 4
# The per-sample summary of a render: channel -> the shape of a pixel, in mcrt_frame_summary order (csrc/mcrt_summary_channels.hpp is the
# same table for the library); mcrt_pixel_stats_buffers is its members 1..3, mcrt_highlight_buffers its members 4..5.
FRAME_SUMMARY_CHANNELS = {"rgb": (3,), "variance": (3,), "half_a": (3,), "half_b": (3,), "tops": (ROBUST_TOPS, 3), "level": ()}
PIXEL_STATS_CHANNELS = tuple(FRAME_SUMMARY_CHANNELS)[1:4]
HIGHLIGHT_CHANNELS = {k: FRAME_SUMMARY_CHANNELS[k] for k in tuple(FRAME_SUMMARY_CHANNELS)[4:6]}


class PixelStatsBuffers(C.Structure):
    """mcrt_pixel_stats_buffers: a null pointer = channel not wanted."""
    _fields_ = [("variance", C.c_void_p), ("half_a", C.c_void_p), ("half_b", C.c_void_p)]


class FrameNoise(C.Structure):
    """mcrt_frame_noise_result."""
    _fields_ = [("noise", C.c_double), ("signal", C.c_double), ("relative_error", C.c_double), ("pixels", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# Frame comparison (include/mcrt.h "Frame comparison")
COMPARE_MAPS = ("squared_error", "relative", "ssim")
COMPARE_ERROR_CHANNELS = {"squared_error": "se", "relative": "rel", "ssim": "ssim"}  # exr_layers(errors=): error.se, error.rel, error.ssim


class CompareParams(C.Structure):
    """mcrt_compare_params: a zero double = the default; want_ssim is taken as it is."""
    _fields_ = [("eps", C.c_double), ("peak", C.c_double), ("ssim_range", C.c_double), ("want_ssim", C.c_int32), ("reserved", C.c_uint32)]


class CompareMaps(C.Structure):
    """mcrt_compare_maps: a null pointer = not wanted."""
    _fields_ = [("squared_error", C.c_void_p), ("relative", C.c_void_p), ("ssim", C.c_void_p)]


class CompareResult(C.Structure):
    """mcrt_compare_result."""
    _fields_ = ([(k, C.c_double) for k in ("sum_se", "sum_ae", "sum_rel", "sum_ssim", "max_abs")] + [("max_abs_pixel", C.c_uint64), ("max_abs_channel", C.c_uint32),
                ("reserved", C.c_uint32)] + [(k, C.c_uint64) for k in ("pixels", "compared", "nonfinite", "masked", "differing", "ssim_centres", "ssim_excluded")] +
                [(k, C.c_double) for k in ("mse", "mae", "relmse", "rmse", "psnr", "mean_ssim")])

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class HighlightBuffers(C.Structure):
    """mcrt_highlight_buffers: a null pointer = channel not wanted."""
    _fields_ = [("tops", C.c_void_p), ("level", C.c_void_p)]


class RobustParams(C.Structure):
    """mcrt_robust_params: a zero field = the default (include/mcrt.h)."""
    _fields_ = [("kappa", C.c_double), ("floor", C.c_double), ("radius", C.c_uint32), ("reserved", C.c_uint32)]


class RobustBuffers(C.Structure):
    """mcrt_robust_buffers: a null pointer = not wanted."""
    _fields_ = [("removed", C.c_void_p), ("clamped", C.c_void_p)]


class FrameSummary(C.Structure):
    """mcrt_frame_summary: a null pointer = channel not given / not wanted."""
    _fields_ = [("rgb", C.c_void_p), ("variance", C.c_void_p), ("half_a", C.c_void_p), ("half_b", C.c_void_p), ("tops", C.c_void_p), ("level", C.c_void_p)]


def _summary_arrays(names, lead, out=None, allowed=FRAME_SUMMARY_CHANNELS):
    """The arrays of the summary channels `names` ("rgb" always allowed) for frames of the leading shape `lead`, from the dict `out` where
    it holds them, otherwise fresh zeros -> dict channel -> array."""
    res = {}
    for name in names:
        assert name == "rgb" or name in allowed, name
        shape = tuple(lead) + FRAME_SUMMARY_CHANNELS[name]
        a = out[name] if out is not None and name in out else np.zeros(shape, dtype=np.float64)
        assert a.dtype == np.float64 and a.shape == shape and a.flags["C_CONTIGUOUS"], name
        res[name] = a
    return res


def _addresses(struct, arrays):
    """The FrameSummary, PixelStatsBuffers or HighlightBuffers of the arrays that are channels of it."""
    return struct(**{k: arrays[k].ctypes.data for k, _ in struct._fields_ if k in arrays})


# the groups that mcrt_frame_merge takes or leaves as a whole
FRAME_SUMMARY_GROUPS = tuple(tuple(FRAME_SUMMARY_CHANNELS)[i:i + 2] for i in (0, 2, 4))
CONVERGE_TRACE = 64


class ConvergeParams(C.Structure):
    """mcrt_converge_params: a zero field = the default (include/mcrt.h)."""
    _fields_ = [("target_relative_error", C.c_double), ("max_spp", C.c_uint32), ("min_batches", C.c_uint32)]


class ConvergeResult(C.Structure):
    """mcrt_converge_result."""
    _fields_ = [("batches", C.c_uint32), ("spp", C.c_uint32), ("final", FrameNoise), ("relative_error", C.c_double * CONVERGE_TRACE)]

    def as_dict(self):
        return {"batches": self.batches, "spp": self.spp, "final": self.final.as_dict(),
                "relative_error": [self.relative_error[i] for i in range(min(self.batches, CONVERGE_TRACE))]}


# Adaptive sampling (include/mcrt.h "Adaptive sampling")
ADAPTIVE_WINDOW_NONE = 0xFFFFFFFF


class AdaptiveParams(C.Structure):
    """mcrt_adaptive_params: a zero field = the default (include/mcrt.h); window ADAPTIVE_WINDOW_NONE = radius 0."""
    _fields_ = [("target_relative_error", C.c_double), ("floor", C.c_double), ("max_spp", C.c_uint32), ("min_batches", C.c_uint32), ("window", C.c_uint32)]


class AdaptiveResult(C.Structure):
    """mcrt_adaptive_result."""
    _fields_ = [("batches", C.c_uint32), ("min_count", C.c_uint32), ("max_count", C.c_uint32), ("samples", C.c_uint64), ("active", C.c_uint32 * CONVERGE_TRACE)]

    def as_dict(self):
        return {"batches": self.batches, "min_count": self.min_count, "max_count": self.max_count, "samples": self.samples,
                "active": [self.active[i] for i in range(min(self.batches, CONVERGE_TRACE))]}


# OpenEXR output (include/mcrt.h "OpenEXR output")
EXR_SRC_F64, EXR_SRC_U32 = 0, 1
EXR_PIXEL_TYPES = {"uint": 0, "half": 1, "float": 2}
EXR_COMPRESSION = {"none": 0x100 | 0, "zip": 0x100 | 3}  # MCRT_EXR_COMPRESSION_SET | OpenEXR's number
EXR_HALF_INF = 1
EXR_LONG_NAMES = 2


class ExrChannel(C.Structure):
    """mcrt_exr_channel: a strided view of a frame under a name."""
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("source_type", C.c_uint32), ("pixel_type", C.c_uint32), ("stride", C.c_uint32), ("offset", C.c_uint32)]


class ExrAttribute(C.Structure):
    """mcrt_exr_attribute: written as type "string"."""
    _fields_ = [("name", C.c_char_p), ("value", C.c_char_p)]


class ExrParams(C.Structure):
    """mcrt_exr_params: a zero field = the default (include/mcrt.h)."""
    _fields_ = [("compression", C.c_uint32), ("zip_level", C.c_uint32), ("threads", C.c_uint32), ("flags", C.c_uint32)]


class ExrResult(C.Structure):
    """mcrt_exr_result."""
    _fields_ = [("file_bytes", C.c_uint64), ("packed_bytes", C.c_uint64), ("chunks", C.c_uint32), ("raw_chunks", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# OpenEXR input (include/mcrt.h "OpenEXR input")
EXR_PIXEL_TYPE_NAMES = {v: k for k, v in EXR_PIXEL_TYPES.items()}


class ExrInfo(C.Structure):
    """mcrt_exr_info."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("data_window", C.c_int32 * 4), ("display_window", C.c_int32 * 4), ("channels", C.c_uint32),
                ("attributes", C.c_uint32), ("compression", C.c_uint32), ("line_order", C.c_uint32), ("lines_per_chunk", C.c_uint32), ("chunks", C.c_uint32),
                ("file_bytes", C.c_uint64)]


class ExrTarget(C.Structure):
    """mcrt_exr_target: where one channel of a file goes, a strided view of a destination."""
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dest_type", C.c_uint32), ("stride", C.c_uint32), ("offset", C.c_uint32), ("reserved", C.c_uint32)]


class ExrLoadParams(C.Structure):
    """mcrt_exr_load_params: a zero field = the default (include/mcrt.h)."""
    _fields_ = [("threads", C.c_uint32), ("flags", C.c_uint32)]


class ExrLoadResult(C.Structure):
    """mcrt_exr_load_result."""
    _fields_ = [("file_bytes", C.c_uint64), ("payload_bytes", C.c_uint64), ("chunks", C.c_uint32), ("raw_chunks", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _exr_attribute_value(typ, value, channels):
    """A header attribute's bytes as tools/exr_probe.py read() decodes them; types it does not know stay bytes."""
    if typ == "string":
        return value.decode("ascii", "replace")
    if typ == "float":
        return struct.unpack("<f", value)[0]
    if typ == "v2f":
        return struct.unpack("<2f", value)
    if typ == "box2i":
        return struct.unpack("<4i", value)
    if typ in ("compression", "lineOrder"):
        return value[0]
    if typ == "chlist":
        return [(n, t.upper()) for n, t in channels]
    return value


# ID mattes (include/mcrt.h "ID mattes")
MATTE_KEYS = {"material": 0, "surface": 1, "custom": 2}
MATTE_DEFAULT_NAMES = {"material": "material%u", "surface": "surface%u", "custom": "key%u"}
MATTE_DEFAULT_RANKS, MATTE_MAX_RANKS = 6, 16
MATTE_CHANNELS = {"id": (np.uint32, ("ranks",)), "coverage": (np.float64, ("ranks",)), "layer": (np.float64, ("ranks", 2)), "distinct": (np.uint32, ())}
NO_KEY = 0xFFFFFFFF


class MatteParams(C.Structure):
    """mcrt_matte_params: a zero field = the default (include/mcrt.h)."""
    _fields_ = [("key", C.c_uint32), ("ranks", C.c_uint32), ("num_keys", C.c_uint32), ("surface_key", C.c_void_p), ("names", C.POINTER(C.c_char_p)),
                ("reserved", C.c_uint64)]


class MatteBuffers(C.Structure):
    """mcrt_matte_buffers: every pointer may be NULL = not wanted."""
    _fields_ = [("id", C.c_void_p), ("coverage", C.c_void_p), ("layer", C.c_void_p), ("distinct", C.c_void_p)]


def matte_code(name):
    """mcrt_matte_code: the Cryptomatte code of a name (str or bytes)."""
    return int(lib().mcrt_matte_code(name if isinstance(name, bytes) else str(name).encode("ascii")))


def _matte_params(key, ranks, names, surface_key, num_keys):
    """(MatteParams, what it points into) of render_matte's arguments. num_keys only matters for key "custom"."""
    par, keep = MatteParams(MATTE_KEYS[key], int(ranks), 0, None, None, 0), []
    if surface_key is not None:
        sk = np.ascontiguousarray(surface_key, dtype=np.uint32)
        keep.append(sk)
        par.surface_key = sk.ctypes.data
    if names is not None:
        arr = (C.c_char_p * max(len(names), 1))(*[n if isinstance(n, bytes) else str(n).encode("latin-1") for n in names])
        keep.append(arr)
        par.names = arr
    if key == "custom":
        par.num_keys = int(num_keys) if num_keys is not None else len(names) if names is not None else int(np.max(surface_key)) + 1
    return par, keep


def matte_manifest(key="material", num_keys=0, names=None):
    """mcrt_matte_manifest: the JSON text {"name":"%08x",...} of the num_keys names (names, or the defaults of `key`) in key order."""
    par, keep = _matte_params(key, 0, names, None, num_keys)
    n = len(names) if names is not None else int(num_keys)
    need = lib().mcrt_matte_manifest(C.byref(par), n, None, 0)
    if need < 0:
        raise McrtError("mcrt_matte_manifest failed (%d): a name is not 1 .. 255 bytes of printable ASCII" % need)
    buf = C.create_string_buffer(need)
    assert lib().mcrt_matte_manifest(C.byref(par), n, buf, need) == need
    return buf.value.decode("ascii")


def matte_attributes(layer_name, result):
    """The string attributes that make the channels exr_layers(mattes={layer_name: result}) writes a Cryptomatte layer: cryptomatte/<K>/name,
    /hash, /conversion and /manifest, <K> the first 7 of the 8 hex digits of matte_code(layer_name) (readers match on /name; the key only
    has to be unique). result: render_matte's dict (its "manifest")."""
    k = "cryptomatte/%s/" % ("%08x" % matte_code(layer_name))[:7]
    return {k + "name": layer_name, k + "hash": "MurmurHash3_32", k + "conversion": "uint32_to_float32", k + "manifest": result["manifest"]}


def _is_tensor(a):
    return hasattr(a, "data_ptr") and hasattr(a, "storage_offset")


def _exr_source(a):
    """A frame view [H,W] of float64 or (u)int32 elements, numpy or torch -> (the array to keep alive, base pointer, source type, stride,
    offset) with element (pixel p) = base[p * stride + offset]. A last-axis view of a packed [H,W,k] buffer keeps the buffer's pointer,
    so that its k channels name one source; a view that is no such thing is copied."""
    tensor = _is_tensor(a)
    if not tensor:
        a = np.asarray(a)
    assert a.ndim == 2, "a channel is a [H,W] view, not %r" % (tuple(a.shape),)
    kind = str(a.dtype).replace("torch.", "")
    assert kind in ("float64", "uint32", "int32"), "a channel is float64 or uint32, not %s" % kind
    item = 8 if kind == "float64" else 4
    height, width = int(a.shape[0]), int(a.shape[1])
    strides = [int(x) for x in a.stride()] if tensor else [int(x) // item if int(x) % item == 0 else -1 for x in a.strides]
    step = strides[1] if width > 1 else (strides[0] if height > 1 else 1)
    packed = step >= 1 and step < (1 << 32) and (height == 1 or width == 1 or strides[0] == width * step)
    if not packed:
        a = a.contiguous() if tensor else np.ascontiguousarray(a)
        step = 1
    if tensor:
        ptr, first = int(a.data_ptr()), int(a.storage_offset())
    else:
        root = a
        while isinstance(root.base, np.ndarray):
            root = root.base
        ptr = int(a.ctypes.data)
        first = (ptr - int(root.ctypes.data)) // item if step > 1 else 0
    offset = first % step
    return a, ptr - offset * item, EXR_SRC_F64 if kind == "float64" else EXR_SRC_U32, step, offset


_EXR_FLOAT_LAYERS = ("depth", "position", "variance", "error", "level")


def exr_layers(rgb=None, aov=None, stats=None, highlights=None, robust=None, denoised=None, pixel_types=None, mattes=None, errors=None, occlusion=None, lighting=None, light_groups=None, path_classes=None, adaptive=None):
    """The channel dict Context.exr_save takes, from what the render_* and denoise_* methods return, under fixed names:
      rgb [H,W,3]                       R, G, B
      aov (render_aov's dict)           depth.Z, position.X/Y/Z, normal.X/Y/Z, shading_normal.X/Y/Z, albedo.R/G/B, coverage.A, surface.id, material.id
      stats (render_pixel_stats')       variance.R/G/B, half_a.R/G/B, half_b.R/G/B          (its "rgb" is not taken: pass it as rgb)
      highlights (render_highlights')   tops0.R .. tops3.B, level.Y
      robust (robust_resolve's)         robust.R/G/B, removed.R/G/B, clamped.count
      denoised {name: frame | (frame, variance) | dict with "rgb" and "variance" / "error"}   name.R/G/B, name.variance.R/G/B, name.error.R/G/B
      mattes {name: render_matte's dict}  name00.R/G/B/A, name01.R/G/B/A, ...: views of its "layer" [H,W,ranks,2] - (id, coverage) of
                                        ranks 2 l and 2 l + 1 -, always FLOAT whatever pixel_types says (HALF would destroy the ids);
                                        matte_attributes gives the attributes that go with them
      errors (frame_compare's maps)     error.se, error.rel, error.ssim: "squared_error", "relative", "ssim" [H,W] of the dict (those
                                        that are there), always FLOAT
      occlusion (render_occlusion's)    occlusion.ao, occlusion.sky, occlusion.bent.X/Y/Z (those that are there): HALF like the AOV
                                        pass's coverage and normals
      lighting (render_lighting's)      lighting.emission.R/G/B, lighting.sky.R/G/B, lighting.direct.R/G/B, lighting.light.R/G/B,
                                        lighting.unoccluded.R/G/B (those that are there): colour, HALF
      light_groups (planes, names)      lightgroup.<name>.R/G/B for every plane of render_light_groups' [P,H,W,3] and its name
                                        (light_group_map's): colour, HALF
      path_classes (planes, names)      pathclass.<name>.R/G/B for every plane of render_path_classes' [P,H,W,3] and its name
                                        (path_class_map's): colour, HALF
      adaptive (render_adaptive's)      samples.count (its "count" [H,W] uint32: UINT) and variance.R/G/B, half_a.R/G/B, half_b.R/G/B under
                                        the statistics' names (those that are there; its "rgb" is not taken: pass it as rgb)
    -> dict name -> (view [H,W], "half" | "float" | "uint"). Colour is HALF; depth, position, variance, error and level FLOAT; ids and
    counts UINT. pixel_types: {channel or layer name: type} overrides that (a layer is a name without its last component). The views
    are of the arrays and tensors given, numpy or torch alike: nothing is copied."""
    out = {}

    def put(layer, parts, frame, kind=None):
        if kind is None:
            kind = "float" if layer.split(".")[-1] in _EXR_FLOAT_LAYERS else "half"
        for i, part in enumerate(parts):
            name = part if layer == "" else "%s.%s" % (layer, part)
            view = frame if len(parts) == 1 and frame.ndim == 2 else frame[..., i]
            assert view.ndim == 2, (name, tuple(frame.shape))
            out[name] = (view, (pixel_types or {}).get(name, (pixel_types or {}).get(layer, kind)))

    if rgb is not None:
        put("", "RGB", rgb)
    for layer, parts in (("depth", "Z"), ("position", "XYZ"), ("normal", "XYZ"), ("shading_normal", "XYZ"), ("albedo", "RGB"), ("coverage", "A")):
        if aov is not None and aov.get(layer) is not None:
            put(layer, parts, aov[layer])
    for layer in ("surface", "material"):
        if aov is not None and aov.get(layer) is not None:
            put(layer, ("id",), aov[layer], "uint")
    for layer in PIXEL_STATS_CHANNELS:
        if stats is not None and stats.get(layer) is not None:
            put(layer, "RGB", stats[layer])
    if highlights is not None and highlights.get("tops") is not None:
        for k in range(ROBUST_TOPS):
            put("tops%d" % k, "RGB", highlights["tops"][:, :, k, :])
    if highlights is not None and highlights.get("level") is not None:
        put("level", "Y", highlights["level"])
    for layer in ("robust", "removed"):
        if robust is not None and robust.get(layer) is not None:
            put(layer, "RGB", robust[layer])
    if robust is not None and robust.get("clamped") is not None:
        put("clamped", ("count",), robust["clamped"], "uint")
    for name, value in (denoised or {}).items():
        if isinstance(value, dict):
            frames = {k: value[k] for k in ("rgb", "variance", "error") if value.get(k) is not None}
        elif isinstance(value, (tuple, list)):
            frames = {k: v for k, v in zip(("rgb", "variance"), value) if v is not None}
        else:
            frames = {"rgb": value}
        for k, frame in frames.items():
            put(name if k == "rgb" else "%s.%s" % (name, k), "RGB", frame)
    for name, result in (mattes or {}).items():
        layer = result["layer"]
        assert layer.ndim == 4 and layer.shape[3] == 2 and layer.shape[2] % 2 == 0, tuple(layer.shape)
        flat = layer.reshape(layer.shape[0], layer.shape[1], 2 * layer.shape[2])
        for i in range(flat.shape[2]):
            out["%s%02d.%s" % (name, i // 4, "RGBA"[i % 4])] = (flat[..., i], "float")
    for key, part in COMPARE_ERROR_CHANNELS.items():
        if errors is not None and errors.get(key) is not None:
            assert errors[key].ndim == 2, (key, tuple(errors[key].shape))
            out["error." + part] = (errors[key], "float")
    for key in ("ao", "sky"):
        if occlusion is not None and occlusion.get(key) is not None:
            put("occlusion", (key,), occlusion[key])
    if occlusion is not None and occlusion.get("bent_normal") is not None:
        put("occlusion.bent", "XYZ", occlusion["bent_normal"])
    for key in LIGHTING_CHANNELS:
        if lighting is not None and lighting.get(key) is not None:
            put("lighting." + key, "RGB", lighting[key])
    if light_groups is not None:
        planes, names = light_groups
        assert len(planes) == len(names) and len(set(names)) == len(names), (len(planes), names)
        for plane, name in zip(planes, names):
            put("lightgroup." + name, "RGB", plane)
    if path_classes is not None:
        planes, names = path_classes
        assert len(planes) == len(names) and len(set(names)) == len(names), (len(planes), names)
        for plane, name in zip(planes, names):
            put("pathclass." + name, "RGB", plane)
    if adaptive is not None:
        assert stats is None, "adaptive and stats name the same channels"
        if adaptive.get("count") is not None:
            put("samples", ("count",), adaptive["count"], "uint")
        for layer in PIXEL_STATS_CHANNELS:
            if adaptive.get(layer) is not None:
                put(layer, "RGB", adaptive[layer])
    return out


def exr_unlayer(channels):
    """The inverse of exr_layers: from a dict name -> frame [H,W] (Context.exr_load's, numpy arrays or torch tensors) the keyword dict
    exr_layers takes, for the names documented there - rgb [H,W,3]; aov with its [H,W,3] and [H,W] members; stats; highlights with tops
    [H,W,4,3] and level; robust; denoised {name: {"rgb", "variance", "error"}} for every other layer that has R, G and B but no A (R, G,
    B, A are a matte's layer); occlusion with ao, sky and bent_normal [H,W,3]; lighting with its [H,W,3] channels; light_groups (planes [P,H,W,3], names) from the lightgroup.<name> layers; path_classes likewise from the pathclass.<name> layers; errors. A layer is taken when all its parts are there; every other name comes back under "other".
    Frames are stacked where they live."""
    left = dict(channels)

    def stack(frames, axis=-1):
        if _is_tensor(frames[0]):
            import torch
            return torch.stack(list(frames), dim=axis)
        return np.stack(frames, axis=axis)

    def take(layer, parts):
        names = [part if layer == "" else "%s.%s" % (layer, part) for part in parts]
        if not all(n in left for n in names):
            return None
        frames = [left.pop(n) for n in names]
        return frames[0] if len(frames) == 1 else stack(frames)

    out = {}
    rgb = take("", "RGB")
    if rgb is not None:
        out["rgb"] = rgb
    groups = {"aov": [(l, p) for l, p in (("depth", "Z"), ("position", "XYZ"), ("normal", "XYZ"), ("shading_normal", "XYZ"), ("albedo", "RGB"), ("coverage", "A"),
                                          ("surface", ("id",)), ("material", ("id",)))],
              "stats": [(l, "RGB") for l in PIXEL_STATS_CHANNELS],
              "robust": [("robust", "RGB"), ("removed", "RGB"), ("clamped", ("count",))]}
    for key, layers in groups.items():
        found = {}
        for layer, parts in layers:
            frame = take(layer, parts)
            if frame is not None:
                found[layer] = frame
        if found:
            out[key] = found
    highlights = {}
    tops = [take("tops%d" % k, "RGB") if all("tops%d.%s" % (j, c) in channels for j in range(ROBUST_TOPS) for c in "RGB") else None for k in range(ROBUST_TOPS)]
    if all(t is not None for t in tops):
        highlights["tops"] = stack(tops, axis=2)
    level = take("level", "Y")
    if level is not None:
        highlights["level"] = level
    if highlights:
        out["highlights"] = highlights
    occlusion = {}
    for key, layer, parts in (("ao", "occlusion", ("ao",)), ("sky", "occlusion", ("sky",)), ("bent_normal", "occlusion.bent", "XYZ")):
        frame = take(layer, parts)
        if frame is not None:
            occlusion[key] = frame
    if occlusion:
        out["occlusion"] = occlusion
    lighting = {}
    for key in LIGHTING_CHANNELS:
        frame = take("lighting." + key, "RGB")
        if frame is not None:
            lighting[key] = frame
    if lighting:
        out["lighting"] = lighting
    group_names = [n[len("lightgroup."):-2] for n in channels if n.startswith("lightgroup.") and n.endswith(".R")]
    group_planes = [(name, take("lightgroup." + name, "RGB")) for name in group_names]
    if any(frame is not None for _, frame in group_planes):
        out["light_groups"] = (stack([frame for _, frame in group_planes if frame is not None], axis=0), [name for name, frame in group_planes if frame is not None])
    class_names = [n[len("pathclass."):-2] for n in channels if n.startswith("pathclass.") and n.endswith(".R")]
    class_planes = [(name, take("pathclass." + name, "RGB")) for name in class_names]
    if any(frame is not None for _, frame in class_planes):
        out["path_classes"] = (stack([frame for _, frame in class_planes if frame is not None], axis=0), [name for name, frame in class_planes if frame is not None])
    errors = {}
    for key, part in COMPARE_ERROR_CHANNELS.items():
        frame = take("error", (part,))
        if frame is not None:
            errors[key] = frame
    if errors:
        out["errors"] = errors
    denoised = {}
    for name in [n[:-2] for n in channels if n.endswith(".R") and n in left]:
        if name.endswith((".variance", ".error")) or name + ".A" in left:  # (R, G, B, A: a matte's layer, not a frame)
            continue
        frame = take(name, "RGB")
        if frame is None:
            continue
        denoised[name] = {"rgb": frame}
        for k in ("variance", "error"):
            extra = take("%s.%s" % (name, k), "RGB")
            if extra is not None:
                denoised[name][k] = extra
    if denoised:
        out["denoised"] = denoised
    if left:
        out["other"] = left
    return out


class PhotonEmissionDevice(C.Structure):
    _fields_ = [("global_count", C.c_uint64), ("caustic_count", C.c_uint64), ("d_global_photons", C.c_void_p), ("d_caustic_photons", C.c_void_p),
                ("emission_paths", C.c_uint64), ("rays", C.c_uint64), ("kernel_ms", C.c_double)]


def render_multi(contexts, cam, global_seed, integrator=INTEGRATOR_PATH_TRACER):
    """mcrt_render_multi: one frame over several contexts (one per GPU, scene already uploaded), one host thread each ->
    (image[H,W,3] float64, stats dict)."""
    out = np.zeros((cam.height, cam.width, 3), dtype=np.float64)
    st = Stats()
    handles = (C.c_void_p * len(contexts))(*[c._h.value for c in contexts])
    rc = lib().mcrt_render_multi(handles, len(contexts), C.byref(cam), int(global_seed), int(integrator), _ptr(out, C.c_double), C.byref(st))
    contexts[0]._check(rc, "mcrt_render_multi")
    return out, st.as_dict()


def photon_pass_multi(contexts, emissions, caustic_factor, global_seed, bb_min, bb_max, max_photons_per_leaf=200, k_nearest=50,
                      direct_visualization=False):
    """mcrt_photon_pass_multi: the photon pass sharded over several contexts of this process (emission shards exchanged on device
    pointers, the same maps built in every context). Returns one stats dict per context."""
    for c in contexts:
        c._sync_env()
    st = (PhotonPassStats * len(contexts))()
    lo, hi = (C.c_double * 3)(*bb_min), (C.c_double * 3)(*bb_max)
    handles = (C.c_void_p * len(contexts))(*[c._h.value for c in contexts])
    rc = lib().mcrt_photon_pass_multi(handles, len(contexts), float(emissions), float(caustic_factor), int(global_seed), lo, hi,
                                      int(max_photons_per_leaf), int(k_nearest), 1 if direct_visualization else 0, st)
    contexts[0]._check(rc, "mcrt_photon_pass_multi")
    return [s.as_dict() for s in st]


def tga_save(path, bgr):
    """mcrt_tga_save: the reference's .tga (HeaderTGA + B,G,R bytes) for a [H,W,3] uint8 array."""
    bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
    rc = lib().mcrt_tga_save(os.fsencode(path), bgr.shape[1], bgr.shape[0], bgr.ctypes.data)
    if rc != 0:
        raise McrtError("mcrt_tga_save(%s) failed: %d" % (path, rc))


class McrtError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libmcrt_hip.so (fails loudly when the HIP extension has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise McrtError(
            "%s is missing: build it with `python __graft_entry__.py build` "
            "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.mcrt_abi_version.restype = C.c_uint32
    L.mcrt_create.argtypes = [C.POINTER(vp), C.c_int]
    if hasattr(L, "mcrt_device_count"):  # (absent from libraries older than round 5: tools/ab_builds.sh loads those too)
        L.mcrt_device_count.argtypes = []
        L.mcrt_device_count.restype = C.c_int
    L.mcrt_destroy.argtypes = [vp]
    L.mcrt_destroy.restype = None
    L.mcrt_last_error.argtypes = [vp]
    L.mcrt_last_error.restype = C.c_char_p
    L.mcrt_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.mcrt_get_option.argtypes = [vp, C.c_char_p]
    L.mcrt_get_option.restype = C.c_char_p
    L.mcrt_upload_scene.argtypes = [vp, C.POINTER(SceneDesc)]
    L.mcrt_upload_photons.argtypes = [vp, C.POINTER(PhotonMapDesc), C.POINTER(PhotonMapDesc),
                                      C.c_uint32, C.c_int]
    L.mcrt_render.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.c_int, _dp, C.POINTER(Stats)]
    L.mcrt_render_device.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.c_int, vp, vp]
    L.mcrt_render_finish.argtypes = [vp, C.POINTER(Stats)]
    L.mcrt_shard_rows.argtypes = [C.POINTER(CameraDesc), _u32p]
    L.mcrt_shard_rows.restype = C.c_uint32
    L.mcrt_emit_photons.argtypes = [vp, C.c_double, C.c_double, C.c_uint32, C.POINTER(PhotonEmission)]
    L.mcrt_emit_photons_shard.argtypes = [vp, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PhotonEmission)]
    L.mcrt_photon_pass_device.argtypes = [vp, C.c_double, C.c_double, C.c_uint32, _dp, _dp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(PhotonPassStats)]
    L.mcrt_emit_photons_device.argtypes = [vp, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PhotonEmissionDevice)]
    L.mcrt_upload_photons_device.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, _dp, _dp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(PhotonPassStats)]
    L.mcrt_photon_map_download.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.mcrt_intersect.argtypes = [vp, C.c_uint64, _dp, _dp, _dp, _u32p, _dp]
    if hasattr(L, "mcrt_render_aov"):  # (absent from older libraries that tools/ab_builds.sh swaps in)
        L.mcrt_intersect_device.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp]
        L.mcrt_render_aov.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(AovBuffers), C.POINTER(Stats)]
        L.mcrt_render_aov_device.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(AovBuffers), C.POINTER(Stats)]
    if hasattr(L, "mcrt_denoise"):  # (likewise)
        L.mcrt_denoise.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.POINTER(AovBuffers), C.POINTER(DenoiseParams), vp, C.POINTER(Stats)]
        L.mcrt_denoise_device.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.POINTER(AovBuffers), C.POINTER(DenoiseParams), vp, C.POINTER(Stats)]
    if hasattr(L, "mcrt_denoise_variance"):  # (likewise)
        L.mcrt_denoise_variance.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(AovBuffers), C.POINTER(DenoiseVarianceParams), vp, vp,
                                            C.POINTER(Stats)]
        L.mcrt_denoise_variance_device.argtypes = L.mcrt_denoise_variance.argtypes
    if hasattr(L, "mcrt_denoise_dual"):  # (likewise)
        L.mcrt_denoise_dual.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(DenoiseDualParams), C.POINTER(DenoiseDualBuffers),
                                        C.POINTER(Stats)]
        L.mcrt_denoise_dual_device.argtypes = L.mcrt_denoise_dual.argtypes
    if hasattr(L, "mcrt_render_pixel_stats"):  # (likewise)
        L.mcrt_render_pixel_stats.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.c_int, vp, C.POINTER(PixelStatsBuffers), C.POINTER(Stats)]
        L.mcrt_render_pixel_stats_device.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.c_int, vp, C.POINTER(PixelStatsBuffers), C.POINTER(Stats)]
        L.mcrt_frame_noise.argtypes = [vp, C.c_uint64, C.c_uint32, vp, vp, C.POINTER(FrameNoise)]
        L.mcrt_frame_noise_device.argtypes = [vp, C.c_uint64, C.c_uint32, vp, vp, C.POINTER(FrameNoise)]
    if hasattr(L, "mcrt_render_highlights"):  # (likewise)
        L.mcrt_render_highlights.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.c_int, vp, C.POINTER(HighlightBuffers), C.POINTER(PixelStatsBuffers), C.POINTER(Stats)]
        L.mcrt_render_highlights_device.argtypes = L.mcrt_render_highlights.argtypes
        L.mcrt_robust_resolve.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(RobustParams), vp, C.POINTER(RobustBuffers), C.POINTER(Stats)]
        L.mcrt_robust_resolve_device.argtypes = L.mcrt_robust_resolve.argtypes
    if hasattr(L, "mcrt_frame_merge"):  # (likewise)
        L.mcrt_frame_merge.argtypes = [vp, C.c_uint64, C.POINTER(FrameSummary), C.c_uint32, C.POINTER(FrameSummary), C.c_uint32, C.POINTER(FrameSummary), C.POINTER(Stats)]
        L.mcrt_frame_merge_device.argtypes = L.mcrt_frame_merge.argtypes
        L.mcrt_render_converged.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.c_int, C.POINTER(ConvergeParams), vp, C.POINTER(PixelStatsBuffers),
                                            C.POINTER(HighlightBuffers), C.POINTER(ConvergeResult), C.POINTER(Stats)]
        L.mcrt_render_converged_device.argtypes = L.mcrt_render_converged.argtypes
    if hasattr(L, "mcrt_render_adaptive"):  # (likewise)
        L.mcrt_render_adaptive.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(AdaptiveParams), vp, C.POINTER(PixelStatsBuffers), vp,
                                           C.POINTER(AdaptiveResult), C.POINTER(Stats)]
        L.mcrt_render_adaptive_device.argtypes = L.mcrt_render_adaptive.argtypes
        L.mcrt_adaptive_list.argtypes = [vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint32)]
    if hasattr(L, "mcrt_exr_save"):  # (likewise)
        L.mcrt_exr_save.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(ExrChannel), C.c_uint32, C.POINTER(ExrAttribute), C.c_uint32,
                                    C.POINTER(ExrParams), C.POINTER(ExrResult), C.POINTER(Stats)]
        L.mcrt_exr_save_device.argtypes = L.mcrt_exr_save.argtypes
    if hasattr(L, "mcrt_exr_open"):  # (likewise)
        L.mcrt_exr_open.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
        L.mcrt_exr_close.argtypes = [vp]
        L.mcrt_exr_close.restype = None
        L.mcrt_exr_file_info.argtypes = [vp, C.POINTER(ExrInfo)]
        L.mcrt_exr_file_channel.argtypes = [vp, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32)]
        L.mcrt_exr_file_attribute.argtypes = [vp, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(C.c_uint32)]
        L.mcrt_exr_load.argtypes = [vp, vp, C.POINTER(ExrTarget), C.c_uint32, C.POINTER(ExrLoadParams), C.POINTER(ExrLoadResult), C.POINTER(Stats)]
        L.mcrt_exr_load_device.argtypes = L.mcrt_exr_load.argtypes
    if hasattr(L, "mcrt_render_matte"):  # (likewise)
        L.mcrt_render_matte.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(MatteParams), C.POINTER(MatteBuffers), C.POINTER(AovBuffers), C.POINTER(Stats)]
        L.mcrt_render_matte_device.argtypes = L.mcrt_render_matte.argtypes
        L.mcrt_matte_rank_device.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(MatteBuffers), C.POINTER(Stats)]
        L.mcrt_matte_code.argtypes = [C.c_char_p]
        L.mcrt_matte_code.restype = C.c_uint32
        L.mcrt_matte_manifest.argtypes = [C.POINTER(MatteParams), C.c_uint32, C.c_char_p, C.c_uint64]
        L.mcrt_matte_manifest.restype = C.c_int64
    if hasattr(L, "mcrt_render_occlusion"):  # (likewise)
        L.mcrt_render_occlusion.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(OcclusionParams), C.POINTER(OcclusionBuffers), C.POINTER(Stats)]
        L.mcrt_render_occlusion_device.argtypes = L.mcrt_render_occlusion.argtypes
    if hasattr(L, "mcrt_render_lighting"):  # (likewise)
        L.mcrt_render_lighting.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(LightingBuffers), C.POINTER(Stats)]
        L.mcrt_render_lighting_device.argtypes = L.mcrt_render_lighting.argtypes
    if hasattr(L, "mcrt_render_light_groups"):  # (likewise)
        L.mcrt_render_light_groups.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(LightGroupParams), vp, C.POINTER(Stats)]
        L.mcrt_render_light_groups_device.argtypes = L.mcrt_render_light_groups.argtypes
        L.mcrt_light_group_planes.argtypes = [C.POINTER(LightGroupParams)]
        L.mcrt_light_group_planes.restype = C.c_uint32
    if hasattr(L, "mcrt_render_path_classes"):  # (likewise)
        L.mcrt_render_path_classes.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(PathClassParams), vp, C.POINTER(Stats)]
        L.mcrt_render_path_classes_device.argtypes = L.mcrt_render_path_classes.argtypes
        L.mcrt_path_class_planes.argtypes = [C.POINTER(PathClassParams)]
        L.mcrt_path_class_planes.restype = C.c_uint32
    if hasattr(L, "mcrt_set_lens"):  # (likewise)
        L.mcrt_set_lens.argtypes = [vp, C.POINTER(LensDesc)]
        L.mcrt_get_lens.argtypes = [vp, C.POINTER(LensDesc)]
        L.mcrt_camera_rays.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, vp, vp, C.POINTER(Stats)]
        L.mcrt_camera_rays_device.argtypes = L.mcrt_camera_rays.argtypes
    if hasattr(L, "mcrt_set_ray_source"):  # (likewise)
        L.mcrt_set_ray_source.argtypes = [vp, C.POINTER(RaySourceDesc)]
        L.mcrt_set_ray_source_host.argtypes = [vp, C.POINTER(RaySourceDesc), C.POINTER(C.c_uint64)]
        L.mcrt_get_ray_source.argtypes = [vp, C.POINTER(RaySourceDesc)]
    if hasattr(L, "mcrt_render_probes"):  # (likewise)
        L.mcrt_probe_coefficients.argtypes = [C.c_uint32]
        L.mcrt_probe_coefficients.restype = C.c_uint32
        L.mcrt_render_probes.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.POINTER(ProbeParams), vp, C.POINTER(Stats)]
        L.mcrt_render_probes_device.argtypes = L.mcrt_render_probes.argtypes
        L.mcrt_probe_rays_device.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, vp, vp, vp, C.POINTER(Stats)]
    if hasattr(L, "mcrt_frame_compare"):  # (likewise)
        L.mcrt_frame_compare.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(CompareParams), C.POINTER(CompareMaps), C.POINTER(CompareResult), C.POINTER(Stats)]
        L.mcrt_frame_compare_device.argtypes = L.mcrt_frame_compare.argtypes
    L.mcrt_sampler.argtypes = [vp, C.c_uint64, _u32p, _u32p, C.c_uint32, C.c_uint32, _dp]
    L.mcrt_knn.argtypes = [vp, C.c_int, C.c_uint64, _dp, C.c_uint32, _u32p, _u32p, _dp]
    L.mcrt_bsdf.argtypes = [vp, C.c_uint64, _dp, _dp, _dp]
    L.mcrt_libm.argtypes = [vp, C.c_int, C.c_uint64, _dp, _dp, _dp, _dp]
    L.mcrt_bvh_build_octree.argtypes = [vp, C.POINTER(SceneDesc), C.POINTER(vp)]
    L.mcrt_bvh_build_sah.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.mcrt_bvh_build_sah_gpu.argtypes = [vp, C.POINTER(SceneDesc), C.c_int, C.c_uint32, C.POINTER(vp)]
    L.mcrt_bvh_get.argtypes = [vp]
    L.mcrt_bvh_get.restype = C.POINTER(BvhDesc)
    L.mcrt_bvh_free.argtypes = [vp]
    L.mcrt_scene_with_bvh.argtypes = [C.POINTER(SceneDesc), C.POINTER(BvhDesc), C.POINTER(vp)]
    L.mcrt_scene_get.argtypes = [vp]
    L.mcrt_scene_get.restype = C.POINTER(SceneDesc)
    L.mcrt_scene_free.argtypes = [vp]
    L.mcrt_photon_map_build.argtypes = [_fp, C.c_uint64, _dp, _dp, C.c_uint32, C.POINTER(vp)]
    L.mcrt_photon_map_build_gpu.argtypes = [vp, _fp, C.c_uint64, _dp, _dp, C.c_uint32, C.POINTER(vp)]
    L.mcrt_photon_map_get.argtypes = [vp]
    L.mcrt_photon_map_get.restype = C.POINTER(PhotonMapDesc)
    L.mcrt_photon_map_free.argtypes = [vp]
    L.mcrt_photon_map_free.restype = None
    L.mcrt_render_multi.argtypes = [C.POINTER(vp), C.c_uint32, C.POINTER(CameraDesc), C.c_uint32, C.c_int, _dp, C.POINTER(Stats)]
    if hasattr(L, "mcrt_photon_pass_multi"):  # (round 6; absent from older libraries that tools/ab_builds.sh swaps in)
        L.mcrt_photon_pass_multi.argtypes = [C.POINTER(vp), C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.c_uint32, C.c_uint32, C.c_int, C.POINTER(PhotonPassStats)]
    L.mcrt_render_film_device.argtypes = [vp, C.POINTER(CameraDesc), C.c_uint32, C.c_int, vp, vp]
    L.mcrt_film_resolve_device.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.mcrt_tonemap_device.argtypes = [vp, vp, C.POINTER(ImageDesc), vp, _dp, vp]
    L.mcrt_tonemap.argtypes = [vp, _dp, C.POINTER(ImageDesc), vp, _dp]
    L.mcrt_tga_save.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, vp]
    L.mcrt_image_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.mcrt_image_free.argtypes = [vp]
    L.mcrt_image_free.restype = None
    L.mcrt_image_scene.argtypes = [vp]
    L.mcrt_image_scene.restype = C.POINTER(SceneDesc)
    L.mcrt_image_camera.argtypes = [vp]
    L.mcrt_image_camera.restype = C.POINTER(CameraDesc)
    L.mcrt_image_photons.argtypes = [vp, C.c_int]
    L.mcrt_image_photons.restype = C.POINTER(PhotonMapDesc)
    L.mcrt_image_param.argtypes = [vp, C.c_char_p]
    L.mcrt_image_param.restype = C.c_uint64
    if L.mcrt_abi_version() != ABI_VERSION:
        raise McrtError("libmcrt_hip.so ABI %d != binding ABI %d" % (L.mcrt_abi_version(), ABI_VERSION))
    _lib = L
    return L


def _ptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


def _pointer_struct(cls, pointers, allowed):
    """The ctypes struct cls of a dict channel -> raw pointer (None = no dict): a channel left out, None or 0 stays NULL = not wanted."""
    s = cls()
    for name, ptr in (pointers or {}).items():
        assert name in allowed, name
        setattr(s, name, int(ptr) if ptr else None)
    return s


def _channel_arrays(cls, names, table, cam, out):
    """The host arrays of the channels `names` of `table` (name -> (dtype, elements per pixel)) for cam's frame, from the dict `out` where
    it holds them, otherwise fresh zeros -> (dict channel -> array, the ctypes struct cls pointing into them)."""
    res, bufs = {}, cls()
    for name in names:
        dtype, k = table[name]
        shape = (cam.height, cam.width) + ((k,) if k > 1 else ())
        a = out[name] if out is not None and name in out else np.zeros(shape, dtype=dtype)
        assert a.dtype == dtype and a.shape == shape and a.flags["C_CONTIGUOUS"], name
        res[name] = a
        setattr(bufs, name, a.ctypes.data)
    return res, bufs


def _guide_buffers(aov, height, width):
    """The filters' guide channels of render_aov's dict as (AovBuffers of host pointers, the contiguous arrays they point into, to keep
    alive over the call). A channel left out or None stays NULL: the library names a channel it misses."""
    bufs, keep = AovBuffers(), []
    for name in DENOISE_GUIDES:
        if aov.get(name) is None:
            continue
        a = np.ascontiguousarray(aov[name], dtype=np.float64)
        assert a.shape == (height, width) + ((3,) if AOV_CHANNELS[name][1] == 3 else ()), (name, a.shape)
        keep.append(a)
        setattr(bufs, name, a.ctypes.data)
    return bufs, keep


class SceneImage:
    """A scene image (*.mcrt) loaded through mcrt_image_load: flattened Scene/BVH/Camera (+ photon
    maps) as written by the flattener inside the reference host."""

    def __init__(self, path):
        self._lib = lib()
        self._h = C.c_void_p()
        rc = self._lib.mcrt_image_load(os.fsencode(path), C.byref(self._h))
        if rc != 0:
            raise McrtError("mcrt_image_load(%s) failed: %d" % (path, rc))
        self.path = path

    @property
    def scene(self):
        return self._lib.mcrt_image_scene(self._h).contents

    @property
    def camera(self):
        return self._lib.mcrt_image_camera(self._h).contents.copy()

    def photons(self, which):
        p = self._lib.mcrt_image_photons(self._h, which)
        return p.contents if p else None

    def param(self, key):
        return int(self._lib.mcrt_image_param(self._h, key.encode()))

    def close(self):
        if self._h:
            self._lib.mcrt_image_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bvh:
    """mcrt_bvh: the reference's default ("octree") BVH of a scene's surfaces, built by sorting centroid path codes
    (mcrt_bvh_build_octree; with a Context the per-surface work and the sort run on its GPU)."""

    def __init__(self, scene_desc, ctx=None, kind="octree", bins_per_axis=0, threads=0, levels=False):
        self._lib = lib()
        self._h = C.c_void_p()
        bins = int(bins_per_axis) if bins_per_axis else (8 if kind == "quaternary_sah" else 16)
        if kind in ("binary_sah", "quaternary_sah") and (ctx is not None or levels):
            # level-synchronous build: on the GPU of ctx, or (levels=True, no ctx) the same passes as host loops. Its per-node bin tables
            # hold at most 16 bins per axis (the reference's defaults are 16 and 8); for more the C entry point itself hands the scene to
            # the recursive host builder, which has no limit and builds the same tree.
            rc = self._lib.mcrt_bvh_build_sah_gpu(ctx._h if ctx is not None else None, C.byref(scene_desc), 2 if kind == "binary_sah" else 4,
                                                  int(bins_per_axis), C.byref(self._h))
            if rc != 0:
                if ctx is not None:
                    ctx._check(rc, "mcrt_bvh_build_sah_gpu")
                raise McrtError("mcrt_bvh_build_sah_gpu failed: %d" % rc)
            return
        if kind in ("binary_sah", "quaternary_sah"):  # the reference's binned-SAH builders on all host threads
            rc = self._lib.mcrt_bvh_build_sah(C.byref(scene_desc), 2 if kind == "binary_sah" else 4, int(bins_per_axis), int(threads), C.byref(self._h))
            if rc != 0:
                raise McrtError("mcrt_bvh_build_sah failed: %d" % rc)
            return
        rc = self._lib.mcrt_bvh_build_octree(ctx._h if ctx is not None else None, C.byref(scene_desc), C.byref(self._h))
        if rc != 0:
            if ctx is not None:
                ctx._check(rc, "mcrt_bvh_build_octree")
            raise McrtError("mcrt_bvh_build_octree failed: %d" % rc)

    @property
    def desc(self):
        return self._lib.mcrt_bvh_get(self._h).contents

    def arrays(self):
        d = self.desc
        n = d.num_nodes

        def grab(ptr, count, dtype):
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count else np.zeros(0, dtype)
        return dict(bounds=grab(d.node_bounds, n * 6, np.float64).reshape(n, 6), start=grab(d.node_start_surface, n, np.uint32),
                    count=grab(d.node_num_surfaces, n, np.uint32), next=grab(d.node_next_sibling, n, np.uint32),
                    order=grab(d.order, d.num_surfaces, np.uint32))

    def apply(self, scene_desc):
        """mcrt_scene_with_bvh -> OwnedScene (surfaces in BVH order, lights re-indexed, this BVH's nodes)."""
        return OwnedScene(scene_desc, self)

    def close(self):
        if self._h:
            self._lib.mcrt_bvh_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OwnedScene:
    def __init__(self, scene_desc, bvh):
        self._lib = lib()
        self._h = C.c_void_p()
        self._keep = (scene_desc, bvh)  # the copy still points into their material / light / quadric / node arrays
        rc = self._lib.mcrt_scene_with_bvh(C.byref(scene_desc), C.byref(bvh.desc), C.byref(self._h))
        if rc != 0:
            raise McrtError("mcrt_scene_with_bvh failed: %d" % rc)

    @property
    def desc(self):
        return self._lib.mcrt_scene_get(self._h).contents

    def close(self):
        if self._h:
            self._lib.mcrt_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PhotonMap:
    """mcrt_photon_map: linear photon octree built from a photon list — on the host (mcrt_photon_map_build) or,
    given a Context, with its GPU (mcrt_photon_map_build_gpu: cell codes, radix sort, gather, leaf boxes)."""

    @classmethod
    def _from_handle(cls, handle):
        m = cls.__new__(cls)
        m._lib = lib()
        m._h = handle
        return m

    def __init__(self, photons, bb_min, bb_max, max_photons_per_leaf=200, ctx=None):
        self._lib = lib()
        self._h = C.c_void_p()
        ph = np.ascontiguousarray(photons, dtype=np.float32).reshape(-1, 8)
        lo = (C.c_double * 3)(*bb_min)
        hi = (C.c_double * 3)(*bb_max)
        if ctx is None:
            rc = self._lib.mcrt_photon_map_build(_ptr(ph, C.c_float), ph.shape[0], lo, hi, int(max_photons_per_leaf), C.byref(self._h))
            if rc != 0:
                raise McrtError("mcrt_photon_map_build failed: %d" % rc)
        else:
            ctx._check(self._lib.mcrt_photon_map_build_gpu(ctx._h, _ptr(ph, C.c_float), ph.shape[0], lo, hi, int(max_photons_per_leaf),
                                                           C.byref(self._h)), "mcrt_photon_map_build_gpu")

    def arrays(self):
        """The descriptor as numpy copies: dict(bounds[n,6], start[n], contained[n], next[n], leaf[n], photons[m,8])."""
        d = self.desc
        n, m = d.num_octants, d.num_photons

        def grab(ptr, count, dtype):
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count else np.zeros(0, dtype)
        return dict(bounds=grab(d.octant_bounds, n * 6, np.float64).reshape(n, 6), start=grab(d.octant_start_data, n, np.uint64),
                    contained=grab(d.octant_contained_data, n, np.uint64), next=grab(d.octant_next_sibling, n, np.uint32),
                    leaf=grab(d.octant_leaf, n, np.uint8), photons=grab(d.photons, m * 8, np.float32).reshape(m, 8))

    @property
    def desc(self):
        return self._lib.mcrt_photon_map_get(self._h).contents

    def close(self):
        if self._h:
            self._lib.mcrt_photon_map_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """mcrt_ctx: one per GPU / process rank. Mirrors the reference's render seam:
    ``Context.sample_image(camera)`` stands where ``Camera::sampleImage()`` stood."""

    def __init__(self, device_id=0):
        self._lib = lib()
        self._h = C.c_void_p()
        self._device_id = int(device_id)
        rc = self._lib.mcrt_create(C.byref(self._h), int(device_id))
        if rc != 0:
            msg = self._lib.mcrt_last_error(None)
            raise McrtError("mcrt_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))

        self._env = {k: v for k, v in os.environ.items() if k.startswith("MCRT_")}  # what mcrt_create seeded the options with

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.mcrt_last_error(self._h)
            raise McrtError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))

    def set_option(self, key, value):
        """mcrt_set_option: a run-time option of this context (value None = back to the default)."""
        self._check(self._lib.mcrt_set_option(self._h, key.encode(), None if value is None else str(value).encode()), "mcrt_set_option")

    def get_option(self, key):
        v = self._lib.mcrt_get_option(self._h, key.encode())
        return v.decode() if v is not None else None

    def _sync_env(self):
        """The library reads the MCRT_* environment once, in mcrt_create. The tests and A/B tools of this repo switch kernels by
        changing os.environ between calls; the binding mirrors such changes into mcrt_set_option before a call that launches."""
        now = {k: v for k, v in os.environ.items() if k.startswith("MCRT_")}
        if now != self._env:
            for k in set(self._env) - set(now):
                self.set_option(k, None)
            for k, v in now.items():
                if self._env.get(k) != v:
                    self.set_option(k, v)
            self._env = now

    def upload_scene(self, scene_desc):
        self._sync_env()
        self._check(self._lib.mcrt_upload_scene(self._h, C.byref(scene_desc)), "mcrt_upload_scene")
        self._scene_counts = {"surface": int(scene_desc.num_surfaces), "material": int(scene_desc.num_materials)}  # (render_matte's default names)

    def upload_photons(self, global_map, caustic_map, k_nearest, direct_visualization=False):
        self._sync_env()
        g = C.byref(global_map) if global_map is not None else None
        c = C.byref(caustic_map) if caustic_map is not None else None
        self._check(self._lib.mcrt_upload_photons(self._h, g, c, int(k_nearest),
                                                  int(bool(direct_visualization))),
                    "mcrt_upload_photons")

    def upload_image(self, image):
        """Upload everything a SceneImage holds (scene + photon maps if present)."""
        self.upload_scene(image.scene)
        g, c = image.photons(0), image.photons(1)
        if g is not None or c is not None:
            self.upload_photons(g, c, image.param("k_nearest_photons") or 50,
                                bool(image.param("direct_visualization")))

    def sample_image(self, cam, global_seed, integrator=INTEGRATOR_PATH_TRACER):
        """mcrt_render -> (image[H,W,3] float64, stats dict)."""
        self._sync_env()
        out = np.zeros((cam.height, cam.width, 3), dtype=np.float64)
        st = Stats()
        self._check(self._lib.mcrt_render(self._h, C.byref(cam), int(global_seed), int(integrator),
                                          _ptr(out, C.c_double), C.byref(st)), "mcrt_render")
        return out, st.as_dict()

    def render_device(self, cam, global_seed, integrator, device_ptr, stream=None):
        self._sync_env()
        self._check(self._lib.mcrt_render_device(self._h, C.byref(cam), int(global_seed),
                                                 int(integrator), C.c_void_p(int(device_ptr)),
                                                 C.c_void_p(int(stream)) if stream else None),
                    "mcrt_render_device")

    def render_film_device(self, cam, global_seed, integrator, rgbw_ptr, stream=None):
        """mcrt_render_film_device: this shard's splats into a full-frame RGBW device buffer (width*height*4 doubles)."""
        self._sync_env()
        self._check(self._lib.mcrt_render_film_device(self._h, C.byref(cam), int(global_seed), int(integrator), C.c_void_p(int(rgbw_ptr)),
                                                      C.c_void_p(int(stream)) if stream else None), "mcrt_render_film_device")

    def film_resolve_device(self, width, height, rgbw_ptr, out_ptr, stream=None):
        """mcrt_film_resolve_device: Splat::get over the (summed) RGBW buffer -> width*height*3 doubles."""
        self._check(self._lib.mcrt_film_resolve_device(self._h, int(width), int(height), C.c_void_p(int(rgbw_ptr)), C.c_void_p(int(out_ptr)),
                                                       C.c_void_p(int(stream)) if stream else None), "mcrt_film_resolve_device")

    def render_finish(self):
        st = Stats()
        self._check(self._lib.mcrt_render_finish(self._h, C.byref(st)), "mcrt_render_finish")
        return st.as_dict()

    def tonemap(self, rgb, image):
        """mcrt_tonemap: Image::save of a host frame [H,W,3] FP64 -> ([H,W,3] uint8 in B,G,R order, (exposure, gain))."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
        assert rgb.shape == (image.height, image.width, 3)
        bgr = np.empty((image.height, image.width, 3), dtype=np.uint8)
        factors = (C.c_double * 2)()
        self._check(self._lib.mcrt_tonemap(self._h, rgb.ctypes.data_as(_dp), C.byref(image), bgr.ctypes.data, factors), "mcrt_tonemap")
        return bgr, (factors[0], factors[1])

    def tonemap_device(self, rgb_ptr, image, bgr_ptr, stream=None):
        """mcrt_tonemap_device on device pointers (e.g. torch tensors' data_ptr()); returns (exposure, gain)."""
        factors = (C.c_double * 2)()
        self._check(self._lib.mcrt_tonemap_device(self._h, C.c_void_p(int(rgb_ptr)), C.byref(image), C.c_void_p(int(bgr_ptr)), factors,
                                                  C.c_void_p(int(stream)) if stream else None), "mcrt_tonemap_device")
        return factors[0], factors[1]

    def emit_photons(self, emissions, caustic_factor, global_seed, shard_index=0, shard_count=1):
        """mcrt_emit_photons[_shard] -> dict(global_=(photons[n,8] f32, keys[n] u64), caustic=(...), paths, rays, kernel_ms)."""
        self._sync_env()
        pe = PhotonEmission()
        self._check(self._lib.mcrt_emit_photons_shard(self._h, float(emissions), float(caustic_factor), int(global_seed),
                                                      int(shard_index), int(shard_count), C.byref(pe)), "mcrt_emit_photons")

        def grab(ptr, kptr, n):
            if n == 0:
                return np.zeros((0, 8), dtype=np.float32), np.zeros(0, dtype=np.uint64)
            return (np.ctypeslib.as_array(ptr, shape=(n * 8,)).reshape(n, 8).copy(),
                    np.ctypeslib.as_array(kptr, shape=(n,)).copy())

        return dict(global_=grab(pe.global_photons, pe.global_keys, pe.global_count),
                    caustic=grab(pe.caustic_photons, pe.caustic_keys, pe.caustic_count),
                    paths=int(pe.emission_paths), rays=int(pe.rays), kernel_ms=pe.kernel_ms)

    def photon_pass_device(self, emissions, caustic_factor, global_seed, bb_min, bb_max, max_photons_per_leaf=200, k_nearest=50,
                           direct_visualization=False):
        """mcrt_photon_pass_device: emission + both maps on the device, installed for the eye pass. Returns the stats dict."""
        self._sync_env()
        st = PhotonPassStats()
        lo, hi = (C.c_double * 3)(*bb_min), (C.c_double * 3)(*bb_max)
        self._check(self._lib.mcrt_photon_pass_device(self._h, float(emissions), float(caustic_factor), int(global_seed), lo, hi,
                                                      int(max_photons_per_leaf), int(k_nearest), 1 if direct_visualization else 0, C.byref(st)),
                    "mcrt_photon_pass_device")
        return st.as_dict()

    def emit_photons_device(self, emissions, caustic_factor, global_seed, shard_index=0, shard_count=1):
        """mcrt_emit_photons_device -> dict(global_=(device pointer, count), caustic=(...), paths, rays, kernel_ms); the lists
        stay in device memory owned by the context."""
        self._sync_env()
        pe = PhotonEmissionDevice()
        self._check(self._lib.mcrt_emit_photons_device(self._h, float(emissions), float(caustic_factor), int(global_seed), int(shard_index),
                                                       int(shard_count), C.byref(pe)), "mcrt_emit_photons_device")
        return dict(global_=(pe.d_global_photons or 0, int(pe.global_count)), caustic=(pe.d_caustic_photons or 0, int(pe.caustic_count)),
                    paths=int(pe.emission_paths), rays=int(pe.rays), kernel_ms=pe.kernel_ms)

    def upload_photons_device(self, d_global, global_count, d_caustic, caustic_count, bb_min, bb_max, max_photons_per_leaf=200, k_nearest=50,
                              direct_visualization=False):
        """mcrt_upload_photons_device: both maps from photon lists in device memory (raw pointers, e.g. tensor.data_ptr())."""
        self._sync_env()
        st = PhotonPassStats()
        lo, hi = (C.c_double * 3)(*bb_min), (C.c_double * 3)(*bb_max)
        self._check(self._lib.mcrt_upload_photons_device(self._h, C.c_void_p(int(d_global)), int(global_count), C.c_void_p(int(d_caustic)),
                                                         int(caustic_count), lo, hi, int(max_photons_per_leaf), int(k_nearest),
                                                         1 if direct_visualization else 0, C.byref(st)), "mcrt_upload_photons_device")
        return st.as_dict()

    def download_map(self, which):
        """mcrt_photon_map_download: host copy (PhotonMap) of installed map 0 (global) / 1 (caustic)."""
        h = C.c_void_p()
        self._check(self._lib.mcrt_photon_map_download(self._h, int(which), C.byref(h)), "mcrt_photon_map_download")
        return PhotonMap._from_handle(h)

    def intersect(self, start, direction):
        self._sync_env()
        start = np.ascontiguousarray(start, dtype=np.float64)
        direction = np.ascontiguousarray(direction, dtype=np.float64)
        n = start.shape[0]
        t = np.empty(n, dtype=np.float64)
        surf = np.empty(n, dtype=np.uint32)
        uv = np.empty((n, 2), dtype=np.float64)
        self._check(self._lib.mcrt_intersect(self._h, n, _ptr(start, C.c_double),
                                             _ptr(direction, C.c_double), _ptr(t, C.c_double),
                                             _ptr(surf, C.c_uint32), _ptr(uv, C.c_double)),
                    "mcrt_intersect")
        return t, surf, uv

    def intersect_device(self, n, d_start, d_direction, d_t, d_surface, d_uv=None):
        """mcrt_intersect_device: mcrt_intersect on raw device pointers (e.g. tensor.data_ptr()): start[n][3], direction[n][3] in,
        t[n], surface[n] (uint32), uv[n][2] (optional) out. The inputs must be complete (torch.cuda.synchronize()) when this is called."""
        self._sync_env()
        self._check(self._lib.mcrt_intersect_device(self._h, int(n), C.c_void_p(int(d_start)), C.c_void_p(int(d_direction)), C.c_void_p(int(d_t)),
                                                    C.c_void_p(int(d_surface)), C.c_void_p(int(d_uv)) if d_uv else None), "mcrt_intersect_device")

    def render_aov(self, cam, global_seed, channels=None, out=None, stats=None):
        """mcrt_render_aov: the first-hit AOV frame -> dict channel -> array [H,W] or [H,W,3]. channels: the names wanted (AOV_CHANNELS;
        None = all). out: a dict of arrays to write into instead of fresh zeros - the call only writes the rows cam's shard owns, the
        others keep their contents. stats: a dict that receives mcrt_stats."""
        self._sync_env()
        names = list(AOV_CHANNELS) if channels is None else list(channels)
        res, bufs = _channel_arrays(AovBuffers, names, AOV_CHANNELS, cam, out)
        st = Stats()
        self._check(self._lib.mcrt_render_aov(self._h, C.byref(cam), int(global_seed), C.byref(bufs), C.byref(st)), "mcrt_render_aov")
        if stats is not None:
            stats.update(st.as_dict())
        return res

    def render_aov_device(self, cam, global_seed, pointers):
        """mcrt_render_aov_device: pointers = dict channel -> raw device pointer (owned rows only, packed like render_device's
        output); channels left out are not computed. Synchronous; returns the stats dict."""
        self._sync_env()
        bufs = _pointer_struct(AovBuffers, pointers, AOV_CHANNELS)
        st = Stats()
        self._check(self._lib.mcrt_render_aov_device(self._h, C.byref(cam), int(global_seed), C.byref(bufs), C.byref(st)), "mcrt_render_aov_device")
        return st.as_dict()

    def render_occlusion(self, cam, global_seed, rays=1, max_distance=0.0, geometric=False, channels=None, out=None, stats=None):
        """mcrt_render_occlusion: the occlusion frame -> dict "ao" [H,W], "sky" [H,W], "bent_normal" [H,W,3] (not normalised). rays:
        occlusion rays per camera sample that hits, 1 .. 64; max_distance: hits farther away do not occlude, 0 = unbounded; geometric:
        directions around the geometric instead of the shading normal. channels: the names wanted (OCCLUSION_CHANNELS; None = all). out:
        a dict of arrays to write into instead of fresh zeros - the call only writes the rows cam's shard owns. stats: a dict that
        receives mcrt_stats."""
        self._sync_env()
        names = list(OCCLUSION_CHANNELS) if channels is None else list(channels)
        res, bufs = _channel_arrays(OcclusionBuffers, names, OCCLUSION_CHANNELS, cam, out)
        par = OcclusionParams(int(rays), OCCLUSION_GEOMETRIC if geometric else 0, float(max_distance))
        st = Stats()
        self._check(self._lib.mcrt_render_occlusion(self._h, C.byref(cam), int(global_seed), C.byref(par), C.byref(bufs), C.byref(st)), "mcrt_render_occlusion")
        if stats is not None:
            stats.update(st.as_dict())
        return res

    def render_occlusion_device(self, cam, global_seed, pointers, rays=1, max_distance=0.0, geometric=False):
        """mcrt_render_occlusion_device: pointers = dict channel -> raw device pointer (owned rows only, packed like render_device's
        output); channels left out are not computed. Synchronous; returns the stats dict."""
        self._sync_env()
        bufs = _pointer_struct(OcclusionBuffers, pointers, OCCLUSION_CHANNELS)
        par = OcclusionParams(int(rays), OCCLUSION_GEOMETRIC if geometric else 0, float(max_distance))
        st = Stats()
        self._check(self._lib.mcrt_render_occlusion_device(self._h, C.byref(cam), int(global_seed), C.byref(par), C.byref(bufs), C.byref(st)),
                    "mcrt_render_occlusion_device")
        return st.as_dict()

    def render_lighting(self, cam, global_seed, channels=None, out=None, stats=None):
        """mcrt_render_lighting: the lighting frame of a path-traced render of cam and global_seed -> dict "emission", "sky", "direct",
        "light", "unoccluded", each [H,W,3]: the path tracer's path cut after its second vertex, split up (include/mcrt.h "Lighting
        passes"); light / unoccluded is the shadow matte. channels: the names wanted (LIGHTING_CHANNELS; None = all). out: a dict of
        arrays to write into instead of fresh zeros - the call only writes the rows cam's shard owns. stats: a dict that receives
        mcrt_stats."""
        self._sync_env()
        names = list(LIGHTING_CHANNELS) if channels is None else list(channels)
        res, bufs = _channel_arrays(LightingBuffers, names, LIGHTING_CHANNELS, cam, out)
        st = Stats()
        self._check(self._lib.mcrt_render_lighting(self._h, C.byref(cam), int(global_seed), C.byref(bufs), C.byref(st)), "mcrt_render_lighting")
        if stats is not None:
            stats.update(st.as_dict())
        return res

    def render_lighting_device(self, cam, global_seed, pointers):
        """mcrt_render_lighting_device: pointers = dict channel -> raw device pointer (owned rows only, packed like render_device's
        output); channels left out are not computed. Synchronous; returns the stats dict."""
        self._sync_env()
        bufs = _pointer_struct(LightingBuffers, pointers, LIGHTING_CHANNELS)
        st = Stats()
        self._check(self._lib.mcrt_render_lighting_device(self._h, C.byref(cam), int(global_seed), C.byref(bufs), C.byref(st)), "mcrt_render_lighting_device")
        return st.as_dict()

    @staticmethod
    def _light_group_params(groups, sky_plane, max_depth, num_groups, film=False, film_clamp=False):
        """-> (LightGroupParams, the array it points into). groups: [num_surfaces] group per surface, or None."""
        keep = None if groups is None else np.ascontiguousarray(groups, dtype=np.uint32)
        if num_groups is None:
            num_groups = 1 if keep is None or keep.size == 0 else int(keep.max()) + 1
        flags = (0 if sky_plane is None else LIGHT_GROUPS_SKY_PLANE) | (LIGHT_GROUPS_FILM if film else 0) | (LIGHT_GROUPS_FILM_CLAMP if film_clamp else 0)
        par = LightGroupParams(int(num_groups), flags, 0 if sky_plane is None else int(sky_plane), int(max_depth), None if keep is None else keep.ctypes.data)
        return par, keep

    def render_light_groups(self, cam, global_seed, groups=None, sky_plane=None, max_depth=0, stats=None, num_groups=None, out=None, film=False, film_clamp=False):
        """mcrt_render_light_groups: the path-traced frame of cam and global_seed split by emitter, every bounce -> [P,H,W,3]: one plane
        per group and the sky's, which add up to the frame (include/mcrt.h "Light groups"). groups: [num_surfaces] the group of every
        surface (light_group_map builds it; entries of surfaces that emit nothing are ignored), None = every emitter in group 0.
        num_groups: default max(groups) + 1. sky_plane: the plane that takes the sky, default a plane of its own after the groups.
        max_depth: 0 = the whole path, 1 = direct light only. out: an array to write into instead of fresh zeros - the call only writes
        the rows cam's shard owns. stats: a dict that receives mcrt_stats. film: the planes through cam's reconstruction filter
        (film_filter, film_radius, film_cache_size) instead of the box mean, gathered in a fixed order - the same bytes run after run
        (include/mcrt.h "Filtered planes"); film_clamp: max(., 0) on every word, as the film's own resolve has it (planes that are to
        add up stay unclamped)."""
        self._sync_env()
        par, keep = self._light_group_params(groups, sky_plane, max_depth, num_groups, film, film_clamp)
        planes = int(self._lib.mcrt_light_group_planes(C.byref(par)))
        shape = (max(planes, 1), cam.height, cam.width, 3)  # (out of range: the call below says what is)
        a = out if out is not None else np.zeros(shape)
        assert a.dtype == np.float64 and a.shape == shape and a.flags["C_CONTIGUOUS"]
        st = Stats()
        self._check(self._lib.mcrt_render_light_groups(self._h, C.byref(cam), int(global_seed), C.byref(par), a.ctypes.data, C.byref(st)), "mcrt_render_light_groups")
        if stats is not None:
            stats.update(st.as_dict())
        return a

    def render_light_groups_device(self, cam, global_seed, pointer, groups=None, sky_plane=None, max_depth=0, num_groups=None, film=False, film_clamp=False):
        """mcrt_render_light_groups_device: pointer = raw device pointer to [P][owned rows][W][3] doubles (packed like render_device's
        output). film, film_clamp: as in render_light_groups. Synchronous; returns the stats dict."""
        self._sync_env()
        par, keep = self._light_group_params(groups, sky_plane, max_depth, num_groups, film, film_clamp)
        st = Stats()
        self._check(self._lib.mcrt_render_light_groups_device(self._h, C.byref(cam), int(global_seed), C.byref(par), int(pointer) if pointer else None, C.byref(st)),
                    "mcrt_render_light_groups_device")
        return st.as_dict()

    @staticmethod
    def _path_class_params(class_plane, max_depth, film=False, film_clamp=False):
        """-> PathClassParams. class_plane: the plane of each of the eight classes, or None = the identity."""
        par = PathClassParams((PATH_CLASSES_FILM if film else 0) | (PATH_CLASSES_FILM_CLAMP if film_clamp else 0), int(max_depth))
        if class_plane is not None:
            entries = [int(p) for p in class_plane]
            assert len(entries) == PATH_CLASSES and all(0 <= p < 256 for p in entries), entries
            par.flags |= PATH_CLASSES_MAP
            par.class_plane[:] = entries
        return par

    def render_path_classes(self, cam, global_seed, class_plane=None, max_depth=0, stats=None, out=None, film=False, film_clamp=False):
        """mcrt_render_path_classes: the path-traced frame of cam and global_seed split by what the first surface did with the light
        -> [P,H,W,3]: emission, background, and direct and indirect of diffuse, glossy and transmission (PATH_CLASS_NAMES), which add up
        to the frame (include/mcrt.h "Path classes"). class_plane: [8] the output plane of every class (path_class_map builds it),
        None = a plane each. max_depth: 0 = the whole path, 1 = no indirect light. out: an array to write into instead of fresh zeros -
        the call only writes the rows cam's shard owns. stats: a dict that receives mcrt_stats. film, film_clamp: the planes through
        cam's reconstruction filter, as in render_light_groups (include/mcrt.h "Filtered planes")."""
        self._sync_env()
        par = self._path_class_params(class_plane, max_depth, film, film_clamp)
        planes = int(self._lib.mcrt_path_class_planes(C.byref(par)))
        shape = (max(planes, 1), cam.height, cam.width, 3)  # (out of range: the call below says what is)
        a = out if out is not None else np.zeros(shape)
        assert a.dtype == np.float64 and a.shape == shape and a.flags["C_CONTIGUOUS"]
        st = Stats()
        self._check(self._lib.mcrt_render_path_classes(self._h, C.byref(cam), int(global_seed), C.byref(par), a.ctypes.data, C.byref(st)), "mcrt_render_path_classes")
        if stats is not None:
            stats.update(st.as_dict())
        return a

    def render_path_classes_device(self, cam, global_seed, pointer, class_plane=None, max_depth=0, film=False, film_clamp=False):
        """mcrt_render_path_classes_device: pointer = raw device pointer to [P][owned rows][W][3] doubles (packed like render_device's
        output). film, film_clamp: as in render_light_groups. Synchronous; returns the stats dict."""
        self._sync_env()
        par = self._path_class_params(class_plane, max_depth, film, film_clamp)
        st = Stats()
        self._check(self._lib.mcrt_render_path_classes_device(self._h, C.byref(cam), int(global_seed), C.byref(par), int(pointer) if pointer else None, C.byref(st)),
                    "mcrt_render_path_classes_device")
        return st.as_dict()

    def set_lens(self, lens_desc):
        """mcrt_set_lens: the camera model that the camera-ray passes (AOV, mattes, occlusion, lighting, light groups, path classes) and
        camera_rays trace under, until the next call. lens_desc: a LensDesc (lens(...) builds one), a model name, or None = the camera's
        own rays. While a lens is set the render calls are refused (include/mcrt.h "Camera models"); render_lens is the beauty frame."""
        if isinstance(lens_desc, str):
            lens_desc = lens(lens_desc)
        self._check(self._lib.mcrt_set_lens(self._h, None if lens_desc is None else C.byref(lens_desc)), "mcrt_set_lens")

    def get_lens(self):
        """mcrt_get_lens -> the LensDesc as it was set (model LENS_NONE with none)."""
        d = LensDesc()
        self._check(self._lib.mcrt_get_lens(self._h, C.byref(d)), "mcrt_get_lens")
        return d

    def camera_rays(self, cam, global_seed, stats=None):
        """mcrt_camera_rays: the camera rays of every sample of the rows cam's shard owns, under the context's lens (none set: the
        perspective camera's) -> (start, direction), each [spp, owned rows, W, 3]: sample-major, what intersect takes after a
        reshape(-1, 3). stats: a dict that receives mcrt_stats."""
        self._sync_env()
        rows = int(self._lib.mcrt_shard_rows(C.byref(cam), None))
        shape = (cam.sqrtspp * cam.sqrtspp, rows, cam.width, 3)
        start, direction = np.zeros(shape), np.zeros(shape)
        st = Stats()
        self._check(self._lib.mcrt_camera_rays(self._h, C.byref(cam), int(global_seed), start.ctypes.data, direction.ctypes.data, C.byref(st)), "mcrt_camera_rays")
        if stats is not None:
            stats.update(st.as_dict())
        return start, direction

    def camera_rays_device(self, cam, global_seed, d_start, d_direction):
        """mcrt_camera_rays_device: raw device pointers to [spp][owned rows][W][3] doubles each. Synchronous; returns the stats dict."""
        self._sync_env()
        st = Stats()
        self._check(self._lib.mcrt_camera_rays_device(self._h, C.byref(cam), int(global_seed), int(d_start) if d_start else None,
                                                      int(d_direction) if d_direction else None, C.byref(st)), "mcrt_camera_rays_device")
        return st.as_dict()

    def render_lens(self, cam, global_seed, max_depth=0, stats=None, out=None, film=False, film_clamp=False):
        """The beauty frame of cam and global_seed under the context's lens -> [H,W,3]: the light groups with every emitter and the sky in
        plane 0, which with no lens (or LENS_PERSPECTIVE) is mcrt_render's path-traced frame bit for bit. max_depth: 0 = the whole path.
        out: an array to write into instead of fresh zeros - the call only writes the rows cam's shard owns. film, film_clamp: through
        cam's reconstruction filter, as in render_light_groups."""
        a = None if out is None else out.reshape((1,) + out.shape)
        return self.render_light_groups(cam, global_seed, groups=None, sky_plane=0, max_depth=max_depth, stats=stats, num_groups=1, out=a, film=film,
                                        film_clamp=film_clamp)[0]

    def render_film(self, cam, global_seed, max_depth=0, stats=None):
        """The filtered beauty frame of cam and global_seed -> [H,W,3], deterministic: one plane of the light groups through cam's
        reconstruction filter, clamped like the film's own resolve (include/mcrt.h "Filtered planes"). It agrees with sample_image's
        frame of the same camera to rounding - that one is splatted with atomics - and is the same bytes run after run, whatever the
        chunking, with or without a lens. A camera with the default box film gives render_lens' frame."""
        return self.render_lens(cam, global_seed, max_depth=max_depth, stats=stats, film=True, film_clamp=True)

    def set_ray_source(self, kind, first=None, second=None, per_pixel=False, offset=None):
        """mcrt_set_ray_source[_host]: the arrays the camera-ray passes (AOV, mattes, occlusion, lighting, light groups, path classes),
        camera_rays and render_lens take their first rays from, until the next call (include/mcrt.h "Ray sources"). kind: "rays"
        (first = start, second = direction, float64 [spp, ..., 3] with the packed pixels of the shard in between - what camera_rays
        returns -, or [..., 3] with per_pixel=True: one ray for all samples of a pixel), "surface" (first = position, second = normal,
        [..., 3]: the AOV pass's frames; offset: how far along the normal a ray starts, default 1e-9), or "none" / None. torch tensors on
        the device are used in place - the context keeps a reference, they must not be written while set -; numpy arrays are copied to
        device memory the context owns, and the call returns how many records will be replaced by the fallback ray (unusable ones:
        non-finite words, an all-zero direction or normal). While a source is set the render calls are refused."""
        if isinstance(kind, str):
            by_name = {v: k for k, v in RAY_SOURCE_NAMES.items()}
            if kind not in by_name:
                raise ValueError("set_ray_source: kind must be one of %s, not %r" % (", ".join(sorted(by_name)), kind))
            kind = by_name[kind]
        if kind is None or int(kind) == RAY_SOURCE_NONE:
            return self.clear_ray_source()
        if first is None or second is None:
            raise ValueError("set_ray_source: two arrays are needed")
        on_device = hasattr(first, "data_ptr")
        if on_device != hasattr(second, "data_ptr"):
            raise ValueError("set_ray_source: both arrays torch tensors on the device, or both numpy arrays")
        if on_device:
            import torch
            for t in (first, second):
                if t.dtype != torch.float64 or not t.is_contiguous() or t.device.type != "cuda":
                    raise ValueError("set_ray_source: tensors must be contiguous float64 on the device")
            shape, size, keep = tuple(first.shape), first.numel(), (first, second)
            if tuple(second.shape) != shape:
                raise ValueError("set_ray_source: the two arrays differ in shape")
            pointers = (first.data_ptr(), second.data_ptr())
        else:
            first, second = np.ascontiguousarray(first, dtype=np.float64), np.ascontiguousarray(second, dtype=np.float64)
            if first.shape != second.shape:
                raise ValueError("set_ray_source: the two arrays differ in shape")
            shape, size, keep = first.shape, first.size, None
            pointers = (first.ctypes.data, second.ctypes.data)
        if len(shape) < 2 or shape[-1] != 3 or size == 0:
            raise ValueError("set_ray_source: arrays of shape [..., 3], not %r" % (shape,))
        per_sample = int(kind) == RAY_SOURCE_RAYS and not per_pixel
        if per_sample and len(shape) < 3:
            raise ValueError("set_ray_source: per-sample rays are [spp, ..., 3]; per_pixel=True takes [..., 3]")
        spp = int(shape[0]) if per_sample else 0
        d = RaySourceDesc(int(kind), RAY_SOURCE_PER_PIXEL if (per_pixel and int(kind) == RAY_SOURCE_RAYS) else 0, size // 3 // max(spp, 1), spp, 0, pointers[0], pointers[1],
                          RAY_SOURCE_DEFAULT_OFFSET if offset is None else float(offset))
        if on_device:
            self._check(self._lib.mcrt_set_ray_source(self._h, C.byref(d)), "mcrt_set_ray_source")
            self._ray_source_arrays = keep
            return None
        sanitised = C.c_uint64(0)
        self._check(self._lib.mcrt_set_ray_source_host(self._h, C.byref(d), C.byref(sanitised)), "mcrt_set_ray_source_host")
        self._ray_source_arrays = None
        return int(sanitised.value)

    def get_ray_source(self):
        """mcrt_get_ray_source -> the RaySourceDesc as it was set (kind RAY_SOURCE_NONE with none; after numpy arrays: the pointers of
        the context's device copies)."""
        d = RaySourceDesc()
        self._check(self._lib.mcrt_get_ray_source(self._h, C.byref(d)), "mcrt_get_ray_source")
        return d

    def clear_ray_source(self):
        """mcrt_set_ray_source(ctx, NULL): no source - the camera's own rays again, every call what it was."""
        self._check(self._lib.mcrt_set_ray_source(self._h, None), "mcrt_set_ray_source")
        self._ray_source_arrays = None

    def gather_irradiance(self, cam, global_seed, position, normal, groups=None, sky_plane=None, max_depth=0, offset=None, num_groups=None, stats=None):
        """The irradiance at surface points, per lamp -> [P,H,W,3]: a SURFACE ray source from position and normal ([H,W,3] or
        [owned rows of cam's shard, W, 3]; numpy arrays or torch device tensors - the AOV pass's frames, or a lightmap's texels), the
        light groups under it (groups, sky_plane, max_depth, num_groups as in render_light_groups), times pi: cam.sqrtspp^2
        cosine-weighted directions per point, whose pdf is cos / pi. cam gives the frame's shape and the sampler keys only. The planes
        add up to the whole irradiance; the point's own material is never read (a gather, not a path vertex). The context's source and
        lens are put back as they were found."""
        before, before_arrays, before_lens = self.get_ray_source(), getattr(self, "_ray_source_arrays", None), self.get_lens()
        if before.kind != RAY_SOURCE_NONE and before_arrays is None:
            raise McrtError("gather_irradiance: the context holds a ray source made from numpy arrays, which cannot be put back; clear_ray_source first")
        if before.kind != RAY_SOURCE_NONE:
            self.clear_ray_source()
        if before_lens.model != LENS_NONE:
            self.set_lens(None)
        try:
            self.set_ray_source(RAY_SOURCE_SURFACE, position, normal, offset=offset)
            planes = self.render_light_groups(cam, global_seed, groups=groups, sky_plane=sky_plane, max_depth=max_depth, stats=stats, num_groups=num_groups)
            planes *= math.pi
            return planes
        finally:
            self.clear_ray_source()
            if before_lens.model != LENS_NONE:
                self.set_lens(before_lens)
            if before.kind != RAY_SOURCE_NONE:
                self._check(self._lib.mcrt_set_ray_source(self._h, C.byref(before)), "mcrt_set_ray_source")
                self._ray_source_arrays = before_arrays

    def _probe_params(self, order, groups, sky_plane, max_depth, num_groups, positions=None, weight=None):
        """-> (ProbeParams, what it points into)."""
        lg, keep = self._light_group_params(groups, sky_plane, max_depth, num_groups)
        return ProbeParams(lg, int(order), 0, positions, weight), keep

    def render_probes(self, cam, global_seed, positions=None, order=2, weight=None, groups=None, sky_plane=None, max_depth=0, num_groups=None, stats=None, out=None):
        """mcrt_render_probes: light probes -> [P,K,H,W,3], K = (order + 1)^2: per plane of the light groups (groups, sky_plane,
        max_depth, num_groups as in render_light_groups) the mean over a pixel's samples of the radiance along the sample's first ray
        times the un-normalised spherical-harmonic basis of that ray's direction (include/mcrt.h "Light probes"; probe_sh normalises,
        probe_irradiance evaluates). cam gives the frame's shape - width * height probes, sqrtspp^2 rays each - and the sampler keys.
        positions: float64 [owned rows, W, 3] (or [pixels, 3]) - the rays leave these points uniformly over the sphere, and a lens or a
        ray source on the context is refused -, or None: the first rays are the context's (camera, lens, ray source). weight: float64
        [spp, owned rows, W] (or [spp, pixels]), 1 / pdf for first rays that are not uniformly distributed, or None. numpy arrays
        (torch tensors are copied to the host). out: an array to write into instead of fresh zeros - the call only writes the rows
        cam's shard owns. stats: a dict that receives mcrt_stats."""
        self._sync_env()
        pixels = len(shard_rows(cam)) * cam.width
        spp = cam.sqrtspp * cam.sqrtspp

        def host(a, size, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "data_ptr") else a, dtype=np.float64)
            if a.size != size:
                raise ValueError("render_probes: %s holds %d values, the camera's shard takes %d" % (what, a.size, size))
            return a
        positions, weight = host(positions, pixels * 3, "positions"), host(weight, pixels * spp, "weight")
        par, keep = self._probe_params(order, groups, sky_plane, max_depth, num_groups, None if positions is None else positions.ctypes.data,
                                       None if weight is None else weight.ctypes.data)
        planes = int(self._lib.mcrt_light_group_planes(C.byref(par.groups)))
        k = int(self._lib.mcrt_probe_coefficients(int(order)))
        shape = (max(planes, 1), max(k, 1), cam.height, cam.width, 3)  # (out of range: the call below says what is)
        a = out if out is not None else np.zeros(shape)
        assert a.dtype == np.float64 and a.shape == shape and a.flags["C_CONTIGUOUS"]
        st = Stats()
        self._check(self._lib.mcrt_render_probes(self._h, C.byref(cam), int(global_seed), C.byref(par), a.ctypes.data, C.byref(st)), "mcrt_render_probes")
        if stats is not None:
            stats.update(st.as_dict())
        return a

    def render_probes_device(self, cam, global_seed, pointer, positions=None, order=2, weight=None, groups=None, sky_plane=None, max_depth=0, num_groups=None):
        """mcrt_render_probes_device: pointer = raw device pointer to [P][K][owned rows][W][3] doubles; positions, weight: raw device
        pointers or None. Synchronous; returns the stats dict."""
        self._sync_env()
        par, keep = self._probe_params(order, groups, sky_plane, max_depth, num_groups, int(positions) if positions else None, int(weight) if weight else None)
        st = Stats()
        self._check(self._lib.mcrt_render_probes_device(self._h, C.byref(cam), int(global_seed), C.byref(par), int(pointer) if pointer else None, C.byref(st)),
                    "mcrt_render_probes_device")
        return st.as_dict()

    def probe_rays_device(self, cam, global_seed, d_positions, d_start, d_direction):
        """mcrt_probe_rays_device: raw device pointers - positions [owned rows][W][3], start and direction [spp][owned rows][W][3]
        doubles each. Synchronous; returns the stats dict."""
        self._sync_env()
        st = Stats()
        self._check(self._lib.mcrt_probe_rays_device(self._h, C.byref(cam), int(global_seed), int(d_positions) if d_positions else None,
                                                     int(d_start) if d_start else None, int(d_direction) if d_direction else None, C.byref(st)), "mcrt_probe_rays_device")
        return st.as_dict()

    def probe_rays(self, cam, global_seed, positions, stats=None):
        """The first rays render_probes traces from positions (float64 [owned rows, W, 3] or [pixels, 3]) -> (start, direction), each
        [spp, owned rows, W, 3]: sample-major, what set_ray_source("rays", ...) takes. The arrays pass through torch tensors on the
        context's device."""
        import torch
        rows = len(shard_rows(cam))
        spp = cam.sqrtspp * cam.sqrtspp
        device = "cuda:%d" % self._device_id
        p = torch.as_tensor(np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)).to(device)
        if p.shape[0] != rows * cam.width:
            raise ValueError("probe_rays: positions holds %d points, the camera's shard takes %d" % (p.shape[0], rows * cam.width))
        start = torch.zeros((spp, rows, cam.width, 3), dtype=torch.float64, device=device)
        direction = torch.zeros_like(start)
        torch.cuda.synchronize(device)
        st = self.probe_rays_device(cam, global_seed, p.data_ptr(), start.data_ptr(), direction.data_ptr())
        if stats is not None:
            stats.update(st)
        return start.cpu().numpy(), direction.cpu().numpy()

    def bake_probes(self, points, rays=1024, order=2, global_seed=0, groups=None, sky_plane=None, max_depth=0, num_groups=None, stats=None):
        """Light probes at points [N, 3] -> dict: "coefficients" [P, K, N, 3], the raw means of render_probes over
        ceil(sqrt(rays))^2 uniform directions per point, and "sh" [P, K, N, 3], probe_sh of them: per plane of the light groups
        (groups, sky_plane, max_depth, num_groups as in render_light_groups) the radiance arriving at each point as coefficients of the
        real spherical harmonics; probe_irradiance(sh[..., None, :, :], normals[None]) is the irradiance for any normal. The camera is
        N x 1 and gives nothing but the sampler keys. A lens or a ray source on the context is refused."""
        points = np.ascontiguousarray(points, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3 or points.shape[0] == 0:
            raise ValueError("bake_probes: points of shape [N, 3], not %r" % (points.shape,))
        cam = CameraDesc()
        cam.width, cam.height, cam.sqrtspp = points.shape[0], 1, max(1, math.isqrt(max(int(rays), 1) - 1) + 1)
        raw = self.render_probes(cam, global_seed, positions=points, order=order, groups=groups, sky_plane=sky_plane, max_depth=max_depth, num_groups=num_groups,
                                 stats=stats)
        return {"coefficients": raw[:, :, 0], "sh": probe_sh(raw)[:, :, 0]}

    def render_matte(self, cam, global_seed, key="material", ranks=MATTE_DEFAULT_RANKS, names=None, surface_key=None, aov=None, out=None, stats=None,
                     num_keys=None):
        """mcrt_render_matte: the ranked id / coverage mattes of the frame -> dict "id" [H,W,ranks] uint32, "coverage" [H,W,ranks],
        "layer" [H,W,ranks,2] (the Cryptomatte channels: exr_layers(mattes=...)), "distinct" [H,W] uint32, plus "names", "codes", "manifest"
        (the JSON text), "key", "ranks". key: "material", "surface" or "custom" (surface_key: [num_surfaces] key per surface; num_keys:
        default len(names), else max(surface_key) + 1). names: a name per key, default "material%u" / "surface%u" / "key%u". aov: AOV
        channel names (True = all) rendered from the same rays and hits -> result["aov"], render_aov's bits. out: a dict of arrays to write
        into instead of fresh ones (the rows cam's shard owns are written). stats: a dict that receives mcrt_stats."""
        self._sync_env()
        ranks = int(ranks) or MATTE_DEFAULT_RANKS
        par, keep = _matte_params(key, ranks, names, surface_key, num_keys)
        n_keys = par.num_keys if key == "custom" else getattr(self, "_scene_counts", {}).get(key, 0)
        res, bufs = {}, MatteBuffers()
        for name, (dtype, tail) in MATTE_CHANNELS.items():
            shape = (cam.height, cam.width) + tuple(int(ranks) if t == "ranks" else t for t in tail)
            a = out[name] if out is not None and name in out else np.zeros(shape, dtype=dtype)
            if not (out is not None and name in out) and name == "id":
                a.fill(NO_KEY)
            assert a.dtype == dtype and a.shape == shape and a.flags["C_CONTIGUOUS"], name
            res[name] = a
            setattr(bufs, name, a.ctypes.data)
        aov_res, aov_bufs = _channel_arrays(AovBuffers, list(AOV_CHANNELS) if aov is True else list(aov or ()), AOV_CHANNELS, cam,
                                            None if out is None else out.get("aov"))
        st = Stats()
        self._check(self._lib.mcrt_render_matte(self._h, C.byref(cam), int(global_seed), C.byref(par), C.byref(bufs), C.byref(aov_bufs) if aov_res else None,
                                                C.byref(st)), "mcrt_render_matte")
        if stats is not None:
            stats.update(st.as_dict())
        res["names"] = [n.decode("latin-1") if isinstance(n, bytes) else str(n) for n in names] if names is not None else \
            [MATTE_DEFAULT_NAMES[key].replace("%u", "%d") % k for k in range(n_keys)]
        res["codes"] = np.array([matte_code(n) for n in res["names"]], dtype=np.uint32)
        res["manifest"] = matte_manifest(key, n_keys, names)
        res["key"], res["ranks"] = key, int(ranks)
        if aov_res:
            res["aov"] = aov_res
        return res

    def render_matte_device(self, cam, global_seed, pointers, key="material", ranks=MATTE_DEFAULT_RANKS, names=None, surface_key=None, aov_pointers=None,
                            num_keys=None):
        """mcrt_render_matte_device: pointers = dict "id" / "coverage" / "layer" / "distinct" -> raw device pointer (owned rows only, packed
        like render_device's output); aov_pointers likewise for the AOV channels. Synchronous; returns the stats dict."""
        self._sync_env()
        par, keep = _matte_params(key, ranks, names, surface_key, num_keys)
        bufs = _pointer_struct(MatteBuffers, pointers, MATTE_CHANNELS)
        aov_bufs = _pointer_struct(AovBuffers, aov_pointers, AOV_CHANNELS)
        st = Stats()
        self._check(self._lib.mcrt_render_matte_device(self._h, C.byref(cam), int(global_seed), C.byref(par), C.byref(bufs),
                                                       C.byref(aov_bufs) if aov_pointers else None, C.byref(st)), "mcrt_render_matte_device")
        return st.as_dict()

    def matte_rank_device(self, pixels, spp, keys_ptr, ranks, codes_ptr, pointers):
        """mcrt_matte_rank_device on raw device pointers: keys [spp][pixels] uint32 (0xFFFFFFFF = none), codes [greater than every key] or
        None, pointers = dict "id" / "coverage" / "layer" / "distinct" -> buffers of `pixels` pixels. The inputs must be complete when
        this is called. Synchronous; returns the stats dict."""
        self._sync_env()
        bufs = _pointer_struct(MatteBuffers, pointers, MATTE_CHANNELS)
        st = Stats()
        self._check(self._lib.mcrt_matte_rank_device(self._h, int(pixels), int(spp), C.c_void_p(int(keys_ptr)) if keys_ptr else None, int(ranks),
                                                     C.c_void_p(int(codes_ptr)) if codes_ptr else None, C.byref(bufs), C.byref(st)), "mcrt_matte_rank_device")
        return st.as_dict()

    def matte_rank(self, keys, ranks=MATTE_DEFAULT_RANKS, codes=None, stats=None):
        """The ranking of mcrt_render_matte on a caller's own ids: keys [spp, pixels] uint32 (numpy; 0xFFFFFFFF = none), codes [num_keys]
        uint32 or None (then no "layer") -> dict "id" [pixels, ranks], "coverage", "layer" [pixels, ranks, 2], "distinct" [pixels]. The
        arrays cross to this context's device and back through torch."""
        import torch
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        assert keys.ndim == 2, keys.shape
        spp, pixels = keys.shape
        if codes is not None:
            codes = np.ascontiguousarray(codes, dtype=np.uint32)
            assert not (keys != NO_KEY).any() or int(keys[keys != NO_KEY].max()) < codes.shape[0], "a key without a code"
        dev = torch.device("cuda", self._device_id)
        up = lambda a: torch.from_numpy((a if a.flags.writeable else a.copy()).view(np.int32)).to(dev)
        d_keys, d_codes = up(keys.reshape(-1)), up(codes) if codes is not None else None
        r = max(int(ranks), 0) or MATTE_DEFAULT_RANKS
        outs = {"id": torch.full((pixels, r), -1, dtype=torch.int32, device=dev), "coverage": torch.zeros((pixels, r), dtype=torch.float64, device=dev),
                "distinct": torch.zeros((pixels,), dtype=torch.int32, device=dev)}
        if codes is not None:
            outs["layer"] = torch.zeros((pixels, r, 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        st = self.matte_rank_device(pixels, spp, d_keys.data_ptr(), ranks, d_codes.data_ptr() if d_codes is not None else None,
                                    {k: v.data_ptr() for k, v in outs.items()})
        if stats is not None:
            stats.update(st)
        res = {k: v.cpu().numpy() for k, v in outs.items()}
        res["id"], res["distinct"] = res["id"].view(np.uint32), res["distinct"].view(np.uint32)
        return res

    def denoise(self, rgb, aov, stats=None, **params):
        """mcrt_denoise: the edge-avoiding a-trous filter on the beauty frame rgb [H,W,3], guided by aov - render_aov's dict of the same
        camera and seed (shading_normal, normal, position, coverage, albedo are read) -> the filtered frame [H,W,3]. params: the fields
        of mcrt_denoise_params (iterations, normal_power_log2, sigma_color, sigma_plane, albedo_floor, flags); left out = the default.
        stats: a dict that receives mcrt_stats."""
        self._sync_env()
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
        assert rgb.ndim == 3 and rgb.shape[2] == 3, rgb.shape
        height, width = rgb.shape[:2]
        par = DenoiseParams(**params)
        bufs, keep = _guide_buffers(aov, height, width)
        out = np.empty_like(rgb)
        st = Stats()
        self._check(self._lib.mcrt_denoise(self._h, width, height, rgb.ctypes.data, C.byref(bufs), C.byref(par), out.ctypes.data, C.byref(st)), "mcrt_denoise")
        if stats is not None:
            stats.update(st.as_dict())
        return out

    def denoise_device(self, width, height, rgb_ptr, pointers, out_ptr, **params):
        """mcrt_denoise_device: rgb_ptr / out_ptr (may be the same) and pointers = dict guide channel -> raw device pointer, all full
        frames that are complete when this is called. Synchronous; returns the stats dict."""
        self._sync_env()
        bufs = _pointer_struct(AovBuffers, pointers, AOV_CHANNELS)
        par = DenoiseParams(**params)
        st = Stats()
        self._check(self._lib.mcrt_denoise_device(self._h, int(width), int(height), C.c_void_p(int(rgb_ptr)) if rgb_ptr else None, C.byref(bufs), C.byref(par),
                                                  C.c_void_p(int(out_ptr)) if out_ptr else None, C.byref(st)), "mcrt_denoise_device")
        return st.as_dict()

    def denoise_variance(self, rgb, variance, aov, spp, stats=None, want_variance=True, **params):
        """mcrt_denoise_variance: the a-trous filter steered by the per-pixel sample variance [H,W,3] of the beauty frame rgb [H,W,3]
        (render_pixel_stats' "variance" at spp samples per pixel), guided by aov as denoise is -> (the filtered frame, its variance in
        the form frame_noise reads; None with want_variance=False). params: the fields of mcrt_denoise_variance_params (iterations,
        normal_power_log2, sigma_variance, sigma_floor, sigma_plane, albedo_floor, flags); left out = the default. stats: a dict that
        receives mcrt_stats."""
        self._sync_env()
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
        variance = np.ascontiguousarray(variance, dtype=np.float64)
        assert rgb.ndim == 3 and rgb.shape[2] == 3 and variance.shape == rgb.shape, (rgb.shape, variance.shape)
        height, width = rgb.shape[:2]
        par = DenoiseVarianceParams(**params)
        bufs, keep = _guide_buffers(aov, height, width)
        out, out_var = np.empty_like(rgb), (np.empty_like(rgb) if want_variance else None)
        st = Stats()
        self._check(self._lib.mcrt_denoise_variance(self._h, width, height, int(spp), rgb.ctypes.data, variance.ctypes.data, C.byref(bufs), C.byref(par),
                                                    out.ctypes.data, out_var.ctypes.data if want_variance else None, C.byref(st)), "mcrt_denoise_variance")
        if stats is not None:
            stats.update(st.as_dict())
        return out, out_var

    def denoise_variance_device(self, width, height, spp, rgb_ptr, variance_ptr, pointers, out_ptr, out_variance_ptr=None, **params):
        """mcrt_denoise_variance_device: rgb_ptr / out_ptr and variance_ptr / out_variance_ptr (each pair may be the same; out_variance_ptr
        None = not wanted) and pointers = dict guide channel -> raw device pointer, all full frames that are complete when this is called.
        Synchronous; returns the stats dict."""
        self._sync_env()
        bufs = _pointer_struct(AovBuffers, pointers, AOV_CHANNELS)
        par = DenoiseVarianceParams(**params)
        st = Stats()
        p = lambda x: C.c_void_p(int(x)) if x else None
        self._check(self._lib.mcrt_denoise_variance_device(self._h, int(width), int(height), int(spp), p(rgb_ptr), p(variance_ptr), C.byref(bufs), C.byref(par),
                                                           p(out_ptr), p(out_variance_ptr), C.byref(st)), "mcrt_denoise_variance_device")
        return st.as_dict()

    def render_denoised(self, cam, global_seed, integrator=INTEGRATOR_PATH_TRACER, **params):
        """A frame with its statistics, its guides and the variance-guided filter in one call: render_pixel_stats ("variance"), render_aov
        (DENOISE_GUIDES) and denoise_variance -> dict "rgb" (the filtered frame), "variance" (its variance), "raw" (the unfiltered frame),
        "noise" and "raw_noise" (frame_noise of the filtered and of the unfiltered frame). cam is one whole frame (no shard: the filter
        reads neighbouring rows)."""
        assert cam.shard_count <= 1, "render_denoised filters a whole frame: gather the shards first"
        spp = cam.sqrtspp * cam.sqrtspp
        raw = self.render_pixel_stats(cam, global_seed, integrator, channels=("variance",))
        aov = self.render_aov(cam, global_seed, channels=DENOISE_GUIDES)
        rgb, variance = self.denoise_variance(raw["rgb"], raw["variance"], aov, spp, **params)
        return {"rgb": rgb, "variance": variance, "raw": raw["rgb"], "noise": self.frame_noise(rgb, variance, spp),
                "raw_noise": self.frame_noise(raw["rgb"], raw["variance"], spp)}

    def denoise_dual(self, half_a, half_b=None, variance=None, spp=None, want=("rgb", "variance"), stats=None, **params):
        """mcrt_denoise_dual: the dual-buffer non-local-means filter on the half-buffers half_a, half_b [H,W,3] of a render of spp samples
        per pixel and its per-pixel sample variance [H,W,3] (render_pixel_stats' channels) -> dict of the outputs in `want`
        (DENOISE_DUAL_OUTPUTS: "rgb" the filtered frame, always there; "variance" its error in the form frame_noise reads; "half_a",
        "half_b" the filtered halves). half_a may be the dict a render_converged or render_pixel_stats returned instead: its "half_a",
        "half_b" and "variance" are read, and spp from its "result" unless given. params: the fields of mcrt_denoise_dual_params
        (window_radius, patch_radius, k, alpha, epsilon); left out = the default. stats: a dict that receives mcrt_stats."""
        self._sync_env()
        if isinstance(half_a, dict):
            summary = half_a
            half_a, half_b, variance = summary["half_a"], summary["half_b"], summary["variance"]
            if spp is None:
                spp = summary["result"]["spp"]
        half_a, half_b, variance = (np.ascontiguousarray(a, dtype=np.float64) for a in (half_a, half_b, variance))
        assert half_a.ndim == 3 and half_a.shape[2] == 3 and half_b.shape == half_a.shape and variance.shape == half_a.shape, (half_a.shape, half_b.shape, variance.shape)
        height, width = half_a.shape[:2]
        names = ["rgb"] + [k for k in want if k != "rgb"]
        assert all(k in DENOISE_DUAL_OUTPUTS for k in names), names
        res = {k: np.empty_like(half_a) for k in names}
        bufs = DenoiseDualBuffers(**{k: a.ctypes.data for k, a in res.items()})
        par = DenoiseDualParams(**params)
        st = Stats()
        self._check(self._lib.mcrt_denoise_dual(self._h, width, height, int(spp), half_a.ctypes.data, half_b.ctypes.data, variance.ctypes.data, C.byref(par),
                                                C.byref(bufs), C.byref(st)), "mcrt_denoise_dual")
        if stats is not None:
            stats.update(st.as_dict())
        return res

    def denoise_dual_device(self, width, height, spp, half_a_ptr, half_b_ptr, variance_ptr, pointers, **params):
        """mcrt_denoise_dual_device: the three input frames and pointers = dict output (DENOISE_DUAL_OUTPUTS) -> raw device pointer, all full
        frames; an output may be the corresponding input, "rgb" any of them; outputs left out or None are not written. Synchronous; returns
        the stats dict."""
        self._sync_env()
        bufs = _pointer_struct(DenoiseDualBuffers, pointers, DENOISE_DUAL_OUTPUTS)
        par = DenoiseDualParams(**params)
        st = Stats()
        p = lambda x: C.c_void_p(int(x)) if x else None
        self._check(self._lib.mcrt_denoise_dual_device(self._h, int(width), int(height), int(spp), p(half_a_ptr), p(half_b_ptr), p(variance_ptr), C.byref(par),
                                                       C.byref(bufs) if pointers is not None else None, C.byref(st)), "mcrt_denoise_dual_device")
        return st.as_dict()

    def render_denoised_dual(self, cam, global_seed, integrator=INTEGRATOR_PATH_TRACER, **params):
        """A frame with its half-buffers and the dual-buffer filter in one call: render_pixel_stats (variance, half_a, half_b), denoise_dual
        and frame_noise of both frames -> dict "rgb" (the filtered frame), "variance" (its error estimate), "raw" (the unfiltered frame),
        "noise" and "raw_noise" (frame_noise of the filtered and of the unfiltered frame). No AOV pass is rendered. cam is one whole frame
        (no shard: the filter reads neighbouring rows)."""
        assert cam.shard_count <= 1, "render_denoised_dual filters a whole frame: gather the shards first"
        spp = cam.sqrtspp * cam.sqrtspp
        raw = self.render_pixel_stats(cam, global_seed, integrator)
        out = self.denoise_dual(raw["half_a"], raw["half_b"], raw["variance"], spp, **params)
        return {"rgb": out["rgb"], "variance": out["variance"], "raw": raw["rgb"], "noise": self.frame_noise(out["rgb"], out["variance"], spp),
                "raw_noise": self.frame_noise(raw["rgb"], raw["variance"], spp)}

    def render_pixel_stats(self, cam, global_seed, integrator=INTEGRATOR_PATH_TRACER, channels=None, stats=None, out=None):
        """mcrt_render_pixel_stats: the frame of sample_image plus the per-pixel sample statistics -> dict "rgb" and the channels wanted
        (PIXEL_STATS_CHANNELS; None = all, () = a plain render), each [H,W,3]. out: a dict of arrays to write into instead of fresh zeros -
        the call only writes the rows cam's shard owns. stats: a dict that receives mcrt_stats."""
        self._sync_env()
        names = list(PIXEL_STATS_CHANNELS) if channels is None else list(channels)
        res = _summary_arrays(["rgb"] + names, (cam.height, cam.width), out, PIXEL_STATS_CHANNELS)
        st = Stats()
        self._check(self._lib.mcrt_render_pixel_stats(self._h, C.byref(cam), int(global_seed), int(integrator), res["rgb"].ctypes.data,
                                                      C.byref(_addresses(PixelStatsBuffers, res)), C.byref(st)), "mcrt_render_pixel_stats")
        if stats is not None:
            stats.update(st.as_dict())
        return res

    def render_pixel_stats_device(self, cam, global_seed, integrator, rgb_ptr, pointers=None):
        """mcrt_render_pixel_stats_device: rgb_ptr and pointers = dict channel -> raw device pointer (owned rows only, packed like
        render_device's output); channels left out or None are not computed. Synchronous; returns the stats dict."""
        self._sync_env()
        bufs = _pointer_struct(PixelStatsBuffers, pointers, PIXEL_STATS_CHANNELS)
        st = Stats()
        self._check(self._lib.mcrt_render_pixel_stats_device(self._h, C.byref(cam), int(global_seed), int(integrator),
                                                             C.c_void_p(int(rgb_ptr)) if rgb_ptr else None, C.byref(bufs) if pointers is not None else None,
                                                             C.byref(st)), "mcrt_render_pixel_stats_device")
        return st.as_dict()

    def frame_noise(self, rgb, variance, spp):
        """mcrt_frame_noise: the summary of a frame [.., 3] and its variance -> dict noise, signal, relative_error, pixels."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
        variance = np.ascontiguousarray(variance, dtype=np.float64)
        assert rgb.shape == variance.shape and rgb.shape[-1] == 3, (rgb.shape, variance.shape)
        r = FrameNoise()
        self._check(self._lib.mcrt_frame_noise(self._h, rgb.size // 3, int(spp), rgb.ctypes.data, variance.ctypes.data, C.byref(r)), "mcrt_frame_noise")
        return r.as_dict()

    def frame_noise_device(self, pixels, spp, rgb_ptr, variance_ptr):
        """mcrt_frame_noise_device on device pointers of frames that are complete when this is called."""
        r = FrameNoise()
        self._check(self._lib.mcrt_frame_noise_device(self._h, int(pixels), int(spp), C.c_void_p(int(rgb_ptr)) if rgb_ptr else None,
                                                      C.c_void_p(int(variance_ptr)) if variance_ptr else None, C.byref(r)), "mcrt_frame_noise_device")
        return r.as_dict()

    def frame_compare(self, rgb, ref, mask=None, eps=None, peak=None, ssim_range=None, ssim=True, maps=False, stats=None):
        """mcrt_frame_compare: the frame rgb [H,W,3] against the reference ref [H,W,3], mask [H,W] or None (a pixel takes part where
        mask > 0) -> dict of mcrt_compare_result's fields; with maps=True also "squared_error", "relative" and - with ssim - "ssim",
        [H,W] each (maps may also name the ones wanted). numpy arrays go through the host-pointer form; torch tensors on this context's
        device (float64, contiguous) through mcrt_frame_compare_device, and the maps come back as tensors of that device. eps, peak,
        ssim_range: None = the default. stats: a dict that receives mcrt_stats."""
        self._sync_env()
        tensors = _is_tensor(rgb)
        wanted = [k for k in COMPARE_MAPS if (maps is True or (maps and k in maps)) and (ssim or k != "ssim")]
        par = CompareParams(eps or 0.0, peak or 0.0, ssim_range or 0.0, 1 if ssim else 0, 0)
        for name, v in (("eps", eps), ("peak", peak), ("ssim_range", ssim_range)):
            if v is not None and not v > 0:  # (0 would mean the default to the library: the caller gave a value)
                raise McrtError("frame_compare: %s must be finite and > 0, not %r" % (name, v))
        res, st, out = CompareResult(), Stats(), {}
        if tensors:
            import torch
            assert _is_tensor(ref) and (mask is None or _is_tensor(mask)), "device tensors and numpy arrays are not mixed"
            frames = [rgb, ref] + ([mask] if mask is not None else [])
            assert all(str(t.dtype) == "torch.float64" and t.is_contiguous() and t.is_cuda for t in frames), "float64, contiguous, on the device"
            height, width = int(rgb.shape[0]), int(rgb.shape[1])
            out = {k: torch.empty((height, width), dtype=torch.float64, device=rgb.device) for k in wanted}
            ptr = lambda t: C.c_void_p(int(t.data_ptr()))
            torch.cuda.synchronize(rgb.device)
            call = self._lib.mcrt_frame_compare_device
        else:
            rgb, ref = np.ascontiguousarray(rgb, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
            mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)
            height, width = rgb.shape[:2]
            out = {k: np.empty((height, width)) for k in wanted}
            ptr = lambda a: C.c_void_p(a.ctypes.data)
            call = self._lib.mcrt_frame_compare
        assert rgb.ndim == 3 and rgb.shape[2] == 3 and tuple(ref.shape) == tuple(rgb.shape), (tuple(rgb.shape), tuple(ref.shape))
        assert mask is None or tuple(mask.shape) == (height, width), tuple(mask.shape)
        bufs = CompareMaps(**{k: ptr(a) for k, a in out.items()})
        self._check(call(self._h, width, height, ptr(rgb), ptr(ref), ptr(mask) if mask is not None else None, C.byref(par), C.byref(bufs), C.byref(res),
                         C.byref(st)), "mcrt_frame_compare")
        if stats is not None:
            stats.update(st.as_dict())
        r = res.as_dict()
        r.update(out)
        return r

    def frame_compare_device(self, width, height, rgb_ptr, ref_ptr, mask_ptr=None, pointers=None, params=None):
        """mcrt_frame_compare_device on raw device pointers of frames that are complete when this is called; pointers = dict map
        (COMPARE_MAPS) -> raw device pointer, params a CompareParams or None. Synchronous -> (result dict, stats dict)."""
        self._sync_env()
        bufs = _pointer_struct(CompareMaps, pointers, COMPARE_MAPS)
        res, st = CompareResult(), Stats()
        p = lambda x: C.c_void_p(int(x)) if x else None
        self._check(self._lib.mcrt_frame_compare_device(self._h, int(width), int(height), p(rgb_ptr), p(ref_ptr), p(mask_ptr), C.byref(params) if params is not None else None,
                                                        C.byref(bufs) if pointers is not None else None, C.byref(res), C.byref(st)), "mcrt_frame_compare_device")
        return res.as_dict(), st.as_dict()

    def render_highlights(self, cam, global_seed, integrator=INTEGRATOR_PATH_TRACER, channels=None, stats_channels=(), stats=None, out=None):
        """mcrt_render_highlights: the frame of sample_image plus the highlights of its samples -> dict "rgb" [H,W,3] and the channels
        wanted (HIGHLIGHT_CHANNELS: "tops" [H,W,4,3], "level" [H,W]; None = both, () = none), plus the per-pixel statistics named in
        stats_channels (PIXEL_STATS_CHANNELS), filled by the same render. out: a dict of arrays to write into instead of fresh zeros -
        the call only writes the rows cam's shard owns. stats: a dict that receives mcrt_stats."""
        self._sync_env()
        names = list(HIGHLIGHT_CHANNELS) if channels is None else list(channels)
        res = _summary_arrays(["rgb"] + names + list(stats_channels), (cam.height, cam.width), out)
        st = Stats()
        self._check(self._lib.mcrt_render_highlights(self._h, C.byref(cam), int(global_seed), int(integrator), res["rgb"].ctypes.data,
                                                     C.byref(_addresses(HighlightBuffers, res)),
                                                     C.byref(_addresses(PixelStatsBuffers, res)) if stats_channels else None, C.byref(st)), "mcrt_render_highlights")
        if stats is not None:
            stats.update(st.as_dict())
        return res

    def render_highlights_device(self, cam, global_seed, integrator, rgb_ptr, pointers=None, stats_pointers=None):
        """mcrt_render_highlights_device: rgb_ptr, pointers = dict highlight channel -> raw device pointer and stats_pointers = dict
        statistics channel -> raw device pointer (owned rows only, packed like render_device's output); channels left out or None are
        not computed. Synchronous; returns the stats dict."""
        self._sync_env()
        hl = _pointer_struct(HighlightBuffers, pointers, HIGHLIGHT_CHANNELS)
        ps = _pointer_struct(PixelStatsBuffers, stats_pointers, PIXEL_STATS_CHANNELS)
        st = Stats()
        self._check(self._lib.mcrt_render_highlights_device(self._h, C.byref(cam), int(global_seed), int(integrator),
                                                            C.c_void_p(int(rgb_ptr)) if rgb_ptr else None, C.byref(hl) if pointers is not None else None,
                                                            C.byref(ps) if stats_pointers is not None else None, C.byref(st)), "mcrt_render_highlights_device")
        return st.as_dict()

    def robust_resolve(self, rgb, tops, level, spp, stats=None, out=None, **params):
        """mcrt_robust_resolve: the robust frame of the full frames rgb [H,W,3], tops [H,W,4,3] and level [H,W] of a render with spp
        samples per pixel -> dict "robust" [H,W,3], "removed" [H,W,3], "clamped" [H,W] uint32. params: the fields of mcrt_robust_params
        (kappa, floor, radius); left out = the default. out: an array to take the robust frame (may be rgb itself). stats: a dict that
        receives mcrt_stats."""
        self._sync_env()
        rgb = rgb if out is rgb else np.ascontiguousarray(rgb, dtype=np.float64)
        tops, level = np.ascontiguousarray(tops, dtype=np.float64), np.ascontiguousarray(level, dtype=np.float64)
        assert rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.dtype == np.float64 and rgb.flags["C_CONTIGUOUS"], rgb.shape
        height, width = rgb.shape[:2]
        assert tops.shape == (height, width, ROBUST_TOPS, 3) and level.shape == (height, width), (tops.shape, level.shape)
        robust = np.empty_like(rgb) if out is None else out
        assert robust.shape == rgb.shape and robust.dtype == np.float64 and robust.flags["C_CONTIGUOUS"]
        res = {"robust": robust, "removed": np.empty((height, width, 3), dtype=np.float64), "clamped": np.empty((height, width), dtype=np.uint32)}
        bufs = RobustBuffers(res["removed"].ctypes.data, res["clamped"].ctypes.data)
        par, st = RobustParams(**params), Stats()
        self._check(self._lib.mcrt_robust_resolve(self._h, width, height, int(spp), rgb.ctypes.data, tops.ctypes.data, level.ctypes.data, C.byref(par),
                                                  robust.ctypes.data, C.byref(bufs), C.byref(st)), "mcrt_robust_resolve")
        if stats is not None:
            stats.update(st.as_dict())
        return res

    def robust_resolve_device(self, width, height, spp, rgb_ptr, tops_ptr, level_ptr, out_ptr, removed_ptr=None, clamped_ptr=None, **params):
        """mcrt_robust_resolve_device on raw device pointers of full frames that are complete when this is called (out_ptr may be
        rgb_ptr; removed_ptr / clamped_ptr None = not wanted). Synchronous; returns the stats dict."""
        self._sync_env()
        p = lambda v: C.c_void_p(int(v)) if v else None
        bufs = RobustBuffers(int(removed_ptr) if removed_ptr else None, int(clamped_ptr) if clamped_ptr else None)
        par, st = RobustParams(**params), Stats()
        self._check(self._lib.mcrt_robust_resolve_device(self._h, int(width), int(height), int(spp), p(rgb_ptr), p(tops_ptr), p(level_ptr), C.byref(par),
                                                         p(out_ptr), C.byref(bufs) if (removed_ptr or clamped_ptr) else None, C.byref(st)),
                    "mcrt_robust_resolve_device")
        return st.as_dict()

    def render_robust(self, cam, global_seed, integrator=INTEGRATOR_PATH_TRACER, stats=None, **params):
        """The two steps for an unsharded camera: render_highlights, then robust_resolve with params -> dict "rgb" (the plain frame),
        "robust", "removed", "clamped". stats: a dict that receives the render's mcrt_stats and the resolve's as "resolve"."""
        assert cam.shard_count <= 1, "the resolve reads neighbouring rows: gather the shards' highlights, then robust_resolve"
        st, st2 = {}, {}
        hl = self.render_highlights(cam, global_seed, integrator, stats=st)
        res = self.robust_resolve(hl["rgb"], hl["tops"], hl["level"], cam.sqrtspp * cam.sqrtspp, stats=st2, **params)
        if stats is not None:
            stats.update(st, resolve=st2)
        return {"rgb": hl["rgb"], "robust": res["robust"], "removed": res["removed"], "clamped": res["clamped"]}

    def frame_merge(self, a, n_a, b, n_b, stats=None, in_place=False):
        """mcrt_frame_merge: the summary of a's n_a samples followed by b's n_b. a and b are dicts channel -> array
        (FRAME_SUMMARY_CHANNELS gives the names and the shape of a pixel: [.., 3], "tops" [.., 4, 3], "level" [..]); the channels both hold
        are merged (whole groups, FRAME_SUMMARY_GROUPS; "rgb" alone gives the mean only) -> dict of the same channels. in_place: the
        outputs are a's own arrays (which must then be contiguous float64). stats: a dict that receives mcrt_stats."""
        self._sync_env()
        names = [k for k in FRAME_SUMMARY_CHANNELS if k in a and k in b]
        assert "rgb" in names or "half_a" in names or "tops" in names, names
        first = names[0]
        lead = np.shape(a[first])[:np.ndim(a[first]) - len(FRAME_SUMMARY_CHANNELS[first])]
        res = _summary_arrays(names, lead, a if in_place else None)
        xa = res if in_place else {k: np.ascontiguousarray(a[k], dtype=np.float64) for k in names}
        xb = {k: np.ascontiguousarray(b[k], dtype=np.float64) for k in names}
        for k in names:
            assert xa[k].shape == res[k].shape and xb[k].shape == res[k].shape, (k, xa[k].shape, xb[k].shape)
        sa, sb, so = (_addresses(FrameSummary, d) for d in (xa, xb, res))
        st = Stats()
        self._check(self._lib.mcrt_frame_merge(self._h, int(np.prod(lead, dtype=np.int64)), C.byref(sa), int(n_a), C.byref(sb), int(n_b), C.byref(so),
                                               C.byref(st)), "mcrt_frame_merge")
        if stats is not None:
            stats.update(st.as_dict())
        return res

    def frame_merge_device(self, pixels, a, n_a, b, n_b, out=None):
        """mcrt_frame_merge_device: a, b, out = dicts channel -> raw device pointer of [pixels]... buffers that are complete when this is
        called; out None = merged into a in place (the channels a and b both name). Synchronous; returns the stats dict."""
        self._sync_env()
        if out is None:
            out = {k: v for k, v in a.items() if v and b.get(k)}
        sums = [_pointer_struct(FrameSummary, d, FRAME_SUMMARY_CHANNELS) for d in (a, b, out)]
        st = Stats()
        self._check(self._lib.mcrt_frame_merge_device(self._h, int(pixels), C.byref(sums[0]), int(n_a), C.byref(sums[1]), int(n_b), C.byref(sums[2]),
                                                      C.byref(st)), "mcrt_frame_merge_device")
        return st.as_dict()

    def exr_save(self, path, channels, attributes=None, compression="zip", zip_level=0, threads=0, half_inf=False, stats=None, long_names=None):
        """mcrt_exr_save / mcrt_exr_save_device: one OpenEXR file of the named channels. channels: dict name -> frame view [H,W] or
        (view, "half" | "float" | "uint") - exr_layers builds it; float64 goes to HALF unless told otherwise, (u)int32 to UINT. The
        views are numpy arrays (the host form: every distinct buffer crosses to the device once) or torch device tensors (the device
        form: only the packed buffer crosses back; all channels must then be tensors of this context's device, complete: the
        producing streams are synchronised here). Last-axis views of one packed buffer become stride / offset of that buffer.
        attributes: dict name -> str, written as strings. compression: "zip" or "none". long_names: channel names of up to 255 bytes
        instead of 31, in a file with OpenEXR's long-names bit (MCRT_EXR_LONG_NAMES); None = when a name needs it
        (pathclass.transmission_indirect.R is 33 bytes). -> dict file_bytes, packed_bytes, chunks, raw_chunks. stats: a dict that
        receives mcrt_stats."""
        self._sync_env()
        assert len(channels) >= 1, "no channel"
        keep, recs, shape, on_device = [], [], None, None
        for name, value in channels.items():
            view, kind = value if isinstance(value, (tuple, list)) else (value, None)
            arr, ptr, source, stride, offset = _exr_source(view)
            if kind is None:
                kind = "half" if source == EXR_SRC_F64 else "uint"
            tensor = _is_tensor(arr)
            if tensor:
                assert arr.is_cuda, "%s: a torch channel lives on the device (numpy arrays take the host form)" % name
            assert on_device in (None, tensor), "channels are all numpy arrays or all torch device tensors"
            assert shape in (None, tuple(arr.shape)), (name, tuple(arr.shape), shape)
            on_device, shape = tensor, tuple(arr.shape)
            keep.append(arr)
            recs.append(ExrChannel(name.encode("ascii"), ptr, source, EXR_PIXEL_TYPES[kind], stride, offset))
        if on_device:
            import torch
            torch.cuda.synchronize()
        attrs = [ExrAttribute(str(k).encode("ascii"), str(v).encode("ascii")) for k, v in (attributes or {}).items()]
        if long_names is None:
            long_names = any(len(name) > 31 for name in channels)
        par = ExrParams(EXR_COMPRESSION[compression], int(zip_level), int(threads), (EXR_HALF_INF if half_inf else 0) | (EXR_LONG_NAMES if long_names else 0))
        res, st = ExrResult(), Stats()
        call = self._lib.mcrt_exr_save_device if on_device else self._lib.mcrt_exr_save
        self._check(call(self._h, os.fsencode(path), shape[1], shape[0], (ExrChannel * len(recs))(*recs), len(recs),
                         (ExrAttribute * len(attrs))(*attrs) if attrs else None, len(attrs), C.byref(par), C.byref(res), C.byref(st)),
                    "mcrt_exr_save_device" if on_device else "mcrt_exr_save")
        if stats is not None:
            stats.update(st.as_dict())
        return res.as_dict()

    def exr_load(self, path, channels=None, device=False, threads=0, stats=None):
        """mcrt_exr_open .. mcrt_exr_load / mcrt_exr_load_device: the channels of an OpenEXR file -> (channels, attributes, info).
        channels: dict name -> [H,W] float64 (the file's HALF and FLOAT channels, widened exactly) or uint32 (UINT) numpy array, in the
        file's order; device=True: torch tensors on this context's device instead (float64, and int32 holding the uint32 bits, as
        exr_save takes them), born there - only the file's own bytes cross. channels= selects a subset, in the order given.
        attributes: dict name -> (type, value) of every header attribute in file order, decoded as tools/exr_probe.py read() does
        (unknown types stay bytes). info: width, height, data_window, display_window, compression, line_order, chunks, raw_chunks,
        file_bytes, payload_bytes. stats: a dict that receives mcrt_stats."""
        self._sync_env()
        f = C.c_void_p()
        self._check(self._lib.mcrt_exr_open(self._h, os.fsencode(path), C.byref(f)), "mcrt_exr_open")
        try:
            fi = ExrInfo()
            self._check(self._lib.mcrt_exr_file_info(f, C.byref(fi)), "mcrt_exr_file_info")
            in_file = []
            for i in range(fi.channels):
                name, ptype = C.c_char_p(), C.c_uint32()
                self._check(self._lib.mcrt_exr_file_channel(f, i, C.byref(name), C.byref(ptype)), "mcrt_exr_file_channel")
                in_file.append((name.value.decode("latin-1"), EXR_PIXEL_TYPE_NAMES[ptype.value]))
            attributes = {}
            for i in range(fi.attributes):
                name, typ, value, size = C.c_char_p(), C.c_char_p(), C.c_void_p(), C.c_uint32()
                self._check(self._lib.mcrt_exr_file_attribute(f, i, C.byref(name), C.byref(typ), C.byref(value), C.byref(size)), "mcrt_exr_file_attribute")
                raw = C.string_at(value.value, size.value) if size.value else b""
                attributes[name.value.decode("latin-1")] = (typ.value.decode("latin-1"), _exr_attribute_value(typ.value.decode("latin-1"), raw, in_file))
            types = dict(in_file)
            wanted = [n for n, _ in in_file] if channels is None else [str(n) for n in channels]
            assert len(wanted) >= 1, "no channel"
            shape = (fi.height, fi.width)
            out, recs = {}, []
            if device:
                import torch
                dev = torch.device("cuda", self._device_id)
            for n in wanted:
                uint = types.get(n) == "uint"  # (a name the file does not hold: the library refuses it, and names it)
                if device:
                    a = torch.empty(shape, dtype=torch.int32 if uint else torch.float64, device=dev)
                    ptr = int(a.data_ptr())
                else:
                    a = np.empty(shape, dtype=np.uint32 if uint else np.float64)
                    ptr = int(a.ctypes.data)
                out[n] = a
                recs.append(ExrTarget(n.encode("latin-1"), ptr, EXR_SRC_U32 if uint else EXR_SRC_F64, 1, 0, 0))
            if device:
                torch.cuda.synchronize()
            par, res, st = ExrLoadParams(int(threads), 0), ExrLoadResult(), Stats()
            call = self._lib.mcrt_exr_load_device if device else self._lib.mcrt_exr_load
            self._check(call(self._h, f, (ExrTarget * len(recs))(*recs), len(recs), C.byref(par), C.byref(res), C.byref(st)),
                        "mcrt_exr_load_device" if device else "mcrt_exr_load")
        finally:
            self._lib.mcrt_exr_close(f)
        if stats is not None:
            stats.update(st.as_dict())
        info = {"width": fi.width, "height": fi.height, "data_window": tuple(fi.data_window), "display_window": tuple(fi.display_window), "compression": fi.compression,
                "line_order": fi.line_order, "chunks": res.chunks, "raw_chunks": res.raw_chunks, "file_bytes": res.file_bytes, "payload_bytes": res.payload_bytes}
        return out, attributes, info

    def render_converged(self, cam, global_seed, target_relative_error=0.0, max_spp=0, integrator=INTEGRATOR_PATH_TRACER, min_batches=0,
                         channels=("variance",), stats=None):
        """mcrt_render_converged: batches of cam.sqrtspp^2 samples at the seeds global_seed, global_seed + 1, ... merged until the
        frame's relative_error is at most target_relative_error (0 = no target) or one more batch would exceed max_spp (0 = the
        default) -> dict "rgb" [H,W,3], the channels wanted (PIXEL_STATS_CHANNELS and HIGHLIGHT_CHANNELS) of the accumulated frame, and
        "result": batches, spp, final (the frame_noise dict of the delivered frame), relative_error (a list, one per batch, the first 64).
        stats: a dict that receives mcrt_stats, summed over the batches."""
        self._sync_env()
        res = _summary_arrays(["rgb"] + list(channels), (cam.height, cam.width))
        par = ConvergeParams(float(target_relative_error), int(max_spp), int(min_batches))
        out, st = ConvergeResult(), Stats()
        self._check(self._lib.mcrt_render_converged(self._h, C.byref(cam), int(global_seed) & 0xFFFFFFFF, int(integrator), C.byref(par), res["rgb"].ctypes.data,
                                                    C.byref(_addresses(PixelStatsBuffers, res)), C.byref(_addresses(HighlightBuffers, res)), C.byref(out), C.byref(st)),
                    "mcrt_render_converged")
        if stats is not None:
            stats.update(st.as_dict())
        res["result"] = out.as_dict()
        return res

    @staticmethod
    def _adaptive_params(target_relative_error, max_spp=0, floor=0.0, window=None, min_batches=0):
        w = 0 if window is None else ADAPTIVE_WINDOW_NONE if int(window) == 0 else int(window)
        return AdaptiveParams(float(target_relative_error), float(floor), int(max_spp), int(min_batches), w)

    def render_adaptive(self, cam, global_seed, target_relative_error, max_spp=0, floor=0.0, window=None, min_batches=0, channels=("variance",), stats=None):
        """mcrt_render_adaptive: the per-pixel stopping rule. Batches of cam.sqrtspp^2 samples at the seeds global_seed, global_seed + 1,
        ...: batch 0 over the frame, every later one over the list of the pixels that are still noisy - the estimated error of the
        pixel's mean above target_relative_error times its radiance (or `floor`, where that is more; 0.0 = the default, derived from the
        frame) - or have such a pixel within `window` pixels (None = the default, 1; 0 = the pixel alone), until the list is empty or
        max_spp (0 = the default) is reached per pixel. Path tracer only. -> dict "rgb" [H,W,3], the channels wanted
        (PIXEL_STATS_CHANNELS) of the accumulated frame, "count" [H,W] uint32 - the samples every pixel received - and "result": batches,
        min_count, max_count, samples, active (the list's length per batch, the first 64). stats: a dict that receives mcrt_stats,
        summed over the batches."""
        self._sync_env()
        res = _summary_arrays(["rgb"] + list(channels), (cam.height, cam.width), allowed=PIXEL_STATS_CHANNELS)
        count = np.zeros((cam.height, cam.width), dtype=np.uint32)
        par = self._adaptive_params(target_relative_error, max_spp, floor, window, min_batches)
        out, st = AdaptiveResult(), Stats()
        self._check(self._lib.mcrt_render_adaptive(self._h, C.byref(cam), int(global_seed) & 0xFFFFFFFF, C.byref(par), res["rgb"].ctypes.data,
                                                   C.byref(_addresses(PixelStatsBuffers, res)), count.ctypes.data, C.byref(out), C.byref(st)), "mcrt_render_adaptive")
        if stats is not None:
            stats.update(st.as_dict())
        res["count"] = count
        res["result"] = out.as_dict()
        return res

    def adaptive_list(self, flags):
        """mcrt_adaptive_list, a diagnostic for the tests (unstable: no part of the interface to build on): the indices of the flags that are set ([n] uint8), ascending, by the pass's three list
        launches -> [length] uint32."""
        flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        out, length = np.full(flags.size, 0xABABABAB, dtype=np.uint32), C.c_uint32(0)
        self._check(self._lib.mcrt_adaptive_list(self._h, flags.size, flags.ctypes.data, out.ctypes.data, C.byref(length)), "mcrt_adaptive_list")
        assert (out[length.value:] == 0xABABABAB).all()  # nothing behind the list is written
        return out[:length.value]

    def render_adaptive_device(self, cam, global_seed, rgb_ptr, target_relative_error, max_spp=0, floor=0.0, window=None, min_batches=0, stats_pointers=None,
                               count_ptr=None):
        """mcrt_render_adaptive_device: rgb_ptr, stats_pointers = dict statistics channel -> raw device pointer and count_ptr ([H][W]
        uint32), all FULL frames; channels left out or None are not delivered. Synchronous; returns (the result dict of render_adaptive,
        the stats dict)."""
        self._sync_env()
        ps = _pointer_struct(PixelStatsBuffers, stats_pointers, PIXEL_STATS_CHANNELS)
        par = self._adaptive_params(target_relative_error, max_spp, floor, window, min_batches)
        out, st = AdaptiveResult(), Stats()
        self._check(self._lib.mcrt_render_adaptive_device(self._h, C.byref(cam), int(global_seed) & 0xFFFFFFFF, C.byref(par), C.c_void_p(int(rgb_ptr)) if rgb_ptr else None,
                                                          C.byref(ps), C.c_void_p(int(count_ptr)) if count_ptr else None, C.byref(out), C.byref(st)),
                    "mcrt_render_adaptive_device")
        return out.as_dict(), st.as_dict()

    def render_converged_device(self, cam, global_seed, integrator, rgb_ptr, target_relative_error=0.0, max_spp=0, min_batches=0, stats_pointers=None,
                                pointers=None):
        """mcrt_render_converged_device: rgb_ptr, stats_pointers = dict statistics channel -> raw device pointer and pointers = dict
        highlight channel -> raw device pointer, all FULL frames; channels left out or None are not delivered. Synchronous; returns
        (the result dict of render_converged, the stats dict)."""
        self._sync_env()
        hl = _pointer_struct(HighlightBuffers, pointers, HIGHLIGHT_CHANNELS)
        ps = _pointer_struct(PixelStatsBuffers, stats_pointers, PIXEL_STATS_CHANNELS)
        par = ConvergeParams(float(target_relative_error), int(max_spp), int(min_batches))
        out, st = ConvergeResult(), Stats()
        self._check(self._lib.mcrt_render_converged_device(self._h, C.byref(cam), int(global_seed) & 0xFFFFFFFF, int(integrator), C.byref(par),
                                                           C.c_void_p(int(rgb_ptr)) if rgb_ptr else None, C.byref(ps), C.byref(hl), C.byref(out),
                                                           C.byref(st)), "mcrt_render_converged_device")
        return out.as_dict(), st.as_dict()

    def sampler(self, pixel, index, shuffles, global_seed):
        pixel = np.ascontiguousarray(pixel, dtype=np.uint32)
        index = np.ascontiguousarray(index, dtype=np.uint32)
        out = np.empty((pixel.shape[0], 7), dtype=np.float64)
        self._check(self._lib.mcrt_sampler(self._h, pixel.shape[0], _ptr(pixel, C.c_uint32),
                                           _ptr(index, C.c_uint32), int(shuffles), int(global_seed),
                                           _ptr(out, C.c_double)), "mcrt_sampler")
        return out

    def bsdf(self, inputs, consts):
        """mcrt_bsdf: inputs [n][11], consts [10] -> [n][18] (Fresnel / GGX / Oren-Nayar lobe values, include/mcrt.h)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        consts = np.ascontiguousarray(consts, dtype=np.float64)
        out = np.zeros((inputs.shape[0], 18))
        self._check(self._lib.mcrt_bsdf(self._h, inputs.shape[0], _ptr(inputs, C.c_double), _ptr(consts, C.c_double), _ptr(out, C.c_double)), "mcrt_bsdf")
        return out

    def libm(self, fn, a, b=None):
        """mcrt_libm: the device's sincos (fn 0 -> (sin, cos)), sin (1), cos (2), asin (3), atan2 (4: a = y, b = x), sincosf (5: float
        values in, (sin, cos) widened out), pow (6: a ** b) on arrays."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        out0, out1 = np.zeros_like(a), np.zeros_like(a)
        bb = np.ascontiguousarray(b, dtype=np.float64) if b is not None else None
        self._check(self._lib.mcrt_libm(self._h, int(fn), a.size, _ptr(a, C.c_double), _ptr(bb, C.c_double) if bb is not None else None,
                                        _ptr(out0, C.c_double), _ptr(out1, C.c_double)), "mcrt_libm")
        return (out0, out1) if fn in (LIBM_SINCOS, LIBM_SINCOSF) else out0

    def knn(self, which, points, k):
        self._sync_env()
        points = np.ascontiguousarray(points, dtype=np.float64)
        n = points.shape[0]
        cnt = np.empty(n, dtype=np.uint32)
        idx = np.empty((n, k), dtype=np.uint32)
        d2 = np.empty((n, k), dtype=np.float64)
        self._check(self._lib.mcrt_knn(self._h, int(which), n, _ptr(points, C.c_double), int(k),
                                       _ptr(cnt, C.c_uint32), _ptr(idx, C.c_uint32),
                                       _ptr(d2, C.c_double)), "mcrt_knn")
        return cnt, idx, d2

    def close(self):
        if self._h:
            self._lib.mcrt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_rows(cam):
    """Row indices owned by cam's (shard_index, shard_count, shard_rows)."""
    L = lib()
    n = L.mcrt_shard_rows(C.byref(cam), None)
    rows = np.empty(n, dtype=np.uint32)
    if n:
        L.mcrt_shard_rows(C.byref(cam), _ptr(rows, C.c_uint32))
    return rows
