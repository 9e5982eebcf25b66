"""ctypes bindings over the two in-tree native libraries of the product:

  csrc/librl_render.so  — the C-ABI drop-in boundary (include/rl_render.h): HIP kernels for gfx950.
  host/librl_host.so    — the C++ host mirror of the reference's scene-building API
                          (CameraParams/Camera::new, Sphere/Bvh/..., World, OBJ loaders, PPM writers).

Python here is plumbing only (tests, bench.py, torch.distributed): no arithmetic of the hot path
lives in this file, and there is NO CPU fallback — if librl_render.so is missing or no GPU is
present, every render call raises.

Class / function names mirror the reference:
  CameraParams, Camera(params).render(world) -> Canvas, render_from_checkpoint, Canvas.merge,
  output_ppm            <- ray-tracing-one-weekend/src/{camera.rs:23-143,263-296, output.rs:5}
  RtcCamera.render(world, aa) -> ppm via canvas_ppm
                        <- ray-tracer-challenge/src/scene/camera.rs:93, draw/canvas.rs:50
"""
import ctypes as C
import os
import threading
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RL_RENDER_LIB selects another build of the same ABI (csrc/librl_render_verify.so, or a build of another commit for an A/B run)
RENDER_LIB = os.environ.get("RL_RENDER_LIB") or os.path.join(_HERE, "csrc", "librl_render.so")
HOST_LIB = os.path.join(_HERE, "host", "librl_host.so")

RL_OK, RL_E_INVALID, RL_E_NO_DEVICE, RL_E_DEVICE, RL_E_UNSUPPORTED, RL_E_DEGENERATE, RL_E_NOMEM = 0, -1, -2, -3, -4, -5, -6


class RLError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rl error {code}: {msg}")
        self.code = code


# ----------------------------------------------------------------------------- C structs
class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("node_tests", C.c_uint64), ("sphere_tests", C.c_uint64),
                ("planar_tests", C.c_uint64), ("instance_enters", C.c_uint64), ("rng_words", C.c_uint64),
                ("flagged", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RtiowCamera(C.Structure):
    _fields_ = [("image_width", C.c_uint32), ("image_height", C.c_uint32),
                ("samples_per_pixel", C.c_uint32), ("max_depth", C.c_uint32),
                ("lookfrom", C.c_double * 3), ("pixel_00", C.c_double * 3),
                ("pixel_du", C.c_double * 3), ("pixel_dv", C.c_double * 3),
                ("defocus_disk_u", C.c_double * 3), ("defocus_disk_v", C.c_double * 3),
                ("defocus_angle", C.c_double), ("background", C.c_double * 3), ("seed", C.c_uint64)]


class RtcCamera(C.Structure):
    _fields_ = [("hsize", C.c_uint32), ("vsize", C.c_uint32), ("inverse", C.c_double * 16),
                ("pixel_size", C.c_double), ("half_width", C.c_double), ("half_height", C.c_double)]


class _HCameraParams(C.Structure):
    _fields_ = [("aspect_ratio", C.c_double), ("image_width", C.c_uint64), ("samples_per_pixel", C.c_uint64),
                ("max_depth", C.c_uint64), ("vfov", C.c_double), ("lookfrom", C.c_double * 3),
                ("lookat", C.c_double * 3), ("vup", C.c_double * 3), ("defocus_angle", C.c_double),
                ("focus_dist", C.c_double), ("background", C.c_double * 3), ("seed", C.c_uint64)]


# numpy dtypes of the POD scene records (include/rl_render.h) for Python-built scenes
HREF = np.dtype([("kind", "<u4"), ("index", "<u4")])
SPHERE = np.dtype([("center0", "<f8", 3), ("center1", "<f8", 3), ("radius", "<f8"), ("moving", "<u4"), ("material", "<u4")])
MATERIAL = np.dtype([("kind", "<u4"), ("texture", "<u4"), ("albedo", "<f8", 3), ("fuzz", "<f8"), ("ior", "<f8")])
TEXTURE = np.dtype([("kind", "<u4"), ("even", "<u4"), ("odd", "<u4"), ("image", "<u4"), ("color", "<f8", 3), ("inv_scale", "<f8")])
PERLIN = np.dtype([("randvec", "<f8", (256, 3)), ("perm_x", "<u4", 256), ("perm_y", "<u4", 256), ("perm_z", "<u4", 256)])
RTC_TRIANGLE = np.dtype([("p1", "<f8", 3), ("e1", "<f8", 3), ("e2", "<f8", 3), ("smooth", "<u4"), ("material", "<u4"),
                         ("n1", "<f8", 3), ("n2", "<f8", 3), ("n3", "<f8", 3)])
RTC_GROUP = np.dtype([("first", "<u4"), ("count", "<u4")])
RTC_BOUNDED = np.dtype([("minimum", "<f8", 3), ("maximum", "<f8", 3), ("child", HREF)])
RTC_TRANSFORMED = np.dtype([("inverse", "<f8", 16), ("inverse_transpose", "<f8", 16), ("child", HREF)])
RTC_MATERIAL = np.dtype([("color", "<f8", 3), ("ambient", "<f8"), ("diffuse", "<f8"), ("specular", "<f8"), ("shininess", "<f8"),
                         ("reflectivity", "<f8"), ("transparency", "<f8"), ("refractive_index", "<f8"), ("pattern", "<u4"), ("reserved", "<u4")])
RTC_SHAPE = np.dtype([("kind", "<u4"), ("material", "<u4"), ("has_minimum", "<u4"), ("has_maximum", "<u4"), ("closed", "<u4"), ("reserved", "<u4"),
                      ("minimum", "<f8"), ("maximum", "<f8")])
RTC_CSG = np.dtype([("operation", "<u4"), ("reserved", "<u4"), ("left", HREF), ("right", HREF)])
RTC_PATTERN = np.dtype([("kind", "<u4"), ("reserved", "<u4"), ("a", "<f8", 3), ("b", "<f8", 3), ("inverse", "<f8", 16)])
RTC_LIGHT = np.dtype([("position", "<f8", 3), ("intensity", "<f8", 3)])
# ray queries (rl_ray / rl_rtiow_hit / rl_rtc_isect)
RAY = np.dtype([("origin", "<f8", 3), ("dir", "<f8", 3), ("time", "<f8")])
RTIOW_HIT = np.dtype([("t", "<f8"), ("p", "<f8", 3), ("normal", "<f8", 3), ("u", "<f8"), ("v", "<f8"),
                      ("hit", "<u4"), ("front_face", "<u4"), ("material", "<u4"), ("_pad", "<u4")])
RTC_ISECT = np.dtype([("t", "<f8"), ("normal", "<f8", 3), ("object", "<u4"), ("_pad", "<u4")])
assert RAY.itemsize == 56 and RTIOW_HIT.itemsize == 88 and RTC_ISECT.itemsize == 40
# material queries (rl_rtiow_scatter)
SCATTER = np.dtype([("attenuation", "<f8", 3), ("emitted", "<f8", 3), ("scattered", RAY), ("scatter", "<u4"), ("_pad", "<u4")])
assert SCATTER.itemsize == 112
# RTC shading queries (rl_rtc_comps / rl_rtc_shade)
RTC_COMPS = np.dtype([("t", "<f8"), ("point", "<f8", 3), ("eye_v", "<f8", 3), ("normal_v", "<f8", 3), ("over_point", "<f8", 3),
                      ("under_point", "<f8", 3), ("reflect_v", "<f8", 3), ("n1", "<f8"), ("n2", "<f8"), ("object_color", "<f8", 3),
                      ("hit", "<u4"), ("inside", "<u4"), ("object", "<u4"), ("material", "<u4")])
RTC_SHADE = np.dtype([("surface", "<f8", 3), ("schlick", "<f8"), ("reflected", RAY), ("refracted", RAY), ("reflect", "<u4"), ("refract", "<u4")])
assert RTC_COMPS.itemsize == 208 and RTC_SHADE.itemsize == 152
# the compiled RTC program as the kernels read it (csrc/rl_program.h DevOp / DevTri / RtcGuard; rtc_program)
RTC_DEV_OP = np.dtype([("box", "<f8", 6), ("code", "<u4"), ("skip", "<u4"), ("a", "<u4"), ("b", "<u4")])
RTC_DEV_TRI = np.dtype([("p1", "<f8", 3), ("e1", "<f8", 3), ("e2", "<f8", 3), ("n1", "<f8", 3), ("n2", "<f8", 3), ("n3", "<f8", 3),
                        ("smooth", "<u4"), ("material", "<u4"), ("_pad", "<f8")])
RTC_GUARD = np.dtype([("box", "<f4", 6), ("skip", "<u4"), ("tri", "<u4")])
assert RTC_DEV_OP.itemsize == 64 and RTC_DEV_TRI.itemsize == 160 and RTC_GUARD.itemsize == 32
ROP_END, ROP_ENTER, ROP_EXIT, ROP_BOUNDS, ROP_TRIS = 0, 1, 2, 3, 4
# one record of the RTIOW launch log (csrc/rl_rtiow_launch.h RtiowLaunchRecord)
RTIOW_LAUNCH = np.dtype([("kernel", "S192"), ("seq", "<u8"), ("work_items", "<u8"), ("lds_bytes", "<u8"), ("funnel", "<u4"), ("wg_size", "<u4"),
                         ("blocks", "<u4"), ("sample_begin", "<u4"), ("sample_end", "<u4"), ("resume", "<u4"), ("tile_order", "<u4"),
                         ("steal_state", "<u4"), ("fg_top", "<u4"), ("tune", "<u4", 4), ("n_pixels", "<u4")])
assert RTIOW_LAUNCH.itemsize == 272
RTIOW_LAUNCH_LOG = 64  # records the library keeps
NEVER_OFFERED = 0xFFFFFFFF  # steal_record: a pixel no lane released
NO_HIT = 0xFFFFFFFF  # out_hit_index of a ray hit() returns None for

MAT_FLAT, MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC = 0, 1, 2, 3, 4, 5
TEX_SOLID, TEX_CHECKER, TEX_IMAGE, TEX_NOISE = 0, 1, 2, 3
O_TRIANGLE, O_GROUP, O_BOUNDED, O_TRANSFORMED, O_SPHERE, O_PLANE, O_CUBE, O_CYLINDER, O_CONE, O_CSG = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
CSG_UNION, CSG_INTERSECTION, CSG_DIFFERENCE = 0, 1, 2
PAT_STRIPE, PAT_RING, PAT_GRADIENT, PAT_CHECKER3D = 1, 2, 3, 4


class RtiowSceneDesc(C.Structure):  # rl_rtiow_scene_desc
    _fields_ = [("spheres", C.c_void_p), ("n_spheres", C.c_uint32),
                ("planars", C.c_void_p), ("n_planars", C.c_uint32),
                ("translates", C.c_void_p), ("n_translates", C.c_uint32),
                ("transforms", C.c_void_p), ("n_transforms", C.c_uint32),
                ("bvh_nodes", C.c_void_p), ("n_bvh_nodes", C.c_uint32),
                ("lists", C.c_void_p), ("n_lists", C.c_uint32),
                ("list_items", C.c_void_p), ("n_list_items", C.c_uint32),
                ("materials", C.c_void_p), ("n_materials", C.c_uint32),
                ("textures", C.c_void_p), ("n_textures", C.c_uint32),
                ("images", C.c_void_p), ("n_images", C.c_uint32),
                ("root", C.c_uint32 * 2),
                ("perlins", C.c_void_p), ("n_perlins", C.c_uint32),
                ("media", C.c_void_p), ("n_media", C.c_uint32)]


class RtcSceneDesc(C.Structure):
    _fields_ = [("triangles", C.c_void_p), ("n_triangles", C.c_uint32),
                ("groups", C.c_void_p), ("n_groups", C.c_uint32),
                ("group_items", C.c_void_p), ("n_group_items", C.c_uint32),
                ("boundeds", C.c_void_p), ("n_boundeds", C.c_uint32),
                ("transformeds", C.c_void_p), ("n_transformeds", C.c_uint32),
                ("materials", C.c_void_p), ("n_materials", C.c_uint32),
                ("objects", C.c_void_p), ("n_objects", C.c_uint32),
                ("lights", C.c_void_p), ("n_lights", C.c_uint32),
                ("max_reflection_depth", C.c_uint32), ("reserved", C.c_uint32),
                ("void_color", C.c_double * 3),
                ("shapes", C.c_void_p), ("n_shapes", C.c_uint32),
                ("csgs", C.c_void_p), ("n_csgs", C.c_uint32),
                ("patterns", C.c_void_p), ("n_patterns", C.c_uint32)]


class RtiowAdaptive(C.Structure):  # rl_rtiow_adaptive
    _fields_ = [("min_samples", C.c_uint32), ("check_every", C.c_uint32), ("abs_variance", C.c_double), ("rel_variance", C.c_double)]


class RtiowFeatures(C.Structure):  # rl_rtiow_features: each pointer optional (None), all None is refused
    _fields_ = [("albedo_sum", C.c_void_p), ("normal_sum", C.c_void_p), ("depth_sum", C.c_void_p), ("hit_count", C.c_void_p)]


# name -> (dtype, trailing shape), in the struct's order
FEATURE_TABLE = {"albedo_sum": (np.float64, (3,)), "normal_sum": (np.float64, (3,)), "depth_sum": (np.float64, ()), "hit_count": (np.uint32, ())}
FEATURE_OUTPUTS = tuple(FEATURE_TABLE)


class AtrousParams(C.Structure):  # rl_atrous_params
    _fields_ = [("color_sigma2", C.c_double), ("variance_floor", C.c_double), ("n_guides", C.c_uint32), ("reserved", C.c_uint32),
                ("guide_inv_sigma", C.c_double * 8)]


class DenoiseInputs(C.Structure):  # rl_denoise_inputs: device pointers in the _device forms, host pointers in rl_denoise_render
    _fields_ = [("sums", C.c_void_p), ("sq", C.c_void_p), ("counts", C.c_void_p), ("albedo_sum", C.c_void_p), ("normal_sum", C.c_void_p),
                ("depth_sum", C.c_void_p), ("hit_count", C.c_void_p), ("samples", C.c_uint32), ("feature_samples", C.c_uint32), ("want", C.c_uint32),
                ("reserved", C.c_uint32)]


GUIDE_BITS = {"albedo": 1, "normal": 2, "depth": 4, "coverage": 8}  # RL_GUIDE_*


# ----------------------------------------------------------------------------- signatures
# One table per library, name -> (restype, argtypes), applied once when the library is loaded (_load): the only statement of a C
# signature on the Python side.  tests/test_binding_signatures.py compares both tables with the C text: include/rl_render.h, the
# rl_debug_* definitions under csrc/ (no header declares them) and the rlh_* definitions in host/*.cpp.  A new entry point costs one line
# here.  restype: None = void; a function that returns a pointer MUST say c_void_p / c_char_p (the default, c_int, would cut it to 32 bits).
_P, _S, _I, _U, _U32, _U64, _D = C.c_void_p, C.c_char_p, C.c_int, C.c_uint, C.c_uint32, C.c_uint64, C.c_double
_PU32, _PU64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_CAM, _RTC_CAM, _STATS = C.POINTER(RtiowCamera), C.POINTER(RtcCamera), C.POINTER(Stats)
_ADAPTIVE, _FEATURES, _ATROUS, _DENOISE_IN = C.POINTER(RtiowAdaptive), C.POINTER(RtiowFeatures), C.POINTER(AtrousParams), C.POINTER(DenoiseInputs)

RENDER_SIGNATURES = {
    # ---- include/rl_render.h, in its order of topics
    "rl_init": (_I, [_I]),
    "rl_init_multi": (_I, [_I]),
    "rl_device_count": (_I, []),
    "rl_shutdown": (None, []),
    "rl_last_error": (_S, []),
    "rl_abi_version": (_I, []),
    "rl_device_info": (_I, [_S, _I]),
    "rl_rtiow_render_progress": (_I, [_P, _PU64, _PU64, _PU32]),
    "rl_scene_destroy": (None, [_P]),
    "rl_render_status": (_I, [_P, _STATS]),
    "rl_rtiow_scene_create": (_P, [_P]),
    "rl_bvh_build": (_I, [_P, _P, _U32, _U32, _P, _U32, _P]),
    "rl_rtiow_render": (_I, [_P, _CAM, _U64, _P, _STATS]),
    "rl_rtiow_render_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _P, _STATS]),
    "rl_rtiow_render_device": (_I, [_P, _CAM, _U64, _U32, _U32, _P, _P, _STATS]),
    "rl_rtiow_render_independent_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _STATS]),
    "rl_rtiow_render_independent_device": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _P, _STATS]),
    "rl_rtiow_render_multi": (_I, [_P, _CAM, _U64, _P, _STATS]),
    "rl_rtiow_render_multi_device": (_I, [_P, _CAM, _U64, _P, _STATS]),
    "rl_rtiow_encode_rgb8_device": (_I, [_P, _U64, _U32, _P, _P]),
    "rl_rtiow_render_rgb8": (_I, [_P, _CAM, _U64, _P, _STATS]),
    "rl_rtc_scene_create": (_P, [_P]),
    "rl_rtc_render": (_I, [_P, _RTC_CAM, _U32, _P, _STATS]),
    "rl_rtc_render_rows": (_I, [_P, _RTC_CAM, _U32, _U32, _U32, _P, _STATS]),
    "rl_rtc_render_device": (_I, [_P, _RTC_CAM, _U32, _U32, _U32, _P, _P, _STATS]),
    "rl_rtc_render_multi": (_I, [_P, _RTC_CAM, _U32, _P, _STATS]),
    "rl_rtc_render_multi_device": (_I, [_P, _RTC_CAM, _U32, _P, _STATS]),
    "rl_rtc_encode_rgb8_device": (_I, [_P, _U64, _P, _P]),
    "rl_rtc_render_rgb8": (_I, [_P, _RTC_CAM, _U32, _P, _STATS]),
    "rl_rtiow_hit_rays": (_I, [_P, _P, _U64, _D, _D, _P, _STATS]),
    "rl_rtiow_hit_rays_device": (_I, [_P, _P, _U64, _D, _D, _P, _P, _STATS]),
    "rl_rtc_intersect_rays": (_I, [_P, _P, _U64, _U32, _P, _P, _P, _STATS]),
    "rl_rtc_intersect_rays_device": (_I, [_P, _P, _U64, _U32, _P, _P, _P, _P, _STATS]),
    "rl_rtc_color_at_rays": (_I, [_P, _P, _U64, _P, _STATS]),
    "rl_rtc_color_at_rays_device": (_I, [_P, _P, _U64, _P, _P, _STATS]),
    "rl_rtiow_camera_rays": (_I, [_CAM, _U64, _P, _P, _P, _P, _P]),
    "rl_rtiow_camera_rays_device": (_I, [_CAM, _U64, _P, _P, _P, _P, _P, _P]),
    "rl_rtiow_ray_color_rays": (_I, [_P, _P, _P, _U64, _U64, _U32, C.POINTER(_D), _P, _P, _P, _STATS]),
    "rl_rtiow_ray_color_rays_device": (_I, [_P, _P, _P, _U64, _U64, _U32, C.POINTER(_D), _P, _P, _P, _P, _STATS]),
    "rl_rtiow_scatter_rays": (_I, [_P, _P, _P, _P, _U64, _U64, _P, _P, _STATS]),
    "rl_rtiow_scatter_rays_device": (_I, [_P, _P, _P, _P, _U64, _U64, _P, _P, _P, _STATS]),
    "rl_rtiow_texture_values": (_I, [_P, _P, _P, _P, _U64, _P]),
    "rl_rtiow_texture_values_device": (_I, [_P, _P, _P, _P, _U64, _P, _P]),
    "rl_rtiow_hit_rays_seeded": (_I, [_P, _P, _P, _U64, _U64, _D, _D, _P, _P, _STATS]),
    "rl_rtiow_hit_rays_seeded_device": (_I, [_P, _P, _P, _U64, _U64, _D, _D, _P, _P, _P, _STATS]),
    "rl_rtc_prepare_rays": (_I, [_P, _P, _U64, _P, _STATS]),
    "rl_rtc_prepare_rays_device": (_I, [_P, _P, _U64, _P, _P, _STATS]),
    "rl_rtc_shade_hits": (_I, [_P, _P, _U64, _P, _P, _STATS]),
    "rl_rtc_shade_hits_device": (_I, [_P, _P, _U64, _P, _P, _P, _STATS]),
    "rl_rtc_shadow_attenuation": (_I, [_P, _P, _P, _U64, _P, _STATS]),
    "rl_rtc_shadow_attenuation_device": (_I, [_P, _P, _P, _U64, _P, _P, _STATS]),
    "rl_rtc_lighting": (_I, [_P, _P, _P, _P, _P, _U64, _P]),
    "rl_rtc_lighting_device": (_I, [_P, _P, _P, _P, _P, _U64, _P, _P]),
    "rl_rtiow_occluded_rays": (_I, [_P, _P, _U64, _D, _D, _P, _STATS]),
    "rl_rtiow_occluded_rays_device": (_I, [_P, _P, _U64, _D, _D, _P, _P, _STATS]),
    "rl_rtiow_render_pixels": (_I, [_P, _CAM, _U64, _P, _P, _U64, _P, _STATS]),
    "rl_rtiow_render_pixels_device": (_I, [_P, _CAM, _U64, _P, _P, _U64, _P, _P, _STATS]),
    "rl_rtc_render_pixels": (_I, [_P, _RTC_CAM, _U32, _P, _P, _U64, _P, _STATS]),
    "rl_rtc_render_pixels_device": (_I, [_P, _RTC_CAM, _U32, _P, _P, _U64, _P, _P, _STATS]),
    "rl_rtiow_render_moments_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _P, _P, _STATS]),
    "rl_rtiow_render_moments_device": (_I, [_P, _CAM, _U64, _U32, _U32, _P, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_moments": (_I, [_P, _CAM, _U64, _P, _P, _U64, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_moments_device": (_I, [_P, _CAM, _U64, _P, _P, _U64, _P, _P, _P, _STATS]),
    "rl_rtiow_render_adaptive_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _ADAPTIVE, _P, _P, _P, _STATS]),
    "rl_rtiow_render_adaptive_device": (_I, [_P, _CAM, _U64, _U32, _U32, _ADAPTIVE, _P, _P, _P, _P, _STATS]),
    "rl_rtiow_render_features_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _FEATURES, _STATS]),
    "rl_rtiow_render_features_device": (_I, [_P, _CAM, _U64, _U32, _U32, _FEATURES, _P, _STATS]),
    "rl_rtiow_render_pixels_features": (_I, [_P, _CAM, _U64, _P, _P, _U64, _FEATURES, _STATS]),
    "rl_rtiow_render_pixels_features_device": (_I, [_P, _CAM, _U64, _P, _P, _U64, _FEATURES, _P, _STATS]),
    "rl_rtiow_render_ao_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _D, _P, _P, _STATS]),
    "rl_rtiow_render_ao_device": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _D, _P, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_ao": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _D, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_ao_device": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _D, _P, _P, _P, _STATS]),
    "rl_rtiow_render_direct_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _U32, _D, _P, _P, _P, _STATS]),
    "rl_rtiow_render_direct_device": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _U32, _D, _P, _P, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_direct": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _P, _U32, _D, _P, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_direct_device": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _P, _U32, _D, _P, _P, _P, _P, _STATS]),
    "rl_rtiow_render_nee_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _U32, _D, _P, _P, _STATS]),
    "rl_rtiow_render_nee_device": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _U32, _D, _P, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_nee": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _P, _U32, _D, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_nee_device": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _P, _U32, _D, _P, _P, _P, _STATS]),
    "rl_rtiow_render_nee_mis_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _U32, _D, _U32, _P, _P, _STATS]),
    "rl_rtiow_render_nee_mis_device": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _U32, _D, _U32, _P, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_nee_mis": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _P, _U32, _D, _U32, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_nee_mis_device": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _P, _U32, _D, _U32, _P, _P, _P, _STATS]),
    "rl_rtiow_render_nee_mis_spheres_rows": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _U32, _P, _U32, _D, _U32, _P, _P, _STATS]),
    "rl_rtiow_render_nee_mis_spheres_device": (_I, [_P, _CAM, _U64, _U32, _U32, _U32, _P, _U32, _P, _U32, _D, _U32, _P, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_nee_mis_spheres": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _P, _U32, _P, _U32, _D, _U32, _P, _P, _STATS]),
    "rl_rtiow_render_pixels_nee_mis_spheres_device": (_I, [_P, _CAM, _U64, _P, _P, _U64, _U32, _P, _U32, _P, _U32, _D, _U32, _P, _P, _P, _STATS]),
    "rl_denoise_atrous_pass_device": (_I, [_U32, _U32, _U32, _ATROUS, _P, _P, _P, _P, _P, _P]),
    "rl_denoise_atrous": (_I, [_U32, _U32, _U32, _ATROUS, _P, _P, _P, _P, _P]),
    "rl_denoise_prepare_device": (_I, [_U32, _U32, _DENOISE_IN, _P, _P, _P, _P]),
    "rl_denoise_finish_device": (_I, [_U32, _U32, _P, _P, _P, _U32, _P, _P, _P, _P]),
    "rl_denoise_render_work_bytes": (_U64, [_U32, _U32, _U32]),
    "rl_denoise_render_device": (_I, [_U32, _U32, _DENOISE_IN, _U32, _ATROUS, _P, _U64, _P, _P, _P, _P]),
    "rl_denoise_render": (_I, [_U32, _U32, _DENOISE_IN, _U32, _ATROUS, _P, _P, _P]),
    "rl_rtiow_render_denoised_rgb8": (_I, [_P, _CAM, _ADAPTIVE, _U32, _U32, _U32, _ATROUS, _P]),
    # ---- the rl_debug_* entry points of csrc/ (switches and read-outs for tests and tools)
    "rl_debug_init_multi_emulated": (_I, [_I]),
    "rl_debug_rccl_loadable": (_I, []),
    "rl_debug_multi_uses_rccl": (_I, []),
    "rl_debug_host_structures": (_I, [_P, _P]),
    "rl_debug_set_rtiow_variant": (None, [_I]),
    "rl_debug_set_lpt": (None, [_I]),
    "rl_debug_set_coop": (None, [_I]),
    "rl_debug_set_coop_pixels_max": (None, [_U64]),
    "rl_debug_set_steal": (None, [_D]),
    "rl_debug_set_fast_traversal": (None, [_I]),
    "rl_debug_set_rtc_blocks": (None, [_I]),
    "rl_debug_set_indep_cap": (None, [_U64]),
    "rl_debug_set_indep_k": (None, [_U]),
    "rl_debug_set_pixel_entry": (None, [_I]),
    "rl_debug_set_pixel_entry_sphere": (None, [_I]),
    "rl_debug_pixel_entry_read": (_I, [_P, _P, _U64]),
    "rl_debug_set_pixel_entry_time": (None, [_I]),
    "rl_debug_set_pixel_entry_reuse": (None, [_I]),
    "rl_debug_pixel_entry_builds": (_U64, []),
    "rl_debug_pixel_entry_time_read": (_I, [_P, _P, _U64, _U32]),
    "rl_debug_pixel_entry_census": (_I, [_P, _P]),
    "rl_debug_fast_tree": (_I, [_P, _P, _U32, _PU32]),
    "rl_debug_set_fastg_one_wave": (None, [_I]),
    "rl_debug_set_status_gap": (_I, [_U, _U]),
    "rl_debug_fast_stats": (None, [_I]),
    "rl_debug_fastg_verify": (_I, [_P, _P]),
    "rl_debug_fastg_counts": (_I, [_P]),
    "rl_debug_slow_traces": (_U64, []),
    "rl_debug_live_buffers": (None, [_P]),
    "rl_debug_sched": (_I, [_P, _P]),
    "rl_debug_pixel_rays": (_I, [_P, _U64]),
    "rl_debug_pixel_rays_read": (_I, [_P, _P, _U64]),
    "rl_debug_last_query": (_I, [_P]),
    "rl_debug_set_query_pass_cap": (None, [_U64]),
    "rl_debug_material_query_lanes": (_U64, []),
    "rl_debug_features_lanes": (_U64, []),
    "rl_debug_set_denoise_route": (None, [_I]),
    "rl_debug_last_denoise_route": (_I, []),
    "rl_debug_set_denoise_blocks": (None, [_U32]),
    "rl_debug_last_denoise_launch": (None, [_P]),
    "rl_debug_rtc_program": (_I, [_P, _P, _P, _P, _PU64, _PU64]),
    "rl_debug_last_rtc_launch": (None, [_P]),
    "rl_debug_rtiow_launch_total": (_U64, []),
    "rl_debug_rtiow_launch_log": (_I, [_P, _U32]),
    "rl_debug_steal_read": (_I, [_P, _PU32, _PU32, _U64]),
}
# every symbol include/rl_render.h declares (checked by tests/test_abi.py)
RENDER_SYMBOLS = [n for n in RENDER_SIGNATURES if not n.startswith("rl_debug_")]

_HPARAMS = C.POINTER(_HCameraParams)
HOST_SIGNATURES = {  # the rlh_* entry points this file calls; test-only probes are declared by the tests that use them
    "rlh_last_error": (_S, []),
    "rlh_free": (None, [_P]),
    "rlh_rtiow_golden_test_scene": (_P, []),
    "rlh_rtiow_bouncing_spheres": (_P, [_U64]),
    "rlh_rtiow_cow_scene": (_P, [_S, _U64, _P, _U32, _U32]),
    "rlh_rtiow_perlin_scene": (_P, [_I]),
    "rlh_rtiow_earth_scene": (_P, [_P, _U32, _U32]),
    "rlh_rtiow_example_scene": (_P, [_S, _S, _U64, _P, _U32, _U32]),
    "rlh_rtiow_stress_scene": (_P, [_I, _I, _S, _U64, _P, _U32, _U32, _U64, _I]),
    "rlh_rtiow_from_spheres": (_P, [_P, _U32, _P, _U32, _P, _U32, _I]),
    "rlh_rtiow_desc": (_P, [_P]),
    "rlh_rtiow_free": (None, [_P]),
    "rlh_rtiow_counts": (None, [_P, _P]),
    "rlh_rtiow_get_params": (None, [_P, _HPARAMS]),
    "rlh_rtiow_camera_new": (_I, [_HPARAMS, _CAM]),
    "rlh_rtiow_output_ppm": (_P, [_P, _U64, _U64, _U64, _PU64]),
    "rlh_canvas_to_bincode": (_P, [_U64, _U64, _U64, _P, _U64, _PU64]),
    "rlh_canvas_from_bincode": (_I, [_S, _U64, _PU64, _PU64, _PU64, _PU64]),
    "rlh_builder_new": (_P, []),
    "rlh_builder_free": (None, [_P]),
    "rlh_b_solid": (_I, [_P, _P]),
    "rlh_b_checker": (_I, [_P, _D, _I, _I]),
    "rlh_b_image": (_I, [_P, _P, _U32, _U32]),
    "rlh_b_noise": (_I, [_P, _D, _U64]),
    "rlh_b_material": (_I, [_P, _U32, _I, _P, _D, _D]),
    "rlh_b_sphere": (_I, [_P, _P, _P, _D, _I]),
    "rlh_b_planar": (_I, [_P, _U32, _P, _P, _P, _I]),
    "rlh_b_triangle": (_I, [_P, _P, _P, _P, _I]),
    "rlh_b_translate": (_I, [_P, _I, _P]),
    "rlh_b_medium": (_I, [_P, _I, _D, _I]),
    "rlh_b_transform": (_I, [_P, _I, _I, _D]),
    "rlh_b_group": (_I, [_P, _P, _U32, _I]),
    "rlh_b_obj": (_I, [_P, _S, _U64, _I]),
    "rlh_b_finish": (_P, [_P, _I]),
    "rlh_rtc_test_obj_scene": (_P, [_S, _U64, _U64, _U64]),
    "rlh_rtc_named_scene": (_P, [_I, _U64, _U64]),
    "rlh_rtc_desc": (_P, [_P]),
    "rlh_rtc_get_camera": (None, [_P, _RTC_CAM]),
    "rlh_rtc_free": (None, [_P]),
    "rlh_rtc_camera_new": (_I, [_U64, _U64, _D, _P, _P, _P, _RTC_CAM]),
    "rlh_rtc_camera_from_matrix": (_I, [_U64, _U64, _D, _P, _RTC_CAM]),
    "rlh_rtc_make_transformed": (_I, [_P, _P]),
    "rlh_rtc_rotation": (None, [_I, _D, _P]),
    "rlh_rtc_matmul": (None, [_P, _P, _P]),
    "rlh_rtc_invert": (_I, [_P, _P]),
    "rlh_rtc_canvas_ppm": (_P, [_P, _U64, _U64, _PU64]),
    "rlh_direct_probe": (_I, [_U64, _U64, _U64, _U32, _P, _U32, _D, _P, _P, _P]),  # (direct.py's cpp_mirror_probe)
    "rlh_nee_probe": (_I, [_U64, _U64, _U64, _U32, _P, _U32, _D, _P, _P]),  # (nee.py's cpp_mirror_probe)
    "rlh_nee_mis_probe": (_I, [_U64, _U64, _U64, _U32, _P, _U32, _D, _U32, _P, _P]),  # (nee.py's cpp_mirror_probe_mis)
    "rlh_nee_spheres_probe": (_I, [_U64, _U64, _U64, _U32, _P, _U32, _P, _U32, _D, _U32, _P, _P]),  # (nee.py's cpp_mirror_probe_spheres)
}


# ----------------------------------------------------------------------------- library loading
_host = None
_render = None
_create_mu = threading.Lock()  # World / RtcWorld.device(): two threads' first renders of one world must not upload it twice


def _one_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7; librl_render.so links the system one (/opt/rocm).  A process that
    ends up with BOTH sees the GPU only through whichever initialises first.  If torch is importable it is therefore imported
    BEFORE the product library is loaded: the dynamic loader then resolves librl_render.so's libamdhip64.so.7 to the copy torch
    already mapped (same SONAME) and the process has one runtime.  RL_NO_TORCH_PRELOAD=1 skips this (pure C / ctypes hosts)."""
    import sys
    if "torch" in sys.modules or os.environ.get("RL_NO_TORCH_PRELOAD"):
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def _pixel_list(xs, ys):
    """The (xs, ys) of a pixel-list render as two contiguous uint32 arrays; ValueError for what is not a list of pixel coordinates."""
    xs, ys = np.asarray(xs), np.asarray(ys)
    for name, a in (("xs", xs), ("ys", ys)):
        if a.ndim != 1:
            raise ValueError(f"{name} must be one-dimensional, got shape {a.shape}")
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must hold integers, got dtype {a.dtype}")
    if xs.shape != ys.shape:
        raise ValueError(f"xs and ys differ in length: {xs.size} and {ys.size}")
    for name, a in (("xs", xs), ("ys", ys)):
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError(f"{name} holds a value that is not a pixel coordinate (negative, or beyond 32 bits)")
    return np.ascontiguousarray(xs, dtype=np.uint32), np.ascontiguousarray(ys, dtype=np.uint32)


def _load(path, signatures, hint):
    """CDLL(path) with every signature of its table applied: the one place that assigns restype / argtypes.  A symbol the library lacks
    is skipped — RL_RENDER_LIB may select an older build of the ABI for an A/B run — and calling it then fails loudly (AttributeError)."""
    _one_hip_runtime()  # (librl_host.so links librl_render.so)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not built — {hint}run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(path)
    for name, (restype, argtypes) in signatures.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


def host_lib():
    global _host
    if _host is None:
        _host = _load(HOST_LIB, HOST_SIGNATURES, "")
    return _host


def render_lib():
    """The HIP product library. Fails loudly when it is not built."""
    global _render
    if _render is None:
        _render = _load(RENDER_LIB, RENDER_SIGNATURES, "the HIP extension is required (no CPU fallback); ")
    return _render


_inited = False


def init(device=-1):
    global _inited
    L = render_lib()
    rc = L.rl_init(int(device))
    if rc != RL_OK:
        raise RLError(rc, L.rl_last_error().decode())
    _inited = True


def init_multi(n_devices=0, emulate=0):
    """rl_init_multi: one process drives n_devices GPUs (0 = all).  emulate=G (tests on a one-GPU box): G device contexts on the
    current GPU.  Scenes must be (re)created afterwards so that every context holds a replica."""
    global _inited
    L = render_lib()
    rc = L.rl_debug_init_multi_emulated(int(emulate)) if emulate else L.rl_init_multi(int(n_devices))
    if rc != RL_OK:
        raise RLError(rc, L.rl_last_error().decode())
    _inited = True
    return L.rl_device_count()


def _ensure_init():
    if not _inited:
        init()


def render_status(world, allow_degenerate=False):
    """rl_render_status: waits for the scene's last asynchronous render; {'rays', 'flagged', 'rc'}."""
    st = Stats()
    rc = _check(render_lib().rl_render_status(world.device(), C.byref(st)), allow_degenerate)
    return {"rays": st.rays, "flagged": st.flagged, "rc": rc, "slow_traces": render_lib().rl_debug_slow_traces()}


def render_progress(world):
    """rl_rtiow_render_progress: (pixel slots claimed so far in the running launch, slots of that launch, phase) — does not wait for the render."""
    a, b, ph = C.c_uint64(), C.c_uint64(), C.c_uint32()
    _check(render_lib().rl_rtiow_render_progress(world.device(), C.byref(a), C.byref(b), C.byref(ph)))
    return a.value, b.value, ph.value


def set_fast_traversal(on):
    """Tests / tools: counter-free renders of small sphere scenes use the fast (ordered, reject-only) traversal unless switched off."""
    render_lib().rl_debug_set_fast_traversal(int(bool(on)))


def set_coop(on):
    """Tests / tools: counter-free renders of SMALL frames of sphere scenes use the cooperative one-wave-per-pixel kernel unless switched off."""
    render_lib().rl_debug_set_coop(int(bool(on)))


def set_lpt(on):
    """rl_debug_set_lpt: the cost-sorted two-launch render of the wave kernels (samples [0, 8), sort, resume; 64 spp and more) on / off.
    Same bits either way; tests take both paths."""
    render_lib().rl_debug_set_lpt(int(bool(on)))


def set_coop_pixels_max(n):
    """Tests / tools: the longest pixel list (render_pixels) of a sphere scene the cooperative kernel takes; 0 = the default, 160 per CU."""
    render_lib().rl_debug_set_coop_pixels_max(int(n))


def set_steal(max_fill):
    """Tests / tools: work stealing on small shards (at most max_fill x as many pixels as the GPU has lanes; 0 switches it off)."""
    render_lib().rl_debug_set_steal(float(max_fill))


def set_indep_cap(nbytes):
    """Tests / tools: cap of the sample-parallel mode's pass buffer in bytes (0: the default 1 GiB); a small cap forces several passes."""
    render_lib().rl_debug_set_indep_cap(int(nbytes))


def set_indep_k(k):
    """Tests / tools: samples of one pixel per claim in the sample-parallel mode (default 1)."""
    render_lib().rl_debug_set_indep_k(int(k))


def set_fastg_one_wave(mode):
    """Tests / tools: the fast general kernel's one-wave-per-SIMD form: -1 by frame size (default), 0 never, 1 always (where it applies)."""
    render_lib().rl_debug_set_fastg_one_wave(int(mode))


def set_pixel_entry(max_entries):
    """Tests / tools: the fast sphere kernel's camera rays start at their pixel's entry cut of up to max_entries (1 .. 3) entries of the
    fast tree; 0: at the root, as scattered rays do (csrc/rl_pixel_entry.h; the same switch as RL_PIXEL_ENTRY)."""
    render_lib().rl_debug_set_pixel_entry(int(max_entries))


def set_pixel_entry_sphere(on):
    """Tests / tools: the entry cut keeps only the leaves whose SPHERE the pixel's beam may touch (default); off: every leaf whose padded box
    it touches, the box-only cut (csrc/rl_pixel_entry.h; the same switch as RL_PIXEL_ENTRY_SPHERE)."""
    render_lib().rl_debug_set_pixel_entry_sphere(int(bool(on)))


def pixel_entry_table(world, n_pixels):
    """Tests: the entry words of the scene's most recent fast-traversal render (finished), one uint32 per pixel of the rows it rendered."""
    out = np.zeros(int(n_pixels), dtype=np.uint32)
    _check(render_lib().rl_debug_pixel_entry_read(world.device(), out.ctypes.data_as(C.c_void_p), int(n_pixels)))
    return out


def fast_tree(world):
    """Tests: the fast traversal tree of a sphere scene as (children [n_inner, 2] entry ids, root entry); entry e < n_inner is an inner
    node, e >= n_inner the sphere e - n_inner.  None when the scene has no fast structure."""
    L = render_lib()
    root = C.c_uint32()
    n = L.rl_debug_fast_tree(world.device(), None, 0, C.byref(root))
    if n < 0:
        return None
    ch = np.zeros((max(n, 1), 2), dtype=np.uint32)
    L.rl_debug_fast_tree(world.device(), ch.ctypes.data_as(C.c_void_p), n, C.byref(root))
    return ch[:n], int(root.value)


def set_status_gap(device_us, host_us=0):
    """Tests only: a wait of device_us on the render's stream before each asynchronous status copy, and a host sleep of host_us
    between a multi-GPU frame and its status post (each capped at 20 ms; 0, 0: off, the default)."""
    _ensure_init()
    _check(render_lib().rl_debug_set_status_gap(int(device_us), int(host_us)))


def live_buffers():
    """Tests: (count, bytes) of the device allocations the library owns right now (rl_debug_live_buffers): scenes' buffers and work
    buffers; the staging of a host-buffer call is gone again when the call returns."""
    out = (C.c_ulonglong * 2)()
    render_lib().rl_debug_live_buffers(out)
    return int(out[0]), int(out[1])


def _check(rc, allow_degenerate=False):
    if rc == RL_OK or (allow_degenerate and rc == RL_E_DEGENERATE):
        return rc
    raise RLError(rc, render_lib().rl_last_error().decode())


def _call(fn, *args, stats=None, counting=False, allow_degenerate=False):
    """The one tail of every wrapper over an entry point whose last parameter is `rl_stats *opt_stats`: fn(*args, opt_stats), checked,
    the counters and "rc" put into `stats` where the caller gave a dict.  opt_stats is what routes the call inside the library: NULL
    takes the counter-free kernels (and, in the device forms, returns without waiting); non-NULL the counting, reference-order ones.
    It is NULL unless the caller gave a dict — or the wrapper is `counting`: one that has always counted, dict or not."""
    st = Stats() if counting or stats is not None else None
    rc = _check(fn(*args, None if st is None else C.byref(st)), allow_degenerate)
    if stats is not None:
        stats.update(st.as_dict())
        stats["rc"] = rc
    return rc


# ---- the four entry forms of the pixel-render families (csrc/rl_pixel_render_api.h): features, ambient occlusion,
# direct lighting, NEE, NEE-MIS with and without sphere lights.  Every wrapper of a family is one of them, handed the C symbol's NAME
# (the library is looked up after every check in Python has passed), the family's particular arguments (the C arguments between the
# form's head and the outputs) and its outputs.  struct: the ctypes structure the outputs travel in (RtiowFeatures) where they are
# not one pointer argument each.  kw: stats, allow_degenerate.
def _subset_wanted(table, want):
    want = tuple(table) if want is None else tuple(want)
    if not want or any(k not in table for k in want):
        raise ValueError(f"want must be a non-empty subset of {tuple(table)}")
    return want


def host_outputs(table, want, shape, alloc=np.zeros, wanted=_subset_wanted):
    """The host arrays of a family's outputs at pixel shape `shape`: {name: array, None where `want` leaves it out}, in the C order.
    table: name -> (dtype, trailing shape)."""
    want = wanted(table, want)
    return {k: alloc(tuple(shape) + tail, dtype=dtype) if k in want else None for k, (dtype, tail) in table.items()}


def _pixel_form(symbol, camera, world, head, particular, outputs, struct, tail, **kw):
    outputs = [None if p is None else C.c_void_p(p) for p in outputs]
    return _call(getattr(render_lib(), symbol), world.device(), C.byref(camera.c), *head, *particular,
                 *([C.byref(struct(*outputs))] if struct else outputs), *tail, **kw)


def _host_pointers(arrays):
    return [None if a is None else a.ctypes.data for a in arrays.values()]


def rows_form(symbol, camera, world, first_sample, row_first, row_step, particular, outputs, want, struct=None, **kw):
    """The compact rows of a shard into host arrays, outputs(want, [nrows, W]) -> those arrays.  Always a counting call."""
    arrays = outputs(want, (rows_for(camera.c.image_height, row_first, row_step), camera.c.image_width))
    _pixel_form(symbol, camera, world, (first_sample, row_first, row_step), particular, _host_pointers(arrays), struct, (), counting=True, **kw)
    return arrays


def rows_device_form(symbol, camera, world, first_sample, row_first, row_step, particular, d_outputs, stream, struct=None, **kw):
    """The same rows into device buffers (d_outputs in the C order; 0 = not wanted), on `stream`."""
    _pixel_form(symbol, camera, world, (first_sample, row_first, row_step), particular, [d or None for d in d_outputs], struct, (C.c_void_p(stream),), **kw)


def list_form(symbol, camera, world, first_sample, xs, ys, particular, outputs, want, struct=None, **kw):
    """The pixels (xs[i], ys[i]) into host arrays, outputs(want, [n]) -> those arrays."""
    xs, ys = _pixel_list(xs, ys)
    arrays = outputs(want, (xs.size,))
    _pixel_form(symbol, camera, world, (first_sample, xs.ctypes.data, ys.ctypes.data, xs.size), particular, _host_pointers(arrays), struct, (), **kw)
    return arrays


def list_device_form(symbol, camera, world, first_sample, d_xs, d_ys, n, particular, d_outputs, stream, struct=None, **kw):
    """A device list of n pixels into device buffers, on `stream`."""
    _pixel_form(symbol, camera, world, (first_sample, C.c_void_p(d_xs), C.c_void_p(d_ys), int(n)), particular, [d or None for d in d_outputs], struct,
                (C.c_void_p(stream),), **kw)


def mirror_probe(scene, width, spp, symbol, args, outputs, result, *extra, max_depth=None):
    """A render of the C++ mirror through the host library's `symbol`(width, spp, *args, *outputs) on scene() at image_width = width
    (the height is the scene's aspect ratio's) -> result(*arrays, *extra).  For tests of the mirror; RLError carries rlh_last_error."""
    H = host_lib()
    world = scene()
    p = world.params
    p.image_width, p.samples_per_pixel = int(width), int(spp)
    if max_depth is not None:
        p.max_depth = max_depth
    cam = Camera(p)
    arrays = outputs(None, (cam.c.image_height, cam.c.image_width))
    if getattr(H, symbol)(int(width), int(spp), *args, *(C.c_void_p(a.ctypes.data) for a in arrays.values())) != 0:
        raise RLError(-1, H.rlh_last_error().decode(errors="replace"))
    return result(*arrays.values(), *extra)


def pack_rays(origins, dirs, times=None):
    """[n, 3] origins and directions (+ optional [n] times) -> the rl_ray records the queries take.  Shape errors are the caller's: ValueError."""
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError(f"origins and dirs must both be [n, 3] (got {o.shape} and {d.shape})")
    rays = np.zeros(o.shape[0], dtype=RAY)
    rays["origin"], rays["dir"] = o, d
    if times is not None:
        t = np.asarray(times, dtype=np.float64)
        if t.shape != (o.shape[0],):
            raise ValueError(f"times must be [n] (got {t.shape})")
        rays["time"] = t
    return rays


RNG_CURSOR = np.dtype([("stream", "<u8"), ("word_pos", "<u8")])  # rl_rng_cursor


def pack_cursors(streams, word_pos=0):
    """[n] ChaCha8 stream numbers (+ a word position, one for all or [n]) -> the rl_rng_cursor records the seeded path queries take.
    camera.rs:161-170 derives the stream of sample s at pixel (x, y) as s*W*H + x*W + y.  Shape errors are the caller's: ValueError."""
    st = np.asarray(streams)
    if st.ndim != 1 or st.dtype.kind not in "iu":
        raise ValueError(f"streams must be [n] integers (got shape {st.shape}, dtype {st.dtype})")
    wp = np.asarray(word_pos)
    if wp.dtype.kind not in "iu" or wp.shape not in ((), st.shape):
        raise ValueError(f"word_pos must be one integer or [n] integers (got shape {wp.shape}, dtype {wp.dtype})")
    if (st.dtype.kind == "i" and (st < 0).any()) or (wp.dtype.kind == "i" and (wp < 0).any()):
        raise ValueError("streams and word positions are unsigned")
    cur = np.zeros(st.shape[0], dtype=RNG_CURSOR)
    cur["stream"], cur["word_pos"] = st, wp
    return cur


def _cursors_arg(cursors, n):
    cur = np.ascontiguousarray(cursors)
    if cur.dtype != RNG_CURSOR or cur.shape != (n,):
        raise ValueError(f"cursors must be [{n}] RNG_CURSOR records (pack_cursors); got shape {cur.shape}, dtype {cur.dtype}")
    return cur


def set_query_pass_cap(rays):
    """rl_debug_set_query_pass_cap: rays per pass of ray_color_rays* (0: what the 32-bit work counter allows); tests force several passes."""
    render_lib().rl_debug_set_query_pass_cap(int(rays))


def last_query():
    """rl_debug_last_query: which kernel served the most recent hit_rays* / ray_color_rays* call ("fast" / "reference") or render_features* call
    ("features_fast" / "features_reference") and, for a synchronous call, how many of its rays the fast walk re-traced in the reference's order."""
    out = (C.c_uint64 * 2)()
    _check(render_lib().rl_debug_last_query(out))
    names = {1: "reference", 2: "fast", 3: "features_reference", 4: "features_fast", 5: "occlusion_reference", 6: "occlusion_fast",
             7: "ao_reference", 8: "ao_fast", 9: "direct_reference", 10: "direct_fast",
             11: "nee_reference", 12: "nee_fast", 13: "nee_mis_reference", 14: "nee_mis_fast", 15: "nee_spheres_reference", 16: "nee_spheres_fast"}
    return {"kernel": names.get(int(out[0]), "none"), "retraced": int(out[1])}


def set_denoise_route(route):
    """rl_debug_set_denoise_route: which route serves a denoising pass.  -1: the default (LDS, the faster one at every step measured);
    0: every tap read from the images; 1: one lattice's tile and halo staged in LDS.  Same bytes either way; tests compare them, tools/denoise_ab.py times them."""
    render_lib().rl_debug_set_denoise_route(int(route))


def last_denoise_route():
    """rl_debug_last_denoise_route: "images" / "lds" for the most recent denoising pass, "none" before the first."""
    return {0: "images", 1: "lds"}.get(int(render_lib().rl_debug_last_denoise_route()), "none")


def set_denoise_blocks(max_blocks):
    """rl_debug_set_denoise_blocks: the most workgroups a denoising pass launches; 0: the default, the CU-derived cap of the route.  With
    fewer workgroups than tiles a workgroup takes several tiles in turn; tests force that on tiny images."""
    render_lib().rl_debug_set_denoise_blocks(int(max_blocks))


def last_denoise_launch():
    """rl_debug_last_denoise_launch: {"tiles", "blocks"} of the most recent denoising pass: its tiles and the workgroups that shared them."""
    out = (C.c_uint64 * 2)()
    render_lib().rl_debug_last_denoise_launch(out)
    return {"tiles": int(out[0]), "blocks": int(out[1])}


def last_rtc_launch():
    """rl_debug_last_rtc_launch: the most recent RTC render launch of this process: {"kernel": "none" / "rtc" (rtc_kernel, rtc_pixels_kernel) /
    "full", "list": the pixel-list flavour, "lds_bytes": its dynamic LDS (0: the scene is read from global memory), "blocks": its workgroups}."""
    out = (C.c_uint64 * 4)()
    render_lib().rl_debug_last_rtc_launch(out)
    return {"kernel": {1: "rtc", 2: "full"}.get(int(out[0]), "none"), "list": bool(out[1]), "lds_bytes": int(out[2]), "blocks": int(out[3])}


def rtiow_launch_total():
    """rl_debug_rtiow_launch_total: how many RTIOW render launches this process has made (frame / moments / adaptive, sample-parallel, pixel
    list and path query: the three launch funnels of csrc/rl_rtiow_launch.h).  Read it before a call, hand it to rtiow_launches() after."""
    return int(render_lib().rl_debug_rtiow_launch_total())


def rtiow_launches(since_total=0):
    """rl_debug_rtiow_launch_log: the launches made since rtiow_launch_total() returned since_total, oldest first, one dict each:
      "kernel"        the instantiation launched, as the runtime names the function pointer that was handed to the launch, without return
                      type, namespace and parameter list: "rtiow_wave_kernel<1024, 4, false, true>"; "name" holds the string as recorded
      "funnel"        "value" / "pointer" (how the persistent kernel takes its parameter block) / "coop"
      "wg_size", "blocks", "lds_bytes" (dynamic LDS), "work_items" (what the grid was sized for)
      "sample_begin", "sample_end", "resume", "tile_order", "steal_state" (the last two: whether the pointer was set), "fg_top", "tune"
      "n_pixels"      of a cooperative launch; 0 otherwise
    The library keeps the last RTIOW_LAUNCH_LOG launches: asking for more than that raises."""
    L = render_lib()
    want = int(L.rl_debug_rtiow_launch_total()) - int(since_total)
    if want < 0 or want > RTIOW_LAUNCH_LOG:
        raise ValueError(f"{want} launches since total {since_total}: the log holds the last {RTIOW_LAUNCH_LOG}")
    buf = np.zeros(max(want, 1), dtype=RTIOW_LAUNCH)
    got = int(L.rl_debug_rtiow_launch_log(buf.ctypes.data_as(C.c_void_p), want)) if want else 0
    out = []
    for r in buf[:got]:
        if int(r["seq"]) <= int(since_total):  # (a launch of another thread moved the ring between the two calls)
            continue
        name = bytes(r["kernel"]).decode()
        short = name[5:] if name.startswith("void ") else name
        depth = 0
        for i, ch in enumerate(short):  # cut the parameter list: the first "(" outside the template arguments
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0 and i > 0:
                short = short[:i]
                break
        short = short.replace("rl::", "")
        out.append({"kernel": short, "name": name, "seq": int(r["seq"]), "funnel": ("value", "pointer", "coop")[int(r["funnel"])],
                    "wg_size": int(r["wg_size"]), "blocks": int(r["blocks"]), "lds_bytes": int(r["lds_bytes"]), "work_items": int(r["work_items"]),
                    "sample_begin": int(r["sample_begin"]), "sample_end": int(r["sample_end"]), "resume": int(r["resume"]),
                    "tile_order": bool(r["tile_order"]), "steal_state": bool(r["steal_state"]), "fg_top": int(r["fg_top"]),
                    "tune": tuple(int(t) for t in r["tune"]), "n_pixels": int(r["n_pixels"])})
    return out


def steal_record(world, n_pixels):
    """rl_debug_steal_read: waits for the device, then (state, n) of the first n_pixels pixels (rows x W of the shard) of the scene's most
    recent stealing launch, two uint32 arrays.  state 3: the pixel finished.  n: the sample at which the lane that rendered the pixel last
    released it to a wave that had asked for it (csrc/rl_rtiow_wave_body.inc, the sample boundary in GEN); NEVER_OFFERED where none did.
    A pixel is offered to one wave at most, so n counts hand-overs: one per pixel whose n is set — but for a request withdrawn in the
    instant of its release, whose pixel stays with its lane.  A render that does not steal leaves the record as it was."""
    state, n = np.zeros(int(n_pixels), dtype=np.uint32), np.zeros(int(n_pixels), dtype=np.uint32)
    _check(render_lib().rl_debug_steal_read(world.device(), state.ctypes.data_as(_PU32), n.ctypes.data_as(_PU32), int(n_pixels)))
    return state, n


def rtc_program(world):
    """rl_debug_rtc_program (host only, no device): the program an RtcWorld compiles to, as the kernels read it ->
    {"ops": RTC_DEV_OP[n_ops], "tris": RTC_DEV_TRI[n_tris], "guards": RTC_GUARD[n_guards], "scene_bytes": what the launch compares with 64 KB}."""
    L = render_lib()
    counts = (C.c_uint64 * 4)()
    _check(L.rl_debug_rtc_program(world.desc, None, None, None, None, counts))
    ops, tris, guards = np.zeros(int(counts[0]), dtype=RTC_DEV_OP), np.zeros(int(counts[1]), dtype=RTC_DEV_TRI), np.zeros(int(counts[2]), dtype=RTC_GUARD)
    cap = (C.c_uint64 * 3)(ops.size, tris.size, guards.size)
    _check(L.rl_debug_rtc_program(world.desc, ops.ctypes.data, tris.ctypes.data, guards.ctypes.data, cap, counts))
    return {"ops": ops, "tris": tris, "guards": guards, "scene_bytes": int(counts[3])}


def material_query_max_lanes():
    """rl_debug_material_query_lanes: the most lanes one scatter_rays* / texture_values* launch has on the current device (the grid cap,
    csrc/rl_material_query.h MATERIAL_QUERY_MAX_BLOCKS_PER_CU workgroups per CU); a larger batch puts several elements through one lane."""
    return int(render_lib().rl_debug_material_query_lanes())


def features_max_lanes():
    """rl_debug_features_lanes: the most lanes one render_features* launch has on the current device; a frame or list with more pixels puts
    several pixels through one lane."""
    return int(render_lib().rl_debug_features_lanes())


def _records_arg(a, dtype, n, what):
    r = np.ascontiguousarray(a)
    if r.dtype != dtype or r.ndim != 1 or (n is not None and r.shape[0] != n):
        raise ValueError(f"{what} must be [{'n' if n is None else n}] {what.upper()} records; got shape {r.shape}, dtype {r.dtype}")
    return r


def rows_for(height, row_first, row_step):
    return 0 if row_first >= height else (height - row_first + row_step - 1) // row_step


# ----------------------------------------------------------------------------- RTIOW host mirror
@dataclass
class CameraParams:  # camera.rs:23-59, defaults as in the reference
    aspect_ratio: float = 1.0
    image_width: int = 100
    samples_per_pixel: int = 10
    max_depth: int = 10
    vfov: float = 90.0
    lookfrom: tuple = (0.0, 0.0, 0.0)
    lookat: tuple = (0.0, 0.0, -1.0)
    vup: tuple = (0.0, 1.0, 0.0)
    defocus_angle: float = 0.0
    focus_dist: float = 10.0
    background: tuple = (0.7, 0.8, 1.0)
    seed: int = 0

    def _c(self):
        p = _HCameraParams()
        p.aspect_ratio, p.image_width, p.samples_per_pixel, p.max_depth = self.aspect_ratio, self.image_width, self.samples_per_pixel, self.max_depth
        p.vfov, p.defocus_angle, p.focus_dist, p.seed = self.vfov, self.defocus_angle, self.focus_dist, self.seed
        p.lookfrom[:], p.lookat[:], p.vup[:], p.background[:] = self.lookfrom, self.lookat, self.vup, self.background
        return p

    @staticmethod
    def _from_c(p):
        return CameraParams(p.aspect_ratio, p.image_width, p.samples_per_pixel, p.max_depth, p.vfov, tuple(p.lookfrom),
                            tuple(p.lookat), tuple(p.vup), p.defocus_angle, p.focus_dist, tuple(p.background), p.seed)


class World:
    """A flattened RTIOW world (host arrays owned by librl_host) — what `world: H` is in camera.rs:122."""

    def __init__(self, handle):
        if not handle:
            raise RuntimeError("host scene build failed: " + host_lib().rlh_last_error().decode())
        self._h = handle
        self.desc = host_lib().rlh_rtiow_desc(handle)
        p = _HCameraParams()
        host_lib().rlh_rtiow_get_params(handle, C.byref(p))
        self.params = CameraParams._from_c(p)  # the example's / test's camera parameters
        self._device = None

    def counts(self):
        """Element counts of the flattened scene (rl_rtiow_scene_desc)."""
        out = (C.c_uint32 * 9)()
        host_lib().rlh_rtiow_counts(self._h, out)
        return dict(zip(("spheres", "planars", "media", "translates", "transforms", "lists", "bvh_nodes", "materials", "textures"), list(out)))

    def _table(self, field, dtype):
        d = RtiowSceneDesc.from_address(self.desc)
        n, ptr = getattr(d, "n_" + field), getattr(d, field)
        if not n:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(ptr), dtype=dtype).copy()

    def materials(self):
        """The flattened scene's material table (MATERIAL records): what RTIOW_HIT.material indexes."""
        return self._table("materials", MATERIAL)

    def textures(self):
        """The flattened scene's texture table (TEXTURE records): what MATERIAL.texture and texture_values index."""
        return self._table("textures", TEXTURE)

    def perlins(self):
        """The flattened scene's Perlin tables (PERLIN records): what a Noise texture's `image` field indexes."""
        return self._table("perlins", PERLIN)

    def __del__(self):
        try:
            if self._device is not None:
                render_lib().rl_scene_destroy(self._device)
            host_lib().rlh_rtiow_free(self._h)
        except Exception:
            pass

    @staticmethod
    def golden_test_scene():  # tests/ray_tracing_one_weekend.rs:14-75
        return World(host_lib().rlh_rtiow_golden_test_scene())

    @staticmethod
    def bouncing_spheres(master_seed=1):  # examples/bouncing_spheres.rs
        return World(host_lib().rlh_rtiow_bouncing_spheres(master_seed))

    @staticmethod
    def cow_scene(obj_text: bytes, rgb8: np.ndarray):  # examples/cow.rs
        rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
        h, w = rgb8.shape[:2]
        return World(host_lib().rlh_rtiow_cow_scene(obj_text, len(obj_text), rgb8.ctypes.data, w, h))

    @staticmethod
    def perlin_spheres():  # examples/perlin_spheres.rs
        return World(host_lib().rlh_rtiow_perlin_scene(0))

    @staticmethod
    def simple_light():  # examples/simple_light.rs
        return World(host_lib().rlh_rtiow_perlin_scene(1))

    @staticmethod
    def earth_scene(rgb8: np.ndarray):  # examples/earth.rs with the caller's image (sRGB8, [H, W, 3])
        rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
        h, w = rgb8.shape[:2]
        return World(host_lib().rlh_rtiow_earth_scene(rgb8.ctypes.data, w, h))

    @staticmethod
    def example_scene(name: str, obj_text: bytes = None, rgb8: np.ndarray = None):
        """The reference's other example scenes (host/scenes.hpp): "checkered_spheres", "quads", "flat_world", "cornell_box",
        "cornell_smoke", "teapot" (obj_text = teapot-low.obj), "final_scene" (rgb8 = the earth image, sRGB8 [H, W, 3])."""
        h = w = 0
        ptr = None
        if rgb8 is not None:
            rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
            h, w = rgb8.shape[:2]
            ptr = rgb8.ctypes.data
        return World(host_lib().rlh_rtiow_example_scene(name.encode(), obj_text, len(obj_text) if obj_text else 0, ptr, w, h))

    @staticmethod
    def stress_scene(n_side=1000, subdiv=2, obj_text: bytes = None, rgb8: np.ndarray = None, seed=5, device_bvh=False):
        """BASELINE configs[4]: n_side^2 small spheres + ground + subdivided spot mesh (see host/scenes.hpp).
        device_bvh: build both BVHs with rl_bvh_build on the GPU instead of the host recursion (same tree)."""
        L = host_lib()
        if device_bvh:
            _ensure_init()
        if obj_text is None:
            return World(L.rlh_rtiow_stress_scene(n_side, subdiv, None, 0, None, 0, 0, seed, int(device_bvh)))
        rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
        h, w = rgb8.shape[:2]
        return World(L.rlh_rtiow_stress_scene(n_side, subdiv, obj_text, len(obj_text), rgb8.ctypes.data, w, h, seed, int(device_bvh)))

    @staticmethod
    def from_spheres(spheres, materials, textures, use_bvh):
        spheres = np.ascontiguousarray(spheres, dtype=SPHERE)
        materials = np.ascontiguousarray(materials, dtype=MATERIAL)
        textures = np.ascontiguousarray(textures, dtype=TEXTURE)
        return World(host_lib().rlh_rtiow_from_spheres(spheres.ctypes.data, len(spheres), materials.ctypes.data, len(materials),
                                                       textures.ctypes.data, len(textures), 1 if use_bvh else 0))

    @staticmethod
    def build(fn):
        """Compose a world with the reference's scene-building vocabulary: fn(SceneBuilder) -> root object id."""
        b = SceneBuilder()
        try:
            root = fn(b)
            return World(host_lib().rlh_b_finish(b._b, root))
        finally:
            host_lib().rlh_builder_free(b._b)

    def device(self):
        """rl_rtiow_scene_create — uploads once, cached."""
        if self._device is None:
            with _create_mu:
                if self._device is None:
                    _ensure_init()
                    L = render_lib()
                    h = L.rl_rtiow_scene_create(self.desc)
                    if not h:
                        raise RLError(RL_E_INVALID, L.rl_last_error().decode())
                    self._device = h
        return self._device

    def hit_rays(self, origins, dirs, times=None, tmin=1e-10, tmax=float("inf"), stats=None, allow_degenerate=False):
        """Hittable::hit(&Ray, &Interval{tmin, tmax}) on the scene root for every ray (hittable/mod.rs:42), on the GPU -> RTIOW_HIT[n]."""
        rays = pack_rays(origins, dirs, times)
        out = np.zeros(rays.shape[0], dtype=RTIOW_HIT)
        # without `stats` the call is counter-free: the fast traversal serves it where it applies (same bits, see last_query())
        _call(render_lib().rl_rtiow_hit_rays, self.device(), rays.ctypes.data, rays.shape[0], tmin, tmax, out.ctypes.data, stats=stats,
              allow_degenerate=allow_degenerate)
        return out

    def hit_rays_device(self, d_rays, d_out, n, tmin=1e-10, tmax=float("inf"), stream=0, stats=None, allow_degenerate=False):
        """Device buffers (n rl_ray in, n rl_rtiow_hit out; e.g. torch tensors' data_ptr).  Asynchronous unless stats is a dict."""
        _call(render_lib().rl_rtiow_hit_rays_device, self.device(), C.c_void_p(d_rays), n, tmin, tmax, C.c_void_p(d_out), C.c_void_p(stream),
              stats=stats, allow_degenerate=allow_degenerate)

    def hit_rays_seeded(self, rays, cursors, seed, tmin=1e-10, tmax=float("inf"), stats=None, allow_degenerate=False):
        """Hittable::hit(&Ray, &Interval{tmin, tmax}) for every ray of RAY[n], ray i drawing from cursors[i] of `seed` where the reference's fold
        evaluates a ConstantMedium (constant_medium.rs:55) -> (RTIOW_HIT[n], cursors behind the draws [n]).  Serves every RTIOW scene: one
        without media gives hit_rays' records and the cursors back unchanged.  With scatter_rays a host writes its own ray_color loop
        through smoke and gets ray_color_rays' bits."""
        rays = _records_arg(rays, RAY, None, "rays")
        n = rays.shape[0]
        out_cur = _cursors_arg(cursors, n).copy()
        out = np.zeros(n, dtype=RTIOW_HIT)
        _call(render_lib().rl_rtiow_hit_rays_seeded, self.device(), rays.ctypes.data, out_cur.ctypes.data, n, int(seed), tmin, tmax, out.ctypes.data,
              out_cur.ctypes.data, stats=stats, allow_degenerate=allow_degenerate)
        return out, out_cur

    def hit_rays_seeded_device(self, d_rays, d_cursors, n, seed, d_out, d_out_cursors=0, tmin=1e-10, tmax=float("inf"), stream=0, stats=None,
                               allow_degenerate=False):
        """Device buffers (n rl_ray and n rl_rng_cursor in; n rl_rtiow_hit and optionally n rl_rng_cursor out, which may be d_cursors).
        Asynchronous unless stats is a dict."""
        _call(render_lib().rl_rtiow_hit_rays_seeded_device, self.device(), C.c_void_p(d_rays), C.c_void_p(d_cursors), n, int(seed), tmin, tmax,
              C.c_void_p(d_out), C.c_void_p(d_out_cursors or None), C.c_void_p(stream), stats=stats, allow_degenerate=allow_degenerate)

    def ray_color_rays(self, origins, dirs, times, cursors, seed, max_depth, background, stats=None, allow_degenerate=False, rays=None):
        """Camera::ray_color(&mut rng, &ray, world, max_depth) (camera.rs:232-260) for every ray, on the GPU, ray i drawing from
        cursors[i] of `seed` -> (rgb [n, 3], cursors behind the paths [n], rays traced per path [n]).  rays=: RAY records as get_rays returns
        them, instead of origins / dirs / times.  Media scenes are accepted.  Without `stats` the call is counter-free (last_query())."""
        rays = pack_rays(origins, dirs, times) if rays is None else np.ascontiguousarray(rays)
        if rays.dtype != RAY or rays.ndim != 1:
            raise ValueError("rays must be [n] RAY records")
        n = rays.shape[0]
        out_cur = _cursors_arg(cursors, n).copy()
        bg = (C.c_double * 3)(*[float(v) for v in background])
        rgb = np.zeros((n, 3), dtype=np.float64)
        counts = np.zeros(n, dtype=np.uint32)
        _call(render_lib().rl_rtiow_ray_color_rays, self.device(), rays.ctypes.data, out_cur.ctypes.data, n, int(seed), int(max_depth), bg,
              rgb.ctypes.data, out_cur.ctypes.data, counts.ctypes.data, stats=stats, allow_degenerate=allow_degenerate)
        return rgb, out_cur, counts

    def ray_color_rays_device(self, d_rays, d_cursors, n, seed, max_depth, background, d_rgb, d_out_cursors=0, d_ray_counts=0, stream=0, stats=None,
                              allow_degenerate=False):
        """Device buffers (n rl_ray and n rl_rng_cursor in; n*3 f64, optionally n rl_rng_cursor and n u32 out).  Asynchronous unless stats is a dict."""
        bg = (C.c_double * 3)(*[float(v) for v in background])
        _call(render_lib().rl_rtiow_ray_color_rays_device, self.device(), C.c_void_p(d_rays), C.c_void_p(d_cursors), n, int(seed), int(max_depth), bg,
              C.c_void_p(d_rgb), C.c_void_p(d_out_cursors or None), C.c_void_p(d_ray_counts or None), C.c_void_p(stream), stats=stats,
              allow_degenerate=allow_degenerate)

    def scatter_rays(self, rays, hits, cursors, seed, stats=None, allow_degenerate=False):
        """Material::scatter(&mut rng, &ray, &hit_record) + Material::emitted(u, v, &p) (material.rs:11-20) for every element, on the GPU,
        element i drawing from cursors[i] of `seed`: RAY[n] (only dir and time are read), RTIOW_HIT[n] as hit_rays returns them (or
        hand-made) -> (SCATTER[n], cursors behind the draws [n]).  With hit_rays a host writes its own ray_color loop and gets
        ray_color_rays' bits."""
        rays = _records_arg(rays, RAY, None, "rays")
        n = rays.shape[0]
        hits = _records_arg(hits, RTIOW_HIT, n, "hits")
        out_cur = _cursors_arg(cursors, n).copy()
        out = np.zeros(n, dtype=SCATTER)
        _call(render_lib().rl_rtiow_scatter_rays, self.device(), rays.ctypes.data, hits.ctypes.data, out_cur.ctypes.data, n, int(seed),
              out.ctypes.data, out_cur.ctypes.data, stats=stats, allow_degenerate=allow_degenerate)
        return out, out_cur

    def scatter_rays_device(self, d_rays, d_hits, d_cursors, n, seed, d_out, d_out_cursors=0, stream=0, stats=None, allow_degenerate=False):
        """Device buffers (n rl_ray, n rl_rtiow_hit and n rl_rng_cursor in; n rl_rtiow_scatter and optionally n rl_rng_cursor out, which may be
        d_cursors).  Asynchronous unless stats is a dict.  A material index outside the scene's table gives a zero record."""
        _call(render_lib().rl_rtiow_scatter_rays_device, self.device(), C.c_void_p(d_rays), C.c_void_p(d_hits), C.c_void_p(d_cursors), n, int(seed),
              C.c_void_p(d_out), C.c_void_p(d_out_cursors or None), C.c_void_p(stream), stats=stats, allow_degenerate=allow_degenerate)

    def texture_values(self, textures, uv, p):
        """Texture::value(u, v, &p) (texture.rs) of the scene's textures[textures[i]] at (uv[i], p[i]), on the GPU -> rgb [n, 3]."""
        tex = np.asarray(textures)
        if tex.shape == (0,):
            tex = tex.astype(np.uint32)
        if tex.ndim != 1 or tex.dtype.kind not in "iu" or (tex.dtype.kind == "i" and (tex < 0).any()) or (tex.size and int(tex.max()) >= 2 ** 32):
            raise ValueError(f"textures must be [n] texture ids (got shape {tex.shape}, dtype {tex.dtype})")
        tex = np.ascontiguousarray(tex, dtype=np.uint32)
        n = tex.shape[0]
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        if uv.shape != (n, 2) or p.shape != (n, 3):
            raise ValueError(f"uv must be [{n}, 2] and p [{n}, 3] (got {uv.shape} and {p.shape})")
        rgb = np.zeros((n, 3), dtype=np.float64)
        _check(render_lib().rl_rtiow_texture_values(self.device(), tex.ctypes.data, uv.ctypes.data, p.ctypes.data, n, rgb.ctypes.data))
        return rgb

    def texture_values_device(self, d_textures, d_uv, d_p, n, d_rgb, stream=0):
        """Device buffers (n u32 texture ids, n*2 and n*3 f64 in; n*3 f64 out).  Asynchronous; an id outside the scene's table gives zeros."""
        _check(render_lib().rl_rtiow_texture_values_device(self.device(), C.c_void_p(d_textures), C.c_void_p(d_uv), C.c_void_p(d_p), n, C.c_void_p(d_rgb),
                                                           C.c_void_p(stream)))


class SceneBuilder:
    """Thin handle over librl_host's builder: textures, materials and hittables by id (names follow the reference)."""

    def __init__(self):
        self._L = host_lib()
        self._b = self._L.rlh_builder_new()

    @staticmethod
    def _v(x):
        return None if x is None else np.ascontiguousarray(x, dtype=np.float64)

    def _chk(self, r):
        if r < 0:
            raise RuntimeError("scene builder: " + self._L.rlh_last_error().decode())
        return r

    def solid(self, color):
        c = self._v(color)
        return self._chk(self._L.rlh_b_solid(self._b, c.ctypes.data))

    def checker(self, scale, even, odd):
        return self._chk(self._L.rlh_b_checker(self._b, scale, even, odd))

    def image(self, rgb_f32):
        a = np.ascontiguousarray(rgb_f32, dtype=np.float32)
        return self._chk(self._L.rlh_b_image(self._b, a.ctypes.data, a.shape[1], a.shape[0]))

    def noise(self, scale, seed):
        """Noise{Perlin::new(&mut Xoshiro256PlusPlus::seed_from_u64(seed)), scale} (texture.rs:84)."""
        return self._chk(self._L.rlh_b_noise(self._b, scale, seed))

    def lambertian(self, tex):
        return self._chk(self._L.rlh_b_material(self._b, MAT_LAMBERTIAN, tex, None, 0.0, 1.0))

    def metal(self, albedo, fuzz):
        a = self._v(albedo)
        return self._chk(self._L.rlh_b_material(self._b, MAT_METAL, -1, a.ctypes.data, fuzz, 1.0))

    def dielectric(self, ior):
        return self._chk(self._L.rlh_b_material(self._b, MAT_DIELECTRIC, -1, None, 0.0, ior))

    def diffuse_light(self, tex):
        return self._chk(self._L.rlh_b_material(self._b, MAT_DIFFUSE_LIGHT, tex, None, 0.0, 1.0))

    def flat(self):
        return self._chk(self._L.rlh_b_material(self._b, MAT_FLAT, -1, None, 0.0, 1.0))

    def isotropic(self, tex):
        return self._chk(self._L.rlh_b_material(self._b, MAT_ISOTROPIC, tex, None, 0.0, 1.0))

    def constant_medium(self, boundary, density, mat):
        """ConstantMedium::new(boundary, density, phase_function) — deterministic variant (rl_render.h rl_medium)."""
        return self._chk(self._L.rlh_b_medium(self._b, boundary, density, mat))

    def sphere(self, center, radius, mat, center2=None):
        c0, c1 = self._v(center), self._v(center2)
        return self._chk(self._L.rlh_b_sphere(self._b, c0.ctypes.data, None if c1 is None else c1.ctypes.data, radius, mat))

    def _planar(self, kind, q, u, v, mat):
        q, u, v = self._v(q), self._v(u), self._v(v)
        return self._chk(self._L.rlh_b_planar(self._b, kind, q.ctypes.data, u.ctypes.data, v.ctypes.data, mat))

    def plane(self, q, u, v, mat):
        return self._planar(0, q, u, v, mat)

    def quad(self, q, u, v, mat):
        return self._planar(1, q, u, v, mat)

    def triangle(self, q, u, v, mat):
        return self._planar(2, q, u, v, mat)

    def triangle_from_model(self, points, mat, uvs=None, normals=None):
        p, t, n = self._v(points), self._v(uvs), self._v(normals)
        return self._chk(self._L.rlh_b_triangle(self._b, p.ctypes.data, None if t is None else t.ctypes.data,
                                                None if n is None else n.ctypes.data, mat))

    def translate(self, obj, offset):
        o = self._v(offset)
        return self._chk(self._L.rlh_b_translate(self._b, obj, o.ctypes.data))

    def rotate_x(self, obj, deg):
        return self._chk(self._L.rlh_b_transform(self._b, obj, 0, deg))

    def rotate_y(self, obj, deg):
        return self._chk(self._L.rlh_b_transform(self._b, obj, 1, deg))

    def rotate_z(self, obj, deg):
        return self._chk(self._L.rlh_b_transform(self._b, obj, 2, deg))

    def scale(self, obj, s):
        return self._chk(self._L.rlh_b_transform(self._b, obj, 3, s))

    def bvh(self, objs):
        a = np.ascontiguousarray(objs, dtype=np.int32)
        return self._chk(self._L.rlh_b_group(self._b, a.ctypes.data, len(a), 1))

    def list(self, objs):
        a = np.ascontiguousarray(objs, dtype=np.int32)
        return self._chk(self._L.rlh_b_group(self._b, a.ctypes.data, len(a), 0))

    def obj_mesh(self, obj_text: bytes, mat):
        return self._chk(self._L.rlh_b_obj(self._b, obj_text, len(obj_text), mat))


def set_rtiow_variant(v):
    """Tests / tools: force a kernel variant (0 auto, 2 general, 4 wave-scheduled general, 1024 / 1025 / 1027 / 1029 wave layouts, 1031 fast general,
    1033 cooperative); a retired number makes the next render fail with RL_E_UNSUPPORTED."""
    render_lib().rl_debug_set_rtiow_variant(int(v))


@dataclass
class Canvas:  # camera.rs:263-296; data = SUMS over samples, [H, W, 3] f64
    samples: int
    width: int
    height: int
    data: np.ndarray = field(repr=False)

    def merge(self, other):  # camera.rs:273-291
        assert self.width == other.width and self.height == other.height and self.data.shape == other.data.shape
        return Canvas(self.samples + other.samples, self.width, self.height, self.data + other.data)

    def pixel_data(self):  # camera.rs:293: c / samples == c * (1/samples)
        return self.data * (1.0 / self.samples)

    def to_bincode(self) -> bytes:
        """The reference's checkpoint bytes: bincode::serialize(&canvas) (examples/common/mod.rs:32)."""
        L = host_lib()
        d = np.ascontiguousarray(self.data, dtype=np.float64)
        n = C.c_uint64()
        p = L.rlh_canvas_to_bincode(self.samples, self.width, self.height, d.ctypes.data, d.size // 3, C.byref(n))
        b = C.string_at(p, n.value)
        L.rlh_free(p)
        return b

    @staticmethod
    def from_bincode(b: bytes):
        """bincode::deserialize::<Canvas> (examples/common/mod.rs:45-46)."""
        L = host_lib()
        s, w, h, n = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        if L.rlh_canvas_from_bincode(b, len(b), C.byref(s), C.byref(w), C.byref(h), C.byref(n)) != 0:
            raise ValueError("malformed checkpoint: " + L.rlh_last_error().decode())
        data = np.frombuffer(b, dtype="<f8", offset=32, count=n.value * 3).copy()
        if n.value == w.value * h.value:
            data = data.reshape(h.value, w.value, 3)
        else:
            data = data.reshape(-1, 3)
        return Canvas(s.value, w.value, h.value, data)


@dataclass
class Moments:
    """First and second moments of a chained render (Camera.render_moments): per pixel and channel the sum of the sample colours (what
    Canvas.data holds) and the sum of their squares, sq = sq + c_n * c_n in sample order.  With a row shard both arrays hold the shard's rows."""
    samples: int
    sums: np.ndarray = field(repr=False)  # [H, W, 3] f64
    sq: np.ndarray = field(repr=False)    # [H, W, 3] f64

    def merge(self, other):  # as Canvas.merge: the moments of renders that continue each other (first_sample) add
        assert self.sums.shape == other.sums.shape and self.sq.shape == other.sq.shape
        return Moments(self.samples + other.samples, self.sums + other.sums, self.sq + other.sq)

    def canvas(self) -> Canvas:
        return Canvas(self.samples, self.sums.shape[1], self.sums.shape[0], self.sums)

    def variance_of_mean(self) -> np.ndarray:
        """An ESTIMATE of the variance of each pixel mean: the unbiased sample variance over n, (sq - sums^2 / n) / (n - 1) / n, clipped at 0
        (round-off can take the difference of the two large terms below it).  Plain numpy on the host; needs n >= 2."""
        n = self.samples
        if n < 2:
            raise ValueError(f"variance_of_mean needs at least 2 samples, got {n}")
        return np.maximum((self.sq - self.sums * self.sums / n) / (n - 1) / n, 0.0)


@dataclass
class Adaptive:
    """The outputs of an adaptive render (Camera.render_adaptive): per pixel the number of samples it took before the stopping rule
    (include/rl_render.h "Adaptive renders") let it stop, and the sums and second moments of exactly those samples — what Moments holds for a
    render of that many samples.  With a row shard the arrays hold the shard's rows."""
    sums: np.ndarray = field(repr=False)    # [H, W, 3] f64
    sq: np.ndarray = field(repr=False)      # [H, W, 3] f64
    counts: np.ndarray = field(repr=False)  # [H, W] uint32

    def mean(self) -> np.ndarray:
        return self.sums / self.counts[..., None]

    def variance_of_mean(self) -> np.ndarray:
        """Moments.variance_of_mean with every pixel's own n: (sq - sums^2 / n) / (n - 1) / n, clipped at 0.  Needs n >= 2 everywhere."""
        n = self.counts[..., None].astype(np.float64)
        if (self.counts < 2).any():
            raise ValueError("variance_of_mean needs at least 2 samples in every pixel")
        return np.maximum((self.sq - self.sums * self.sums / n) / (n - 1) / n, 0.0)


GUIDE_KINDS = ("albedo", "normal", "depth", "coverage")  # Features.guides: 3 + 3 + 1 + 1 channels


@dataclass
class Features:
    """The outputs of a feature render (Camera.render_features; include/rl_render.h "Feature renders"): per pixel, over the `samples` jittered
    camera rays, the sums of the first hit's colour factor (background where the ray misses), normal and ray parameter t, and the number of
    rays that hit.  An output that was not asked for (want=) is None.  With a row shard the arrays hold the shard's rows; a list render
    holds [n, ...] arrays."""
    samples: int
    albedo_sum: Optional[np.ndarray] = field(default=None, repr=False)  # [H, W, 3] f64
    normal_sum: Optional[np.ndarray] = field(default=None, repr=False)  # [H, W, 3] f64
    depth_sum: Optional[np.ndarray] = field(default=None, repr=False)   # [H, W] f64
    hit_count: Optional[np.ndarray] = field(default=None, repr=False)   # [H, W] uint32

    def albedo(self) -> np.ndarray:  # as Canvas.pixel_data: c * (1/samples)
        return self.albedo_sum * (1.0 / self.samples)

    def normal(self) -> np.ndarray:
        """normal_sum normalised; zeros where it is zero (no ray hit, or the normals cancelled)."""
        n = np.sqrt((self.normal_sum * self.normal_sum).sum(axis=-1, keepdims=True))
        return np.divide(self.normal_sum, n, out=np.zeros_like(self.normal_sum), where=n != 0.0)

    def depth(self) -> np.ndarray:
        """depth_sum / hit_count: the mean t of the rays that hit; inf where none did."""
        k = self.hit_count.astype(np.float64)
        return np.divide(self.depth_sum, k, out=np.full_like(self.depth_sum, np.inf), where=k != 0.0)

    def coverage(self) -> np.ndarray:
        return self.hit_count / self.samples

    def guides(self, want=GUIDE_KINDS) -> np.ndarray:
        """The guide image [H, W, G] denoise_atrous takes, channels in the order of `want`: albedo (3), normal (3), depth (1), coverage (1).
        Depth here is depth_sum / max(hit_count, 1): 0 where no ray hit, never inf (an inf guide would make the filter's output NaN);
        coverage tells those pixels apart."""
        make = {"albedo": self.albedo, "normal": self.normal, "depth": lambda: (self.depth_sum / np.maximum(self.hit_count, 1))[..., None],
                "coverage": lambda: self.coverage()[..., None]}
        for k in want:
            if k not in make:
                raise ValueError(f"want holds {k!r}; the guides are {GUIDE_KINDS}")
        if not want:
            raise ValueError("no guide asked for")
        return np.ascontiguousarray(np.concatenate([make[k]() for k in want], axis=-1), dtype=np.float64)

    def merge(self, other):  # as Moments.merge: the sums of renders that continue each other (first_sample) add
        def add(a, b):
            assert (a is None) == (b is None) and (a is None or a.shape == b.shape)
            return None if a is None else a + b
        return Features(self.samples + other.samples, *(add(getattr(self, k), getattr(other, k)) for k in FEATURE_OUTPUTS))


def _features_want(want):
    want = FEATURE_OUTPUTS if want is None else tuple(want)
    for k in want:
        if k not in FEATURE_OUTPUTS:
            raise ValueError(f"want holds {k!r}; the outputs are {FEATURE_OUTPUTS}")
    return want


def _features_outputs(want, shape):
    """The feature renders' host arrays: uninitialised, and an empty `want` goes through (the library refuses the all-NULL struct)."""
    return host_outputs(FEATURE_TABLE, want, shape, alloc=np.empty, wanted=lambda table, want: _features_want(want))


class Camera:
    def __init__(self, params: CameraParams):  # Camera::new camera.rs:72
        self.params = params
        self.c = RtiowCamera()
        pc = params._c()
        if host_lib().rlh_rtiow_camera_new(C.byref(pc), C.byref(self.c)) != 0:
            raise RuntimeError("Camera::new: " + host_lib().rlh_last_error().decode())
        self.image_height = self.c.image_height

    def _render(self, first_sample, world: World, row_first=0, row_step=1, stats=None, allow_degenerate=False):
        nrows = rows_for(self.c.image_height, row_first, row_step)
        out = np.empty((nrows, self.c.image_width, 3), dtype=np.float64)
        _call(render_lib().rl_rtiow_render_rows, world.device(), C.byref(self.c), first_sample, row_first, row_step, out.ctypes.data, stats=stats,
              counting=True, allow_degenerate=allow_degenerate)
        return out

    def render(self, world: World, stats=None, allow_degenerate=False) -> Canvas:  # camera.rs:122
        data = self._render(0, world, stats=stats, allow_degenerate=allow_degenerate)
        return Canvas(self.params.samples_per_pixel, self.c.image_width, self.c.image_height, data)

    def render_rgb8(self, world: World) -> np.ndarray:
        """render + the device output stage (sRGB, floor(v*255.999)): the [H, W, 3] bytes output_ppm prints."""
        out = np.empty((self.c.image_height, self.c.image_width, 3), dtype=np.uint8)
        _check(render_lib().rl_rtiow_render_rgb8(world.device(), C.byref(self.c), 0, out.ctypes.data, None), allow_degenerate=True)
        return out

    def render_denoised_rgb8(self, world: World, feature_samples, rule=None, iterations=5, color_sigma=None, guide_sigma=None, variance_floor=None,
                             want=GUIDE_KINDS, params: AtrousParams = None) -> np.ndarray:
        """rl_rtiow_render_denoised_rgb8, one call from scene to picture: render_moments (rule=None) or render_adaptive (rule = an
        RtiowAdaptive or its (min_samples, check_every, abs_variance, rel_variance)), render_features at `feature_samples` samples and
        denoise_render_device composed on the library's stream -> the [H, W, 3] bytes.  Sigmas and defaults are denoise_render's."""
        bits = guide_bits(want)
        if params is None:
            kinds = [k for k in GUIDE_KINDS if bits & GUIDE_BITS[k]]
            params = atrous_params(guide_channels(bits), DENOISE_COLOR_SIGMA if color_sigma is None else color_sigma, _guide_sigmas(guide_sigma, kinds),
                                   DENOISE_VARIANCE_FLOOR if variance_floor is None else variance_floor)
        if rule is not None and not isinstance(rule, RtiowAdaptive):
            rule = RtiowAdaptive(*rule)
        out = np.empty((self.c.image_height, self.c.image_width, 3), dtype=np.uint8)
        _check(render_lib().rl_rtiow_render_denoised_rgb8(world.device(), C.byref(self.c), None if rule is None else C.byref(rule), int(feature_samples), bits,
                                                          int(iterations), C.byref(params), out.ctypes.data), allow_degenerate=True)
        return out

    def render_from_checkpoint(self, world: World, checkpoint: Canvas) -> Canvas:  # camera.rs:136-143
        data = self._render(checkpoint.samples, world)
        return Canvas(self.params.samples_per_pixel, self.c.image_width, self.c.image_height, data).merge(checkpoint)

    def render_rows(self, world: World, row_first, row_step, first_sample=0, stats=None):
        return self._render(first_sample, world, row_first, row_step, stats)

    # ---- sample-parallel rendering with independent sample streams (include/rl_render.h rl_rtiow_render_independent*): every sample is
    # rendered as the first sample of a render is (fresh ChaCha8 stream at word 0), and the S colours are added to the sums left to right
    def render_independent(self, world: World, checkpoint: Canvas = None, stats=None, allow_degenerate=False) -> Canvas:
        """S = samples_per_pixel independent samples; with a checkpoint they continue its sums from sample checkpoint.samples on, and the
        canvas holds checkpoint.samples + S samples.  Bit for bit S repetitions of render_from_checkpoint with samples_per_pixel = 1."""
        if checkpoint is None:
            data = self.render_independent_rows(world, 0, 1, stats=stats, allow_degenerate=allow_degenerate)
            return Canvas(self.params.samples_per_pixel, self.c.image_width, self.c.image_height, data)
        assert checkpoint.width == self.c.image_width and checkpoint.height == self.c.image_height
        data = np.array(checkpoint.data, dtype=np.float64, order="C").reshape(self.c.image_height, self.c.image_width, 3)
        self.render_independent_rows(world, 0, 1, first_sample=checkpoint.samples, accumulate=True, out=data, stats=stats,
                                     allow_degenerate=allow_degenerate)
        return Canvas(checkpoint.samples + self.params.samples_per_pixel, self.c.image_width, self.c.image_height, data)

    def render_independent_rows(self, world: World, row_first, row_step, first_sample=0, accumulate=False, out=None, stats=None,
                                allow_degenerate=False):
        """Compact shard rows [nrows, W, 3] of samples first_sample .. first_sample + S - 1; accumulate=True adds them to `out`
        (a C-contiguous f64 array of that shape, updated in place)."""
        nrows = rows_for(self.c.image_height, row_first, row_step)
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs the sums to continue from (out=)")
            out = np.empty((nrows, self.c.image_width, 3), dtype=np.float64)
        if out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"] or out.size != nrows * self.c.image_width * 3:
            raise ValueError("out must be a C-contiguous float64 array of nrows * W * 3 values")
        _call(render_lib().rl_rtiow_render_independent_rows, world.device(), C.byref(self.c), first_sample, row_first, row_step,
              int(bool(accumulate)), out.ctypes.data, stats=stats, counting=True, allow_degenerate=allow_degenerate)
        return out

    def render_independent_device(self, world: World, d_ptr, stream=0, row_first=0, row_step=1, first_sample=0, accumulate=False, stats=None,
                                  allow_degenerate=False):
        """Output stays in HBM (d_ptr: nrows*W*3 f64, read first when accumulate).  Async unless stats is a dict."""
        _call(render_lib().rl_rtiow_render_independent_device, world.device(), C.byref(self.c), first_sample, row_first, row_step,
              int(bool(accumulate)), C.c_void_p(d_ptr), C.c_void_p(stream), stats=stats, allow_degenerate=allow_degenerate)

    # ---- seeded path queries (include/rl_render.h rl_rtiow_camera_rays*): Camera::get_ray for a batch of pixels, each with its own RNG cursor
    def get_rays(self, px, py, cursors):
        """cam.get_ray(&mut rng_i, px[i], py[i]) (camera.rs:203-216), rng_i = cursors[i] of the camera's seed -> (RAY[n], cursors behind the draws)."""
        x = np.ascontiguousarray(px, dtype=np.uint32)
        y = np.ascontiguousarray(py, dtype=np.uint32)
        if x.ndim != 1 or y.shape != x.shape:
            raise ValueError(f"px and py must both be [n] (got {x.shape} and {y.shape})")
        n = x.shape[0]
        out_cur = _cursors_arg(cursors, n).copy()
        _ensure_init()
        rays = np.zeros(n, dtype=RAY)
        _check(render_lib().rl_rtiow_camera_rays(C.byref(self.c), n, x.ctypes.data, y.ctypes.data, out_cur.ctypes.data, rays.ctypes.data, out_cur.ctypes.data))
        return rays, out_cur

    def get_rays_device(self, d_px, d_py, d_cursors, d_rays, d_out_cursors, n, stream=0):
        """Device buffers (n u32 px, n u32 py, n rl_rng_cursor in; n rl_ray and n rl_rng_cursor out, which may be d_cursors).  Asynchronous."""
        _ensure_init()
        _check(render_lib().rl_rtiow_camera_rays_device(C.byref(self.c), n, C.c_void_p(d_px), C.c_void_p(d_py), C.c_void_p(d_cursors), C.c_void_p(d_rays),
                                                        C.c_void_p(d_out_cursors), C.c_void_p(stream)))

    def render_multi(self, world: World, first_sample=0, stats=None, allow_degenerate=False) -> Canvas:
        """rl_rtiow_render_multi: the whole frame over every GPU of init_multi (rows interleaved, one RCCL exchange)."""
        out = np.empty((self.c.image_height, self.c.image_width, 3), dtype=np.float64)
        _call(render_lib().rl_rtiow_render_multi, world.device(), C.byref(self.c), first_sample, out.ctypes.data, stats=stats, counting=True,
              allow_degenerate=allow_degenerate)
        return Canvas(self.params.samples_per_pixel, self.c.image_width, self.c.image_height, out)

    def render_multi_device(self, world: World, d_ptr, first_sample=0, stats=None):
        """Frame left in GPU 0's HBM; asynchronous unless stats is a dict (api.render_status(world) waits)."""
        _call(render_lib().rl_rtiow_render_multi_device, world.device(), C.byref(self.c), first_sample, C.c_void_p(d_ptr), stats=stats)

    def render_device(self, world: World, d_ptr, stream=0, row_first=0, row_step=1, first_sample=0, stats=None):
        """Output stays in HBM: d_ptr = device pointer of nrows*W*3 f64. Async unless stats is a dict."""
        _call(render_lib().rl_rtiow_render_device, world.device(), C.byref(self.c), first_sample, row_first, row_step, C.c_void_p(d_ptr),
              C.c_void_p(stream), stats=stats)

    # ---- pixel-list renders (include/rl_render.h rl_rtiow_render_pixels*): the pixels of the caller's choosing, each bit for bit the
    # frame's pixel; compact output
    def render_pixels(self, world: World, xs, ys, first_sample=0, stats=None, allow_degenerate=False) -> np.ndarray:
        """[n, 3] sums of pixels (xs[i], ys[i]): what render_rows(world, 0, 1, first_sample) holds at [ys[i], xs[i]].  The list may be
        unsorted and hold duplicates.  stats (a dict): a counting call, the reference's counters for exactly the listed pixels; without
        it the call is counter-free.  A pixel outside the image: RLError(RL_E_INVALID)."""
        xs, ys = _pixel_list(xs, ys)
        out = np.empty((xs.size, 3), dtype=np.float64)
        _call(render_lib().rl_rtiow_render_pixels, world.device(), C.byref(self.c), first_sample, xs.ctypes.data, ys.ctypes.data, xs.size,
              out.ctypes.data, stats=stats, allow_degenerate=allow_degenerate)
        return out

    def render_pixels_device(self, world: World, d_xs, d_ys, n, d_out, stream=0, first_sample=0, stats=None):
        """d_xs / d_ys: device pointers of n uint32; d_out: of n*3 f64.  Async unless stats is a dict; an element outside the image is
        written as zeros."""
        _call(render_lib().rl_rtiow_render_pixels_device, world.device(), C.byref(self.c), first_sample, C.c_void_p(d_xs), C.c_void_p(d_ys), int(n),
              C.c_void_p(d_out), C.c_void_p(stream), stats=stats)

    # ---- renders with second moments (include/rl_render.h rl_rtiow_render_moments*, rl_rtiow_render_pixels_moments*): the sums of the plain
    # call, bit for bit, and beside them the sums of the squared sample colours — what an adaptive pass picks its pixels by
    def render_moments(self, world: World, first_sample=0, row_first=0, row_step=1, stats=None, allow_degenerate=False) -> Moments:
        """render_rows(world, row_first, row_step, first_sample) with the second moments: Moments.sums is that call's array."""
        nrows = rows_for(self.c.image_height, row_first, row_step)
        sums = np.empty((nrows, self.c.image_width, 3), dtype=np.float64)
        sq = np.empty((nrows, self.c.image_width, 3), dtype=np.float64)
        _call(render_lib().rl_rtiow_render_moments_rows, world.device(), C.byref(self.c), first_sample, row_first, row_step, sums.ctypes.data,
              sq.ctypes.data, stats=stats, counting=True, allow_degenerate=allow_degenerate)
        return Moments(self.params.samples_per_pixel, sums, sq)

    def render_moments_device(self, world: World, d_sums, d_sq, stream=0, row_first=0, row_step=1, first_sample=0, stats=None):
        """Both outputs stay in HBM: d_sums, d_sq = device pointers of nrows*W*3 f64 each.  Async unless stats is a dict."""
        _call(render_lib().rl_rtiow_render_moments_device, world.device(), C.byref(self.c), first_sample, row_first, row_step, C.c_void_p(d_sums),
              C.c_void_p(d_sq), C.c_void_p(stream), stats=stats)

    def render_pixels_moments(self, world: World, xs, ys, first_sample=0, stats=None, allow_degenerate=False):
        """(sums [n, 3], sq [n, 3]) of pixels (xs[i], ys[i]): render_pixels' sums and the second moments, each what render_moments holds at
        [ys[i], xs[i]].  The list rules are render_pixels'."""
        xs, ys = _pixel_list(xs, ys)
        sums = np.empty((xs.size, 3), dtype=np.float64)
        sq = np.empty((xs.size, 3), dtype=np.float64)
        _call(render_lib().rl_rtiow_render_pixels_moments, world.device(), C.byref(self.c), first_sample, xs.ctypes.data, ys.ctypes.data, xs.size,
              sums.ctypes.data, sq.ctypes.data, stats=stats, allow_degenerate=allow_degenerate)
        return sums, sq

    def render_pixels_moments_device(self, world: World, d_xs, d_ys, n, d_sums, d_sq, stream=0, first_sample=0, stats=None):
        """d_xs / d_ys: device pointers of n uint32; d_sums, d_sq: of n*3 f64 each.  Async unless stats is a dict; an element outside the image
        is written as zeros in both."""
        _call(render_lib().rl_rtiow_render_pixels_moments_device, world.device(), C.byref(self.c), first_sample, C.c_void_p(d_xs), C.c_void_p(d_ys),
              int(n), C.c_void_p(d_sums), C.c_void_p(d_sq), C.c_void_p(stream), stats=stats)

    # ---- adaptive renders (include/rl_render.h rl_rtiow_render_adaptive*): render_moments with a stopping rule evaluated inside the launch.
    # A pixel stops at the first checkpoint n = min_samples + k * check_every (n < samples_per_pixel) at which, in every channel,
    # n * sq - sum^2 <= (n - 1) * (abs_variance * n^2 + rel_variance * sum^2): variance of the mean <= abs_variance + rel_variance * mean^2
    def render_adaptive(self, world: World, min_samples, check_every, abs_variance=0.0, rel_variance=0.0, first_sample=0, row_first=0, row_step=1, stats=None,
                        allow_degenerate=False) -> Adaptive:
        """Every pixel's sums and sq are render_moments' for a camera of counts[pixel] samples, bit for bit."""
        nrows = rows_for(self.c.image_height, row_first, row_step)
        sums = np.empty((nrows, self.c.image_width, 3), dtype=np.float64)
        sq = np.empty((nrows, self.c.image_width, 3), dtype=np.float64)
        counts = np.empty((nrows, self.c.image_width), dtype=np.uint32)
        rule = RtiowAdaptive(min_samples, check_every, abs_variance, rel_variance)
        _call(render_lib().rl_rtiow_render_adaptive_rows, world.device(), C.byref(self.c), first_sample, row_first, row_step, C.byref(rule),
              sums.ctypes.data, sq.ctypes.data, counts.ctypes.data, stats=stats, counting=True, allow_degenerate=allow_degenerate)
        return Adaptive(sums, sq, counts)

    def render_adaptive_device(self, world: World, min_samples, check_every, d_sums, d_sq, d_counts, abs_variance=0.0, rel_variance=0.0, stream=0, row_first=0,
                               row_step=1, first_sample=0, stats=None):
        """All three outputs stay in HBM: d_sums, d_sq = device pointers of nrows*W*3 f64 each, d_counts of nrows*W uint32.  Async unless stats is a dict."""
        rule = RtiowAdaptive(min_samples, check_every, abs_variance, rel_variance)
        _call(render_lib().rl_rtiow_render_adaptive_device, world.device(), C.byref(self.c), first_sample, row_first, row_step, C.byref(rule),
              C.c_void_p(d_sums), C.c_void_p(d_sq), C.c_void_p(d_counts), C.c_void_p(stream), stats=stats)


    # ---- feature renders (include/rl_render.h rl_rtiow_render_features*): per pixel the sums of the first hit's colour factor, normal and
    # depth over the S jittered camera rays of render_independent, and the number of rays that hit; want= a subset of FEATURE_OUTPUTS
    def render_features(self, world: World, first_sample=0, row_first=0, row_step=1, want=None, stats=None, allow_degenerate=False) -> Features:
        """Compact shard rows.  Always a counting call (reference-order trace), as render_rows."""
        arrays = rows_form("rl_rtiow_render_features_rows", self, world, first_sample, row_first, row_step, (), _features_outputs, want, RtiowFeatures,
                           stats=stats, allow_degenerate=allow_degenerate)
        return Features(self.params.samples_per_pixel, **arrays)

    def render_features_device(self, world: World, stream=0, row_first=0, row_step=1, first_sample=0, stats=None, allow_degenerate=False, *, d_albedo_sum=0,
                               d_normal_sum=0, d_depth_sum=0, d_hit_count=0):
        """Outputs stay in HBM: device pointers of nrows*W*3 f64 (albedo, normal), nrows*W f64 (depth), nrows*W uint32 (hit count); 0 = not
        wanted.  Async unless stats is a dict."""
        rows_device_form("rl_rtiow_render_features_device", self, world, first_sample, row_first, row_step, (),
                         (d_albedo_sum, d_normal_sum, d_depth_sum, d_hit_count), stream, RtiowFeatures, stats=stats, allow_degenerate=allow_degenerate)

    def render_pixels_features(self, world: World, xs, ys, first_sample=0, want=None, stats=None, allow_degenerate=False) -> Features:
        """Features of pixels (xs[i], ys[i]), [n, ...]: what render_features(world, first_sample) holds at [ys[i], xs[i]].  The list rules
        are render_pixels'.  stats (a dict): a counting call; without it the call is counter-free and may take the fast walk."""
        arrays = list_form("rl_rtiow_render_pixels_features", self, world, first_sample, xs, ys, (), _features_outputs, want, RtiowFeatures, stats=stats,
                           allow_degenerate=allow_degenerate)
        return Features(self.params.samples_per_pixel, **arrays)

    def render_pixels_features_device(self, world: World, d_xs, d_ys, n, stream=0, first_sample=0, stats=None, allow_degenerate=False, *, d_albedo_sum=0,
                                      d_normal_sum=0, d_depth_sum=0, d_hit_count=0):
        """d_xs / d_ys: device pointers of n uint32; outputs as render_features_device with n pixels.  Async unless stats is a dict; an element
        outside the image is written as zeros in every given output."""
        list_device_form("rl_rtiow_render_pixels_features_device", self, world, first_sample, d_xs, d_ys, n, (),
                         (d_albedo_sum, d_normal_sum, d_depth_sum, d_hit_count), stream, RtiowFeatures, stats=stats, allow_degenerate=allow_degenerate)


# ---- denoising (include/rl_render.h "Denoising", rl_denoise_atrous*).  The default sigmas below are UNMEASURED defaults:
# plausible for unit-scale colours and the guides of Features.guides(), tuned on nothing.
DENOISE_COLOR_SIGMA = 2.0        # color_sigma2 = 4: a tap whose squared colour difference is 4 (summed) variances has half weight
DENOISE_VARIANCE_FLOOR = 1e-8
DENOISE_GUIDE_SIGMA = {"albedo": 0.1, "normal": 0.25, "depth": 1.0, "coverage": 0.25}  # per channel of that kind; depth in scene units of t


def atrous_params(n_guides=0, color_sigma=DENOISE_COLOR_SIGMA, guide_sigma=None, variance_floor=DENOISE_VARIANCE_FLOOR, guide_inv_sigma=None) -> AtrousParams:
    """The rl_atrous_params of a call: color_sigma2 = color_sigma * color_sigma; guide_inv_sigma[k] = 1 / guide_sigma[k], guide_sigma one number
    for all or one per channel, None / inf switching the channel off (default: every guide at sigma 1); guide_inv_sigma= gives the
    reciprocals themselves (0 = off) and wins.  Range errors are the library's to refuse (RL_E_INVALID); a wrong length is a ValueError."""
    n_guides = int(n_guides)
    if guide_inv_sigma is None:
        gs = 1.0 if guide_sigma is None else guide_sigma
        gs = [gs] * n_guides if np.ndim(gs) == 0 else list(gs)
        guide_inv_sigma = [0.0 if g is None or g == float("inf") else 1.0 / float(g) for g in gs]
    inv = [float(guide_inv_sigma)] * n_guides if np.ndim(guide_inv_sigma) == 0 else [float(v) for v in guide_inv_sigma]
    if len(inv) != n_guides:
        raise ValueError(f"{len(inv)} guide sigmas for {n_guides} guide channels")
    return AtrousParams(float(color_sigma) * float(color_sigma), float(variance_floor), n_guides, 0, (C.c_double * 8)(*inv[:8]))  # n_guides > 8: the library refuses it


def _denoise_images(color, variance, guides):
    color, variance = np.ascontiguousarray(color, dtype=np.float64), np.ascontiguousarray(variance, dtype=np.float64)
    if color.ndim != 3 or color.shape[2] != 3 or variance.shape != color.shape:
        raise ValueError(f"color and variance must both be [H, W, 3] (got {color.shape} and {variance.shape})")
    if guides is not None:
        guides = np.ascontiguousarray(guides, dtype=np.float64)
        if guides.ndim != 3 or guides.shape[:2] != color.shape[:2]:
            raise ValueError(f"guides must be [H, W, G] beside a colour image of {color.shape} (got {guides.shape})")
        if guides.shape[2] == 0:
            guides = None
    return color, variance, guides


def denoise_atrous(color, variance, guides=None, iterations=5, color_sigma=DENOISE_COLOR_SIGMA, guide_sigma=None, variance_floor=DENOISE_VARIANCE_FLOOR,
                   guide_inv_sigma=None, out_variance=True, params: AtrousParams = None):
    """rl_denoise_atrous: `iterations` passes of the edge-avoiding a-trous filter (step 1, 2, 4, ..) over color [H, W, 3] with the variance
    of each pixel mean [H, W, 3] and optional guides [H, W, G <= 8] -> (color, variance), both [H, W, 3] f64; out_variance=False: (color,
    None).  The sigmas go through atrous_params (params= gives the struct itself)."""
    color, variance, guides = _denoise_images(color, variance, guides)
    H, W = color.shape[:2]
    G = 0 if guides is None else guides.shape[2]
    p = params if params is not None else atrous_params(G, color_sigma, guide_sigma, variance_floor, guide_inv_sigma)
    if p.n_guides != G:
        raise ValueError(f"params has n_guides = {p.n_guides}, the guide image {G} channels")
    out_c = np.empty_like(color)
    out_v = np.empty_like(color) if out_variance else None
    _check(render_lib().rl_denoise_atrous(W, H, int(iterations), C.byref(p), color.ctypes.data, variance.ctypes.data, None if guides is None else guides.ctypes.data,
                                          out_c.ctypes.data, None if out_v is None else out_v.ctypes.data))
    return out_c, out_v


def denoise_atrous_pass_device(width, height, step, params: AtrousParams, d_color, d_variance, d_guides, d_out_color, d_out_variance=0, stream=0):
    """rl_denoise_atrous_pass_device: one pass on `stream` over device images (pointers; d_guides 0 with no guides, d_out_variance 0 = not
    wanted).  Asynchronous; the outputs must not be the inputs."""
    _check(render_lib().rl_denoise_atrous_pass_device(int(width), int(height), int(step), C.byref(params), C.c_void_p(d_color or None), C.c_void_p(d_variance or None),
                                                      C.c_void_p(d_guides or None), C.c_void_p(d_out_color or None), C.c_void_p(d_out_variance or None),
                                                      C.c_void_p(stream)))


def _denoise_render_inputs(estimate, features, guide_sigma, want):
    """What denoise_render hands to denoise_atrous: (colour, variance, guides, per-channel guide sigmas, the albedo it divided by)."""
    mean = estimate.mean() if isinstance(estimate, Adaptive) else estimate.sums * (1.0 / estimate.samples)
    var = estimate.variance_of_mean()
    albedo = features.albedo()
    if albedo.shape != mean.shape:
        raise ValueError(f"the estimate is {mean.shape}, the features' albedo {albedo.shape}")
    a = np.where(albedo > 0.0, albedo, 1.0)
    sig = dict(DENOISE_GUIDE_SIGMA, **(guide_sigma or {}))
    per_channel = [s for k in want for s in [sig[k]] * (3 if k in ("albedo", "normal") else 1)]
    return mean / a, var / (a * a), features.guides(want), per_channel, a


def denoise_render(estimate, features: Features, iterations=5, color_sigma=DENOISE_COLOR_SIGMA, guide_sigma=None, variance_floor=DENOISE_VARIANCE_FLOOR,
                   want=GUIDE_KINDS):
    """A Moments or Adaptive render denoised with the guides of a Features render of the same camera -> (color, variance) of the pixel MEANS,
    [H, W, 3] f64.  Plain numpy around one denoise_atrous: mean and variance of the mean are divided by the albedo and its square where
    the albedo is > 0 (so that texture detail is not what the filter sees as noise), filtered with features.guides(want), and multiplied
    back.  guide_sigma: {kind: sigma} over DENOISE_GUIDE_SIGMA's unmeasured defaults."""
    color, variance, guides, per_channel, a = _denoise_render_inputs(estimate, features, guide_sigma, want)
    color, variance = denoise_atrous(color, variance, guides, iterations, color_sigma, per_channel, variance_floor)
    return color * a, variance * (a * a)


# ---- denoise_render on the device (include/rl_render.h rl_denoise_prepare_device .. rl_rtiow_render_denoised_rgb8): what
# _denoise_render_inputs and denoise_render's last line compute in numpy, as two kernels around the passes — the same bytes
def guide_bits(want) -> int:
    """The RL_GUIDE_* bits of `want`: the bits themselves, or kinds of GUIDE_KINDS, which must come in GUIDE_KINDS' order (the order of the
    guide image's channels is fixed on the device; Features.guides takes any)."""
    if isinstance(want, (int, np.integer)):
        return int(want)
    want = tuple(want)
    for k in want:
        if k not in GUIDE_BITS:
            raise ValueError(f"want holds {k!r}; the guides are {GUIDE_KINDS}")
    if want != tuple(k for k in GUIDE_KINDS if k in want):
        raise ValueError(f"want must hold each of {GUIDE_KINDS} at most once and in that order, got {want}")
    return sum(GUIDE_BITS[k] for k in want)


def guide_channels(want) -> int:
    bits = guide_bits(want)
    return 3 * bool(bits & 1) + 3 * bool(bits & 2) + bool(bits & 4) + bool(bits & 8)


def denoise_inputs(estimate, features: Features = None, want=GUIDE_KINDS, *, samples=0, feature_samples=0) -> DenoiseInputs:
    """The rl_denoise_inputs of a call.  estimate: a Moments or Adaptive beside a Features (host arrays, for rl_denoise_render; the struct
    keeps them alive), or a dict of pointers {"sums", "sq", "albedo_sum"[, "counts", "normal_sum", "depth_sum", "hit_count"]} (0 / absent =
    NULL) with samples= (read where there are no counts) and feature_samples=."""
    bits = guide_bits(want)
    if isinstance(estimate, dict):
        unknown = set(estimate) - {f[0] for f in DenoiseInputs._fields_[:7]}
        if unknown:
            raise ValueError(f"not a pointer of rl_denoise_inputs: {sorted(unknown)}")
        return DenoiseInputs(**{k: (int(v) or None) for k, v in estimate.items()}, samples=int(samples), feature_samples=int(feature_samples), want=bits)
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
    keep = {"sums": f64(estimate.sums), "sq": f64(estimate.sq), "counts": u32(estimate.counts) if isinstance(estimate, Adaptive) else None,
            "albedo_sum": f64(features.albedo_sum), "normal_sum": f64(features.normal_sum), "depth_sum": f64(features.depth_sum),
            "hit_count": u32(features.hit_count)}
    d = DenoiseInputs(**{k: (None if a is None else a.ctypes.data) for k, a in keep.items()}, samples=0 if isinstance(estimate, Adaptive) else int(estimate.samples),
                      feature_samples=int(features.samples), want=bits)
    d._keep = keep
    return d


def denoise_prepare_device(width, height, inputs: DenoiseInputs, d_color, d_variance, d_guides=0, stream=0):
    """rl_denoise_prepare_device: one kernel on `stream`, from the renders' device buffers to the colour, variance ([H, W, 3] f64 each) and
    guide image ([H, W, G] f64) a pass reads.  Asynchronous."""
    _check(render_lib().rl_denoise_prepare_device(int(width), int(height), C.byref(inputs), C.c_void_p(d_color or None), C.c_void_p(d_variance or None),
                                                  C.c_void_p(d_guides or None), C.c_void_p(stream)))


def denoise_finish_device(width, height, d_color, d_variance, d_albedo_sum, feature_samples, d_out_color=0, d_out_variance=0, d_out_rgb8=0, stream=0):
    """rl_denoise_finish_device: one kernel on `stream`: the filtered images times the albedo (and its square), and / or the picture's
    bytes; 0 = not wanted.  The outputs may be the inputs.  Asynchronous."""
    _check(render_lib().rl_denoise_finish_device(int(width), int(height), C.c_void_p(d_color or None), C.c_void_p(d_variance or None), C.c_void_p(d_albedo_sum or None),
                                                 int(feature_samples), C.c_void_p(d_out_color or None), C.c_void_p(d_out_variance or None),
                                                 C.c_void_p(d_out_rgb8 or None), C.c_void_p(stream)))


def denoise_render_work_bytes(width, height, n_guides) -> int:
    """rl_denoise_render_work_bytes: the size of denoise_render_device's work buffer, width * height * 8 * (12 + n_guides)."""
    return int(render_lib().rl_denoise_render_work_bytes(int(width), int(height), int(n_guides)))


def denoise_render_device(width, height, inputs: DenoiseInputs, iterations, params: AtrousParams, d_work, work_bytes, d_out_color=0, d_out_variance=0,
                          d_out_rgb8=0, stream=0):
    """rl_denoise_render_device: prepare, `iterations` passes (step 1, 2, 4, ..) and finish enqueued on `stream` over device buffers; the
    images in between live in d_work (denoise_render_work_bytes).  0 = output not wanted.  Asynchronous."""
    _check(render_lib().rl_denoise_render_device(int(width), int(height), C.byref(inputs), int(iterations), C.byref(params), C.c_void_p(d_work or None),
                                                 int(work_bytes), C.c_void_p(d_out_color or None), C.c_void_p(d_out_variance or None), C.c_void_p(d_out_rgb8 or None),
                                                 C.c_void_p(stream)))


def _guide_sigmas(guide_sigma, want):
    sig = dict(DENOISE_GUIDE_SIGMA, **(guide_sigma or {}))
    return [s for k in want for s in [sig[k]] * (3 if k in ("albedo", "normal") else 1)]


def denoise_render_gpu(estimate, features: Features, iterations=5, color_sigma=DENOISE_COLOR_SIGMA, guide_sigma=None, variance_floor=DENOISE_VARIANCE_FLOOR,
                       want=GUIDE_KINDS, rgb8=False):
    """denoise_render with what it does in numpy around the passes done on the device too (rl_denoise_render): the same arguments,
    defaults, ValueErrors and bytes -> (color, variance), and with rgb8=True (color, variance, [H, W, 3] uint8 picture).  `want` must be
    in GUIDE_KINDS' order."""
    want = tuple(want)
    if not want:
        raise ValueError("no guide asked for")
    bits = guide_bits(want)
    if isinstance(estimate, Adaptive):
        if (estimate.counts < 2).any():
            raise ValueError("variance_of_mean needs at least 2 samples in every pixel")
    elif estimate.samples < 2:
        raise ValueError(f"variance_of_mean needs at least 2 samples, got {estimate.samples}")
    shape = estimate.sums.shape
    needed = {"albedo_sum": shape, "normal_sum": shape if bits & 2 else None, "depth_sum": shape[:2] if bits & 4 else None,
              "hit_count": shape[:2] if bits & 12 else None}
    if len(shape) != 3 or shape[2] != 3 or estimate.sq.shape != shape or (isinstance(estimate, Adaptive) and estimate.counts.shape != shape[:2]):
        raise ValueError(f"the estimate's sums must be [H, W, 3] beside sq and counts of that frame (got {shape})")
    for k, s in needed.items():
        a = getattr(features, k)
        if s is not None and (a is None or a.shape != s):
            raise ValueError(f"the estimate is {shape}, the features' {k} {None if a is None else a.shape}")
    H, W = shape[:2]
    d = denoise_inputs(estimate, features, bits)
    p = atrous_params(guide_channels(bits), color_sigma, _guide_sigmas(guide_sigma, want), variance_floor)
    color, variance = np.empty(shape, dtype=np.float64), np.empty(shape, dtype=np.float64)
    picture = np.empty(shape, dtype=np.uint8) if rgb8 else None
    _check(render_lib().rl_denoise_render(W, H, C.byref(d), int(iterations), C.byref(p), color.ctypes.data, variance.ctypes.data,
                                          None if picture is None else picture.ctypes.data))
    return (color, variance, picture) if rgb8 else (color, variance)


def _take_string(ptr, n):
    s = C.string_at(ptr, n.value)
    host_lib().rlh_free(ptr)
    return s.decode("ascii")


def output_ppm(canvas_or_sums, samples=None) -> str:  # output.rs:5-14
    if isinstance(canvas_or_sums, Canvas):
        data, samples = canvas_or_sums.data, canvas_or_sums.samples
    else:
        data = canvas_or_sums
    data = np.ascontiguousarray(data, dtype=np.float64)
    h, w = data.shape[:2]
    n = C.c_uint64()
    return _take_string(host_lib().rlh_rtiow_output_ppm(data.ctypes.data, w, h, samples, C.byref(n)), n)


# ----------------------------------------------------------------------------- RTC host mirror
class RtcWorld:
    """A flattened ray-tracer-challenge World (scene/world.rs:26) + the scene's Camera."""

    def __init__(self, handle=None, desc_struct=None, keep=None, camera=None):
        self._h = handle
        self._keep = keep
        self._device = None
        if handle is not None:
            if not handle:
                raise RuntimeError("host scene build failed: " + host_lib().rlh_last_error().decode())
            self.desc = host_lib().rlh_rtc_desc(handle)
            self.camera = RtcCamera()
            host_lib().rlh_rtc_get_camera(handle, C.byref(self.camera))
        else:
            self._desc_struct = desc_struct
            self.desc = C.addressof(desc_struct)
            self.camera = camera

    def __del__(self):
        try:
            if self._device is not None:
                render_lib().rl_scene_destroy(self._device)
            if self._h:
                host_lib().rlh_rtc_free(self._h)
        except Exception:
            pass

    @staticmethod
    def test_obj_scene(obj_text: bytes, res_x=300, res_y=200):  # tests/ray_tracer.rs:242-275
        return RtcWorld(host_lib().rlh_rtc_test_obj_scene(obj_text, len(obj_text), res_x, res_y))

    @staticmethod
    def test_mirror_scene(res_x=300, res_y=200):  # tests/ray_tracer.rs:56-240
        return RtcWorld(host_lib().rlh_rtc_named_scene(0, res_x, res_y))

    @staticmethod
    def test_csg_scene(res_x=300, res_y=200):  # tests/ray_tracer.rs:277-368
        return RtcWorld(host_lib().rlh_rtc_named_scene(1, res_x, res_y))

    @staticmethod
    def from_arrays(triangles, materials, objects, lights, groups=(), group_items=(), boundeds=(), transformeds=(),
                    max_reflection_depth=5, void_color=(0.0, 0.0, 0.0), camera=None, shapes=(), csgs=(), patterns=()):
        def arr(x, dt):
            return np.zeros(0, dtype=dt) if len(x) == 0 else np.ascontiguousarray(x, dtype=dt)
        arrs = dict(triangles=arr(triangles, RTC_TRIANGLE), groups=arr(groups, RTC_GROUP), group_items=arr(group_items, HREF),
                    boundeds=arr(boundeds, RTC_BOUNDED), transformeds=arr(transformeds, RTC_TRANSFORMED),
                    materials=arr(materials, RTC_MATERIAL), objects=arr(objects, HREF), lights=arr(lights, RTC_LIGHT),
                    shapes=arr(shapes, RTC_SHAPE), csgs=arr(csgs, RTC_CSG), patterns=arr(patterns, RTC_PATTERN))
        d = RtcSceneDesc()
        for k, a in arrs.items():
            setattr(d, k, a.ctypes.data if len(a) else None)
            setattr(d, "n_" + k, len(a))
        d.max_reflection_depth = max_reflection_depth
        d.void_color[:] = void_color
        return RtcWorld(desc_struct=d, keep=arrs, camera=camera)

    def device(self):
        if self._device is None:
            with _create_mu:
                if self._device is None:
                    _ensure_init()
                    L = render_lib()
                    h = L.rl_rtc_scene_create(self.desc)
                    if not h:
                        raise RLError(RL_E_INVALID, L.rl_last_error().decode())
                    self._device = h
        return self._device

    def render(self, aa_samples=1, camera=None, row_first=0, row_step=1, stats=None, allow_degenerate=False):
        """Camera::render(&world, &RenderOpts{anti_aliasing_samples}) on the GPU -> [rows, W, 3] means."""
        cam = camera or self.camera
        nrows = rows_for(cam.vsize, row_first, row_step)
        out = np.empty((nrows, cam.hsize, 3), dtype=np.float64)
        _call(render_lib().rl_rtc_render_rows, self.device(), C.byref(cam), aa_samples, row_first, row_step, out.ctypes.data, stats=stats,
              counting=True, allow_degenerate=allow_degenerate)
        return out

    def render_rgb8(self, aa_samples=1, camera=None) -> np.ndarray:
        """render + the device output stage (round(c*255)): the [H, W, 3] bytes Canvas::ppm prints."""
        cam = camera or self.camera
        out = np.empty((cam.vsize, cam.hsize, 3), dtype=np.uint8)
        _check(render_lib().rl_rtc_render_rgb8(self.device(), C.byref(cam), aa_samples, out.ctypes.data, None), allow_degenerate=True)
        return out

    def render_multi(self, aa_samples=1, camera=None, stats=None, allow_degenerate=False):
        """rl_rtc_render_multi: the whole frame over every GPU of init_multi."""
        cam = camera or self.camera
        out = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        _call(render_lib().rl_rtc_render_multi, self.device(), C.byref(cam), aa_samples, out.ctypes.data, stats=stats, counting=True,
              allow_degenerate=allow_degenerate)
        return out

    def render_device(self, d_ptr, aa_samples=1, camera=None, stream=0, row_first=0, row_step=1, stats=None):
        cam = camera or self.camera
        _call(render_lib().rl_rtc_render_device, self.device(), C.byref(cam), aa_samples, row_first, row_step, C.c_void_p(d_ptr), C.c_void_p(stream),
              stats=stats)

    def render_pixels(self, xs, ys, aa_samples=1, camera=None, stats=None, allow_degenerate=False):
        """rl_rtc_render_pixels: [n, 3] means of pixels (xs[i], ys[i]), each bit for bit render(aa_samples)[ys[i], xs[i]]."""
        cam = camera or self.camera
        xs, ys = _pixel_list(xs, ys)
        out = np.empty((xs.size, 3), dtype=np.float64)
        _call(render_lib().rl_rtc_render_pixels, self.device(), C.byref(cam), aa_samples, xs.ctypes.data, ys.ctypes.data, xs.size, out.ctypes.data,
              stats=stats, counting=True, allow_degenerate=allow_degenerate)
        return out

    def render_pixels_device(self, d_xs, d_ys, n, d_out, aa_samples=1, camera=None, stream=0, stats=None):
        cam = camera or self.camera
        _call(render_lib().rl_rtc_render_pixels_device, self.device(), C.byref(cam), aa_samples, C.c_void_p(d_xs), C.c_void_p(d_ys), int(n),
              C.c_void_p(d_out), C.c_void_p(stream), stats=stats)

    def intersect_rays(self, origins, dirs, k=8, stats=None, allow_degenerate=False):
        """World::intersect (world.rs:46) + hit (intersect.rs:159-168) for every ray -> (counts[n], isects RTC_ISECT[n, k], hit_index[n]);
        isects[i, :min(counts[i], k)] are the first entries of the sorted list, hit_index[i] == NO_HIT when hit() returns None."""
        rays = pack_rays(origins, dirs)
        n = rays.shape[0]
        counts = np.zeros(n, dtype=np.uint32)
        isects = np.zeros((n, k), dtype=RTC_ISECT)
        hit_index = np.full(n, NO_HIT, dtype=np.uint32)
        _call(render_lib().rl_rtc_intersect_rays, self.device(), rays.ctypes.data, n, k, isects.ctypes.data if k else None, counts.ctypes.data,
              hit_index.ctypes.data, stats=stats, counting=True, allow_degenerate=allow_degenerate)
        return counts, isects, hit_index

    def intersect_rays_device(self, d_rays, n, k, d_isects, d_counts, d_hit_index=0, stream=0, stats=None, allow_degenerate=False):
        _call(render_lib().rl_rtc_intersect_rays_device, self.device(), C.c_void_p(d_rays), n, k, C.c_void_p(d_isects) if d_isects else None,
              C.c_void_p(d_counts), C.c_void_p(d_hit_index) if d_hit_index else None, C.c_void_p(stream), stats=stats,
              allow_degenerate=allow_degenerate)

    def color_at_rays(self, origins, dirs, stats=None, allow_degenerate=False):
        """World::color_at(&ray) (world.rs:100) for every ray, with the world's max_reflection_depth -> [n, 3]."""
        rays = pack_rays(origins, dirs)
        out = np.zeros((rays.shape[0], 3), dtype=np.float64)
        _call(render_lib().rl_rtc_color_at_rays, self.device(), rays.ctypes.data, rays.shape[0], out.ctypes.data, stats=stats, counting=True,
              allow_degenerate=allow_degenerate)
        return out

    def color_at_rays_device(self, d_rays, d_rgb, n, stream=0, stats=None, allow_degenerate=False):
        _call(render_lib().rl_rtc_color_at_rays_device, self.device(), C.c_void_p(d_rays), n, C.c_void_p(d_rgb), C.c_void_p(stream), stats=stats,
              allow_degenerate=allow_degenerate)

    # ---- shading queries (include/rl_render.h "RTC shading queries")
    def _table(self, field, dtype):
        d = RtcSceneDesc.from_address(self.desc)
        n, ptr = getattr(d, "n_" + field), getattr(d, field)
        if not n:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(ptr), dtype=dtype).copy()

    def materials(self):
        """The flattened world's material table (RTC_MATERIAL records): what RTC_COMPS.material indexes."""
        return self._table("materials", RTC_MATERIAL)

    def lights(self):
        """The world's lights in order (RTC_LIGHT records)."""
        return self._table("lights", RTC_LIGHT)

    def prepare_rays(self, origins, dirs, stats=None, allow_degenerate=False):
        """hit(&World::intersect(&ray)).map(|h| h.prepare_computations(&ray, &xs)) (intersect.rs:159-168, :48-115) for every ray, on the GPU
        -> RTC_COMPS[n]; hit == 0 (and zeros) where hit() returns None."""
        rays = pack_rays(origins, dirs)
        n = rays.shape[0]
        out = np.zeros(n, dtype=RTC_COMPS)
        _call(render_lib().rl_rtc_prepare_rays, self.device(), rays.ctypes.data, n, out.ctypes.data, stats=stats, allow_degenerate=allow_degenerate)
        return out

    def prepare_rays_device(self, d_rays, n, d_comps, stream=0, stats=None, allow_degenerate=False):
        """Device buffers (n rl_ray in, n rl_rtc_comps out).  Asynchronous unless stats is a dict."""
        _call(render_lib().rl_rtc_prepare_rays_device, self.device(), C.c_void_p(d_rays), n, C.c_void_p(d_comps), C.c_void_p(stream), stats=stats,
              allow_degenerate=allow_degenerate)

    def shade_hits(self, comps, stats=None, allow_degenerate=False):
        """What World::shade_hit (world.rs:57-87) computes before it recurses, for every RTC_COMPS record (from prepare_rays or hand-made)
        -> (RTC_SHADE[n], shadow attenuations [n, n_lights]).  With prepare_rays a host writes its own color_at loop and gets
        color_at_rays' bits."""
        comps = _records_arg(comps, RTC_COMPS, None, "comps")
        n = comps.shape[0]
        out = np.zeros(n, dtype=RTC_SHADE)
        shadow = np.zeros((n, RtcSceneDesc.from_address(self.desc).n_lights), dtype=np.float64)
        _call(render_lib().rl_rtc_shade_hits, self.device(), comps.ctypes.data, n, out.ctypes.data, shadow.ctypes.data if shadow.size else None,
              stats=stats, allow_degenerate=allow_degenerate)
        return out, shadow

    def shade_hits_device(self, d_comps, n, d_out, d_out_shadow=0, stream=0, stats=None, allow_degenerate=False):
        """Device buffers (n rl_rtc_comps in; n rl_rtc_shade and optionally n * n_lights f64 out).  Asynchronous unless stats is a dict.
        A material index outside the scene's table gives a zero record."""
        _call(render_lib().rl_rtc_shade_hits_device, self.device(), C.c_void_p(d_comps), n, C.c_void_p(d_out), C.c_void_p(d_out_shadow or None),
              C.c_void_p(stream), stats=stats, allow_degenerate=allow_degenerate)

    @staticmethod
    def _vec3_arg(a, n, what):
        v = np.asarray(a, dtype=np.float64)
        if n is not None and v.shape == (3,):
            v = np.broadcast_to(v, (n, 3))
        if v.ndim != 2 or v.shape[1] != 3 or (n is not None and v.shape[0] != n):
            raise ValueError(f"{what} must be [{'n' if n is None else n}, 3] (got {v.shape})")
        return np.ascontiguousarray(v)

    def shadow_attenuation(self, points, light_positions, stats=None, allow_degenerate=False):
        """World::shadow_attenuation(&point, light) (world.rs:104-126) for arbitrary points [n, 3] and light positions ([n, 3], or one [3]
        for all) -> [n]."""
        pts = self._vec3_arg(points, None, "points")
        n = pts.shape[0]
        lp = self._vec3_arg(light_positions, n, "light_positions")
        out = np.zeros(n, dtype=np.float64)
        _call(render_lib().rl_rtc_shadow_attenuation, self.device(), pts.ctypes.data, lp.ctypes.data, n, out.ctypes.data, stats=stats,
              allow_degenerate=allow_degenerate)
        return out

    def shadow_attenuation_device(self, d_points, d_light_positions, n, d_out, stream=0, stats=None, allow_degenerate=False):
        """Device buffers (n * 3 and n * 3 f64 in, n f64 out).  Asynchronous unless stats is a dict."""
        _call(render_lib().rl_rtc_shadow_attenuation_device, self.device(), C.c_void_p(d_points), C.c_void_p(d_light_positions), n, C.c_void_p(d_out),
              C.c_void_p(stream), stats=stats, allow_degenerate=allow_degenerate)

    def lighting(self, comps, light_positions, light_intensities, shadow_att):
        """material::lighting (material.rs:54-90) of every RTC_COMPS record under PointLight{light_positions[i], light_intensities[i]} ([n, 3],
        or one [3] for all) with shadow_att ([n], or one number) -> rgb [n, 3]."""
        comps = _records_arg(comps, RTC_COMPS, None, "comps")
        n = comps.shape[0]
        lp = self._vec3_arg(light_positions, n, "light_positions")
        li = self._vec3_arg(light_intensities, n, "light_intensities")
        att = np.asarray(shadow_att, dtype=np.float64)
        if att.shape == ():
            att = np.broadcast_to(att, (n,))
        if att.shape != (n,):
            raise ValueError(f"shadow_att must be [{n}] (got {att.shape})")
        att = np.ascontiguousarray(att)
        rgb = np.zeros((n, 3), dtype=np.float64)
        _check(render_lib().rl_rtc_lighting(self.device(), comps.ctypes.data, lp.ctypes.data, li.ctypes.data, att.ctypes.data, n, rgb.ctypes.data))
        return rgb

    def lighting_device(self, d_comps, d_light_positions, d_light_intensities, d_shadow_att, n, d_rgb, stream=0):
        """Device buffers (n rl_rtc_comps, n * 3, n * 3 and n f64 in; n * 3 f64 out).  Asynchronous; a material outside the table gives zeros."""
        _check(render_lib().rl_rtc_lighting_device(self.device(), C.c_void_p(d_comps), C.c_void_p(d_light_positions), C.c_void_p(d_light_intensities),
                                                   C.c_void_p(d_shadow_att), n, C.c_void_p(d_rgb), C.c_void_p(stream)))


def rtc_camera(hsize, vsize, fov, frm, to, up) -> RtcCamera:  # Camera::new + view_transform
    c = RtcCamera()
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (frm, to, up)]
    if host_lib().rlh_rtc_camera_new(hsize, vsize, fov, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, C.byref(c)) != 0:
        raise RuntimeError("rtc Camera::new: " + host_lib().rlh_last_error().decode())
    return c


def rtc_transformed(matrix4, child_kind, child_index):
    """Transformed::new(child, transform): one RTC_TRANSFORMED record (inverse + inverse-transpose by cofactors)."""
    rec = np.zeros(1, dtype=RTC_TRANSFORMED)
    m = np.ascontiguousarray(matrix4, dtype=np.float64).reshape(16)
    if host_lib().rlh_rtc_make_transformed(m.ctypes.data, rec.ctypes.data) != 0:
        raise RuntimeError("Matrix is not invertible.")
    rec["child"]["kind"], rec["child"]["index"] = child_kind, child_index
    return rec[0]


def canvas_ppm(rgb) -> str:  # draw/canvas.rs:50-97
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    h, w = rgb.shape[:2]
    n = C.c_uint64()
    return _take_string(host_lib().rlh_rtc_canvas_ppm(rgb.ctypes.data, w, h, C.byref(n)), n)
