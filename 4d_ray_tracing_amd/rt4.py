"""Python host mirror of the reference's host interface, over the C ABI of librt4.so (include/rt4.h).

The reference's host is C++ on SFML; this module gives the same operations to Python callers
(tests, bench.py) without re-implementing any of them: every call goes into librt4.so.

  Properties            <- Properties (inc/properties.h:8-18, src/properties.cpp:12-77)
  Orientation.update    <- Orientation::update (src/controls.cpp:72-86)
  uniforms_from_properties <- initShader/initControls/drawShaderImage uniform producers
                           (src/main.cpp:25-39,86-91, src/controls.cpp:140-159, src/windows/windows.cpp:41-44)
  Scene.load_frag/parse <- pasting scenes/<name>.frag into executable/shader.frag (executable/README.md:9-11)
  Tracer.render_*       <- CellsWindow::drawShaderImage -> texture.draw(sprite, &shader) (windows.cpp:40-47)

There is no fallback: if librt4.so is missing or fails to load, importing this module raises.
"""
from __future__ import annotations

import ctypes
import os
import sys
from ctypes import POINTER, Structure, byref, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT4_LIB", os.path.join(_HERE, "lib", "librt4.so"))

F4 = c_float * 4
F3 = c_float * 3
F2 = c_float * 2


class Material(Structure):  # shader.frag:163-167
    _fields_ = [("glow", c_float), ("refl_prob", c_float), ("color", F3)]


class Space(Structure):  # visible_space, shader.frag:225-228
    _fields_ = [("point", F4), ("norm", F4), ("material", Material)]


class Sphere(Structure):  # visible_sphere, shader.frag:189-192
    _fields_ = [("center", F4), ("r", c_float), ("material", Material)]


class Cylinder(Structure):  # visible_cylinder, shader.frag:243-247
    _fields_ = [("point", F4), ("axis1", F4), ("axis2", F4), ("r", c_float), ("material", Material)]


class CylindersUnion(Structure):  # shader.frag:279-281
    _fields_ = [("cylinder1", Cylinder), ("cylinder2", Cylinder)]


class Tiger(Structure):  # shader.frag:298-300
    _fields_ = [("inner_cyl1", Cylinder), ("outer_cyl1", Cylinder), ("inner_cyl2", Cylinder), ("outer_cyl2", Cylinder)]


class Cube(Structure):  # visible_cube, shader.frag:345-350
    _fields_ = [("point", F4), ("norm", F4), ("x", F4), ("y", F4), ("z", F4), ("r", c_float), ("material", Material)]


class Hypercube(Structure):  # shader.frag:370-372
    _fields_ = [("cubes", Cube * 8)]


class Sun(Structure):  # sun_properties, shader.frag:404-409
    _fields_ = [("drct", F4), ("angular_size", c_float), ("light", F3), ("sharpness", c_float)]


class Group(Structure):
    _fields_ = [("kind", c_int32), ("first", c_int32), ("count", c_int32), ("outer", c_int32), ("new_first", c_int32)]


MAX_GROUPS, MAX_SPACES, MAX_SPHERES, MAX_CYLINDERS = 16, 32, 32, 16
MAX_UNIONS, MAX_HYPERCUBES, MAX_TIGERS = 4, 4, 4

GROUP_SPACES, GROUP_SPHERES, GROUP_CYLINDERS, GROUP_CYLINDERS_UNION, GROUP_HYPERCUBE, GROUP_TIGER = 1, 2, 3, 4, 5, 6
FINAL_LIGHT_SUN_SKY, FINAL_LIGHT_CONSTANT = 0, 1
SECTION_YXZ, SECTION_YWZ, SECTION_YXW = 0, 1, 2
FLAG_SAMPLER_LUT = 0x1
FLAG_GENERIC_KERNEL = 0x2
FLAG_PRIMARY_REUSE = 0x4
FLAG_SERIAL_FRAMES = 0x8
FLAG_OVERLAP_SHALLOW = 0x10  # rt4.h RT4_FLAG_OVERLAP_SHALLOW: at most 3 overlapped launches in flight
FRAME_RGBA32F, FRAME_RGBA16F, FRAME_RGBA8 = 0, 1, 2
KEY_FORWARD, KEY_BACK, KEY_RIGHT, KEY_LEFT, KEY_UP, KEY_DOWN, KEY_W_POS, KEY_W_NEG = (1 << i for i in range(8))
MAX_SECTIONS = 3
EVAL_ACOS, EVAL_ASIN, EVAL_SIN, EVAL_COS, EVAL_VOLUME_BY_W, EVAL_W_BY_VOLUME, EVAL_HASH, EVAL_SQRT = range(8)


class SceneDesc(Structure):
    _fields_ = [
        ("sky_light", F3),
        ("sun", Sun),
        ("final_light_mode", c_int32),
        ("final_light_const", F3),
        ("n_groups", c_int32),
        ("groups", Group * MAX_GROUPS),
        ("n_spaces", c_int32),
        ("spaces", Space * MAX_SPACES),
        ("n_spheres", c_int32),
        ("spheres", Sphere * MAX_SPHERES),
        ("n_cylinders", c_int32),
        ("cylinders", Cylinder * MAX_CYLINDERS),
        ("n_unions", c_int32),
        ("unions", CylindersUnion * MAX_UNIONS),
        ("n_hypercubes", c_int32),
        ("hypercubes", Hypercube * MAX_HYPERCUBES),
        ("n_tigers", c_int32),
        ("tigers", Tiger * MAX_TIGERS),
    ]


class Uniforms(Structure):  # shader.frag:5-19
    _fields_ = [
        ("seed", c_int32),
        ("samples", c_int32),
        ("reflections_amount", c_int32),
        ("small_indent", c_float),
        ("resolution", F2),
        ("part", c_float),
        ("light_to_color_conversion_coefficient", c_float),
        ("mtr_sizes", F2),
        ("focus", F4),
        ("vec_to_mtr", F4),
        ("top_drct", F4),
        ("right_drct", F4),
    ]


class OrientationStruct(Structure):  # struct Orientation, inc/controls.h:9-14
    _fields_ = [(n, F4) for n in ("forward", "top", "right", "w_drct", "horizontal_forward", "horizontal_right", "vertical_top")]


class CameraStruct(Structure):  # rt4.h rt4_camera (SphOrientation + controls.cpp state)
    _fields_ = [("fi", c_float), ("te", c_float), ("psi", c_float), ("psi_range_center", c_float),
                ("psi_range_radius", c_float), ("constrain_psi_range", c_int32), ("mouse_sensitivity", c_float),
                ("wheel_sensitivity", c_float), ("movement_speed", c_float), ("focus_to_matrix_distance", c_float),
                ("focus", F4), ("frame_number", c_uint32), ("orientation", OrientationStruct)]


class Region(Structure):
    _fields_ = [("x0", c_int32), ("y0", c_int32), ("w", c_int32), ("h", c_int32), ("band_rows", c_int32), ("band_step", c_int32)]


class SectionJob(Structure):  # rt4.h rt4_section_job
    _fields_ = [("u", Uniforms), ("region", Region), ("d_frame", c_void_p), ("row_stride_px", c_int64)]


class GBufferPx(Structure):  # rt4.h rt4_gbuffer_px: the primary hit of one pixel
    _fields_ = [("normal", F4), ("depth", c_float), ("surface", c_int32), ("refl_prob", c_float), ("glow", c_float)]


class DenoiseParams(Structure):  # rt4.h rt4_denoise_params
    _fields_ = [("levels", c_int32), ("cos_min", c_float), ("depth_tol", c_float), ("max_refl_prob", c_float)]


DENOISE_MAX_LEVELS = 6


class ReprojectParams(Structure):  # rt4.h rt4_reproject_params
    _fields_ = [("cos_min", c_float), ("plane_tol", c_float), ("slice_tol", c_float), ("max_refl_prob", c_float),
                ("max_history", c_int32)]


class UpscaleParams(Structure):  # rt4.h rt4_upscale_params
    _fields_ = [("mode", c_int32), ("cos_min", c_float), ("plane_tol", c_float)]


UPSCALE_NEAREST, UPSCALE_GUIDED = 0, 1  # rt4.h rt4_upscale_mode
UPSCALE_MAX_SCALE = 64
MAX_FRAMES = 64  # rt4.h RT4_MAX_FRAMES


class LightPx(Structure):  # rt4.h rt4_light_px: one pixel of a light accumulator
    _fields_ = [("mean", F3), ("mean_y", c_float), ("m2", c_float), ("n", c_int32), ("reserved", F2)]


class NoiseStats(Structure):  # rt4.h rt4_noise_stats
    _fields_ = [("pixels", c_uint64), ("measured", c_uint64), ("above", c_uint64), ("max_q", c_float), ("max_se", c_float)]


class LightDenoiseParams(Structure):  # rt4.h rt4_light_denoise_params
    _fields_ = [("levels", c_int32), ("cos_min", c_float), ("depth_tol", c_float), ("max_refl_prob", c_float),
                ("sigma", c_float), ("eps", c_float)]


LIGHT_DENOISE_MAX_LEVELS = 6


class TileSelectParams(Structure):  # rt4.h rt4_tile_select_params
    _fields_ = [("threshold", c_float), ("min_above", c_int32), ("min_frames", c_int32), ("dilate", c_int32)]


SELECT_MAX_DILATE = 2  # rt4.h RT4_SELECT_MAX_DILATE
LIGHT_MERGE_MAX = 16  # rt4.h RT4_LIGHT_MERGE_MAX
SUPERSAMPLE_MAX = 8  # rt4.h RT4_SUPERSAMPLE_MAX
LIGHT_POOLED = 0x1  # rt4.h RT4_LIGHT_POOLED: a light checkpoint of several seeds, not resumable


class RetinaParams(Structure):  # rt4.h rt4_retina_params
    _fields_ = [("alpha_sky", c_float), ("alpha_fill", c_float), ("alpha_edge", c_float), ("t_min", c_float),
                ("background", c_float * 3)]


class RetinaView(Structure):  # rt4.h rt4_retina_view: the picture's rays in voxel coordinates
    _fields_ = [("origin", c_float * 3), ("du", c_float * 3), ("dv", c_float * 3), ("dt", c_float * 3), ("steps", c_int32)]


RETINA_MAX_DEPTH = 256  # rt4.h RT4_RETINA_MAX_DEPTH
RETINA_MAX_STEPS = 4096  # rt4.h RT4_RETINA_MAX_STEPS


def _gbuffer_dtype():
    import numpy as np

    return np.dtype([("normal", "<f4", (4,)), ("depth", "<f4"), ("surface", "<i4"), ("refl_prob", "<f4"), ("glow", "<f4")])


# numpy layout of rt4_gbuffer_px (32 B): arrays of shape (h, stride) for Tracer.render_gbuffer_host / denoise_host
GBUFFER_DTYPE = _gbuffer_dtype()


def _light_dtype():
    import numpy as np

    return np.dtype([("mean", "<f4", (3,)), ("mean_y", "<f4"), ("m2", "<f4"), ("n", "<i4"), ("reserved", "<f4", (2,))])


# numpy layout of rt4_light_px (32 B): arrays of shape (h, stride); np.zeros is the empty accumulator
LIGHT_DTYPE = _light_dtype()


def _load(path=None):
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(f"librt4.so not found at {path}: build it first (python -c 'import __graft_entry__ as g; g.build()')")
    lib = ctypes.CDLL(path)
    E = [c_char_p, c_size_t]  # err, errlen
    sig = {
        "rt4_abi_version": ([], c_int),
        "rt4_build_info": ([], c_char_p),
        "rt4_scene_desc_size": ([], c_size_t),
        "rt4_uniforms_size": ([], c_size_t),
        "rt4_properties_load": ([c_char_p, POINTER(c_void_p)] + E, c_int),
        "rt4_properties_parse": ([c_char_p, c_size_t, POINTER(c_void_p)] + E, c_int),
        "rt4_properties_free": ([c_void_p], None),
        "rt4_properties_has": ([c_void_p, c_char_p], c_int),
        "rt4_properties_get_string": ([c_void_p, c_char_p, c_char_p, c_size_t, POINTER(c_size_t)] + E, c_int),
        "rt4_properties_get_int": ([c_void_p, c_char_p, POINTER(c_int32)] + E, c_int),
        "rt4_properties_get_uint": ([c_void_p, c_char_p, POINTER(c_uint32)] + E, c_int),
        "rt4_properties_get_float": ([c_void_p, c_char_p, POINTER(c_float)] + E, c_int),
        "rt4_properties_get_bool": ([c_void_p, c_char_p, POINTER(c_int)] + E, c_int),
        "rt4_orientation_update": ([c_float, c_float, c_float, POINTER(OrientationStruct)], None),
        "rt4_section_basis": ([POINTER(OrientationStruct), c_int, POINTER(c_float), POINTER(c_float)], c_int),
        "rt4_uniforms_from_properties": ([c_void_p, c_int32, c_int32, c_int, POINTER(Uniforms), POINTER(OrientationStruct)] + E, c_int),
        "rt4_window_cells": ([c_void_p, c_char_p, POINTER(c_int32), POINTER(c_int32)] + E, c_int),
        "rt4_scene_load_frag": ([c_char_p, POINTER(SceneDesc)] + E, c_int),
        "rt4_scene_parse_frag": ([c_char_p, c_size_t, POINTER(SceneDesc)] + E, c_int),
        "rt4_scene_validate": ([POINTER(SceneDesc)] + E, c_int),
        "rt4_scene_builtin": ([c_char_p, POINTER(SceneDesc)] + E, c_int),
        "rt4_context_create": ([c_int, c_uint32, POINTER(c_void_p)] + E, c_int),
        "rt4_context_set_scene": ([c_void_p, POINTER(SceneDesc)] + E, c_int),
        "rt4_context_destroy": ([c_void_p], None),
        "rt4_render_device": ([c_void_p, POINTER(Uniforms), POINTER(Region), c_void_p, c_int64, c_void_p, c_void_p] + E, c_int),
        "rt4_render_host": ([c_void_p, POINTER(Uniforms), POINTER(Region), c_void_p, c_int64, POINTER(c_uint64)] + E, c_int),
        "rt4_debug_eval": ([c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64] + E, c_int),
        "rt4_debug_find_intersection": ([c_void_p, c_void_p, c_void_p, c_void_p, c_int64] + E, c_int),
        "rt4_debug_final_light": ([c_void_p, c_void_p, c_void_p, c_int64] + E, c_int),
        "rt4_debug_bound_skip": ([c_void_p, c_void_p, c_void_p, c_int64] + E, c_int),
        "rt4_debug_cull": ([c_void_p, c_void_p, c_void_p, c_int64] + E, c_int),
        "rt4_debug_sqrt_thresholds": ([c_float, POINTER(c_float), POINTER(c_float)], c_int),
        "rt4_context_kernel_shape": ([c_void_p], c_uint32),
        "rt4_debug_verify_sqrt": ([c_void_p, POINTER(c_uint64)] + E, c_int),
        "rt4_frame_format_bytes": ([c_int32], c_int32),
        "rt4_camera_init": ([c_void_p, POINTER(CameraStruct)] + E, c_int),
        "rt4_camera_rotate": ([POINTER(CameraStruct), c_float, c_float, c_float], None),
        "rt4_camera_mouse_move": ([POINTER(CameraStruct), c_int32, c_int32, c_uint32], c_int),
        "rt4_camera_wheel": ([POINTER(CameraStruct), c_float], None),
        "rt4_camera_move": ([POINTER(CameraStruct), c_uint32, c_float], None),
        "rt4_camera_frame_uniforms": ([POINTER(CameraStruct), POINTER(Uniforms), c_int, c_int32, POINTER(Uniforms)], c_int),
        "rt4_write_ppm": ([c_char_p, c_void_p, c_int32, c_int32, c_int32, c_int64] + E, c_int),
        "rt4_write_png": ([c_char_p, c_void_p, c_int32, c_int32, c_int32, c_int64] + E, c_int),
        "rt4_render_device_ex": ([c_void_p, POINTER(Uniforms), POINTER(Region), c_void_p, c_int32, c_int64, c_void_p,
                                  c_void_p] + E, c_int),
        "rt4_render_host_ex": ([c_void_p, POINTER(Uniforms), POINTER(Region), c_void_p, c_int32, c_int64,
                                POINTER(c_uint64)] + E, c_int),
        "rt4_progressive_uniforms": ([POINTER(Uniforms), c_uint32, POINTER(Uniforms)], c_int),
        "rt4_render_sections_device": ([c_void_p, POINTER(SectionJob), c_int32, c_int32, c_void_p, c_void_p] + E, c_int),
        "rt4_render_frames_device": ([c_void_p, POINTER(Uniforms), c_int32, POINTER(Region), c_void_p, c_int32, c_int64,
                                      c_void_p, c_void_p] + E, c_int),
        "rt4_context_reserve_frames": ([c_void_p, c_int32, c_int32] + E, c_int),
        "rt4_context_frames_per_launch": ([c_void_p, c_int32, c_int32], c_int32),
        "rt4_debug_verify_div": ([c_void_p, c_float, c_int32, POINTER(c_uint64)] + E, c_int),
        "rt4_context_evaluated": ([c_void_p, POINTER(c_uint64), c_int32] + E, c_int),
        "rt4_debug_sky_threshold": ([c_void_p, c_float, c_int32, POINTER(c_float)] + E, c_int),
        "rt4_band_plan": ([c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(Region), POINTER(c_int32)] + E, c_int),
        "rt4_bands_unpermute_device": ([c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                        c_void_p] + E, c_int),
        "rt4_context_frame_scratch_bytes": ([c_void_p], c_uint64),
        "rt4_context_overlap_bytes": ([c_void_p], c_uint64),
        "rt4_context_reserve_overlap": ([c_void_p, c_int32, c_int32] + E, c_int),
        "rt4_accum_save": ([c_char_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_uint32] + E, c_int),
        "rt4_accum_info": ([c_char_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int64),
                            POINTER(c_uint32)] + E, c_int),
        "rt4_accum_load": ([c_char_p, c_void_p, c_int32, c_int32, c_int32, c_int64, POINTER(c_int64), POINTER(c_uint32)]
                           + E, c_int),
        "rt4_accum_save_key": ([c_char_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_uint32, c_uint32] + E,
                               c_int),
        "rt4_accum_key": ([c_void_p, c_void_p], c_uint32),
        "rt4_accum_key_of": ([c_char_p, POINTER(c_uint32)] + E, c_int),
        "rt4_scene_surface_count": ([POINTER(SceneDesc)], c_int32),
        "rt4_scene_surface": ([POINTER(SceneDesc), c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                               POINTER(Material)] + E, c_int),
        "rt4_render_gbuffer_device": ([c_void_p, POINTER(Uniforms), POINTER(Region), c_void_p, c_int64, c_void_p] + E, c_int),
        "rt4_render_gbuffer_host": ([c_void_p, POINTER(Uniforms), POINTER(Region), c_void_p, c_int64] + E, c_int),
        "rt4_denoise_params_default": ([POINTER(DenoiseParams)], None),
        "rt4_denoise_device": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                POINTER(DenoiseParams), c_void_p] + E, c_int),
        "rt4_denoise_host": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int64,
                              POINTER(DenoiseParams)] + E, c_int),
        "rt4_context_denoise_bytes": ([c_void_p], c_uint64),
        "rt4_reproject_params_default": ([POINTER(ReprojectParams)], None),
        "rt4_reproject_device": ([c_void_p, POINTER(Uniforms), c_void_p, c_int64, POINTER(Uniforms), c_void_p, c_int64,
                                  c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32,
                                  c_int32, c_int32, POINTER(ReprojectParams), c_void_p] + E, c_int),
        "rt4_reproject_host": ([c_void_p, POINTER(Uniforms), c_void_p, c_int64, POINTER(Uniforms), c_void_p, c_int64,
                                c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32,
                                c_int32, c_int32, POINTER(ReprojectParams)] + E, c_int),
        "rt4_temporal_blend_device": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32,
                                       c_int32, c_void_p] + E, c_int),
        "rt4_temporal_create": ([c_void_p, c_int32, c_int32, c_int32, POINTER(c_void_p)] + E, c_int),
        "rt4_temporal_destroy": ([c_void_p], None),
        "rt4_temporal_reset": ([c_void_p], None),
        "rt4_temporal_frame_device": ([c_void_p, POINTER(Uniforms), POINTER(ReprojectParams), c_void_p, c_void_p] + E, c_int),
        "rt4_temporal_image": ([c_void_p], c_void_p),
        "rt4_temporal_history": ([c_void_p], c_void_p),
        "rt4_temporal_gbuffer": ([c_void_p], c_void_p),
        "rt4_temporal_read_host": ([c_void_p, c_void_p, c_void_p, c_void_p] + E, c_int),
        "rt4_temporal_bytes": ([c_void_p], c_uint64),
        "rt4_upscale_params_default": ([POINTER(UpscaleParams)], None),
        "rt4_upscale_uniforms": ([POINTER(Uniforms), c_int32, POINTER(Uniforms)], c_int),
        "rt4_upscale_device": ([c_void_p, POINTER(Uniforms), c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                c_void_p, c_int64, c_int32, c_int32, c_int32, POINTER(UpscaleParams), c_void_p] + E, c_int),
        "rt4_upscale_host": ([c_void_p, POINTER(Uniforms), c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                              c_void_p, c_int64, c_int32, c_int32, c_int32, POINTER(UpscaleParams)] + E, c_int),
        "rt4_window_create": ([c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_void_p)] + E, c_int),
        "rt4_window_destroy": ([c_void_p], None),
        "rt4_window_reset": ([c_void_p], None),
        "rt4_window_present_device": ([c_void_p, POINTER(Uniforms), c_void_p, c_int64, c_void_p, c_int64,
                                       POINTER(UpscaleParams), c_void_p] + E, c_int),
        "rt4_window_image": ([c_void_p], c_void_p),
        "rt4_window_gbuffer": ([c_void_p], c_void_p),
        "rt4_window_read_host": ([c_void_p, c_void_p, c_void_p] + E, c_int),
        "rt4_window_bytes": ([c_void_p], c_uint64),
        "rt4_render_light_device": ([c_void_p, POINTER(Uniforms), c_int32, POINTER(Region), c_void_p, c_int64, c_void_p,
                                     c_void_p] + E, c_int),
        "rt4_render_light_host": ([c_void_p, POINTER(Uniforms), c_int32, POINTER(Region), c_void_p, c_int64,
                                   POINTER(c_uint64)] + E, c_int),
        "rt4_light_resolve_device": ([c_void_p, c_void_p, c_int64, c_float, c_void_p, c_int32, c_int64, c_int32, c_int32,
                                      c_void_p] + E, c_int),
        "rt4_light_resolve_host": ([c_void_p, c_void_p, c_int64, c_float, c_void_p, c_int32, c_int64, c_int32, c_int32] + E,
                                   c_int),
        "rt4_light_noise_device": ([c_void_p, c_void_p, c_int64, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p,
                                    c_int64, c_void_p, c_void_p, c_void_p] + E, c_int),
        "rt4_light_noise_host": ([c_void_p, c_void_p, c_int64, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p,
                                  c_int64, c_void_p, POINTER(NoiseStats)] + E, c_int),
        "rt4_light_denoise_params_default": ([POINTER(LightDenoiseParams)], None),
        "rt4_light_denoise_device": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_float, POINTER(LightDenoiseParams),
                                      c_void_p, c_int32, c_int64, c_void_p, c_int64, c_int32, c_int32, c_void_p] + E, c_int),
        "rt4_light_denoise_host": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_float, POINTER(LightDenoiseParams),
                                    c_void_p, c_int32, c_int64, c_void_p, c_int64, c_int32, c_int32] + E, c_int),
        "rt4_context_light_denoise_bytes": ([c_void_p], c_uint64),
        "rt4_tile_select_params_default": ([POINTER(TileSelectParams)], None),
        "rt4_light_select_tiles_device": ([c_void_p, c_void_p, c_int64, c_int32, c_int32, c_float, POINTER(TileSelectParams),
                                           c_void_p, c_void_p, c_void_p, c_void_p] + E, c_int),
        "rt4_light_select_tiles_host": ([c_void_p, c_void_p, c_int64, c_int32, c_int32, c_float, POINTER(TileSelectParams),
                                         c_void_p, POINTER(c_uint32), c_void_p] + E, c_int),
        "rt4_render_light_tiles_device": ([c_void_p, POINTER(Uniforms), c_int32, POINTER(Region), c_void_p, c_int32, c_void_p,
                                           c_int64, c_void_p, c_void_p] + E, c_int),
        "rt4_render_light_tiles_host": ([c_void_p, POINTER(Uniforms), c_int32, POINTER(Region), c_void_p, c_int32, c_void_p,
                                         c_int64, POINTER(c_uint64)] + E, c_int),
        "rt4_context_select_bytes": ([c_void_p], c_uint64),
        "rt4_light_merge_device": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32,
                                    c_void_p] + E, c_int),
        "rt4_light_merge_host": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32] + E,
                                 c_int),
        "rt4_light_downsample_device": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                         c_void_p] + E, c_int),
        "rt4_light_downsample_host": ([c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32] + E, c_int),
        "rt4_light_bands_unpermute_device": ([c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p] + E,
                                             c_int),
        "rt4_frame_split": ([c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)] + E, c_int),
        "rt4_light_save": ([c_char_p, c_void_p, c_int32, c_int32, c_int64, c_int64, c_uint32, c_uint32, c_uint32] + E, c_int),
        "rt4_light_info": ([c_char_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int64), POINTER(c_uint32),
                            POINTER(c_uint32), POINTER(c_uint32)] + E, c_int),
        "rt4_light_load": ([c_char_p, c_void_p, c_int32, c_int32, c_int64, POINTER(c_int64), POINTER(c_uint32),
                            POINTER(c_uint32), POINTER(c_uint32)] + E, c_int),
        "rt4_retina_slice_uniforms": ([POINTER(Uniforms), POINTER(c_float), c_int32, c_float, c_int32, POINTER(Uniforms)], c_int),
        "rt4_retina_params_default": ([POINTER(RetinaParams)], None),
        "rt4_retina_view_make": ([c_int32, c_int32, c_int32, POINTER(c_float), c_float, c_float, c_float, c_int32, c_int32,
                                  c_float, POINTER(RetinaView)] + E, c_int),
        "rt4_retina_voxelize_device": ([c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_float,
                                        POINTER(RetinaParams), c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32,
                                        c_void_p] + E, c_int),
        "rt4_retina_voxelize_host": ([c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_float,
                                      POINTER(RetinaParams), c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32] + E, c_int),
        "rt4_retina_project_device": ([c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, POINTER(RetinaView),
                                       POINTER(RetinaParams), c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p] + E, c_int),
        "rt4_retina_project_host": ([c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, POINTER(RetinaView),
                                     POINTER(RetinaParams), c_void_p, c_int32, c_int64, c_int32, c_int32] + E, c_int),
        "rt4_retina_create": ([c_void_p, c_int32, c_int32, c_int32, POINTER(c_void_p)] + E, c_int),
        "rt4_retina_destroy": ([c_void_p], None),
        "rt4_retina_reset": ([c_void_p], None),
        "rt4_retina_accumulate_device": ([c_void_p, POINTER(Uniforms), POINTER(c_float), c_float, c_int32, c_void_p,
                                          c_void_p] + E, c_int),
        "rt4_retina_present_device": ([c_void_p, POINTER(RetinaView), POINTER(RetinaParams), c_float, c_void_p, c_int32,
                                       c_int64, c_int32, c_int32, c_void_p] + E, c_int),
        "rt4_retina_frames_done": ([c_void_p], c_int64),
        "rt4_retina_light": ([c_void_p], c_void_p),
        "rt4_retina_gbuffer": ([c_void_p], c_void_p),
        "rt4_retina_voxels": ([c_void_p], c_void_p),
        "rt4_retina_read_host": ([c_void_p, c_void_p, c_void_p, c_void_p] + E, c_int),
        "rt4_retina_bytes": ([c_void_p], c_uint64),
    }
    tolerant = os.environ.get("RT4_AB_TOLERANT") == "1"  # tools/abtest.sh: older builds lack newer exports
    for name, (argtypes, restype) in sig.items():
        if tolerant and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared export
        fn.argtypes = argtypes
        fn.restype = restype
    return lib


lib = _load()


def load_variant(path: str):
    """Another build of librt4.so (e.g. the native-math diagnostic build, lib_native/librt4.so) with the
    same C ABI, for Tracer(library=...): two builds side by side in one process."""
    return _load(path)
EXPORTED = (
    "rt4_abi_version rt4_build_info rt4_scene_desc_size rt4_uniforms_size rt4_properties_load rt4_properties_parse "
    "rt4_properties_free rt4_properties_has rt4_properties_get_string rt4_properties_get_int rt4_properties_get_uint "
    "rt4_properties_get_float rt4_properties_get_bool rt4_orientation_update rt4_section_basis "
    "rt4_uniforms_from_properties rt4_window_cells rt4_scene_load_frag rt4_scene_parse_frag rt4_scene_validate "
    "rt4_scene_builtin rt4_context_create rt4_context_set_scene rt4_context_destroy rt4_render_device rt4_render_host "
    "rt4_debug_eval rt4_debug_find_intersection rt4_context_kernel_shape rt4_debug_verify_sqrt "
    "rt4_camera_init rt4_camera_rotate rt4_camera_mouse_move rt4_camera_wheel rt4_camera_move "
    "rt4_camera_frame_uniforms rt4_write_ppm rt4_frame_format_bytes rt4_render_device_ex rt4_render_host_ex rt4_progressive_uniforms rt4_render_sections_device "
    "rt4_debug_verify_div rt4_debug_sky_threshold rt4_context_evaluated rt4_render_frames_device rt4_context_reserve_frames rt4_context_frames_per_launch "
    "rt4_band_plan rt4_bands_unpermute_device rt4_context_frame_scratch_bytes rt4_context_overlap_bytes rt4_context_reserve_overlap rt4_accum_save rt4_accum_info rt4_accum_load rt4_write_png "
    "rt4_accum_save_key rt4_accum_key rt4_accum_key_of "
    "rt4_scene_surface_count rt4_scene_surface rt4_render_gbuffer_device rt4_render_gbuffer_host "
    "rt4_denoise_params_default rt4_denoise_device rt4_denoise_host rt4_context_denoise_bytes "
    "rt4_debug_final_light rt4_debug_bound_skip rt4_debug_cull rt4_debug_sqrt_thresholds "
    "rt4_reproject_params_default rt4_reproject_device rt4_reproject_host rt4_temporal_blend_device rt4_temporal_create "
    "rt4_temporal_destroy rt4_temporal_reset rt4_temporal_frame_device rt4_temporal_image rt4_temporal_history "
    "rt4_temporal_gbuffer rt4_temporal_read_host rt4_temporal_bytes "
    "rt4_upscale_params_default rt4_upscale_uniforms rt4_upscale_device rt4_upscale_host rt4_window_create "
    "rt4_window_destroy rt4_window_reset rt4_window_present_device rt4_window_image rt4_window_gbuffer "
    "rt4_window_read_host rt4_window_bytes "
    "rt4_render_light_device rt4_render_light_host rt4_light_resolve_device rt4_light_resolve_host "
    "rt4_light_noise_device rt4_light_noise_host "
    "rt4_light_denoise_params_default rt4_light_denoise_device rt4_light_denoise_host rt4_context_light_denoise_bytes "
    "rt4_tile_select_params_default rt4_light_select_tiles_device rt4_light_select_tiles_host "
    "rt4_render_light_tiles_device rt4_render_light_tiles_host rt4_context_select_bytes "
    "rt4_light_merge_device rt4_light_merge_host rt4_light_bands_unpermute_device rt4_frame_split "
    "rt4_light_save rt4_light_info rt4_light_load rt4_light_downsample_device rt4_light_downsample_host "
    "rt4_retina_slice_uniforms rt4_retina_params_default rt4_retina_view_make rt4_retina_voxelize_device "
    "rt4_retina_voxelize_host rt4_retina_project_device rt4_retina_project_host rt4_retina_create rt4_retina_destroy "
    "rt4_retina_reset rt4_retina_accumulate_device rt4_retina_present_device rt4_retina_frames_done rt4_retina_light "
    "rt4_retina_gbuffer rt4_retina_voxels rt4_retina_read_host rt4_retina_bytes"
).split()

if ctypes.sizeof(SceneDesc) != lib.rt4_scene_desc_size() or ctypes.sizeof(Uniforms) != lib.rt4_uniforms_size():
    raise ImportError("rt4.py struct layout does not match librt4.so (rebuild the library)")


class RT4Error(RuntimeError):
    """A non-zero status from librt4.so (the reference aborts on these: src/util/util.cpp:9-12)."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"rt4 status {status}: {msg}")
        self.status = status


def _errbuf():
    return ctypes.create_string_buffer(1024)


def _check(status: int, err) -> None:
    if status != 0:
        raise RT4Error(status, err.value.decode("utf-8", "replace"))


class Properties:
    """properties.txt reader with the reference's getters (inc/properties.h:8-18)."""

    def __init__(self, path: str | None = None, text: str | None = None):
        h = c_void_p()
        err = _errbuf()
        if text is not None:
            raw = text.encode("utf-8")
            _check(lib.rt4_properties_parse(raw, len(raw), byref(h), err, len(err)), err)
        else:
            _check(lib.rt4_properties_load(os.fsencode(path), byref(h), err, len(err)), err)
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            lib.rt4_properties_free(self._h)
            self._h = None

    def has(self, key: str) -> bool:
        return bool(lib.rt4_properties_has(self._h, key.encode()))

    def getString(self, key: str) -> str:
        need = c_size_t()
        err = _errbuf()
        _check(lib.rt4_properties_get_string(self._h, key.encode(), None, 0, byref(need), err, len(err)), err)
        buf = ctypes.create_string_buffer(need.value + 1)
        _check(lib.rt4_properties_get_string(self._h, key.encode(), buf, len(buf), None, err, len(err)), err)
        return buf.value.decode("utf-8")

    def getStringOrNull(self, key: str) -> str:  # properties.cpp:31-33 (map[key] -> "" when absent)
        return self.getString(key) if self.has(key) else ""

    def _get(self, fn, ctype, key):
        v = ctype()
        err = _errbuf()
        _check(fn(self._h, key.encode(), byref(v), err, len(err)), err)
        return v.value

    def getInt(self, key: str) -> int:
        return self._get(lib.rt4_properties_get_int, c_int32, key)

    def getUnsignedInt(self, key: str) -> int:
        return self._get(lib.rt4_properties_get_uint, c_uint32, key)

    def getFloat(self, key: str) -> float:
        return self._get(lib.rt4_properties_get_float, c_float, key)

    def getBool(self, key: str) -> bool:
        return bool(self._get(lib.rt4_properties_get_bool, c_int, key))


class Orientation:
    """Camera basis from (fi, te, psi) in radians (src/controls.cpp:72-86)."""

    def __init__(self, fi: float = 0.0, te: float = 0.0, psi: float = 0.0):
        self.s = OrientationStruct()
        lib.rt4_orientation_update(fi, te, psi, byref(self.s))

    def __getattr__(self, name):
        return list(getattr(self.s, name))

    def section_basis(self, section: int):
        top, right = F4(), F4()
        if lib.rt4_section_basis(byref(self.s), section, top, right) != 0:
            raise RT4Error(-1, f"bad section {section}")
        return list(top), list(right)


def uniforms_from_properties(props: Properties, cells_w: int, cells_h: int, section: int = SECTION_YXZ):
    u = Uniforms()
    o = OrientationStruct()
    err = _errbuf()
    _check(lib.rt4_uniforms_from_properties(props._h, cells_w, cells_h, section, byref(u), byref(o), err, len(err)), err)
    return u


def window_cells(props: Properties, window_type: str = "main"):
    w, h = c_int32(), c_int32()
    err = _errbuf()
    _check(lib.rt4_window_cells(props._h, window_type.encode(), byref(w), byref(h), err, len(err)), err)
    return w.value, h.value


def make_uniforms(width: int, height: int, samples: int, reflections: int, seed: int = 12345, *, small_indent=0.005,
                  k=1.0, matrix_height=2.0, focus_to_matrix=1.5, focus=(0.0, -2.0, 0.0, 0.0), part=1.0,
                  fi=0.0, te=0.0, psi=0.0, section=SECTION_YXZ):
    """Uniforms of the default camera built through the library's own producers."""
    text = (
        f"ray_tracing.samples = {samples}\nray_tracing.reflections_amount = {reflections}\n"
        f"ray_tracing.small_indent = {small_indent!r}\nlight_to_color_conversion_coefficient = {k!r}\n"
        f"camera.matrix_height = {matrix_height!r}\ncamera.focus_to_matrix_distance = {focus_to_matrix!r}\n"
        f"camera.initial_position.x = {focus[0]!r}\ncamera.initial_position.y = {focus[1]!r}\n"
        f"camera.initial_position.z = {focus[2]!r}\ncamera.initial_position.w = {focus[3]!r}\n"
        f"camera.initial_position.fi = {fi!r}\ncamera.initial_position.te = {te!r}\n"
        f"camera.initial_position.psi = {psi!r}\nconstrain_psi_range = false\n"
    )
    u = uniforms_from_properties(Properties(text=text), width, height, section)
    u.seed = ctypes.c_int32(seed & 0xFFFFFFFF if seed >= 0 else seed).value
    u.part = part
    return u


BUILTIN_SCENES = ("sphere", "room", "tiger", "cylinder4d", "hypercube")
SCENES_DIR = os.path.join(os.path.dirname(_HERE), "scenes")


class Scene:
    """A parsed scene (rt4_scene_desc)."""

    def __init__(self, desc: SceneDesc):
        self.desc = desc

    @classmethod
    def builtin(cls, name: str) -> "Scene":
        d = SceneDesc()
        err = _errbuf()
        _check(lib.rt4_scene_builtin(name.encode(), byref(d), err, len(err)), err)
        return cls(d)

    @classmethod
    def load_frag(cls, path: str) -> "Scene":
        d = SceneDesc()
        err = _errbuf()
        _check(lib.rt4_scene_load_frag(os.fsencode(path), byref(d), err, len(err)), err)
        return cls(d)

    @classmethod
    def parse(cls, text: str) -> "Scene":
        d = SceneDesc()
        err = _errbuf()
        raw = text.encode("utf-8")
        _check(lib.rt4_scene_parse_frag(raw, len(raw), byref(d), err, len(err)), err)
        return cls(d)

    @classmethod
    def named(cls, name: str) -> "Scene":
        """A builtin reference scene, or scenes/<name>.frag of this repository, or a path to a .frag file."""
        if name in BUILTIN_SCENES:
            return cls.builtin(name)
        path = name if name.endswith(".frag") else os.path.join(SCENES_DIR, name + ".frag")
        return cls.load_frag(path)

    def to_bytes(self) -> bytes:
        return bytes(self.desc)

    def groups(self):
        return [(g.kind, g.first, g.count, g.outer, g.new_first) for g in self.desc.groups[: self.desc.n_groups]]

    def surface_count(self) -> int:
        """Surfaces of the scene: everything a G-buffer pixel can name (rt4_scene_surface_count)."""
        return int(lib.rt4_scene_surface_count(byref(self.desc)))

    def surface(self, i: int) -> dict:
        """Surface i (rt4_scene_surface): kind (GROUP_*), index in the kind's array, part inside a composite and
        the material (glow, refl_prob, color)."""
        kind, index, part, m = c_int32(), c_int32(), c_int32(), Material()
        err = _errbuf()
        _check(lib.rt4_scene_surface(byref(self.desc), i, byref(kind), byref(index), byref(part), byref(m), err, len(err)), err)
        return {"kind": kind.value, "index": index.value, "part": part.value, "glow": m.glow, "refl_prob": m.refl_prob,
                "color": tuple(m.color)}


def denoise_params(levels: int | None = None, cos_min: float | None = None, depth_tol: float | None = None,
                   max_refl_prob: float | None = None) -> DenoiseParams:
    """rt4_denoise_params_default (3 levels, 0.9, 0.1, 0.5) with the given fields replaced."""
    p = DenoiseParams()
    lib.rt4_denoise_params_default(byref(p))
    for name, v in (("levels", levels), ("cos_min", cos_min), ("depth_tol", depth_tol), ("max_refl_prob", max_refl_prob)):
        if v is not None:
            setattr(p, name, v)
    return p


def light_denoise_params(levels: int | None = None, cos_min: float | None = None, depth_tol: float | None = None,
                         max_refl_prob: float | None = None, sigma: float | None = None,
                         eps: float | None = None) -> LightDenoiseParams:
    """rt4_light_denoise_params_default (5 levels, 0.9, 0.1, 0.5, sigma 4, eps 1e-6) with the given fields replaced."""
    p = LightDenoiseParams()
    lib.rt4_light_denoise_params_default(byref(p))
    for name, v in (("levels", levels), ("cos_min", cos_min), ("depth_tol", depth_tol), ("max_refl_prob", max_refl_prob),
                    ("sigma", sigma), ("eps", eps)):
        if v is not None:
            setattr(p, name, v)
    return p


def tile_select_params(threshold: float | None = None, min_above: int | None = None, min_frames: int | None = None,
                       dilate: int | None = None) -> TileSelectParams:
    """rt4_tile_select_params_default (threshold 1/255, min_above 4, min_frames 8, dilate 1: the values of the study in
    DESIGN.md §4.39) with the given fields replaced."""
    p = TileSelectParams()
    lib.rt4_tile_select_params_default(byref(p))
    for name, v in (("threshold", threshold), ("min_above", min_above), ("min_frames", min_frames), ("dilate", dilate)):
        if v is not None:
            setattr(p, name, v)
    return p


# The adaptive loop's defaults (Tracer.render_light_adaptive, rt4_render --light --adaptive): the values of the study in
# whole frames first, frames per pass, every how many passes a whole-frame pass.
ADAPTIVE_WARMUP = 8
ADAPTIVE_PASS_FRAMES = 4
ADAPTIVE_FULL_EVERY = 4


def reproject_params(cos_min: float | None = None, plane_tol: float | None = None, slice_tol: float | None = None,
                     max_refl_prob: float | None = None, max_history: int | None = None) -> ReprojectParams:
    """rt4_reproject_params_default (0.9, 0.02, 0.01, 0.5, 255) with the given fields replaced."""
    p = ReprojectParams()
    lib.rt4_reproject_params_default(byref(p))
    for name, v in (("cos_min", cos_min), ("plane_tol", plane_tol), ("slice_tol", slice_tol),
                    ("max_refl_prob", max_refl_prob), ("max_history", max_history)):
        if v is not None:
            setattr(p, name, v)
    return p


def upscale_params(mode: int | None = None, cos_min: float | None = None, plane_tol: float | None = None) -> UpscaleParams:
    """rt4_upscale_params_default (UPSCALE_GUIDED, 0.9, 0.02) with the given fields replaced."""
    p = UpscaleParams()
    lib.rt4_upscale_params_default(byref(p))
    for name, v in (("mode", mode), ("cos_min", cos_min), ("plane_tol", plane_tol)):
        if v is not None:
            setattr(p, name, v)
    return p


def upscale_uniforms(u_cells: Uniforms, scale: int) -> Uniforms:
    """The uniforms of the window a cell image of `u_cells` is stretched over: resolution * scale, nothing else
    (rt4_upscale_uniforms)."""
    out = Uniforms()
    st = lib.rt4_upscale_uniforms(byref(u_cells), scale, byref(out))
    if st != 0:
        raise RT4Error(st, f"scale {scale} outside 1..{UPSCALE_MAX_SCALE}, or a window beyond 65535 x 16383")
    return out


def retina_params(alpha_sky: float | None = None, alpha_fill: float | None = None, alpha_edge: float | None = None,
                  t_min: float | None = None, background=None) -> RetinaParams:
    """rt4_retina_params: the library's defaults, overridden by the arguments given."""
    p = RetinaParams()
    lib.rt4_retina_params_default(byref(p))
    for name, v in (("alpha_sky", alpha_sky), ("alpha_fill", alpha_fill), ("alpha_edge", alpha_edge), ("t_min", t_min)):
        if v is not None:
            setattr(p, name, v)
    if background is not None:
        p.background[0], p.background[1], p.background[2] = background
    return p


def retina_slice_uniforms(u: Uniforms, w_drct, depth: int, depth_size: float, slice_index: int) -> Uniforms:
    """The uniforms of one slice of a `depth`-slice retina of the view u (rt4_retina_slice_uniforms): the matrix centre
    shifted along w_drct, the seed decorrelated; the middle slice of an odd depth is u itself."""
    out = Uniforms()
    wd = (c_float * 4)(*w_drct)
    if lib.rt4_retina_slice_uniforms(byref(u), wd, depth, depth_size, slice_index, byref(out)) != 0:
        raise RT4Error(-1, f"retina_slice_uniforms: depth {depth}, slice {slice_index}, depth_size {depth_size}")
    return out


def retina_view(w: int, h: int, d: int, size, yaw: float = 0.0, pitch: float = 0.0, extent: float = 0.0, ow: int = 0,
                oh: int = 0, step_voxels: float = 1.0) -> RetinaView:
    """An orthographic view of the w x h x d retina box of `size` scene units (mtr_sizes[0], mtr_sizes[1], depth_size)
    for an ow x oh picture (rt4_retina_view_make); angles in radians, extent 0 = the box diagonal."""
    v = RetinaView()
    sz = (c_float * 3)(*size)
    err = _errbuf()
    _check(lib.rt4_retina_view_make(w, h, d, sz, yaw, pitch, extent, ow, oh, step_voxels, byref(v), err, len(err)), err)
    return v


VOXEL_DTYPE = "float32"  # a voxel volume: (d, h, row stride, 4) of premultiplied r, g, b, a


def region(w: int, h: int, x0: int = 0, y0: int = 0, band_rows: int = 0, band_step: int = 0) -> Region:
    return Region(x0, y0, w, h, band_rows, band_step)


def band_plan(width: int, height: int, world: int, rank: int, band: int = 8):
    """(region of `rank`, rows_max) of the C ABI's pixel-band plan (rt4_band_plan; shard.py make_plan)."""
    reg, rows_max = Region(), c_int32()
    err = _errbuf()
    _check(lib.rt4_band_plan(width, height, world, band, rank, byref(reg), byref(rows_max), err, len(err)), err)
    return reg, rows_max.value


def bands_unpermute_device(gathered_ptr: int, image_ptr: int, width: int, height: int, world: int, rows_max: int,
                           fmt: int = FRAME_RGBA32F, band: int = 8, stream: int = 0) -> None:
    """The frame from world x rows_max gathered shard rows on the device (rt4_bands_unpermute_device)."""
    err = _errbuf()
    _check(lib.rt4_bands_unpermute_device(c_void_p(gathered_ptr), c_void_p(image_ptr), width, height, world, band,
                                          rows_max, fmt, c_void_p(stream), err, len(err)), err)


class Camera:
    """The reference's camera controller (src/controls.cpp) over rt4_camera: mouse/wheel rotation,
    WASD/Space/Shift/E/Q motion and per-frame uniforms (main.cpp:86-91)."""

    def __init__(self, props: "Properties"):
        self.s = CameraStruct()
        err = _errbuf()
        _check(lib.rt4_camera_init(props._h, byref(self.s), err, len(err)), err)

    def rotate(self, d_fi=0.0, d_te=0.0, d_psi=0.0):
        lib.rt4_camera_rotate(byref(self.s), d_fi, d_te, d_psi)

    def mouse_move(self, dx: int, dy: int, max_offset: int) -> bool:
        """True when the move only re-centres the cursor (out of the allowed offset)."""
        return bool(lib.rt4_camera_mouse_move(byref(self.s), dx, dy, max_offset))

    def wheel(self, delta: float):
        lib.rt4_camera_wheel(byref(self.s), delta)

    def move(self, keys: int, seconds: float):
        lib.rt4_camera_move(byref(self.s), keys, seconds)

    def frame_uniforms(self, base: Uniforms, section: int = SECTION_YXZ, seed: int = 0) -> Uniforms:
        out = Uniforms()
        seed = ctypes.c_int32(seed & 0xFFFFFFFF).value
        if lib.rt4_camera_frame_uniforms(byref(self.s), byref(base), section, seed, byref(out)) != 0:
            raise RT4Error(-1, "rt4_camera_frame_uniforms failed")
        return out


def write_ppm(path: str, frame, fmt: int | None = None) -> None:
    """Binary PPM of an (h, w, 4) frame (float32 / float16 / uint8), rows top first (rt4_write_ppm)."""
    import numpy as np

    frame = np.ascontiguousarray(frame)
    if fmt is None:
        fmt = {np.dtype("float32"): FRAME_RGBA32F, np.dtype("float16"): FRAME_RGBA16F,
               np.dtype("uint8"): FRAME_RGBA8}[frame.dtype]
    h, w = frame.shape[:2]
    err = _errbuf()
    _check(lib.rt4_write_ppm(os.fsencode(path), c_void_p(frame.ctypes.data), fmt, w, h, w, err, len(err)), err)


def accum_save(path: str, frame, frames_done: int, seed: int, fmt: int | None = None, key: int = 0) -> None:
    """Checkpoint of a progressive accumulator (rt4_accum_save_key): the (h, w, 4) host frame and the number of
    frames already blended into it, with the base seed of its rt4_progressive_uniforms and the run's key
    (accum_key; 0 = not recorded). Written to path + ".tmp" and renamed over path."""
    import numpy as np

    frame = np.ascontiguousarray(frame)
    if fmt is None:
        fmt = {np.dtype("float32"): FRAME_RGBA32F, np.dtype("float16"): FRAME_RGBA16F,
               np.dtype("uint8"): FRAME_RGBA8}[frame.dtype]
    h, w = frame.shape[:2]
    err = _errbuf()
    _check(lib.rt4_accum_save_key(os.fsencode(path), c_void_p(frame.ctypes.data), fmt, w, h, w, frames_done,
                                  seed & 0xFFFFFFFF, key & 0xFFFFFFFF, err, len(err)), err)


def accum_key(scene, u) -> int:
    """The run key a checkpoint records (rt4_accum_key): scene + image-deciding uniforms, not seed or part."""
    return lib.rt4_accum_key(byref(scene.desc if hasattr(scene, "desc") else scene), byref(u))


def accum_key_of(path: str) -> int:
    """The key a checkpoint was saved with (0: not recorded)."""
    k = c_uint32()
    err = _errbuf()
    _check(lib.rt4_accum_key_of(os.fsencode(path), byref(k), err, len(err)), err)
    return k.value


def accum_info(path: str) -> dict:
    """The checkpoint's header (rt4_accum_info): w, h, format, frames_done, seed."""
    w, h, f, n, sd = c_int32(), c_int32(), c_int32(), c_int64(), c_uint32()
    err = _errbuf()
    _check(lib.rt4_accum_info(os.fsencode(path), byref(w), byref(h), byref(f), byref(n), byref(sd), err, len(err)), err)
    return {"w": w.value, "h": h.value, "format": f.value, "frames_done": n.value, "seed": sd.value}


def accum_load(path: str):
    """(frame, frames_done, seed) from a checkpoint (rt4_accum_load); frame is an (h, w, 4) numpy array of the
    checkpoint's format."""
    import numpy as np

    info = accum_info(path)
    frame = np.empty((info["h"], info["w"], 4), dtype=FRAME_NUMPY[info["format"]])
    n, sd = c_int64(), c_uint32()
    err = _errbuf()
    _check(lib.rt4_accum_load(os.fsencode(path), c_void_p(frame.ctypes.data), info["format"], info["w"], info["h"],
                              info["w"], byref(n), byref(sd), err, len(err)), err)
    return frame, n.value, sd.value


def light_bands_unpermute_device(gathered_ptr: int, image_ptr: int, width: int, height: int, world: int, rows_max: int,
                                 band: int = 8, stream: int = 0) -> None:
    """The light accumulator from world x rows_max gathered shard rows of rt4_light_px on the device
    (rt4_light_bands_unpermute_device)."""
    err = _errbuf()
    _check(lib.rt4_light_bands_unpermute_device(c_void_p(gathered_ptr or None), c_void_p(image_ptr or None), width, height,
                                                world, band, rows_max, c_void_p(stream or None), err, len(err)), err)


def frame_split(n_frames: int, world: int, rank: int):
    """(first, count) of the C ABI's frame split (rt4_frame_split; shard.py frame_split): `rank` renders the progressive
    frames first + 1 .. first + count."""
    first, count = c_int32(), c_int32()
    err = _errbuf()
    _check(lib.rt4_frame_split(n_frames, world, rank, byref(first), byref(count), err, len(err)), err)
    return first.value, count.value


def light_save(path: str, light, frames_issued: int, seed: int, key: int = 0, flags: int = 0, w: int | None = None) -> None:
    """Checkpoint of a host light accumulator (h, stride) of LIGHT_DTYPE (rt4_light_save): frames_issued is the last
    progressive frame number folded in, seed the base seed, key the run's accum_key (0 = not recorded), flags
    LIGHT_POOLED for a pool of several seeds; w: the image width when rows are padded."""
    assert light.dtype == LIGHT_DTYPE and light.flags["C_CONTIGUOUS"]
    h = light.shape[0]
    w = light.shape[1] if w is None else w
    err = _errbuf()
    _check(lib.rt4_light_save(os.fsencode(path), c_void_p(light.ctypes.data), w, h, light.shape[1], frames_issued,
                              seed & 0xFFFFFFFF, key & 0xFFFFFFFF, flags & 0xFFFFFFFF, err, len(err)), err)


def light_info(path: str) -> dict:
    """The light checkpoint's header (rt4_light_info): w, h, frames_issued, seed, key, flags."""
    w, h, n, sd, k, fl = c_int32(), c_int32(), c_int64(), c_uint32(), c_uint32(), c_uint32()
    err = _errbuf()
    _check(lib.rt4_light_info(os.fsencode(path), byref(w), byref(h), byref(n), byref(sd), byref(k), byref(fl), err,
                              len(err)), err)
    return {"w": w.value, "h": h.value, "frames_issued": n.value, "seed": sd.value, "key": k.value, "flags": fl.value}


def light_load(path: str, light=None, w: int | None = None):
    """(light, info) from a light checkpoint (rt4_light_load): light is an (h, w) array of LIGHT_DTYPE, or the array
    given ((h, stride >= w), w: the image width when rows are padded); info as light_info."""
    import numpy as np

    if light is None:
        info = light_info(path)
        light = np.zeros((info["h"], info["w"]), LIGHT_DTYPE)
    assert light.dtype == LIGHT_DTYPE and light.flags["C_CONTIGUOUS"]
    h = light.shape[0]
    w = light.shape[1] if w is None else w
    n, sd, k, fl = c_int64(), c_uint32(), c_uint32(), c_uint32()
    err = _errbuf()
    _check(lib.rt4_light_load(os.fsencode(path), c_void_p(light.ctypes.data), w, h, light.shape[1], byref(n), byref(sd),
                              byref(k), byref(fl), err, len(err)), err)
    return light, {"w": w, "h": h, "frames_issued": n.value, "seed": sd.value, "key": k.value, "flags": fl.value}


def write_png(path: str, frame, fmt: int | None = None) -> None:
    """8-bit RGB PNG of an (h, w, 4) frame, the same pixels as write_ppm (rt4_write_png)."""
    import numpy as np

    frame = np.ascontiguousarray(frame)
    if fmt is None:
        fmt = {np.dtype("float32"): FRAME_RGBA32F, np.dtype("float16"): FRAME_RGBA16F,
               np.dtype("uint8"): FRAME_RGBA8}[frame.dtype]
    h, w = frame.shape[:2]
    err = _errbuf()
    _check(lib.rt4_write_png(os.fsencode(path), c_void_p(frame.ctypes.data), fmt, w, h, w, err, len(err)), err)


def frame_format_bytes(fmt: int) -> int:
    return lib.rt4_frame_format_bytes(fmt)


FRAME_NUMPY = {FRAME_RGBA32F: "float32", FRAME_RGBA16F: "float16", FRAME_RGBA8: "uint8"}


def debug_sqrt_thresholds(r: float, library=None):
    """(gt, lt) of rt4_debug_sqrt_thresholds: the band-filter thresholds set_scene makes from the radius r, as
    Python floats holding float32 values. Host only: no context, no device."""
    gt, lt = c_float(), c_float()
    if (library or lib).rt4_debug_sqrt_thresholds(c_float(r), byref(gt), byref(lt)) != 0:
        raise RT4Error(-1, "rt4_debug_sqrt_thresholds failed")
    return gt.value, lt.value


def progressive_uniforms(base: Uniforms, frame_number: int) -> Uniforms:
    """Uniforms of progressive frame n >= 1: part = 1/n, seed_n = seed ^ n*0x9E3779B9 (rt4.h)."""
    out = Uniforms()
    if lib.rt4_progressive_uniforms(byref(base), frame_number, byref(out)) != 0:
        raise RT4Error(-1, f"bad progressive frame number {frame_number}")
    return out


class Tracer:
    """Device context: scene on the device (+ optional sampler table) and the trace kernel."""

    def __init__(self, device: int = 0, flags: int = 0, scene: Scene | None = None, library=None):
        self._lib = library or lib  # library: load_variant(...) of another build (diagnostics)
        # librt4.so links the system HIP runtime; PyTorch-ROCm brings its own copy. In one process the
        # torch runtime must initialise first (torch.cuda reports no GPU when it comes second).
        torch = sys.modules.get("torch")
        if torch is not None and hasattr(torch, "cuda") and not torch.cuda.is_initialized():
            try:
                torch.cuda.init()
            except Exception:  # no GPU for torch: librt4.so reports its own error below
                pass
        h = c_void_p()
        err = _errbuf()
        _check(self._lib.rt4_context_create(device, flags, byref(h), err, len(err)), err)
        self._h = h
        self.device = device
        if scene is not None:
            self.set_scene(scene)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt4_context_destroy(self._h)
            self._h = None

    __del__ = close

    def set_scene(self, scene: Scene) -> None:
        err = _errbuf()
        _check(self._lib.rt4_context_set_scene(self._h, byref(scene.desc), err, len(err)), err)
        self._scene = scene  # pick() names the object under the cursor with it

    def render_device(self, u: Uniforms, reg: Region, frame_ptr: int, row_stride_px: int, counter_ptr: int = 0,
                      stream: int = 0) -> None:
        """Asynchronous launch on `stream` into a device float4 framebuffer (e.g. a torch tensor's data_ptr())."""
        err = _errbuf()
        _check(self._lib.rt4_render_device(self._h, byref(u), byref(reg), c_void_p(frame_ptr), row_stride_px,
                                     c_void_p(counter_ptr or None), c_void_p(stream or None), err, len(err)), err)

    def render_device_ex(self, u: Uniforms, reg: Region, frame_ptr: int, fmt: int, row_stride_px: int,
                         counter_ptr: int = 0, stream: int = 0) -> None:
        """render_device into a device frame of any rt4_frame_format."""
        err = _errbuf()
        _check(self._lib.rt4_render_device_ex(self._h, byref(u), byref(reg), c_void_p(frame_ptr), fmt, row_stride_px,
                                        c_void_p(counter_ptr or None), c_void_p(stream or None), err, len(err)), err)

    def render_frames_device(self, us, reg: Region, frame_ptr: int, fmt: int, row_stride_px: int,
                             counter_ptr: int = 0, stream: int = 0) -> None:
        """len(us) consecutive frames into one device frame, pipelined (rt4_render_frames_device): the same
        result as render_device_ex(us[0]), render_device_ex(us[1]), ... in order."""
        arr = (Uniforms * len(us))(*us)
        err = _errbuf()
        _check(self._lib.rt4_render_frames_device(self._h, arr, len(us), byref(reg), c_void_p(frame_ptr), fmt, row_stride_px,
                                            c_void_p(counter_ptr or None), c_void_p(stream or None), err, len(err)), err)

    def frames_per_launch(self, w: int, h: int) -> int:
        """Frames per pipelined launch for a w x h region with the current scene (1: frame by frame)."""
        return int(self._lib.rt4_context_frames_per_launch(self._h, w, h))

    def reserve_frames(self, w: int, h: int) -> None:
        """Allocate the frame-colour scratch of pipelined launches of a w x h region up front."""
        err = _errbuf()
        _check(self._lib.rt4_context_reserve_frames(self._h, w, h, err, len(err)), err)

    def frame_scratch_bytes(self) -> int:
        """Bytes of the context's frame-colour scratch (0: none allocated)."""
        return int(self._lib.rt4_context_frame_scratch_bytes(self._h))

    def overlap_bytes(self) -> int:
        """Bytes of the context's overlap slot buffers (rt4.h rt4_context_overlap_bytes)."""
        return int(self._lib.rt4_context_overlap_bytes(self._h))

    def reserve_overlap(self, w: int, h: int) -> None:
        """Allocate the slot buffers overlapped single-frame launches of a w x h image use, up front."""
        err = _errbuf()
        _check(self._lib.rt4_context_reserve_overlap(self._h, w, h, err, len(err)), err)

    def render_sections_device(self, jobs, fmt: int = FRAME_RGBA32F, counter_ptr: int = 0, stream: int = 0) -> None:
        """One launch over up to three images: jobs = [(uniforms, region, frame_ptr, row_stride_px), ...]."""
        arr = (SectionJob * len(jobs))()
        for q, (u, reg, ptr, stride) in enumerate(jobs):
            arr[q].u = u
            arr[q].region = reg
            arr[q].d_frame = ptr
            arr[q].row_stride_px = stride
        err = _errbuf()
        _check(self._lib.rt4_render_sections_device(self._h, arr, len(jobs), fmt, c_void_p(counter_ptr or None),
                                              c_void_p(stream or None), err, len(err)), err)

    def render_host_ex(self, u: Uniforms, reg: Region, frame, fmt: int, row_stride_px: int | None = None) -> int:
        """Synchronous render into a host array (h, stride, 4) of the format's dtype (FRAME_NUMPY)."""
        import numpy as np

        assert frame.dtype == np.dtype(FRAME_NUMPY[fmt]) and frame.flags["C_CONTIGUOUS"]
        stride = row_stride_px if row_stride_px is not None else frame.shape[1]
        n = c_uint64()
        err = _errbuf()
        _check(self._lib.rt4_render_host_ex(self._h, byref(u), byref(reg), c_void_p(frame.ctypes.data), fmt, stride,
                                      byref(n), err, len(err)), err)
        return n.value

    def render_host(self, u: Uniforms, reg: Region, frame, row_stride_px: int | None = None) -> int:
        """Synchronous render into a host float32 array of shape (h, stride, 4); returns the intersection count."""
        import numpy as np

        assert frame.dtype == np.float32 and frame.flags["C_CONTIGUOUS"]
        stride = row_stride_px if row_stride_px is not None else frame.shape[1]
        n = c_uint64()
        err = _errbuf()
        _check(self._lib.rt4_render_host(self._h, byref(u), byref(reg), c_void_p(frame.ctypes.data), stride, byref(n), err,
                                   len(err)), err)
        return n.value

    def render_gbuffer_device(self, u: Uniforms, reg: Region, gbuf_ptr: int, row_stride_px: int, stream: int = 0) -> None:
        """Asynchronous: the primary hit of every pixel of `reg` into a device array of rt4_gbuffer_px (32 B each)."""
        err = _errbuf()
        _check(self._lib.rt4_render_gbuffer_device(self._h, byref(u), byref(reg), c_void_p(gbuf_ptr), row_stride_px,
                                                   c_void_p(stream or None), err, len(err)), err)

    def render_gbuffer_host(self, u: Uniforms, reg: Region, gbuf=None, row_stride_px: int | None = None):
        """Synchronous: the G-buffer of `reg` into a host array (h, stride) of GBUFFER_DTYPE (a new one if None)."""
        import numpy as np

        if gbuf is None:
            gbuf = np.zeros((reg.h, row_stride_px or reg.w), GBUFFER_DTYPE)
        assert gbuf.dtype == GBUFFER_DTYPE and gbuf.flags["C_CONTIGUOUS"]
        stride = row_stride_px if row_stride_px is not None else gbuf.shape[1]
        err = _errbuf()
        _check(self._lib.rt4_render_gbuffer_host(self._h, byref(u), byref(reg), c_void_p(gbuf.ctypes.data), stride, err,
                                                 len(err)), err)
        return gbuf

    def pick(self, u: Uniforms, x: int, y: int) -> dict:
        """What is under the cursor at pixel (x, y) of the image of `u` (row 0 on top): the pixel's G-buffer record
        under "px" (a GBUFFER_DTYPE scalar: normal, depth, surface, refl_prob, glow), "hit", and under "object"
        rt4_scene_surface's answer for the surface hit (None on a miss)."""
        px = self.render_gbuffer_host(u, region(1, 1, x, y))[0, 0]
        hit = bool(px["surface"] >= 0)
        scene = getattr(self, "_scene", None)
        return {"px": px, "hit": hit, "object": scene.surface(int(px["surface"])) if hit and scene is not None else None}

    def denoise_device(self, in_ptr: int, in_stride_px: int, out_ptr: int, out_stride_px: int, fmt: int, w: int, h: int,
                       gbuf_ptr: int, gbuf_stride_px: int, params: DenoiseParams | None = None, stream: int = 0) -> None:
        """Asynchronous edge-stopping filter of a device frame into another one (rt4_denoise_device). For display:
        keep accumulating into the input frame, never into the filtered one."""
        p = params if params is not None else denoise_params()
        err = _errbuf()
        _check(self._lib.rt4_denoise_device(self._h, c_void_p(in_ptr or None), in_stride_px, c_void_p(out_ptr or None),
                                            out_stride_px, fmt, w, h, c_void_p(gbuf_ptr or None), gbuf_stride_px, byref(p),
                                            c_void_p(stream or None), err, len(err)), err)

    def denoise_host(self, frame, gbuf, params: DenoiseParams | None = None, out=None, fmt: int | None = None,
                     w: int | None = None):
        """Synchronous filter of a host frame (h, stride, 4) guided by a host G-buffer (h, stride) of GBUFFER_DTYPE;
        w: the image width when the rows are padded (default: every column). Returns `out` (a new array if None)."""
        import numpy as np

        if fmt is None:
            fmt = {np.dtype("float32"): FRAME_RGBA32F, np.dtype("float16"): FRAME_RGBA16F,
                   np.dtype("uint8"): FRAME_RGBA8}[frame.dtype]
        assert frame.dtype == np.dtype(FRAME_NUMPY[fmt]) and frame.flags["C_CONTIGUOUS"]
        assert gbuf.dtype == GBUFFER_DTYPE and gbuf.flags["C_CONTIGUOUS"]
        h = frame.shape[0]
        w = frame.shape[1] if w is None else w
        if out is None:
            out = np.zeros((h, w, 4), frame.dtype)
        assert out.dtype == frame.dtype and out.flags["C_CONTIGUOUS"]
        p = params if params is not None else denoise_params()
        err = _errbuf()
        _check(self._lib.rt4_denoise_host(self._h, c_void_p(frame.ctypes.data), frame.shape[1], c_void_p(out.ctypes.data),
                                          out.shape[1], fmt, w, h, c_void_p(gbuf.ctypes.data), gbuf.shape[1], byref(p), err,
                                          len(err)), err)
        return out

    def denoise_bytes(self) -> int:
        """Bytes of the context's denoise scratch (rt4.h rt4_context_denoise_bytes)."""
        return int(self._lib.rt4_context_denoise_bytes(self._h))

    def reproject_device(self, u_cur: Uniforms, gcur_ptr: int, gcur_stride: int, u_prev: Uniforms, gprev_ptr: int,
                         gprev_stride: int, accp_ptr: int, accp_stride: int, histp_ptr: int, histp_stride: int, acco_ptr: int,
                         acco_stride: int, histo_ptr: int, histo_stride: int, fmt: int, w: int, h: int,
                         params: ReprojectParams | None = None, stream: int = 0) -> None:
        """Asynchronous temporal reprojection of a device image and its history from the view of u_prev into the view
        of u_cur (rt4_reproject_device)."""
        p = params if params is not None else reproject_params()
        err = _errbuf()
        _check(self._lib.rt4_reproject_device(
            self._h, byref(u_cur) if u_cur is not None else None, c_void_p(gcur_ptr or None), gcur_stride,
            byref(u_prev) if u_prev is not None else None, c_void_p(gprev_ptr or None), gprev_stride, c_void_p(accp_ptr or None),
            accp_stride, c_void_p(histp_ptr or None), histp_stride, c_void_p(acco_ptr or None), acco_stride,
            c_void_p(histo_ptr or None), histo_stride, fmt, w, h, byref(p), c_void_p(stream or None), err, len(err)), err)

    def reproject_host(self, u_cur: Uniforms, gcur, u_prev: Uniforms, gprev, acc_prev, hist_prev,
                       params: ReprojectParams | None = None, acc_out=None, hist_out=None, fmt: int | None = None,
                       w: int | None = None):
        """Synchronous reprojection of host arrays: G-buffers (h, stride) of GBUFFER_DTYPE, acc_prev (h, stride, 4) of
        the format's dtype, hist_prev (h, stride) int32; w: the image width when rows are padded. Returns (acc_out,
        hist_out) (new arrays if None)."""
        import numpy as np

        if fmt is None:
            fmt = {np.dtype("float32"): FRAME_RGBA32F, np.dtype("float16"): FRAME_RGBA16F,
                   np.dtype("uint8"): FRAME_RGBA8}[acc_prev.dtype]
        h = acc_prev.shape[0]
        w = acc_prev.shape[1] if w is None else w
        if acc_out is None:
            acc_out = np.zeros((h, w, 4), acc_prev.dtype)
        if hist_out is None:
            hist_out = np.zeros((h, w), np.int32)
        for a, dt in ((gcur, GBUFFER_DTYPE), (gprev, GBUFFER_DTYPE), (acc_prev, np.dtype(FRAME_NUMPY[fmt])),
                      (acc_out, np.dtype(FRAME_NUMPY[fmt])), (hist_prev, np.dtype(np.int32)), (hist_out, np.dtype(np.int32))):
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"] and a.shape[0] == h
        p = params if params is not None else reproject_params()
        err = _errbuf()
        _check(self._lib.rt4_reproject_host(
            self._h, byref(u_cur), c_void_p(gcur.ctypes.data), gcur.shape[1], byref(u_prev), c_void_p(gprev.ctypes.data),
            gprev.shape[1], c_void_p(acc_prev.ctypes.data), acc_prev.shape[1], c_void_p(hist_prev.ctypes.data),
            hist_prev.shape[1], c_void_p(acc_out.ctypes.data), acc_out.shape[1], c_void_p(hist_out.ctypes.data),
            hist_out.shape[1], fmt, w, h, byref(p), err, len(err)), err)
        return acc_out, hist_out

    def upscale_device(self, u_cells: Uniforms, scale: int, cells_ptr: int, cells_stride: int, gcells_ptr: int,
                       gcells_stride: int, gwin_ptr: int, gwin_stride: int, out_ptr: int, out_stride: int, fmt: int,
                       cells_w: int, cells_h: int, params: UpscaleParams | None = None, stream: int = 0) -> None:
        """Asynchronous upscale of a device cell frame to the window of cells_w*scale x cells_h*scale pixels
        (rt4_upscale_device). UPSCALE_NEAREST takes 0 for both G-buffers."""
        p = params if params is not None else upscale_params()
        err = _errbuf()
        _check(self._lib.rt4_upscale_device(
            self._h, byref(u_cells) if u_cells is not None else None, scale, c_void_p(cells_ptr or None), cells_stride,
            c_void_p(gcells_ptr or None), gcells_stride, c_void_p(gwin_ptr or None), gwin_stride, c_void_p(out_ptr or None),
            out_stride, fmt, cells_w, cells_h, byref(p), c_void_p(stream or None), err, len(err)), err)

    def upscale_host(self, u_cells: Uniforms, scale: int, cells, gcells=None, gwin=None, params: UpscaleParams | None = None,
                     out=None, fmt: int | None = None, cells_w: int | None = None):
        """Synchronous upscale of host arrays: cells (h, stride, 4) of the format's dtype, G-buffers (h, stride) and
        (h*scale, stride) of GBUFFER_DTYPE (None with UPSCALE_NEAREST); cells_w: the cell image's width when rows are
        padded. Returns `out` (h*scale, stride >= cells_w*scale, 4) (a new array if None)."""
        import numpy as np

        if fmt is None:
            fmt = {np.dtype("float32"): FRAME_RGBA32F, np.dtype("float16"): FRAME_RGBA16F,
                   np.dtype("uint8"): FRAME_RGBA8}[cells.dtype]
        ch = cells.shape[0]
        cw = cells.shape[1] if cells_w is None else cells_w
        if out is None:
            out = np.zeros((ch * scale, cw * scale, 4), cells.dtype)
        for a, dt in ((cells, np.dtype(FRAME_NUMPY[fmt])), (out, np.dtype(FRAME_NUMPY[fmt])), (gcells, GBUFFER_DTYPE),
                      (gwin, GBUFFER_DTYPE)):
            assert a is None or (a.dtype == dt and a.flags["C_CONTIGUOUS"])
        p = params if params is not None else upscale_params()
        err = _errbuf()
        _check(self._lib.rt4_upscale_host(
            self._h, byref(u_cells), scale, c_void_p(cells.ctypes.data), cells.shape[1],
            c_void_p(gcells.ctypes.data) if gcells is not None else None, gcells.shape[1] if gcells is not None else 0,
            c_void_p(gwin.ctypes.data) if gwin is not None else None, gwin.shape[1] if gwin is not None else 0,
            c_void_p(out.ctypes.data), out.shape[1], fmt, cw, ch, byref(p), err, len(err)), err)
        return out

    def temporal_blend_device(self, new_ptr: int, new_stride: int, acc_ptr: int, acc_stride: int, fmt: int, hist_ptr: int,
                              hist_stride: int, w: int, h: int, stream: int = 0) -> None:
        """Asynchronous per-pixel progressive blend of an RGBA32F sample frame into a device accumulator of `fmt`,
        part = 1 / (history + 1) per pixel; the history counts up (rt4_temporal_blend_device)."""
        err = _errbuf()
        _check(self._lib.rt4_temporal_blend_device(self._h, c_void_p(new_ptr or None), new_stride, c_void_p(acc_ptr or None),
                                                   acc_stride, fmt, c_void_p(hist_ptr or None), hist_stride, w, h,
                                                   c_void_p(stream or None), err, len(err)), err)

    def render_light_device(self, us, reg: Region, light_ptr: int, row_stride_px: int, counter_ptr: int = 0,
                            stream: int = 0) -> None:
        """Asynchronous: len(us) frames folded in order onto a device light accumulator (rt4_light_px, 32 B per pixel;
        zero bytes = empty), rt4_render_light_device. us may differ only in seed and part; part is ignored."""
        arr = (Uniforms * len(us))(*us)
        err = _errbuf()
        _check(self._lib.rt4_render_light_device(self._h, arr, len(us), byref(reg), c_void_p(light_ptr or None), row_stride_px,
                                                 c_void_p(counter_ptr or None), c_void_p(stream or None), err, len(err)), err)

    def render_light_host(self, us, reg: Region, light=None, row_stride_px: int | None = None):
        """Synchronous: len(us) frames folded onto a host accumulator (h, stride) of LIGHT_DTYPE (a new, empty one if
        None). Returns (light, intersection count)."""
        import numpy as np

        if light is None:
            light = np.zeros((reg.h, row_stride_px or reg.w), LIGHT_DTYPE)
        assert light.dtype == LIGHT_DTYPE and light.flags["C_CONTIGUOUS"]
        stride = row_stride_px if row_stride_px is not None else light.shape[1]
        arr = (Uniforms * len(us))(*us)
        n = c_uint64()
        err = _errbuf()
        _check(self._lib.rt4_render_light_host(self._h, arr, len(us), byref(reg), c_void_p(light.ctypes.data), stride,
                                               byref(n), err, len(err)), err)
        return light, n.value

    def light_resolve_device(self, light_ptr: int, light_stride: int, k: float, frame_ptr: int, fmt: int, frame_stride: int,
                             w: int, h: int, stream: int = 0) -> None:
        """Asynchronous: the image of a device light accumulator in `fmt`, tone-mapped with k (rt4_light_resolve_device)."""
        err = _errbuf()
        _check(self._lib.rt4_light_resolve_device(self._h, c_void_p(light_ptr or None), light_stride, k,
                                                  c_void_p(frame_ptr or None), fmt, frame_stride, w, h,
                                                  c_void_p(stream or None), err, len(err)), err)

    def light_resolve_host(self, light, k: float, fmt: int = FRAME_RGBA32F, out=None, w: int | None = None):
        """Synchronous: the image of a host accumulator (h, stride) of LIGHT_DTYPE as (h, stride >= w, 4) of the
        format's dtype; w: the image width when rows are padded. Returns `out` (a new array if None)."""
        import numpy as np

        assert light.dtype == LIGHT_DTYPE and light.flags["C_CONTIGUOUS"]
        h = light.shape[0]
        w = light.shape[1] if w is None else w
        if out is None:
            out = np.zeros((h, w, 4), FRAME_NUMPY[fmt])
        assert out.dtype == np.dtype(FRAME_NUMPY[fmt]) and out.flags["C_CONTIGUOUS"] and out.shape[0] == h
        err = _errbuf()
        _check(self._lib.rt4_light_resolve_host(self._h, c_void_p(light.ctypes.data), light.shape[1], k,
                                                c_void_p(out.ctypes.data), fmt, out.shape[1], w, h, err, len(err)), err)
        return out

    def light_noise_device(self, light_ptr: int, light_stride: int, w: int, h: int, k: float, threshold: float,
                           se_ptr: int, q_ptr: int, map_stride: int, tile_ptr: int, stats_ptr: int, stream: int = 0) -> None:
        """Asynchronous: the standard-error map, the display-error map q (float, row stride map_stride), `above` per 8x8
        tile (int32, ceil(w/8) x ceil(h/8)) and the rt4_noise_stats of a device accumulator (rt4_light_noise_device).
        Any of se_ptr, q_ptr, tile_ptr may be 0."""
        err = _errbuf()
        _check(self._lib.rt4_light_noise_device(self._h, c_void_p(light_ptr or None), light_stride, w, h, k, threshold,
                                                c_void_p(se_ptr or None), c_void_p(q_ptr or None), map_stride,
                                                c_void_p(tile_ptr or None), c_void_p(stats_ptr or None),
                                                c_void_p(stream or None), err, len(err)), err)

    def light_noise_host(self, light, k: float, threshold: float, w: int | None = None, se=True, q=True, tiles=True):
        """Synchronous: (se, q, tile_above, stats) of a host accumulator (h, stride) of LIGHT_DTYPE: float32 (h, w) maps,
        the int32 (ceil(h/8), ceil(w/8)) tile image and a dict of rt4_noise_stats. se / q / tiles: True for a new array,
        an array to write into (maps: shape (h, stride >= w), one stride for both), or False / None to leave it out."""
        import numpy as np

        assert light.dtype == LIGHT_DTYPE and light.flags["C_CONTIGUOUS"]
        h = light.shape[0]
        w = light.shape[1] if w is None else w
        se = np.zeros((h, w), np.float32) if se is True else (se if se is not False else None)
        q = np.zeros((h, w), np.float32) if q is True else (q if q is not False else None)
        tiles = np.zeros(((h + 7) // 8, (w + 7) // 8), np.int32) if tiles is True else (tiles if tiles is not False else None)
        maps = [m for m in (se, q) if m is not None]
        for m in maps:
            assert m.dtype == np.float32 and m.flags["C_CONTIGUOUS"] and m.shape[0] == h and m.shape[1] == maps[0].shape[1]
        assert tiles is None or (tiles.dtype == np.int32 and tiles.flags["C_CONTIGUOUS"])
        st = NoiseStats()
        err = _errbuf()
        _check(self._lib.rt4_light_noise_host(
            self._h, c_void_p(light.ctypes.data), light.shape[1], w, h, k, threshold,
            c_void_p(se.ctypes.data) if se is not None else None, c_void_p(q.ctypes.data) if q is not None else None,
            maps[0].shape[1] if maps else w, c_void_p(tiles.ctypes.data) if tiles is not None else None, byref(st), err,
            len(err)), err)
        return se, q, tiles, {"pixels": st.pixels, "measured": st.measured, "above": st.above, "max_q": st.max_q,
                              "max_se": st.max_se}

    def light_merge_device(self, dst_ptr: int, dst_stride: int, srcs_ptr: int, src_stride: int, src_plane_stride: int,
                           n_srcs: int, w: int, h: int, stream: int = 0) -> None:
        """Asynchronous: n_srcs device light accumulators (source s, pixel (i, j) at s * src_plane_stride + i * src_stride
        + j pixels) merged in order into the one at dst_ptr (rt4_light_merge_device)."""
        err = _errbuf()
        _check(self._lib.rt4_light_merge_device(self._h, c_void_p(dst_ptr or None), dst_stride, c_void_p(srcs_ptr or None),
                                                src_stride, src_plane_stride, n_srcs, w, h, c_void_p(stream or None), err,
                                                len(err)), err)

    def light_merge_host(self, dst, srcs, w: int | None = None):
        """Synchronous: the host accumulators srcs (K, rows >= h, stride) of LIGHT_DTYPE (or a list of K equal 2-D arrays)
        merged in order into dst (h, stride) in place; w: the image width when rows are padded. Rows of a source past
        h pad its plane, as the rows past a rank's own do in a gather. Returns dst."""
        import numpy as np

        if isinstance(srcs, (list, tuple)):
            srcs = np.stack(srcs)
        assert dst.dtype == LIGHT_DTYPE and dst.flags["C_CONTIGUOUS"] and dst.ndim == 2
        assert srcs.dtype == LIGHT_DTYPE and srcs.flags["C_CONTIGUOUS"] and srcs.ndim == 3
        h = dst.shape[0]
        w = dst.shape[1] if w is None else w
        err = _errbuf()
        _check(self._lib.rt4_light_merge_host(self._h, c_void_p(dst.ctypes.data), dst.shape[1], c_void_p(srcs.ctypes.data),
                                              srcs.shape[2], srcs.shape[1] * srcs.shape[2], srcs.shape[0], w, h, err,
                                              len(err)), err)
        return dst

    def light_downsample_device(self, fine_ptr: int, fine_stride: int, out_ptr: int, out_stride: int, w: int, h: int, s: int,
                                stream: int = 0) -> None:
        """Asynchronous: the (w*s) x (h*s) device light accumulator at fine_ptr, the s x s sub-pixel strata of every
        pixel of the view at 1/s the resolution, into the w x h accumulator at out_ptr (rt4_light_downsample_device)."""
        err = _errbuf()
        _check(self._lib.rt4_light_downsample_device(self._h, c_void_p(fine_ptr or None), fine_stride, c_void_p(out_ptr or None),
                                                     out_stride, w, h, s, c_void_p(stream or None), err, len(err)), err)

    def light_downsample_host(self, fine, s: int, out=None, w: int | None = None, h: int | None = None):
        """Synchronous: the host accumulator fine (h*s rows, stride >= w*s) of LIGHT_DTYPE into out (h, stride >= w; a
        new, empty (h, w) one if None). w, h: the output size when rows are padded (default: fine's shape over s).
        The padding of out keeps its bytes. Returns out."""
        import numpy as np

        assert fine.dtype == LIGHT_DTYPE and fine.flags["C_CONTIGUOUS"] and fine.ndim == 2
        h = (out.shape[0] if out is not None else fine.shape[0] // max(s, 1)) if h is None else h
        w = (out.shape[1] if out is not None else fine.shape[1] // max(s, 1)) if w is None else w
        if out is None:
            out = np.zeros((h, w), LIGHT_DTYPE)
        assert out.dtype == LIGHT_DTYPE and out.flags["C_CONTIGUOUS"] and out.ndim == 2
        # the library reads and writes whole strided images: the arrays must hold them (s itself is the library's to refuse)
        assert out.shape[0] >= h and out.shape[1] >= w
        assert s < 1 or (fine.shape[0] >= h * s and fine.shape[1] >= w * s)
        err = _errbuf()
        _check(self._lib.rt4_light_downsample_host(self._h, c_void_p(fine.ctypes.data), fine.shape[1],
                                                   c_void_p(out.ctypes.data), out.shape[1], w, h, s, err, len(err)), err)
        return out

    def light_denoise_device(self, light_ptr: int, light_stride: int, gbuf_ptr: int, gbuf_stride: int, k: float,
                             frame_ptr: int, fmt: int, frame_stride: int, w: int, h: int,
                             params: LightDenoiseParams | None = None, filtered_ptr: int = 0, filtered_stride: int = 0,
                             stream: int = 0) -> None:
        """Asynchronous: the variance-guided a-trous filter of a device light accumulator, guided by the G-buffer of
        the same view, tone-mapped with k into a frame of `fmt` (rt4_light_denoise_device). filtered_ptr: an optional
        float4 image {L_r, L_g, L_b, V} (row stride in float4). For display: the accumulator is only read."""
        p = params if params is not None else light_denoise_params()
        err = _errbuf()
        _check(self._lib.rt4_light_denoise_device(self._h, c_void_p(light_ptr or None), light_stride,
                                                  c_void_p(gbuf_ptr or None), gbuf_stride, k, byref(p),
                                                  c_void_p(frame_ptr or None), fmt, frame_stride,
                                                  c_void_p(filtered_ptr or None), filtered_stride, w, h,
                                                  c_void_p(stream or None), err, len(err)), err)

    def light_denoise_host(self, light, gbuf, k: float, params: LightDenoiseParams | None = None, fmt: int = FRAME_RGBA32F,
                           out=None, filtered=False, w: int | None = None):
        """Synchronous: the filtered image of a host accumulator (h, stride) of LIGHT_DTYPE and a host G-buffer
        (h, stride) of GBUFFER_DTYPE as (h, stride >= w, 4) of the format's dtype; w: the image width when rows are
        padded. filtered: True for a new float32 (h, w, 4) array {L_r, L_g, L_b, V}, or an array (h, stride >= w, 4) to
        write into. Returns `out` (a new array if None), or (out, filtered) when the filtered light was asked for."""
        import numpy as np

        assert light.dtype == LIGHT_DTYPE and light.flags["C_CONTIGUOUS"]
        assert gbuf.dtype == GBUFFER_DTYPE and gbuf.flags["C_CONTIGUOUS"] and gbuf.shape[0] == light.shape[0]
        h = light.shape[0]
        w = light.shape[1] if w is None else w
        if out is None:
            out = np.zeros((h, w, 4), FRAME_NUMPY[fmt])
        assert out.dtype == np.dtype(FRAME_NUMPY[fmt]) and out.flags["C_CONTIGUOUS"] and out.shape[0] == h
        fl = np.zeros((h, w, 4), np.float32) if filtered is True else (filtered if filtered is not False else None)
        assert fl is None or (fl.dtype == np.float32 and fl.flags["C_CONTIGUOUS"] and fl.shape[0] == h and fl.shape[2] == 4)
        p = params if params is not None else light_denoise_params()
        err = _errbuf()
        _check(self._lib.rt4_light_denoise_host(
            self._h, c_void_p(light.ctypes.data), light.shape[1], c_void_p(gbuf.ctypes.data), gbuf.shape[1], k, byref(p),
            c_void_p(out.ctypes.data), fmt, out.shape[1], c_void_p(fl.ctypes.data) if fl is not None else None,
            fl.shape[1] if fl is not None else 0, w, h, err, len(err)), err)
        return out if fl is None else (out, fl)

    def light_denoise_bytes(self) -> int:
        """Bytes of the context's light-denoise scratch (rt4.h rt4_context_light_denoise_bytes)."""
        return int(self._lib.rt4_context_light_denoise_bytes(self._h))

    def light_select_tiles_device(self, light_ptr: int, light_stride: int, w: int, h: int, k: float,
                                  params: TileSelectParams | None, tiles_ptr: int, count_ptr: int, state_ptr: int = 0,
                                  stream: int = 0) -> None:
        """Asynchronous: the 8x8 tiles of a device accumulator worth more frames, ascending, into tiles_ptr (uint32,
        ceil(w/8) * ceil(h/8) entries), their number into count_ptr (uint32) and, if state_ptr is not 0, 2 / 1 / 0 per
        tile (int32: qualifies / selected by dilation / not selected). rt4_light_select_tiles_device."""
        p = params if params is not None else tile_select_params()
        err = _errbuf()
        _check(self._lib.rt4_light_select_tiles_device(self._h, c_void_p(light_ptr or None), light_stride, w, h, k, byref(p),
                                                       c_void_p(tiles_ptr or None), c_void_p(count_ptr or None),
                                                       c_void_p(state_ptr or None), c_void_p(stream or None), err,
                                                       len(err)), err)

    def light_select_tiles_host(self, light, k: float, params: TileSelectParams | None = None, w: int | None = None,
                                state=True):
        """Synchronous: (tiles, state) of a host accumulator (h, stride) of LIGHT_DTYPE: the selected tiles as a uint32
        array of the selected count, ascending, and the int32 (ceil(h/8), ceil(w/8)) state image (None with
        state=False)."""
        import numpy as np

        assert light.dtype == LIGHT_DTYPE and light.flags["C_CONTIGUOUS"]
        h = light.shape[0]
        w = light.shape[1] if w is None else w
        ty, tx = (h + 7) // 8, (w + 7) // 8
        tiles = np.zeros(ty * tx, np.uint32)
        st = np.zeros((ty, tx), np.int32) if state else None
        n = c_uint32()
        p = params if params is not None else tile_select_params()
        err = _errbuf()
        _check(self._lib.rt4_light_select_tiles_host(self._h, c_void_p(light.ctypes.data), light.shape[1], w, h, k, byref(p),
                                                     c_void_p(tiles.ctypes.data), byref(n),
                                                     c_void_p(st.ctypes.data) if st is not None else None, err, len(err)), err)
        return tiles[:n.value].copy(), st

    def render_light_tiles_device(self, us, reg: Region, tiles_ptr: int, n_tiles: int, light_ptr: int, row_stride_px: int,
                                  counter_ptr: int = 0, stream: int = 0) -> None:
        """Asynchronous: render_light_device for the n_tiles region-local tile numbers (uint32) at tiles_ptr only; every
        other byte of the accumulator keeps its value (rt4_render_light_tiles_device). n_tiles is a host value."""
        arr = (Uniforms * len(us))(*us)
        err = _errbuf()
        _check(self._lib.rt4_render_light_tiles_device(self._h, arr, len(us), byref(reg), c_void_p(tiles_ptr or None), n_tiles,
                                                       c_void_p(light_ptr or None), row_stride_px,
                                                       c_void_p(counter_ptr or None), c_void_p(stream or None), err,
                                                       len(err)), err)

    def render_light_tiles_host(self, us, reg: Region, tiles, light=None, row_stride_px: int | None = None):
        """Synchronous: len(us) frames of the listed tiles folded onto a host accumulator (a new, empty one if None).
        Returns (light, intersection count)."""
        import numpy as np

        if light is None:
            light = np.zeros((reg.h, row_stride_px or reg.w), LIGHT_DTYPE)
        assert light.dtype == LIGHT_DTYPE and light.flags["C_CONTIGUOUS"]
        stride = row_stride_px if row_stride_px is not None else light.shape[1]
        tiles = np.ascontiguousarray(tiles, np.uint32)
        arr = (Uniforms * len(us))(*us)
        n = c_uint64()
        err = _errbuf()
        _check(self._lib.rt4_render_light_tiles_host(self._h, arr, len(us), byref(reg),
                                                     c_void_p(tiles.ctypes.data) if tiles.size else None, int(tiles.size),
                                                     c_void_p(light.ctypes.data), stride, byref(n), err, len(err)), err)
        return light, n.value

    def select_bytes(self) -> int:
        """Bytes of the context's tile scratch (rt4.h rt4_context_select_bytes)."""
        return int(self._lib.rt4_context_select_bytes(self._h))

    def render_light_adaptive(self, base: Uniforms, w: int, h: int, budget_frames: int, select: TileSelectParams | None = None,
                              warmup: int = ADAPTIVE_WARMUP, pass_frames: int = ADAPTIVE_PASS_FRAMES,
                              full_every: int = ADAPTIVE_FULL_EVERY, light=None):
        """The adaptive loop of DESIGN.md §4.39 on a host accumulator (h, w) of LIGHT_DTYPE (a new, empty one if None),
        the loop rt4_render --light --adaptive runs. The budget is budget_frames whole-frame equivalents:
        budget_frames * tiles tile-frames. `warmup` whole frames first (select.min_frames is set to it), then passes of
        pass_frames frames of the selected tiles; every full_every-th pass (0: never), and a pass whose selection is
        empty, is a whole-frame pass. Frame g uses progressive_uniforms(base, g), g running on across passes. The last
        pass is clipped to the frames the remaining budget pays for; the loop never stops early. Returns (light,
        intersection count, log) with log a list of (kind, listed tiles, frames), kind one of "warmup", "full", "empty",
        "tiles"."""
        import numpy as np

        if light is None:
            light = np.zeros((h, w), LIGHT_DTYPE)
        assert light.dtype == LIGHT_DTYPE and light.shape == (h, w) and light.flags["C_CONTIGUOUS"]
        reg = region(w, h)
        tiles = ((w + 7) // 8) * ((h + 7) // 8)
        budget = budget_frames * tiles
        sel = TileSelectParams.from_buffer_copy(bytes(select if select is not None else tile_select_params()))
        k = base.light_to_color_conversion_coefficient
        count, spent, g, log = 0, 0, 0, []

        def frames(n):
            nonlocal g
            us = [progressive_uniforms(base, f) for f in range(g + 1, g + n + 1)]
            g += n
            return us

        warm = min(warmup, budget_frames)
        sel.min_frames = warm
        if warm > 0:
            count += self.render_light_host(frames(warm), reg, light)[1]
            spent += warm * tiles
            log.append(("warmup", tiles, warm))
        n_pass = 0
        while True:
            n_pass += 1
            kind, listed, lst = "full", tiles, None
            if not (full_every > 0 and n_pass % full_every == 0):
                lst, _ = self.light_select_tiles_host(light, k, sel, state=False)
                if len(lst) == 0:
                    kind, lst = "empty", None
                else:
                    kind, listed = "tiles", len(lst)
            n = min(pass_frames, (budget - spent) // listed)
            if n <= 0:
                break
            us = frames(n)
            count += (self.render_light_host(us, reg, light) if lst is None else self.render_light_tiles_host(us, reg, lst, light))[1]
            spent += n * listed
            log.append((kind, listed, n))
        return light, count, log

    def retina_voxelize_device(self, light_ptr: int, light_strides, gbuf_ptr: int, gbuf_strides, k: float,
                               params: RetinaParams | None, vox_ptr: int, vox_strides, w: int, h: int, d: int,
                               stream: int = 0) -> None:
        """Asynchronous: the premultiplied float4 voxel volume of a device light volume and G-buffer volume
        (rt4_retina_voxelize_device); every *_strides is (row stride, slice stride) in elements."""
        p = params if params is not None else retina_params()
        err = _errbuf()
        _check(self._lib.rt4_retina_voxelize_device(
            self._h, c_void_p(light_ptr or None), light_strides[0], light_strides[1], c_void_p(gbuf_ptr or None),
            gbuf_strides[0], gbuf_strides[1], k, byref(p), c_void_p(vox_ptr or None), vox_strides[0], vox_strides[1], w, h, d,
            c_void_p(stream or None), err, len(err)), err)

    def retina_voxelize_host(self, light, gbuf, k: float, params: RetinaParams | None = None, out=None, w: int | None = None,
                             h: int | None = None):
        """Synchronous: light (d, rows, stride) of LIGHT_DTYPE and gbuf (d, rows, stride) of GBUFFER_DTYPE into `out`
        (d, rows, stride, 4) float32 (a new array if None). w, h: the slice size when rows or slices are padded."""
        import numpy as np

        assert light.dtype == LIGHT_DTYPE and gbuf.dtype == GBUFFER_DTYPE and light.ndim == 3 and gbuf.ndim == 3
        d = light.shape[0]
        h = light.shape[1] if h is None else h
        w = light.shape[2] if w is None else w
        if out is None:
            out = np.zeros((d, h, w, 4), np.float32)
        for a in (light, gbuf, out):
            assert a.flags["C_CONTIGUOUS"] and a.shape[0] == d
        assert out.dtype == np.float32 and out.ndim == 4 and out.shape[3] == 4
        p = params if params is not None else retina_params()
        err = _errbuf()
        _check(self._lib.rt4_retina_voxelize_host(
            self._h, c_void_p(light.ctypes.data), light.shape[2], light.shape[1] * light.shape[2], c_void_p(gbuf.ctypes.data),
            gbuf.shape[2], gbuf.shape[1] * gbuf.shape[2], k, byref(p), c_void_p(out.ctypes.data), out.shape[2],
            out.shape[1] * out.shape[2], w, h, d, err, len(err)), err)
        return out

    def retina_project_device(self, vox_ptr: int, vox_strides, w: int, h: int, d: int, view: RetinaView,
                              params: RetinaParams | None, frame_ptr: int, fmt: int, frame_stride: int, ow: int, oh: int,
                              stream: int = 0) -> None:
        """Asynchronous: the ow x oh picture of `view` in `fmt` from a device voxel volume (rt4_retina_project_device)."""
        p = params if params is not None else retina_params()
        err = _errbuf()
        _check(self._lib.rt4_retina_project_device(
            self._h, c_void_p(vox_ptr or None), vox_strides[0], vox_strides[1], w, h, d,
            byref(view) if view is not None else None, byref(p), c_void_p(frame_ptr or None), fmt, frame_stride, ow, oh,
            c_void_p(stream or None), err, len(err)), err)

    def retina_project_host(self, voxels, view: RetinaView, ow: int, oh: int, params: RetinaParams | None = None,
                            fmt: int = FRAME_RGBA32F, out=None, w: int | None = None, h: int | None = None):
        """Synchronous: voxels (d, rows, stride, 4) float32 into `out` (oh, stride >= ow, 4) of the format's dtype (a new
        array if None). w, h: the slice size when rows or slices are padded."""
        import numpy as np

        assert voxels.dtype == np.float32 and voxels.ndim == 4 and voxels.shape[3] == 4 and voxels.flags["C_CONTIGUOUS"]
        d = voxels.shape[0]
        h = voxels.shape[1] if h is None else h
        w = voxels.shape[2] if w is None else w
        if out is None:
            out = np.zeros((oh, ow, 4), FRAME_NUMPY[fmt])
        assert out.dtype == np.dtype(FRAME_NUMPY[fmt]) and out.flags["C_CONTIGUOUS"] and out.shape[0] == oh
        p = params if params is not None else retina_params()
        err = _errbuf()
        _check(self._lib.rt4_retina_project_host(
            self._h, c_void_p(voxels.ctypes.data), voxels.shape[2], voxels.shape[1] * voxels.shape[2], w, h, d, byref(view),
            byref(p), c_void_p(out.ctypes.data), fmt, out.shape[1], ow, oh, err, len(err)), err)
        return out

    @property
    def kernel_shape(self) -> int:
        """Shape code of the trace kernel the scene runs on (rt4.h rt4_context_kernel_shape)."""
        return self._lib.rt4_context_kernel_shape(self._h)

    def debug_eval(self, fn: int, x):
        import numpy as np

        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        aux = np.empty(x.shape, np.int32)
        err = _errbuf()
        _check(self._lib.rt4_debug_eval(self._h, fn, c_void_p(x.ctypes.data), c_void_p(out.ctypes.data),
                                  c_void_p(aux.ctypes.data), x.size, err, len(err)), err)
        return out, aux

    def debug_verify_sqrt(self) -> int:
        """Mismatches of the kernel's sqrt against IEEE sqrt over all 2^32 inputs (rt4.h)."""
        n = c_uint64(0)
        err = _errbuf()
        _check(self._lib.rt4_debug_verify_sqrt(self._h, ctypes.byref(n), err, len(err)), err)
        return n.value

    def evaluated(self, reset: bool = True) -> int:
        """find_intersection calls evaluated by RT4_FLAG_PRIMARY_REUSE launches since the last reset."""
        n = c_uint64(0)
        err = _errbuf()
        _check(self._lib.rt4_context_evaluated(self._h, ctypes.byref(n), 1 if reset else 0, err, len(err)), err)
        return n.value

    def debug_verify_div(self, b: float, full: bool = False) -> int:
        """Mismatches of the verified-divisor quotient x / b (reduced sweep, or all 2^32 numerators)."""
        n = c_uint64(0)
        err = _errbuf()
        _check(self._lib.rt4_debug_verify_div(self._h, b, 1 if full else 0, ctypes.byref(n), err, len(err)), err)
        return n.value

    def debug_sky_threshold(self, ang: float, full: bool = False) -> float:
        """Smallest float c with acos(c) < ang in the kernel's acos (NaN: none)."""
        c = c_float(0.0)
        err = _errbuf()
        _check(self._lib.rt4_debug_sky_threshold(self._h, ang, 1 if full else 0, ctypes.byref(c), err, len(err)), err)
        return c.value

    def debug_find_intersection(self, rays):
        import numpy as np

        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        out = np.empty((rays.shape[0], 8), np.float32)
        col = np.empty((rays.shape[0], 3), np.float32)
        err = _errbuf()
        _check(self._lib.rt4_debug_find_intersection(self._h, c_void_p(rays.ctypes.data), c_void_p(out.ctypes.data),
                                               c_void_p(col.ctypes.data), rays.shape[0], err, len(err)), err)
        return out, col

    def debug_final_light(self, drct):
        """final_light of the trace kernels for directions (n, 4), as they are (rt4_debug_final_light): (n, 3)."""
        import numpy as np

        drct = np.ascontiguousarray(drct, dtype=np.float32).reshape(-1, 4)
        out = np.empty((drct.shape[0], 3), np.float32)
        err = _errbuf()
        _check(self._lib.rt4_debug_final_light(self._h, c_void_p(drct.ctypes.data), c_void_p(out.ctypes.data),
                                               drct.shape[0], err, len(err)), err)
        return out

    def debug_bound_skip(self, rays):
        """The trace kernels' bounding-ball decisions for rays (n, 8) (rt4_debug_bound_skip): (n,) uint32, bit 0 the
        union's skip, bit 1 the tiger's, bit 2 the hypercube's far flag, bits 8-15 its rejected cells."""
        import numpy as np

        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        out = np.empty(rays.shape[0], np.uint32)
        err = _errbuf()
        _check(self._lib.rt4_debug_bound_skip(self._h, c_void_p(rays.ctypes.data), c_void_p(out.ctypes.data),
                                              rays.shape[0], err, len(err)), err)
        return out

    def debug_cull(self, rays):
        """The trace kernels' sphere-cull decisions for rays (n, 8) (rt4_debug_cull): (n, 2) uint32, word 0 bit i
        sphere i not pending after the cull pass, word 1 bit i cylinder i culled, bit 16 + 2u + c union u's
        cylinder c culled."""
        import numpy as np

        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        out = np.empty((rays.shape[0], 2), np.uint32)
        err = _errbuf()
        _check(self._lib.rt4_debug_cull(self._h, c_void_p(rays.ctypes.data), c_void_p(out.ctypes.data),
                                        rays.shape[0], err, len(err)), err)
        return out


class Temporal:
    """rt4_temporal: a progressive image that survives camera moves. Every frame() renders one sample frame and
    blends it per pixel; when the pose changed, the image and its per-pixel frame counts are first reprojected into
    the new view (rt4.h rt4_temporal_frame_device). Close it before its Tracer. After Tracer.set_scene call reset()."""

    def __init__(self, tracer: Tracer, w: int, h: int, fmt: int = FRAME_RGBA32F):
        self._lib = tracer._lib
        self._tracer = tracer  # keeps the context alive
        self.w, self.h, self.fmt = w, h, fmt
        t = c_void_p()
        err = _errbuf()
        _check(self._lib.rt4_temporal_create(tracer._h, w, h, fmt, byref(t), err, len(err)), err)
        self._t = t

    def close(self):
        if getattr(self, "_t", None):
            if getattr(self._tracer, "_h", None):  # a closed Tracer took the device buffers' context with it
                self._lib.rt4_temporal_destroy(self._t)
            self._t = None

    __del__ = close

    def reset(self) -> None:
        self._lib.rt4_temporal_reset(self._t)

    def frame(self, u: Uniforms, params: ReprojectParams | None = None, counter_ptr: int = 0, stream: int = 0) -> None:
        """Asynchronous: one frame of `u` (u.part is ignored)."""
        err = _errbuf()
        _check(self._lib.rt4_temporal_frame_device(self._t, byref(u), byref(params) if params is not None else None,
                                                   c_void_p(counter_ptr or None), c_void_p(stream or None), err, len(err)), err)

    # device pointers (row stride w); they change with every frame()
    def image_ptr(self) -> int:
        return int(self._lib.rt4_temporal_image(self._t) or 0)

    def history_ptr(self) -> int:
        return int(self._lib.rt4_temporal_history(self._t) or 0)

    def gbuffer_ptr(self) -> int:
        return int(self._lib.rt4_temporal_gbuffer(self._t) or 0)

    def bytes(self) -> int:
        return int(self._lib.rt4_temporal_bytes(self._t))

    def _read(self, which: int):
        import numpy as np

        out = [np.zeros((self.h, self.w, 4), FRAME_NUMPY[self.fmt]), np.zeros((self.h, self.w), np.int32),
               np.zeros((self.h, self.w), GBUFFER_DTYPE)][which]
        ptrs = [None, None, None]
        ptrs[which] = c_void_p(out.ctypes.data)
        err = _errbuf()
        _check(self._lib.rt4_temporal_read_host(self._t, ptrs[0], ptrs[1], ptrs[2], err, len(err)), err)
        return out

    def image(self):
        """Synchronous: the current image on the host, (h, w, 4) of the format's dtype."""
        return self._read(0)

    def history(self):
        """Synchronous: the frames blended into every pixel, (h, w) int32."""
        return self._read(1)

    def gbuffer(self):
        """Synchronous: the G-buffer of the last frame's pose, (h, w) of GBUFFER_DTYPE."""
        return self._read(2)


class Window:
    """rt4_window: cell frames presented at window resolution (cells * scale). present() upscales a device cell frame
    into the owned window image; the G-buffers it needs are rendered only when the pose changed (rt4.h
    rt4_window_present_device). Close it before its Tracer. After Tracer.set_scene call reset()."""

    def __init__(self, tracer: Tracer, cells_w: int, cells_h: int, scale: int, fmt: int = FRAME_RGBA32F):
        self._lib = tracer._lib
        self._tracer = tracer  # keeps the context alive
        self.cells_w, self.cells_h, self.scale, self.fmt = cells_w, cells_h, scale, fmt
        self.w, self.h = cells_w * scale, cells_h * scale
        t = c_void_p()
        err = _errbuf()
        _check(self._lib.rt4_window_create(tracer._h, cells_w, cells_h, scale, fmt, byref(t), err, len(err)), err)
        self._t = t

    def close(self):
        if getattr(self, "_t", None):
            if getattr(self._tracer, "_h", None):  # a closed Tracer took the device buffers' context with it
                self._lib.rt4_window_destroy(self._t)
            self._t = None

    __del__ = close

    def reset(self) -> None:
        self._lib.rt4_window_reset(self._t)

    def present(self, u_cells: Uniforms, cells_ptr: int, cells_stride: int | None = None, gcells_ptr: int = 0,
                gcells_stride: int | None = None, params: UpscaleParams | None = None, stream: int = 0) -> None:
        """Asynchronous: the device cell frame at cells_ptr (the view u_cells, this window's format) into the window
        image. gcells_ptr: the G-buffer of u_cells when the caller has one (Temporal.gbuffer_ptr()), else 0."""
        err = _errbuf()
        _check(self._lib.rt4_window_present_device(
            self._t, byref(u_cells), c_void_p(cells_ptr or None), self.cells_w if cells_stride is None else cells_stride,
            c_void_p(gcells_ptr or None), self.cells_w if gcells_stride is None else gcells_stride,
            byref(params) if params is not None else None, c_void_p(stream or None), err, len(err)), err)

    # device pointers (row stride w)
    def image_ptr(self) -> int:
        return int(self._lib.rt4_window_image(self._t) or 0)

    def gbuffer_ptr(self) -> int:
        return int(self._lib.rt4_window_gbuffer(self._t) or 0)

    def bytes(self) -> int:
        return int(self._lib.rt4_window_bytes(self._t))

    def image(self):
        """Synchronous: the window image on the host, (h, w, 4) of the format's dtype."""
        import numpy as np

        out = np.zeros((self.h, self.w, 4), FRAME_NUMPY[self.fmt])
        err = _errbuf()
        _check(self._lib.rt4_window_read_host(self._t, c_void_p(out.ctypes.data), None, err, len(err)), err)
        return out

    def gbuffer(self):
        """Synchronous: the window G-buffer of the last guided present's pose, (h, w) of GBUFFER_DTYPE."""
        import numpy as np

        out = np.zeros((self.h, self.w), GBUFFER_DTYPE)
        err = _errbuf()
        _check(self._lib.rt4_window_read_host(self._t, None, c_void_p(out.ctypes.data), err, len(err)), err)
        return out


class Retina:
    """rt4_retina: the 3D retina of a view as w x h x depth volumes. accumulate() folds frames into every slice's light
    accumulator (and renders the G-buffer volume when the view is new); present() voxelizes when it must and projects a
    RetinaView into a device frame, so another view of the same volume costs one projection. Close it before its Tracer.
    After Tracer.set_scene call reset()."""

    def __init__(self, tracer: Tracer, w: int, h: int, depth: int):
        self._lib = tracer._lib
        self._tracer = tracer  # keeps the context alive
        self.w, self.h, self.depth = w, h, depth
        t = c_void_p()
        err = _errbuf()
        _check(self._lib.rt4_retina_create(tracer._h, w, h, depth, byref(t), err, len(err)), err)
        self._t = t

    def close(self):
        if getattr(self, "_t", None):
            if getattr(self._tracer, "_h", None):  # a closed Tracer took the device buffers' context with it
                self._lib.rt4_retina_destroy(self._t)
            self._t = None

    __del__ = close

    def reset(self) -> None:
        self._lib.rt4_retina_reset(self._t)

    def accumulate(self, u: Uniforms, w_drct, depth_size: float, n_frames: int = 1, counter_ptr: int = 0,
                   stream: int = 0) -> None:
        """Asynchronous: n_frames more frames of the view u into every slice (rt4_retina_accumulate_device); another u,
        w_drct or depth_size than the accumulated ones starts over."""
        wd = (c_float * 4)(*w_drct)
        err = _errbuf()
        _check(self._lib.rt4_retina_accumulate_device(self._t, byref(u), wd, depth_size, n_frames, c_void_p(counter_ptr or None),
                                                      c_void_p(stream or None), err, len(err)), err)

    def present(self, view: RetinaView, k: float, frame_ptr: int, fmt: int, ow: int, oh: int, frame_stride: int | None = None,
                params: RetinaParams | None = None, stream: int = 0) -> None:
        """Asynchronous: the ow x oh picture of `view` into the device frame at frame_ptr (rt4_retina_present_device)."""
        err = _errbuf()
        _check(self._lib.rt4_retina_present_device(
            self._t, byref(view), byref(params) if params is not None else None, k, c_void_p(frame_ptr or None), fmt,
            ow if frame_stride is None else frame_stride, ow, oh, c_void_p(stream or None), err, len(err)), err)

    def frames_done(self) -> int:
        return int(self._lib.rt4_retina_frames_done(self._t))

    # device pointers (row stride w, slice stride w * h)
    def light_ptr(self) -> int:
        return int(self._lib.rt4_retina_light(self._t) or 0)

    def gbuffer_ptr(self) -> int:
        return int(self._lib.rt4_retina_gbuffer(self._t) or 0)

    def voxels_ptr(self) -> int:
        return int(self._lib.rt4_retina_voxels(self._t) or 0)

    def bytes(self) -> int:
        return int(self._lib.rt4_retina_bytes(self._t))

    def _read(self, which: int):
        import numpy as np

        shape = (self.depth, self.h, self.w)
        out = np.zeros(shape + (4,), np.float32) if which == 2 else np.zeros(shape, (LIGHT_DTYPE, GBUFFER_DTYPE)[which])
        ptrs = [None, None, None]
        ptrs[which] = c_void_p(out.ctypes.data)
        err = _errbuf()
        _check(self._lib.rt4_retina_read_host(self._t, ptrs[0], ptrs[1], ptrs[2], err, len(err)), err)
        return out

    def light(self):
        """Synchronous: the light volume on the host, (depth, h, w) of LIGHT_DTYPE."""
        return self._read(0)

    def gbuffer(self):
        """Synchronous: the G-buffer volume, (depth, h, w) of GBUFFER_DTYPE."""
        return self._read(1)

    def voxels(self):
        """Synchronous: the voxel volume of the last present, (depth, h, w, 4) float32."""
        return self._read(2)
