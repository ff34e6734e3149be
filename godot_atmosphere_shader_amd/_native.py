"""ctypes binding of the C ABI in include/atmo.h (libatmo_hip.so).

There is no CPU fallback: if the library is missing or no gfx950 device is present, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

from .build import LIB_PATH

ATMO_OK, ATMO_E_NAME, ATMO_E_ARG, ATMO_E_STATE, ATMO_E_HIP, ATMO_E_NO_DEVICE = range(6)
VARIANT_NO_CLOUDS, VARIANT_CLOUDS, VARIANT_CLOUDS_HIGH, VARIANT_CLOUDS_HIGH_RM = range(4)
VARIANT_V1_NO_CLOUDS, VARIANT_V1_CLOUDS, VARIANT_V1_CLOUDS_HIGH = 4, 5, 6
LIGHT_LUT, LIGHT_DIRECT = 0, 1
TEX_2D_R32F, TEX_2D_R8, TEX_3D_R8, TEX_CUBE_R8 = range(4)
MEM_HOST, MEM_DEVICE = 0, 1
ABI_VERSION = 5

# every symbol include/atmo.h declares: the surface a host binds (each replaces a reference interface)
CORE_SYMBOLS = (
    "atmo_abi_version", "atmo_device_count", "atmo_create", "atmo_destroy", "atmo_set_param_f32", "atmo_get_param_f32",
    "atmo_set_texture", "atmo_get_texture_size", "atmo_set_sampler_lod", "atmo_bake_optical_depth",
    "atmo_generate_noise_cubemap", "atmo_read_optical_depth", "atmo_render", "atmo_render_composite", "atmo_render_tiles", "atmo_render_tiles_split", "atmo_measure_tile_costs", "atmo_set_precision",
    "atmo_set_host_double_precision", "atmo_set_target_cleared", "atmo_set_tile_feedback", "atmo_last_error_string",
)
# every symbol include/atmo_debug.h declares: experiment knobs and diagnostics (tests, bench.py, tools/)
DEBUG_SYMBOLS = (
    "atmo_set_lane_split", "atmo_debug_motion_px", "atmo_get_feedback_stats", "atmo_set_timing", "atmo_get_timing", "atmo_host_layout_cubemap", "atmo_host_layout_shape",
    "atmo_host_layout_lut", "atmo_host_cubemap_mip", "atmo_read_texture_layout", "atmo_selftest_exact_math", "atmo_debug_marched_optical_depth", "atmo_debug_log2_cr", "atmo_kernel_name", "atmo_build_id",
    "atmo_get_host_wait_stats", "atmo_get_split_stats", "atmo_debug_create_host_only", "atmo_debug_frame_constants", "atmo_debug_proxy_launch_rect",
    "atmo_debug_store_target", "atmo_debug_views_layout", "atmo_debug_views_proxy_layout", "atmo_debug_tile_order", "atmo_debug_heavy_tile_count", "atmo_debug_feedback_plan",
    "atmo_debug_decode_depth",
)
# every symbol include/atmo_scene.h declares: drawing several atmospheres into one frame (the far-mode BoxMesh draw)
SCENE_SYMBOLS = ("atmo_render_proxy", "atmo_render_proxy_composite")
# every symbol include/atmo_target.h declares: the same draws into a renderer's colour buffer (RGBA32F, RGBA16F, RGBA8_UNORM / _SRGB, BGRA8_UNORM / _SRGB,
# A2B10G10R10_UNORM, with a row pitch).
# The ABI version stays 5: a host detects the feature by these symbols and atmo_target_pixel_bytes(format) != 0.
TARGET_SYMBOLS = ("atmo_target_pixel_bytes", "atmo_render_target", "atmo_render_proxy_target")
# every symbol include/atmo_views.h declares: several views of one planet in one launch (stereo eyes, split screen, probe faces).  The ABI version stays 5:
# a host detects the feature by the symbol.
VIEWS_SYMBOLS = ("atmo_render_views",)
MAX_VIEWS = 8
# every symbol include/atmo_views_target.h declares: the same batch into packed and pitched colour targets (RGBA16F / RGBA8_UNORM / RGBA32F per view).
# The ABI version stays 5: a host detects the feature by the symbol.
VIEWS_TARGET_SYMBOLS = ("atmo_render_views_target",)
# every symbol include/atmo_views_proxy.h declares: the far-mode (proxy) form of both batches -- several views of one planet's BoxMesh proxy in one launch.
# The ABI version stays 5: a host detects the feature by the symbols.
VIEWS_PROXY_SYMBOLS = ("atmo_render_views_proxy", "atmo_render_views_proxy_target")
# every symbol include/atmo_planets.h declares: a frame's far planets -- several contexts -- in as few launches as blending allows.  The ABI version stays
# 5 and EXPORTED_SYMBOLS stays the union of the seven older headers' tuples (NOTES.md): a host detects the feature by these symbols.
PLANETS_SYMBOLS = ("atmo_render_planets", "atmo_plan_planets")
MAX_PLANET_DRAWS = 64
# every symbol include/atmo_depth.h declares: the target draws with the depth buffer in its own format (D32_SFLOAT, D16_UNORM, X8_D24_UNORM) and row pitch.
# The ABI version stays 5 and the tuple stands beside EXPORTED_SYMBOLS, as PLANETS_SYMBOLS (NOTES.md): a host detects the feature by these symbols and
# atmo_depth_texel_bytes(format) != 0.
DEPTH_SYMBOLS = ("atmo_depth_texel_bytes", "atmo_render_depth_target", "atmo_render_proxy_depth_target", "atmo_render_views_depth_target",
                 "atmo_render_views_proxy_depth_target")
DEPTH_D32_SFLOAT, DEPTH_D16_UNORM, DEPTH_X8_D24_UNORM = range(3)
# every symbol include/atmo_debug_prologue.h declares: the camera-prologue mask of a draw and the constants handed to the cloudless direct-light kernels.
# The ABI version stays 5 and the tuple stands beside EXPORTED_SYMBOLS, as PLANETS_SYMBOLS (NOTES.md).
PROLOGUE_SYMBOLS = ("atmo_debug_prologue_mode", "atmo_debug_prologue_constants")
PROLOGUE_CAMERA, PROLOGUE_POW2_STEPS, PROLOGUE_NO_SPHERE_DEPTH = 1, 2, 4
# every symbol include/atmo_noise_volume.h declares: the cloud shape volume generated on the device (a NoiseTexture3D mirror; noise_volume.py).
# The ABI version stays 5 and the tuple stands beside EXPORTED_SYMBOLS, as PLANETS_SYMBOLS (NOTES.md): a host detects the feature by the symbol.
NOISE_VOLUME_SYMBOLS = ("atmo_generate_noise_volume",)
# every symbol include/atmo_cloud_detail.h declares: the cloud variants with the reference's CLOUDS_ALWAYS_LOW_QUALITY off (the detail fetch, live TIME).
# The ABI version stays 5 and the tuple stands beside EXPORTED_SYMBOLS, as PLANETS_SYMBOLS (NOTES.md): a host detects the feature by these symbols, and
# load() binds them where the library has them (a library without them still loads; PlanetAtmosphere(cloud_detail=True) then raises).
CLOUD_DETAIL_SYMBOLS = ("atmo_set_cloud_detail", "atmo_get_cloud_detail", "atmo_debug_cloud_detail_constants")
# every symbol include/atmo_rays.h declares: caller-supplied rays (origin, direction and distance per ray) shaded as atmosphere_fragment shades a fragment,
# and a frame's camera rays from the library's own prologue.  The ABI version stays 5 and the tuple stands beside EXPORTED_SYMBOLS, as PLANETS_SYMBOLS
# (NOTES.md): a host detects the feature by these symbols, and load() binds them where the library has them (PlanetAtmosphere.shade_rays raises without).
RAYS_SYMBOLS = ("atmo_shade_rays", "atmo_debug_frame_rays")
# every symbol include/atmo_ray_quads.h declares: caller-supplied rays in 2 x 2 quads, shaded under the declared cubemap sampler.  The RAYS_SYMBOLS rule:
# the ABI version stays 5, the tuple stands beside EXPORTED_SYMBOLS, load() binds it where the library has it (PlanetAtmosphere.shade_ray_quads raises without).
RAY_QUADS_SYMBOLS = ("atmo_shade_ray_quads",)
# every symbol include/atmo_ray_order.h declares: the device's coherence order of a ray queue and the ray kernels through an index list.  The RAYS_SYMBOLS
# rule: the ABI version stays 5, the tuple stands beside EXPORTED_SYMBOLS, load() binds it where the library has it (PlanetAtmosphere.ray_order and
# shade_rays(index=...) raise without).
RAY_ORDER_SYMBOLS = ("atmo_ray_order_scratch_bytes", "atmo_ray_order", "atmo_shade_rays_indexed", "atmo_debug_ray_keys", "atmo_debug_sort_ray_keys")
RAY_KEY_BITS = 18   # ATMO_RAY_KEY_BITS
# every symbol include/atmo_ray_list.h declares: index lists built on the device for a queue whose length is a device word, with the sure-miss cull.  The
# RAYS_SYMBOLS rule: the ABI version stays 5, the tuple stands beside EXPORTED_SYMBOLS, load() binds it where the library has it
# (PlanetAtmosphere.ray_list raises without).
RAY_LIST_SYMBOLS = ("atmo_ray_list_scratch_bytes", "atmo_ray_list", "atmo_debug_ray_cull_constants")
RAY_LIST_ORDER, RAY_LIST_CULL, RAY_LIST_END = 1, 2, 0xFFFFFFFF   # ATMO_RAY_LIST_ORDER, ATMO_RAY_LIST_CULL, ATMO_RAY_LIST_END
# every symbol include/atmo_ray_detail.h declares: the ray batches, ray lists and ray quads of a cloud context with cloud detail on.  The RAYS_SYMBOLS
# rule: the ABI version stays 5, the tuple stands beside EXPORTED_SYMBOLS, load() binds it where the library has it (PlanetAtmosphere.shade_rays and
# shade_ray_quads raise without, on a cloud node with cloud_detail on).
RAY_DETAIL_SYMBOLS = ("atmo_shade_rays_detail", "atmo_shade_ray_quads_detail")
# every symbol include/atmo_detail_target.h declares: the depth-source target draw and its view batch for a cloud context with cloud detail on.  The
# RAYS_SYMBOLS rule: the ABI version stays 5, the tuple stands beside EXPORTED_SYMBOLS, load() binds it where the library has it (PlanetAtmosphere's
# target draws raise without, on a cloud node with cloud_detail on).
DETAIL_TARGET_SYMBOLS = ("atmo_render_detail_target", "atmo_render_views_detail_target")
# every symbol include/atmo_lens.h declares: the rays of a lens image formed on the device (panorama, fisheye, octahedral map, cube face; lens.py), row-major
# with the 16 x 4 tile index or in quad order.  The RAYS_SYMBOLS rule: the ABI version stays 5, the tuple stands beside EXPORTED_SYMBOLS, load() binds it
# where the library has it (PlanetAtmosphere.lens_rays and render_lens raise without).
LENS_SYMBOLS = ("atmo_lens_ray_counts", "atmo_lens_rays")
LENS_EQUIRECT, LENS_FISHEYE, LENS_OCTAHEDRAL, LENS_CUBE_FACE = range(4)   # AtmoLensKind
LENS_QUADS = 1                                                            # ATMO_LENS_QUADS
EXPORTED_SYMBOLS = CORE_SYMBOLS + DEBUG_SYMBOLS + SCENE_SYMBOLS + TARGET_SYMBOLS + VIEWS_SYMBOLS + VIEWS_PROXY_SYMBOLS + VIEWS_TARGET_SYMBOLS
TARGET_RGBA32F, TARGET_RGBA16F, TARGET_RGBA8_UNORM = range(3)
TARGET_RGBA8_SRGB, TARGET_BGRA8_UNORM, TARGET_BGRA8_SRGB, TARGET_A2B10G10R10_UNORM = range(16, 20)   # 3 .. 15 and 20 up: unknown formats


class AtmoFrame(C.Structure):
    _fields_ = [
        ("inv_projection_matrix", C.c_float * 16),
        ("inv_view_matrix", C.c_float * 16),
        ("viewport_w", C.c_int32),
        ("viewport_h", C.c_int32),
        ("planet_center_viewspace", C.c_float * 3),
        ("sun_center_viewspace", C.c_float * 3),
        ("time", C.c_float),
        ("x0", C.c_int32),
        ("y0", C.c_int32),
        ("x1", C.c_int32),
        ("y1", C.c_int32),
    ]


class AtmoTarget(C.Structure):
    _fields_ = [
        ("pixels", C.c_void_p),
        ("format", C.c_int32),
        ("row_pitch_bytes", C.c_int32),
    ]


class AtmoView(C.Structure):
    _fields_ = [
        ("frame", AtmoFrame),
        ("depth_dev", C.c_void_p),
        ("rgba_dev", C.c_void_p),
    ]


class AtmoViewTarget(C.Structure):
    _fields_ = [
        ("frame", AtmoFrame),
        ("depth_dev", C.c_void_p),
        ("target", AtmoTarget),
    ]


class AtmoDepth(C.Structure):   # include/atmo_depth.h
    _fields_ = [
        ("texels", C.c_void_p),
        ("format", C.c_int32),
        ("row_pitch_bytes", C.c_int32),
    ]


class AtmoViewDepthTarget(C.Structure):   # include/atmo_depth.h
    _fields_ = [
        ("frame", AtmoFrame),
        ("depth", AtmoDepth),
        ("target", AtmoTarget),
    ]


class AtmoRay(C.Structure):   # include/atmo_rays.h: 32 bytes, what one row of a (n, 8) float32 tensor holds
    _fields_ = [
        ("origin", C.c_float * 3),
        ("tmax", C.c_float),
        ("dir", C.c_float * 3),
        ("reserved", C.c_float),
    ]


class AtmoLens(C.Structure):   # include/atmo_lens.h: 20 words
    _fields_ = [
        ("kind", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("y0", C.c_int32),
        ("y1", C.c_int32),
        ("face", C.c_int32),
        ("fov", C.c_float),
        ("tmax", C.c_float),
        ("origin", C.c_float * 3),
        ("basis", C.c_float * 9),
    ]


class AtmoNoiseVolume(C.Structure):   # include/atmo_noise_volume.h
    _fields_ = [
        ("size", C.c_int32),
        ("seed", C.c_uint32),
        ("frequency", C.c_float),
        ("octaves", C.c_int32),
        ("gain", C.c_float),
        ("offset", C.c_float * 3),
        ("seamless", C.c_int32),
        ("invert", C.c_int32),
        ("normalize", C.c_int32),
    ]


class AtmoPlanetDraw(C.Structure):   # include/atmo_planets.h
    _fields_ = [
        ("ctx", C.c_void_p),
        ("frame", AtmoFrame),
        ("model_matrix", C.c_float * 16),
        ("box_size", C.c_float),
        ("depth_dev", C.c_void_p),
        ("target", AtmoTarget),
    ]


class AtmoFeedbackPlanIn(C.Structure):   # include/atmo_debug.h
    _fields_ = [
        ("fb_period", C.c_uint32), ("moving_period", C.c_uint32), ("reach_scale", C.c_float), ("instream", C.c_int32), ("axis_windows", C.c_int32),
        ("cloud_steps", C.c_int32), ("flags", C.c_int32), ("tile_h", C.c_int32), ("batch", C.c_int32), ("n", C.c_uint32), ("last_record", C.c_uint32),
        ("pending", C.c_int32), ("active", C.c_int32), ("order_born", C.c_uint32), ("order_reach_px", C.c_float), ("is_last_n", C.c_uint32),
        ("motion_px", C.c_float), ("sil_px", C.c_float * 2),
    ]


class AtmoFeedbackPlanOut(C.Structure):   # include/atmo_debug.h
    _fields_ = [
        ("order", C.c_int32), ("record", C.c_int32), ("sort_side", C.c_int32), ("sort_instream", C.c_int32), ("dil_rx", C.c_int32), ("dil_ry", C.c_int32),
        ("reach_px", C.c_float), ("invalidate_active", C.c_int32),
    ]


class AtmoError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libatmo_hip error {code}: {message}")
        self.code = code


_lib = None

_vp, _cp, _ip, _fp, _u32, _sz = C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_uint32, C.c_size_t
_ipp, _upp, _frame = C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(AtmoFrame)
_rays = [_vp, _frame, _vp, _vp, _u32, _u32, _u32]   # ctx, frame, rays_dev, rgba_dev, n, width, first
# THE signatures of the C ABI, one block a header: header -> (its `*_SYMBOLS` tuple, required?, what the missing-symbol message of an optional header adds
# behind the header's name, name -> (restype, argtypes) in the tuple's order).  load() binds from it and holds every block to its tuple: a symbol added
# to a tuple and forgotten here fails the load instead of running with ctypes' default int signature.  A library must export the required headers
# (ATMO_HIP_LIB's A/B rule apart); the optional ones are detected by symbol (each `*_SYMBOLS` comment above says what raises without).
HEADERS = {
    "atmo.h": (CORE_SYMBOLS, True, "", {
        "atmo_abi_version": (_ip, []),
        "atmo_device_count": (_ip, []),
        "atmo_create": (_ip, [_ip, _ip, _ip, _ip, _ip, _ip, C.POINTER(_vp)]),
        "atmo_destroy": (_ip, [_vp]),
        "atmo_set_param_f32": (_ip, [_vp, _cp, _fp, _ip]),
        "atmo_get_param_f32": (_ip, [_vp, _cp, _fp, _ip]),
        "atmo_set_texture": (_ip, [_vp, _cp, _ip, _ip, _ip, _ip, _ip, _vp, _ip, _vp]),
        "atmo_get_texture_size": (_ip, [_vp, _cp, _ipp, _ipp, _ipp, _ipp]),
        "atmo_set_sampler_lod": (_ip, [_vp, _ip]),
        "atmo_bake_optical_depth": (_ip, [_vp, _vp]),
        "atmo_generate_noise_cubemap": (_ip, [_vp, _ip, _u32, C.c_float, _ip, C.c_float, _fp, _ip, _vp, C.POINTER(C.c_double)]),
        "atmo_read_optical_depth": (_ip, [_vp, _vp, _vp, _ip, _vp]),
        "atmo_render": (_ip, [_vp, _frame, _vp, _vp, _vp]),
        "atmo_render_composite": (_ip, [_vp, _frame, _vp, _vp, _vp]),
        "atmo_render_tiles": (_ip, [_vp, _frame, _vp, _vp, _vp, _ip, _vp]),
        "atmo_render_tiles_split": (_ip, [_vp, _frame, _vp, _vp, _vp, _ip, _ip, _vp]),
        "atmo_measure_tile_costs": (_ip, [_vp, _frame, _vp, _vp, _vp, _vp, _ip, _ipp, _ipp, _ipp, _ipp]),
        "atmo_set_precision": (_ip, [_vp, _ip]),
        "atmo_set_host_double_precision": (_ip, [_vp, _ip]),
        "atmo_set_target_cleared": (_ip, [_vp, _ip]),
        "atmo_set_tile_feedback": (_ip, [_vp, _ip]),
        "atmo_last_error_string": (_cp, [_vp]),
    }),
    "atmo_debug.h": (DEBUG_SYMBOLS, True, "", {
        "atmo_set_lane_split": (_ip, [_vp, _ip]),
        "atmo_debug_motion_px": (C.c_float, [_frame, _frame, C.c_float, _ip]),
        "atmo_get_feedback_stats": (_ip, [_vp, _ipp, _upp, _upp, _upp]),
        "atmo_set_timing": (_ip, [_vp, _ip]),
        "atmo_get_timing": (_ip, [_vp, _ipp, C.POINTER(C.c_double)]),
        "atmo_host_layout_cubemap": (_ip, [_vp, _ip, _vp]),
        "atmo_host_layout_shape": (_ip, [_vp, _ip, _vp]),
        "atmo_host_layout_lut": (_ip, [_vp, _ip, _ip, _vp]),
        "atmo_host_cubemap_mip": (_ip, [_vp, _ip, _vp]),
        "atmo_read_texture_layout": (_ip, [_vp, _cp, _vp, _sz, C.POINTER(_sz), _vp]),
        "atmo_selftest_exact_math": (_ip, [_vp, _u32, _u32, C.c_float, C.POINTER(_u32), C.POINTER(_u32)]),
        "atmo_debug_marched_optical_depth": (_ip, [_vp, _ip, _vp, _vp, _ip, _vp]),
        "atmo_debug_log2_cr": (_ip, [_vp, _ip, _vp, _vp]),
        "atmo_kernel_name": (_cp, [_vp]),
        "atmo_build_id": (_cp, []),
        "atmo_get_host_wait_stats": (_ip, [_vp, _upp]),
        "atmo_get_split_stats": (_ip, [_vp, _upp, _upp]),
        "atmo_debug_create_host_only": (_ip, [_ip, _ip, _ip, _ip, _ip, C.POINTER(_vp)]),
        "atmo_debug_frame_constants": (_ip, [_vp, _frame, _ip, _fp, _ip, _ipp]),
        "atmo_debug_proxy_launch_rect": (_ip, [_vp, _frame, _fp, C.c_float, _ipp, _ipp]),
        "atmo_debug_store_target": (_ip, [_vp, _ip, _ip, _vp, _vp, _sz, _vp]),
        "atmo_debug_views_layout": (_ip, [_vp, C.POINTER(AtmoView), _ip, _ipp, _ipp]),
        "atmo_debug_views_proxy_layout": (_ip, [_vp, C.POINTER(AtmoView), _ip, _fp, C.c_float, _ipp, _ipp, _ipp]),
        "atmo_debug_tile_order": (_ip, [_vp, _vp, _ip, _ip, _ip, _ip, _vp, _vp, _vp, _vp, _ipp]),
        "atmo_debug_heavy_tile_count": (_ip, [_vp, _ip, _ip, C.c_float, C.c_float, _ip]),
        "atmo_debug_feedback_plan": (_ip, [C.POINTER(AtmoFeedbackPlanIn), C.POINTER(AtmoFeedbackPlanOut)]),
        "atmo_debug_decode_depth": (_ip, [_ip, _vp, _vp, _sz, _vp]),
    }),
    "atmo_scene.h": (SCENE_SYMBOLS, True, "", {
        "atmo_render_proxy": (_ip, [_vp, _frame, _fp, C.c_float, _vp, _vp, _vp]),
        "atmo_render_proxy_composite": (_ip, [_vp, _frame, _fp, C.c_float, _vp, _vp, _vp]),
    }),
    "atmo_target.h": (TARGET_SYMBOLS, True, "", {
        "atmo_target_pixel_bytes": (_ip, [_ip]),
        "atmo_render_target": (_ip, [_vp, _frame, _vp, C.POINTER(AtmoTarget), _ip, _vp]),
        "atmo_render_proxy_target": (_ip, [_vp, _frame, _fp, C.c_float, _vp, C.POINTER(AtmoTarget), _ip, _vp]),
    }),
    "atmo_views.h": (VIEWS_SYMBOLS, True, "", {
        "atmo_render_views": (_ip, [_vp, C.POINTER(AtmoView), _ip, _ip, _vp]),
    }),
    "atmo_views_target.h": (VIEWS_TARGET_SYMBOLS, True, "", {
        "atmo_render_views_target": (_ip, [_vp, C.POINTER(AtmoViewTarget), _ip, _ip, _vp]),
    }),
    "atmo_views_proxy.h": (VIEWS_PROXY_SYMBOLS, True, "", {
        "atmo_render_views_proxy": (_ip, [_vp, C.POINTER(AtmoView), _ip, _fp, C.c_float, _ip, _vp]),
        "atmo_render_views_proxy_target": (_ip, [_vp, C.POINTER(AtmoViewTarget), _ip, _fp, C.c_float, _ip, _vp]),
    }),
    "atmo_planets.h": (PLANETS_SYMBOLS, True, "", {
        "atmo_render_planets": (_ip, [C.POINTER(AtmoPlanetDraw), _ip, _vp]),
        "atmo_plan_planets": (_ip, [C.POINTER(AtmoPlanetDraw), _ip, _ipp, _ipp]),
    }),
    "atmo_depth.h": (DEPTH_SYMBOLS, True, "", {
        "atmo_depth_texel_bytes": (_ip, [_ip]),
        "atmo_render_depth_target": (_ip, [_vp, _frame, C.POINTER(AtmoDepth), C.POINTER(AtmoTarget), _ip, _vp]),
        "atmo_render_proxy_depth_target": (_ip, [_vp, _frame, _fp, C.c_float, C.POINTER(AtmoDepth), C.POINTER(AtmoTarget), _ip, _vp]),
        "atmo_render_views_depth_target": (_ip, [_vp, C.POINTER(AtmoViewDepthTarget), _ip, _ip, _vp]),
        "atmo_render_views_proxy_depth_target": (_ip, [_vp, C.POINTER(AtmoViewDepthTarget), _ip, _fp, C.c_float, _ip, _vp]),
    }),
    "atmo_debug_prologue.h": (PROLOGUE_SYMBOLS, True, "", {
        "atmo_debug_prologue_mode": (_ip, [_vp, _frame, _upp, _ipp, _ipp]),
        "atmo_debug_prologue_constants": (_ip, [_vp, _frame, _fp, _ip, _ipp]),
    }),
    "atmo_noise_volume.h": (NOISE_VOLUME_SYMBOLS, True, "", {
        "atmo_generate_noise_volume": (_ip, [_vp, C.POINTER(AtmoNoiseVolume), _ip, _vp, _vp]),
    }),
    "atmo_cloud_detail.h": (CLOUD_DETAIL_SYMBOLS, False, "", {
        "atmo_set_cloud_detail": (_ip, [_vp, _ip]),
        "atmo_get_cloud_detail": (_ip, [_vp, _ipp]),
        "atmo_debug_cloud_detail_constants": (_ip, [_vp, _frame, _fp, _ip, _ipp]),
    }),
    "atmo_rays.h": (RAYS_SYMBOLS, False, "", {
        "atmo_shade_rays": (_ip, _rays + [_vp]),
        "atmo_debug_frame_rays": (_ip, [_vp, _frame, _vp, _vp, _vp]),
    }),
    "atmo_ray_quads.h": (RAY_QUADS_SYMBOLS, False, "", {
        "atmo_shade_ray_quads": (_ip, _rays + [_vp]),
    }),
    "atmo_ray_order.h": (RAY_ORDER_SYMBOLS, False, "", {
        "atmo_ray_order_scratch_bytes": (_ip, [_u32, C.POINTER(_sz)]),
        "atmo_ray_order": (_ip, [_vp, _vp, _u32, _vp, _vp, _sz, _vp]),
        "atmo_shade_rays_indexed": (_ip, _rays + [_vp, _u32, _vp]),
        "atmo_debug_ray_keys": (_ip, [_vp, _vp, _u32, _vp, _vp]),
        "atmo_debug_sort_ray_keys": (_ip, [_vp, _vp, _u32, _vp, _vp, _sz, _vp]),
    }),
    "atmo_ray_list.h": (RAY_LIST_SYMBOLS, False, "", {
        "atmo_ray_list_scratch_bytes": (_ip, [_u32, C.POINTER(_sz)]),
        "atmo_ray_list": (_ip, [_vp, _frame, _vp, _vp, _u32, _ip, _vp, _vp, _vp, _vp, _sz, _vp]),
        "atmo_debug_ray_cull_constants": (_ip, [_vp, _frame, _fp, _ip, _ipp]),
    }),
    "atmo_ray_detail.h": (RAY_DETAIL_SYMBOLS, False, ": no cloud detail for rays", {
        "atmo_shade_rays_detail": (_ip, _rays + [_vp, _u32, _vp]),
        "atmo_shade_ray_quads_detail": (_ip, _rays + [_vp]),
    }),
    "atmo_detail_target.h": (DETAIL_TARGET_SYMBOLS, False, ": no cloud detail into targets", {
        "atmo_render_detail_target": (_ip, [_vp, _frame, C.POINTER(AtmoDepth), C.POINTER(AtmoTarget), _ip, _vp]),
        "atmo_render_views_detail_target": (_ip, [_vp, C.POINTER(AtmoViewDepthTarget), _ip, _ip, _vp]),
    }),
    "atmo_lens.h": (LENS_SYMBOLS, False, ": no lens rays", {
        "atmo_lens_ray_counts": (_ip, [C.POINTER(AtmoLens), _u32, C.POINTER(_u32), C.POINTER(_u32)]),
        "atmo_lens_rays": (_ip, [_vp, C.POINTER(AtmoLens), _u32, _vp, _u32, _vp, _vp, _vp]),
    }),
}


def optional_headers() -> dict:
    """The headers whose symbols a library may lack (each `*_SYMBOLS` comment above says what then raises): header -> (its symbols' tuple, what the
    missing-symbol message adds behind the header's name, name -> (restype, argtypes))."""
    return {header: (symbols, suffix, signatures) for header, (symbols, required, suffix, signatures) in HEADERS.items() if not required}


def optional_entry(lib, name: str):
    """An optional header's entry point of `lib`; RuntimeError naming the header where the library lacks it."""
    fn = getattr(lib, name, None)
    if fn is None:
        header, suffix = next((h, sfx) for h, (symbols, sfx, _) in optional_headers().items() if name in symbols)
        raise RuntimeError(f"libatmo_hip.so does not export {name} (include/{header}){suffix}; rebuild it")
    return fn


def load() -> C.CDLL:
    """Load libatmo_hip.so; raises if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the gfx950 HIP extension has not been built "
            "(python -m godot_atmosphere_shader_amd.build). There is no CPU fallback.")
    # PyTorch ships its own HIP runtime; whichever libamdhip64 is loaded first serves the whole process, and
    # loading /opt/rocm's copy (through this library) before torch's leaves the later-initialised side without a
    # device.  torch is this package's plumbing layer, so let it load its runtime first when it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    # ATMO_HIP_LIB names an A/B build (tools/ab_build_commit.sh: possibly an OLDER commit's library): entry points it lacks are skipped
    # (callers of those guard with hasattr) and its ABI version is not held against it.  The in-tree library must match exactly.
    # The optional headers are detected by symbol: bound where present, and a library without them loads all the same.
    ab_build = bool(os.environ.get("ATMO_HIP_LIB"))
    for header, (symbols, required, _, signatures) in HEADERS.items():
        assert tuple(signatures) == symbols, header
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name, None)
            if fn is None:
                if required and not ab_build:
                    raise RuntimeError(f"libatmo_hip.so does not export {name}; rebuild it")
                continue
            fn.restype = res
            fn.argtypes = args
    have = lib.atmo_abi_version()
    if have != ABI_VERSION:
        # An A/B library may be older, but only a version whose AtmoFrame layout and shared entry points are KNOWN to be what this binding
        # declares may be driven with it, and the caller has to name it: ATMO_HIP_LIB_ABI=3 (ABI 3 = round 3: the same AtmoFrame, no
        # atmo_set_target_cleared / atmo_render_tiles, atmo_set_sampler_lod without the -1 mode) or 4 (ABI 4: the same AtmoFrame and atmo.h calls,
        # no atmo_scene.h).  Anything else could corrupt memory silently.
        allowed = {3, 4}
        named = os.environ.get("ATMO_HIP_LIB_ABI", "")
        if not (ab_build and named.isdigit() and int(named) == have and have in allowed):
            raise RuntimeError(f"libatmo_hip.so has ABI version {have}, this binding is written for {ABI_VERSION}; rebuild it"
                               + (f" (an older A/B library needs ATMO_HIP_LIB_ABI={have}; known-compatible: {sorted(allowed)})" if ab_build else ""))
    _lib = lib
    return lib


def check(ctx, code: int) -> None:
    if code != ATMO_OK:
        msg = load().atmo_last_error_string(ctx)
        raise AtmoError(code, msg.decode() if msg else "")
