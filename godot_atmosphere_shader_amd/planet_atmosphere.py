"""Host-side mirror of the reference's `PlanetAtmosphere` node (addons/zylann.atmosphere/
planet_atmosphere.gd), driving the gfx950 kernels through the C ABI of include/atmo.h.

The reference host is GDScript; Godot is not available here, so the host side is Python with the same
names, argument meaning and (silent) error behaviour:

  reference (planet_atmosphere.gd)                     here
  ---------------------------------------------------  ------------------------------------------
  planet_radius / atmosphere_height (:20-33,230-253)   properties, trigger a LUT re-bake
  sun_path (:36-41)                                    `sun_path`: anything with `.global_position`, or an xyz
  custom_shader (:44-49,118-141)                       `custom_shader`: a `Shader` from `load_shader()`
  clouds_rotation_speed, force_fullscreen (:52-54)     same
  set/get_shader_parameter (:175-180)                  same (unknown names are kept and ignored, as Godot does)
  set/get_shader_param (:164-172)                      same, with a DeprecationWarning
  _get/_set "shader_params/<name>" (:200-218)          `get()` / `set()`; u_density triggers a re-bake (:79-81)
  _get_property_list (:185-197)                        `get_property_list()`
  _process (:285-341)                                  `_process(delta, camera, time)`: per-frame uniforms
  (the draw itself: Godot renderer)                    `render(camera, depth, out, rect, stream)`
  far mode's BoxMesh (:1-3,56-58,98-101,300-321)       `render_proxy*`, `proxy_box_size`; `draw` = the current mode's draw
  (several nodes in one frame: Godot renderer)         `draw_atmospheres(nodes, camera, depth, scene_rgba)`: back to front
  (the same, far nodes batched: include/atmo_planets.h) `draw_atmospheres_batched(...)`, `render_planets(draws)`
  (the renderer's own depth buffer: include/atmo_depth.h) `depth_source(tensor)` in place of any draw's `depth`

The fragment work runs only on the GPU: `render` raises if libatmo_hip.so or a gfx950 device is missing.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import operator
import time as _time
import warnings

import numpy as np

from . import _native as N
from .scene import col_major, srgb_to_linear

MODE_NEAR = 0
MODE_FAR = 1
SWITCH_MARGIN_RATIO = 1.1

_SHADER_DIR = "res://addons/zylann.atmosphere/shaders/"

# uniforms each shader variant declares (used by get_property_list and by the baker's "does it use the LUT" test)
_V2_UNIFORMS = [
    "u_planet_radius", "u_atmosphere_height", "u_sun_position", "u_density", "u_optical_depth_texture",
    "u_scattering_strength", "u_scattering_wavelengths", "u_atmosphere_modulate", "u_atmosphere_ambient_color",
    "u_clip_mode", "u_sphere_depth_factor", "u_blue_noise_texture",
]
_V1_UNIFORMS = [
    "u_planet_radius", "u_atmosphere_height", "u_sun_position", "u_density", "u_day_color0", "u_day_color1",
    "u_night_color0", "u_night_color1", "u_day_night_transition_scale", "u_clip_mode", "u_sphere_depth_factor",
    "u_blue_noise_texture",
]
_CLOUD_UNIFORMS = [
    "u_cloud_density_scale", "u_cloud_bottom", "u_cloud_top", "u_cloud_blend", "u_world_to_model_matrix",
    "u_cloud_shape_texture", "u_cloud_shape_invert", "u_cloud_coverage_bias", "u_cloud_shape_factor",
    "u_cloud_shape_scale", "u_cloud_coverage_cubemap", "u_cloud_coverage_rotation",
]

# GDShader defaults
SHADER_DEFAULTS = {
    "u_planet_radius": 1.0, "u_atmosphere_height": 0.1, "u_sun_position": (0.0, 0.0, 0.0), "u_density": 0.2,
    "u_scattering_strength": 20.0, "u_scattering_wavelengths": (700.0, 530.0, 440.0),
    "u_atmosphere_modulate": (1.0, 1.0, 1.0), "u_atmosphere_ambient_color": (0.0, 0.0, 0.002),
    "u_clip_mode": False, "u_sphere_depth_factor": 0.0, "u_cloud_density_scale": 50.0, "u_cloud_bottom": 0.2,
    "u_cloud_top": 0.5, "u_cloud_blend": 0.5, "u_cloud_shape_invert": 0.0, "u_cloud_coverage_bias": 0.0,
    "u_cloud_shape_factor": 0.8, "u_cloud_shape_scale": 1.0,
    # `source_color` uniforms hold the sRGB values written in the shader / shown by the inspector; `_forward` applies
    # the engine's sRGB -> linear conversion on upload (atmosphere_funcs_v2.gdshaderinc:10-11, _v1.gdshaderinc:8-12)
    "u_day_color0": (0.5, 0.8, 1.0, 1.0), "u_day_color1": (0.5, 0.8, 1.0, 1.0),
    "u_night_color0": (0.2, 0.4, 0.8, 1.0), "u_night_color1": (0.2, 0.4, 0.8, 1.0),
    "u_day_night_transition_scale": 2.0,
}

_FLOAT_COUNTS = {
    "u_planet_radius": 1, "u_atmosphere_height": 1, "u_sun_position": 3, "u_density": 1, "u_scattering_strength": 1,
    "u_scattering_wavelengths": 3, "u_atmosphere_modulate": 3, "u_atmosphere_ambient_color": 3, "u_clip_mode": 1,
    "u_sphere_depth_factor": 1, "u_cloud_density_scale": 1, "u_cloud_bottom": 1, "u_cloud_top": 1, "u_cloud_blend": 1,
    "u_world_to_model_matrix": 16, "u_cloud_shape_invert": 1, "u_cloud_coverage_bias": 1, "u_cloud_shape_factor": 1,
    "u_cloud_shape_scale": 1, "u_cloud_coverage_rotation": 4,
    "u_day_color0": 4, "u_day_color1": 4, "u_night_color0": 4, "u_night_color1": 4, "u_day_night_transition_scale": 1,
}
# uniforms declared `source_color`: Godot converts their rgb from sRGB to linear when the material uploads them
_SOURCE_COLOR = frozenset(["u_atmosphere_modulate", "u_atmosphere_ambient_color", "u_day_color0", "u_day_color1",
                           "u_night_color0", "u_night_color1"])


class LinearColor(tuple):
    """A colour value that is ALREADY linear: `set_shader_parameter(name, LinearColor(rgb))` uploads it unchanged
    (the opt-out of the `source_color` conversion, for hosts that keep linear colours)."""

    def __new__(cls, *v):
        if len(v) == 1 and not isinstance(v[0], (int, float)):
            v = tuple(v[0])
        return super().__new__(cls, tuple(float(x) for x in v))


_TEXTURES = {
    "u_optical_depth_texture": N.TEX_2D_R32F, "u_blue_noise_texture": N.TEX_2D_R8,
    "u_cloud_shape_texture": N.TEX_3D_R8, "u_cloud_coverage_cubemap": N.TEX_CUBE_R8,
}


class Shader:
    """Stands for one of the reference's .gdshader variant files: a set of #defines
    (shaders/planet_atmosphere_*.gdshader:4-7)."""

    def __init__(self, name, variant, view_steps, cloud_steps, cloud_light_rm, lite=False):
        self.name = name
        self.variant = variant
        self.lite = lite                      # ATMOSPHERE_LITE
        self.view_steps = view_steps          # ATMOSPHERE_RAYMARCH_STEPS
        self.cloud_steps = cloud_steps        # CLOUDS_MAX_RAYMARCH_STEPS (0: CLOUDS_ENABLED undefined)
        self.cloud_light_rm = cloud_light_rm  # CLOUDS_RAYMARCHED_LIGHTING
        self.resource_path = _SHADER_DIR + name + ".gdshader"

    def get_shader_uniform_list(self):
        names = list(_V1_UNIFORMS if self.lite else _V2_UNIFORMS) + (list(_CLOUD_UNIFORMS) if self.cloud_steps else [])
        return [{"name": n} for n in names]

    def __repr__(self):
        return f"Shader({self.name})"


SHADERS = {
    "planet_atmosphere_no_clouds": Shader("planet_atmosphere_no_clouds", N.VARIANT_NO_CLOUDS, 8, 0, False),
    "planet_atmosphere_clouds": Shader("planet_atmosphere_clouds", N.VARIANT_CLOUDS, 8, 32, False),
    "planet_atmosphere_clouds_high": Shader("planet_atmosphere_clouds_high", N.VARIANT_CLOUDS_HIGH, 8, 64, False),
    "planet_atmosphere_clouds_high_rm": Shader("planet_atmosphere_clouds_high_rm", N.VARIANT_CLOUDS_HIGH_RM, 8, 64, True),
    "planet_atmosphere_v1_no_clouds": Shader("planet_atmosphere_v1_no_clouds", N.VARIANT_V1_NO_CLOUDS, 16, 0, False, lite=True),
    "planet_atmosphere_v1_clouds": Shader("planet_atmosphere_v1_clouds", N.VARIANT_V1_CLOUDS, 16, 32, False, lite=True),
    "planet_atmosphere_v1_clouds_high": Shader("planet_atmosphere_v1_clouds_high", N.VARIANT_V1_CLOUDS_HIGH, 16, 64, False, lite=True),
}
DefaultShader = SHADERS["planet_atmosphere_no_clouds"]  # planet_atmosphere.gd:13-14


def load_shader(path: str) -> Shader:
    """`preload("./shaders/<name>.gdshader")`: accepts a res:// path, a file name or a bare variant name.
    README.md:35 calls the raymarched-lighting variant `..._clouds_high_m`; the file is `..._clouds_high_rm`."""
    name = path.rsplit("/", 1)[-1]
    if name.endswith(".gdshader"):
        name = name[: -len(".gdshader")]
    if name == "planet_atmosphere_clouds_high_m":
        name = "planet_atmosphere_clouds_high_rm"
    if name not in SHADERS:
        raise FileNotFoundError(path)
    return SHADERS[name]


class Transform2D:
    """Just enough of Godot's Transform2D for u_cloud_coverage_rotation (planet_atmosphere.gd:340-341)."""

    def __init__(self, x=(1.0, 0.0), y=(0.0, 1.0)):
        self.x, self.y = tuple(x), tuple(y)  # basis columns

    def rotated(self, angle: float) -> "Transform2D":
        c, s = math.cos(angle), math.sin(angle)
        return Transform2D((c, s), (-s, c))

    def as_mat2_col_major(self):
        return np.array([self.x[0], self.x[1], self.y[0], self.y[1]], dtype=np.float32)


def _mat4_vec4_f32(m: np.ndarray, v) -> np.ndarray:
    """fp32 mat4*vec4 summed left to right (what the vertex stage computes)."""
    m = np.asarray(m, dtype=np.float32)
    v = [np.float32(x) for x in v]
    out = np.empty(4, dtype=np.float32)
    for r in range(4):
        out[r] = ((m[r, 0] * v[0] + m[r, 1] * v[1]) + m[r, 2] * v[2]) + m[r, 3] * v[3]
    return out


def atmosphere_vertex(view_matrix, model_matrix, sun_position):
    """The per-draw constants of atmosphere_vertex (shaders/include/planet_atmosphere_main.gdshaderinc:101-103):
    (v_planet_center_viewspace, v_sun_center_viewspace), fp32."""
    world_pos = _mat4_vec4_f32(model_matrix, (0.0, 0.0, 0.0, 1.0))
    planet = _mat4_vec4_f32(view_matrix, world_pos)[:3]
    sun = _mat4_vec4_f32(view_matrix, (sun_position[0], sun_position[1], sun_position[2], 1.0))[:3]
    return planet.copy(), sun.copy()


def make_frame(camera, model_matrix, sun_position, time=0.0, rect=None) -> dict:
    """Frame description shared by the product binding and the test oracle: plain dict of numpy values."""
    planet, sun = atmosphere_vertex(camera.view, model_matrix, sun_position)
    w, h = camera.width, camera.height
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, w, h)
    return dict(
        inv_projection_matrix=col_major(camera.inv_projection), inv_view_matrix=col_major(camera.inv_view),
        viewport_w=w, viewport_h=h, planet_center_viewspace=planet, sun_center_viewspace=sun, time=float(time),
        rect=(int(x0), int(y0), int(x1), int(y1)),
    )


def _to_native_frame(frame: dict) -> N.AtmoFrame:
    f = N.AtmoFrame()
    f.inv_projection_matrix[:] = [float(x) for x in frame["inv_projection_matrix"]]
    f.inv_view_matrix[:] = [float(x) for x in frame["inv_view_matrix"]]
    f.viewport_w, f.viewport_h = int(frame["viewport_w"]), int(frame["viewport_h"])
    f.planet_center_viewspace[:] = [float(x) for x in frame["planet_center_viewspace"]]
    f.sun_center_viewspace[:] = [float(x) for x in frame["sun_center_viewspace"]]
    f.time = float(frame.get("time", 0.0))
    f.x0, f.y0, f.x1, f.y1 = frame.get("rect", (0, 0, f.viewport_w, f.viewport_h))
    return f


# The C entry point of one draw, by (through the far mode's box proxy?, into an N.AtmoTarget -- a packed or pitched tensor --?, the depth a
# `depth_source` -- an N.AtmoDepth --?): (plain, composite).
# The float entry points end (..., depth, rgba, stream), the *_target ones (..., depth, &target, composite, stream), the *_depth_target ones the same with
# &depth (every colour tensor is an N.AtmoTarget there: include/atmo_depth.h has no float4-only form); the proxy ones take (model, box_size) behind the
# frame.  `PlanetAtmosphere._render_one` builds the call from the row; a new entry point is a new row.
_SINGLE_DRAWS = {
    (False, False, False): ("atmo_render", "atmo_render_composite"),
    (False, True, False): ("atmo_render_target", "atmo_render_target"),
    (True, False, False): ("atmo_render_proxy", "atmo_render_proxy_composite"),
    (True, True, False): ("atmo_render_proxy_target", "atmo_render_proxy_target"),
    (False, True, True): ("atmo_render_depth_target", "atmo_render_depth_target"),
    (True, True, True): ("atmo_render_proxy_depth_target", "atmo_render_proxy_depth_target"),
}
# ... and of a view batch, by the same key: all six take (views, n, [model, box_size,] composite, stream) (`PlanetAtmosphere._enqueue_views`)
_BATCH_DRAWS = {
    (False, False, False): "atmo_render_views", (False, True, False): "atmo_render_views_target",
    (True, False, False): "atmo_render_views_proxy", (True, True, False): "atmo_render_views_proxy_target",
    (False, True, True): "atmo_render_views_depth_target", (True, True, True): "atmo_render_views_proxy_depth_target",
}
# The C entry point of a batch of caller-supplied rays, by (in 2 x 2 quads?, with cloud detail -- `_serves_cloud_detail` --?, through an index list?).
# All take (ctx, &frame, rays, rgba, n or n_quads, width, first or first_quad, [index, n_index,] stream); the quads have no indexed form.  Cloud detail
# has ONE entry point for rays, plain and indexed: atmo_shade_rays_detail takes (None, 0) for the whole batch (`_WHOLE_BATCH`).
# `PlanetAtmosphere._shade_batch` builds the call from the row; a new entry point is a new row.
_RAY_ENTRIES = {
    (False, False, False): "atmo_shade_rays", (False, False, True): "atmo_shade_rays_indexed",
    (False, True, False): "atmo_shade_rays_detail", (False, True, True): "atmo_shade_rays_detail",
    (True, False, False): "atmo_shade_ray_quads", (True, True, False): "atmo_shade_ray_quads_detail",
}
_WHOLE_BATCH = {"atmo_shade_rays_detail": (None, 0)}
# ... and what the two public methods call their arguments, by the rows of a unit: (the tensor, the first unit's number, the count of units, `out`'s shape
# as the message states it, the bits of first + count)
_RAY_BATCH_NAMES = {1: ("rays", "first", "n", "(n, 4)", 32), 4: ("quads", "first_quad", "n_quads", "(4 * n_quads, 4)", 30)}


class DepthSource:
    """A depth buffer in its own format and row pitch (include/atmo_depth.h), as `depth_source` returns it: `tensor`, `format` (the AtmoDepthFormat
    value) and `pitch_bytes`.  Every draw method that takes `depth` takes one in its place."""

    __slots__ = ("tensor", "format", "pitch_bytes")

    def __init__(self, tensor, format, pitch_bytes):
        self.tensor, self.format, self.pitch_bytes = tensor, format, pitch_bytes

    @property
    def device(self):
        return self.tensor.device

    def native(self, camera, prefix: str = "") -> N.AtmoDepth:
        """The N.AtmoDepth of this buffer as `camera`'s viewport; ValueError where the shape is not (viewport_h, viewport_w)."""
        if tuple(self.tensor.shape) != (camera.height, camera.width):
            raise ValueError(prefix + "depth must have shape (viewport_h, viewport_w)")
        return N.AtmoDepth(self.tensor.data_ptr(), self.format, self.pitch_bytes)


def depth_source(tensor, format=None) -> DepthSource:
    """Wraps a renderer's depth buffer for the draws of include/atmo_depth.h: a CUDA 2-D (viewport_h, viewport_w) tensor whose elements of a row are
    contiguous and whose rows may be further apart than a row (a row pitch: a view of one half of a double-wide image, say).  The dtype says the format:
    float32 is "d32f", int16 (or uint16) "d16", int32 "x8d24" (depth in bits 0-23 of each word, the top byte ignored; depth_formats states the decoding).
    `format` names the format only where it must agree with the dtype; a mismatch raises ValueError."""
    import torch

    from . import depth_formats as D

    fmts = {torch.float32: D.D32F, torch.int16: D.D16, torch.int32: D.X8D24}
    if hasattr(torch, "uint16"):
        fmts[torch.uint16] = D.D16
    if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype in fmts):
        raise TypeError("a depth source must be a CUDA float32 (d32f), int16 / uint16 (d16) or int32 (x8d24) tensor")
    fmt = fmts[tensor.dtype]
    if format is not None and D.format_id(format) != fmt:
        raise ValueError(f"format={format!r} does not agree with the tensor's dtype {tensor.dtype}, which is {D.NAMES[fmt]!r}")
    if tensor.dim() != 2:
        raise ValueError("a depth source must have shape (viewport_h, viewport_w)")
    rows, cols = tensor.shape
    if not ((cols == 1 or tensor.stride(1) == 1) and (rows == 1 or tensor.stride(0) >= cols)):
        raise ValueError("a depth source: the texels of a row must be contiguous and the row stride at least a row (a row pitch is the only stride supported)")
    return DepthSource(tensor, fmt, (tensor.stride(0) if rows > 1 else cols) * tensor.element_size())


class PlanetAtmosphere:
    """See module docstring.  One instance owns one AtmoContext on one GPU."""

    # parameters assigned internally (planet_atmosphere.gd:68-77)
    _api_shader_params = {
        "u_planet_radius": True, "u_atmosphere_height": True, "u_clip_mode": True, "u_sun_position": True,
        "u_world_to_model_matrix": True, "u_blue_noise_texture": True, "u_cloud_coverage_rotation": True,
        "u_optical_depth_texture": True,
    }
    _shader_params_affecting_optical_depth = {"u_density": True}  # planet_atmosphere.gd:79-81

    def __init__(self, device: int = 0, light_mode: str = "lut", light_steps: int = 0,
                 view_steps: int | None = None, cloud_steps: int | None = None, blue_noise=None,
                 precise_clouds: bool = True, precise_atmosphere: bool = False, double_precision: bool = False, lane_split: int = 0,
                 tile_feedback: int = -1, cubemap_lod: bool | None = None, target_cleared: bool = False, cloud_detail: bool = False):
        self._lib = N.load()
        self._device = int(device)
        self._light_mode = {"lut": N.LIGHT_LUT, "direct": N.LIGHT_DIRECT}[light_mode]
        self._light_steps = int(light_steps)
        self._view_steps_override = view_steps    # macro override of ATMOSPHERE_RAYMARCH_STEPS
        self._cloud_steps_override = cloud_steps  # macro override of CLOUDS_MAX_RAYMARCH_STEPS
        self._precise_clouds = bool(precise_clouds)  # atmo_set_precision: bit-faithful cloud density (default); False = fast mode
        self._precise_atmosphere = bool(precise_atmosphere)  # atmo_set_precision 2: the v2 atmosphere march of a no-cloud variant in reference order
        self._double_precision = bool(double_precision)  # `#define DOUBLE_PRECISION` (main:25): engine negates INV_VIEW origin
        self._lane_split = int(lane_split)  # atmo_set_lane_split: 0 auto, 1 / 2 lanes per ray
        self._tile_feedback = int(tile_feedback)  # atmo_set_tile_feedback: -1 default (on), 0 off, 1 on
        self._target_cleared = bool(target_cleared)  # atmo_set_target_cleared: discarded fragments write nothing (the shader's `discard`)
        # atmo_set_cloud_detail: `#define CLOUDS_ALWAYS_LOW_QUALITY` (main:49) commented out -- the detail fetch of the cloud density, moving with `time`
        self._cloud_detail = bool(cloud_detail)
        # atmo_set_sampler_lod: None = as the shader declares the samplerCube (linear-mipmap: implicit LOD from the 2x2 pixel quad when a mip
        # chain is bound), True = the same, required (an error if the draw cannot use it), False = level 0 only
        self._cubemap_lod = None if cubemap_lod is None else bool(cubemap_lod)
        self._ctx = C.c_void_p()
        self._planet_radius = 1.0
        self._atmosphere_height = 0.1
        self._sun_path = None
        self._custom_shader = None
        self._shader = DefaultShader
        self.clouds_rotation_speed = 1.0  # degrees per second
        self.force_fullscreen = False
        self.global_transform = np.eye(4)
        self._mode = MODE_FAR
        self._uses_baked_optical_depth = False
        self._bake_pending = False
        self._params = {}  # the ShaderMaterial's parameter dictionary
        self._start_time = _time.monotonic()
        self._create_context()
        # defaults for the builtin shader (planet_atmosphere.gd:105-108)
        self.set_shader_parameter("u_sun_position", (5000.0, 0.0, 0.0))
        if blue_noise is not None:
            self.set_shader_parameter("u_blue_noise_texture", blue_noise)
        self.set_shader_parameter("u_clip_mode", 0.0)
        # _ready (planet_atmosphere.gd:111-115)
        self.set_shader_parameter("u_planet_radius", self._planet_radius)
        self.set_shader_parameter("u_atmosphere_height", self._atmosphere_height)
        self._sync_bake_flag()

    # ---- context management --------------------------------------------------------------------
    def _create_context(self):
        sh = self._shader
        vs = self._view_steps_override or sh.view_steps
        cs = (self._cloud_steps_override or sh.cloud_steps) if sh.cloud_steps else 0
        ctx = C.c_void_p()
        rc = self._lib.atmo_create(self._device, sh.variant, vs, cs, self._light_mode, self._light_steps, C.byref(ctx))
        N.check(None, rc)
        self._ctx = ctx
        N.check(ctx, self._lib.atmo_set_precision(ctx, 2 if self._precise_atmosphere else (1 if self._precise_clouds else 0)))
        N.check(ctx, self._lib.atmo_set_host_double_precision(ctx, 1 if self._double_precision else 0))
        N.check(ctx, self._lib.atmo_set_lane_split(ctx, self._lane_split))
        N.check(ctx, self._lib.atmo_set_tile_feedback(ctx, self._tile_feedback))
        if self._target_cleared:  # (an A/B library older than round 4 has no such entry point: only asked for when wanted)
            N.check(ctx, self._lib.atmo_set_target_cleared(ctx, 1))
        N.check(ctx, self._lib.atmo_set_sampler_lod(ctx, -1 if self._cubemap_lod is None else (1 if self._cubemap_lod else 0)))
        if self._cloud_detail:  # (only asked for when wanted: a library without include/atmo_cloud_detail.h draws everything else)
            self._set_cloud_detail(True)

    def _set_cloud_detail(self, on: bool):
        if not hasattr(self._lib, "atmo_set_cloud_detail"):
            raise RuntimeError("this libatmo_hip.so has no cloud detail (include/atmo_cloud_detail.h); rebuild it")
        N.check(self._ctx, self._lib.atmo_set_cloud_detail(self._ctx, 1 if on else 0))

    @property
    def cloud_detail(self) -> bool:
        """The cloud variants with the reference's CLOUDS_ALWAYS_LOW_QUALITY off (include/atmo_cloud_detail.h): render / render_composite draw the detail
        fetch, which moves with `time`, and so do shade_rays (plain or through an index list) and shade_ray_quads (include/atmo_ray_detail.h), and -- into
        packed or pitched colour tensors, or from a `depth_source(...)` -- render, render_composite, draw and the target forms of render_views / draw_views
        (atmo_render_detail_target, atmo_render_views_detail_target; include/atmo_detail_target.h); every other
        draw of a cloud variant is refused while it is on."""
        return self._cloud_detail

    @cloud_detail.setter
    def cloud_detail(self, on):
        on = bool(on)
        if on != self._cloud_detail:
            self._set_cloud_detail(on)
            self._cloud_detail = on

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.atmo_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def kernel_name(self) -> str:
        return self._lib.atmo_kernel_name(self._ctx).decode()

    # ---- exported properties -------------------------------------------------------------------
    @property
    def planet_radius(self):
        return self._planet_radius

    @planet_radius.setter
    def planet_radius(self, v):
        self.set_planet_radius(v)

    @property
    def atmosphere_height(self):
        return self._atmosphere_height

    @atmosphere_height.setter
    def atmosphere_height(self, v):
        self.set_atmosphere_height(v)

    @property
    def sun_path(self):
        return self._sun_path

    @sun_path.setter
    def sun_path(self, v):
        self._sun_path = v

    @property
    def custom_shader(self):
        return self._custom_shader

    @custom_shader.setter
    def custom_shader(self, v):
        self.set_custom_shader(v)

    def set_planet_radius(self, new_radius: float):  # planet_atmosphere.gd:230-238
        if self._planet_radius == new_radius:
            return
        self._planet_radius = max(float(new_radius), 0.0)
        self.set_shader_parameter("u_planet_radius", self._planet_radius)
        if self._uses_baked_optical_depth:
            self._request_bake_optical_depth()

    def set_atmosphere_height(self, new_height: float):  # planet_atmosphere.gd:245-253
        if self._atmosphere_height == new_height:
            return
        self._atmosphere_height = max(float(new_height), 0.0)
        self.set_shader_parameter("u_atmosphere_height", self._atmosphere_height)
        if self._uses_baked_optical_depth:
            self._request_bake_optical_depth()

    def set_custom_shader(self, shader):  # planet_atmosphere.gd:118-141
        if isinstance(shader, str):
            shader = load_shader(shader)
        self._custom_shader = shader
        new = DefaultShader if shader is None else shader
        if new is not self._shader:
            self._shader = new
            self.close()
            self._create_context()
            for k, v in list(self._params.items()):  # the material keeps its parameters across shader changes
                if k == "u_optical_depth_texture" and isinstance(v, str):
                    self._bake_pending = True  # device-baked LUT: re-bake into the new context
                    continue
                self._forward(k, v)
        self._sync_bake_flag()

    def _sync_bake_flag(self):
        uses = any(u["name"] == "u_optical_depth_texture" for u in self._shader.get_shader_uniform_list())
        uses = uses and self._light_mode == N.LIGHT_LUT
        self._uses_baked_optical_depth = uses
        if uses:
            self._request_bake_optical_depth()

    # ---- shader parameters -----------------------------------------------------------------------
    def set_shader_param(self, param_name, value):  # planet_atmosphere.gd:164-166
        warnings.warn("set_shader_param is deprecated, use set_shader_parameter", DeprecationWarning, stacklevel=2)
        self.set_shader_parameter(param_name, value)

    def get_shader_param(self, param_name):  # planet_atmosphere.gd:170-172
        warnings.warn("get_shader_param is deprecated, use get_shader_parameter", DeprecationWarning, stacklevel=2)
        return self.get_shader_parameter(param_name)

    def set_shader_parameter(self, param_name: str, value):  # planet_atmosphere.gd:175-176
        self._params[param_name] = value
        self._forward(param_name, value)

    def get_shader_parameter(self, param_name: str):  # planet_atmosphere.gd:179-180
        return self._params.get(param_name)

    def _forward(self, name: str, value):
        """ShaderMaterial -> RenderingServer uniform upload.  Unknown names are ignored silently (Godot)."""
        if name in _TEXTURES:
            self._upload_texture(name, value)
            return
        n = _FLOAT_COUNTS.get(name)
        if n is None or value is None:
            return
        if isinstance(value, Transform2D):
            arr = value.as_mat2_col_major()
        elif isinstance(value, (bool, int, float, np.floating, np.integer)):
            arr = np.array([float(value)], dtype=np.float32)
        else:
            a = np.asarray(value, dtype=np.float64)
            if a.shape == (4, 4) or a.shape == (2, 2):
                arr = col_major(a)
            else:
                arr = a.reshape(-1).astype(np.float32)
        if arr.size != n:
            raise ValueError(f"{name} takes {n} floats, got {arr.size}")
        if name in _SOURCE_COLOR and not isinstance(value, LinearColor):
            a = np.asarray(arr, dtype=np.float64).copy()
            a[:3] = srgb_to_linear(a[:3])  # alpha (v1 colours) is not converted
            arr = a.astype(np.float32)
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        rc = self._lib.atmo_set_param_f32(self._ctx, name.encode(), arr.ctypes.data_as(C.POINTER(C.c_float)), n)
        N.check(self._ctx, rc)

    def _upload_texture(self, name: str, value):
        kind = _TEXTURES[name]
        if hasattr(value, "bind_to"):  # a NoiseVolume resource: generated straight into this node's context, no host copy of the texels
            if name != "u_cloud_shape_texture":
                raise ValueError(f"{name} does not take a NoiseVolume (u_cloud_shape_texture does)")
            value.bind_to(self)
            return
        if hasattr(value, "get_images"):  # a NoiseCubemap resource
            value = value.get_images()
        if value is None:
            rc = self._lib.atmo_set_texture(self._ctx, name.encode(), kind, 0, 0, 0, 0, None, N.MEM_HOST, None)
            N.check(self._ctx, rc)
            return
        mips = 1
        if name == "u_optical_depth_texture":
            a = np.ascontiguousarray(value, dtype=np.float32)
            h, w = a.shape
            d = 1
        elif name == "u_blue_noise_texture":
            a = np.ascontiguousarray(value, dtype=np.uint8)
            h, w = a.shape
            d = 1
        elif name == "u_cloud_shape_texture":
            a = np.ascontiguousarray(value, dtype=np.uint8)
            d, h, w = a.shape
        else:
            # a cubemap is (6, n, n) = level 0 (its mip chain is generated on the device, as Image.generate_mipmaps
            # does in noise_cubemap.gd:135), or a list of levels [(6, n, n), (6, n/2, n/2), ...] given explicitly
            if isinstance(value, (list, tuple)):
                levels = [np.ascontiguousarray(v, dtype=np.uint8) for v in value]
                d, h, w = levels[0].shape
                mips = len(levels)
                a = np.concatenate([lv.reshape(-1) for lv in levels])
            else:
                a = np.ascontiguousarray(value, dtype=np.uint8)
                d, h, w = a.shape
                mips = 0
        rc = self._lib.atmo_set_texture(self._ctx, name.encode(), kind, w, h, d, mips, a.ctypes.data_as(C.c_void_p), N.MEM_HOST, None)
        N.check(self._ctx, rc)

    # Object.get / Object.set with the "shader_params/<name>" convention (planet_atmosphere.gd:200-218)
    def get(self, key: str):
        if key.startswith("shader_params/"):
            param_name = key[len("shader_params/"):]
            value = self.get_shader_parameter(param_name)
            if value is None:
                value = SHADER_DEFAULTS.get(param_name)
            return value
        return getattr(self, key, None)

    def set(self, key: str, value):
        if key.startswith("shader_params/"):
            param_name = key[len("shader_params/"):]
            self.set_shader_parameter(param_name, value)
            if self._uses_baked_optical_depth and param_name in self._shader_params_affecting_optical_depth:
                self._request_bake_optical_depth()
            return
        setattr(self, key, value)

    def get_property_list(self):  # planet_atmosphere.gd:185-197
        props = []
        for p in self._shader.get_shader_uniform_list():
            if p["name"] in self._api_shader_params:
                continue
            props.append({"name": "shader_params/" + p["name"]})
        return props

    def get_configuration_warnings(self):  # planet_atmosphere.gd:221-227
        if self._sun_path is None:
            return ["The path to the sun is not assigned."]
        return []

    # ---- optical depth bake ----------------------------------------------------------------------
    def _request_bake_optical_depth(self):
        """planet_atmosphere.gd:144-150.  The reference defers the bake by two frames through a SubViewport
        (optical_depth_baker.gd:67-85); here it is one kernel enqueued before the next draw."""
        self._bake_pending = True

    def _bake_if_needed(self, stream=None):
        if self._bake_pending and self._uses_baked_optical_depth:
            rc = self._lib.atmo_bake_optical_depth(self._ctx, C.c_void_p(stream or 0))
            N.check(self._ctx, rc)
            self._params["u_optical_depth_texture"] = "<baked on device>"
        self._bake_pending = False

    def read_optical_depth(self, with_rgba8: bool = False, stream=None):
        """The baked LUT as the reference's baker would hand it to ImageTexture (FORMAT_RF), optionally with the
        RGBA8 packing of optical_depth.gdshader:33-43."""
        self._bake_if_needed(stream)
        w, h = C.c_int(0), C.c_int(0)
        N.check(self._ctx, self._lib.atmo_get_texture_size(self._ctx, b"u_optical_depth_texture", C.byref(w), C.byref(h), None, None))
        lut = np.empty((h.value, w.value), dtype=np.float32)
        rgba8 = np.empty((h.value, w.value, 4), dtype=np.uint8) if with_rgba8 else None
        rc = self._lib.atmo_read_optical_depth(
            self._ctx, lut.ctypes.data_as(C.c_void_p),
            rgba8.ctypes.data_as(C.c_void_p) if with_rgba8 else None, w.value * h.value, C.c_void_p(stream or 0))
        N.check(self._ctx, rc)
        return (lut, rgba8) if with_rgba8 else lut

    # ---- per frame -------------------------------------------------------------------------------
    def _sun_position(self):
        s = self._sun_path
        if s is None:
            return None
        if hasattr(s, "global_position"):
            return tuple(float(x) for x in s.global_position)
        return tuple(float(x) for x in s)

    def _set_mode(self, mode: int):  # planet_atmosphere.gd:261-282 (the mesh swap: `draw` picks the quad or the BoxMesh by _mode)
        if mode == self._mode:
            return
        self._mode = mode
        self.set_shader_parameter("u_clip_mode", 1.0 if mode == MODE_NEAR else 0.0)

    def _process(self, delta: float = 0.0, camera=None, time: float | None = None):
        """planet_atmosphere.gd:285-341: near/far switch and the per-frame uniforms."""
        cam_pos = np.zeros(3) if camera is None else np.asarray(camera.inv_view)[:3, 3]
        atmo_clip_distance = self.proxy_box_size(camera)
        d = float(np.linalg.norm(np.asarray(self.global_transform)[:3, 3] - cam_pos))
        self._set_mode(MODE_NEAR if (d < atmo_clip_distance or self.force_fullscreen) else MODE_FAR)

        sun = self._sun_position()
        if sun is not None:
            self.set_shader_parameter("u_sun_position", sun)
        # planet_atmosphere.gd:335 calls Transform3D.inverse(), which assumes an orthonormal basis (transpose + rotated origin); the general
        # inverse used here equals it for every rigid transform and stays a true inverse when the node is scaled (what affine_inverse() gives)
        self.set_shader_parameter("u_world_to_model_matrix", np.linalg.inv(np.asarray(self.global_transform, dtype=np.float64)))
        if time is None:
            time = _time.monotonic() - self._start_time
        self.set_shader_parameter("u_cloud_coverage_rotation",
                                  Transform2D().rotated(time * math.radians(self.clouds_rotation_speed)))

    def make_frame(self, camera, time: float = 0.0, rect=None) -> dict:
        sun = self.get_shader_parameter("u_sun_position")
        if sun is None:
            sun = (0.0, 0.0, 0.0)
        return make_frame(camera, self.global_transform, sun, time, rect)

    def render(self, camera, depth, out=None, rect=None, stream=None, time: float = 0.0, target=None):
        """One draw: shades `rect` (default: whole viewport) of the camera's viewport.

        depth: CUDA float32 tensor (H, W), Godot reversed-Z depth -- or a `depth_source(...)` of the renderer's own D32 / D16 / X8_D24 buffer, with a row
        pitch if it has one (atmo_render_depth_target), here and in every other draw method.  out: CUDA float32 tensor
        (rect_h, rect_w, 4), allocated when None.  Work is enqueued on `stream` (a torch stream, a raw
        hipStream_t int, or None for torch's current stream).  Returns `out`.
        `out` may also be a float16 (RGBA16F) or uint8 (RGBA8_UNORM) tensor, and its rows may be further apart than a row (a row pitch): the draw then
        stores in that format (atmo_render_target; godot_atmosphere_shader_amd.targets states the encoding).  `target` names a packed format
        (`_new_target` lists the names): alone it allocates such a tensor, next to a uint8 `out` it says that its bytes are that format's instead of
        RGBA8_UNORM's (`_colour_target`).  A name that contradicts the tensor's dtype raises ValueError."""
        return self._render_one(camera, depth, out, rect, stream, time, target, False, None, split_depth_errors=True)

    def _render_one(self, camera, depth, colour, rect, stream, time, target, composite, proxy, split_depth_errors=False, reduced=None):
        """The four single draws: `composite` blends into the whole viewport's buffer, else `colour` holds the rect (allocated when None);
        `proxy` is None or `_proxy`'s (model, box_size): zero-filled allocations, the proxy entry points.  `reduced` is None or `render_reduced`'s
        (entry point, what makes its (&options, scratch) of a camera and a device): atmo_render_reduced_target takes the two behind the depth, and a
        depth source and a target structure always."""
        frame = self.make_frame(camera, time, rect)
        x0, y0, x1, y1 = frame["rect"]
        src = depth.native(camera) if isinstance(depth, DepthSource) else None   # (a plain tensor: today's path, checks and messages)
        if src is None:
            _check_depth(depth, camera, split=split_depth_errors)
        rows, cols = (camera.height, camera.width) if composite else (y1 - y0, x1 - x0)
        if colour is None and not composite:
            colour = _new_target(rows, cols, target, depth.device, zero=proxy is not None)
        # a contiguous float32 tensor (None), or the N.AtmoTarget of a float16 / uint8 / pitched one
        tgt = _colour_target(colour, rows, cols, "scene_rgba" if composite else "out", target)
        if (src is not None or reduced is not None) and tgt is None:   # the depth-source entry points take every colour tensor as an N.AtmoTarget
            tgt = N.AtmoTarget(colour.data_ptr(), N.TARGET_RGBA32F, 0)
        # cloud detail into a packed or pitched colour tensor, or from a depth source (include/atmo_detail_target.h): one entry point, which takes both as
        # structures -- a plain depth tensor is a tight D32 source.  Float colour with float depth stays atmo_render; the proxy draws have no detail form.
        # A reduced draw (include/atmo_reduced.h) takes the same two structures, with cloud detail or without: its low draw is atmo_render's
        fn = None
        if reduced is not None:
            fn = reduced[0]
        elif proxy is None and tgt is not None and self._serves_cloud_detail():
            fn = self._entry("atmo_render_detail_target")
        if fn is not None and src is None:
            src = N.AtmoDepth(depth.data_ptr(), N.DEPTH_D32_SFLOAT, 0)
        stream = _stream_handle(stream, depth)
        self._bake_if_needed(stream)
        nf = _to_native_frame(frame)
        if fn is None:
            fn = getattr(self._lib, _SINGLE_DRAWS[proxy is not None, tgt is not None, src is not None][bool(composite)])
        box = () if proxy is None else (proxy[0], C.c_float(proxy[1]))
        where = (C.c_void_p(colour.data_ptr()),) if tgt is None else (C.byref(tgt), int(composite))
        depth_arg = C.c_void_p(depth.data_ptr()) if src is None else C.byref(src)
        extra = () if reduced is None else reduced[1](camera, depth.device)   # (&options, scratch) behind the depth
        N.check(self._ctx, fn(self._ctx, C.byref(nf), *box, depth_arg, *extra, *where, C.c_void_p(stream or 0)))
        return colour

    # ---- reduced-resolution draws (include/atmo_reduced.h) -------------------------------------------------------------------------
    def render_reduced(self, camera, depth, target=None, out=None, *, scale: int = 2, depth_tolerance: float = 0.1, composite: bool = False,
                       scratch=None, stream=None, time: float = 0.0):
        """One draw of the whole viewport at 1 / `scale` (2 or 4) of the resolution along each axis, upsampled into the full-resolution colour buffer by a
        filter that respects depth edges (atmo_render_reduced_target; include/atmo_reduced.h states every step, godot_atmosphere_shader_amd.reduced
        restates it in numpy).  `depth` and `out` / `target` are `render`'s: a float32 depth tensor or a `depth_source(...)`; a float32, float16 or uint8
        (H, W, 4) tensor whose rows may be further apart than a row, `target` naming a packed format.  composite=False: `out` is written whole (allocated
        when None).  composite=True: `out` is the scene colour buffer, blended in place; pixels the atmosphere does not cover keep their bytes.
        `depth_tolerance`: the relative difference of reciprocal eye depth up to which a low-resolution neighbour is averaged into a pixel.
        `scratch`: a contiguous CUDA tensor of at least `reduced.scratch_layout(W, H, scale)[1]` bytes, 16-byte aligned, for the low depth and the low
        frame; None: one is allocated on the first call and kept for the later ones (calls that share it must be ordered on one stream, and a call
        captured into a graph should be given its own: the node's is replaced when a later draw needs a larger one).
        Returns `out`."""
        from . import reduced as R

        if scale not in R.SCALES:
            raise ValueError(f"scale must be 2 or 4, not {scale!r}")
        if composite and out is None:
            raise ValueError("composite=True blends into `out`, the scene colour buffer: it must be given")
        fn = R.bind(self._lib).atmo_render_reduced_target
        opt = R.AtmoReduced(int(scale), float(depth_tolerance))

        def extra(cam, device):
            return C.byref(opt), C.c_void_p(self._reduced_scratch(cam, scale, scratch, device).data_ptr())

        return self._render_one(camera, depth, out, None, stream, time, target, composite, None, split_depth_errors=True, reduced=(fn, extra))

    def _reduced_scratch(self, camera, scale, scratch, device):
        """The scratch tensor of a reduced draw: the caller's, checked, or this node's own, grown when a draw needs more (or another device)."""
        import torch

        from . import reduced as R

        need = R.scratch_layout(camera.width, camera.height, scale)[1]
        if scratch is not None:
            if not (isinstance(scratch, torch.Tensor) and scratch.is_cuda and scratch.is_contiguous()):
                raise TypeError("scratch must be a contiguous CUDA tensor")
            if scratch.numel() * scratch.element_size() < need or scratch.data_ptr() % 16:
                raise ValueError(f"scratch must hold at least {need} bytes (reduced.scratch_layout) and be 16-byte aligned")
            return scratch
        own = getattr(self, "_reduced_scratch_tensor", None)
        if own is None or own.device != torch.device(device) or own.numel() < need:
            own = self._reduced_scratch_tensor = torch.empty(need, dtype=torch.uint8, device=device)
        return own

    # ---- temporal draws (include/atmo_temporal.h) -------------------------------------------------------------------------------------
    def render_temporal(self, camera, depth, target="rgba16f", out=None, *, scale: int = 2, history=None, depth_tolerance: float = 0.1,
                        history_tolerance: float = 0.1, max_age=None, phase=None, reset: bool = False, composite: bool = False, scratch=None,
                        stream=None, time: float = 0.0):
        """One draw of the whole viewport that marches one pixel of every `scale` x `scale` block and takes the others from the last call's result,
        reprojected, or from `render_reduced`'s spatial filter where that history is gone (atmo_render_temporal_target; include/atmo_temporal.h states
        every step, godot_atmosphere_shader_amd.temporal restates it in numpy).  `depth`, `target`, `out`, `composite`, `depth_tolerance`, `scratch`,
        `stream` and `time` are `render_reduced`'s.
        `history`: the `temporal.TemporalHistory` an earlier call returned, or None for a new one.  It owns the two history buffers, the previous camera's
        matrices and the frame index; the call swaps the buffers, and starts over (as with reset=True) when the history is new or was made for another
        viewport, scale or device.  Calls that share a history must be ordered on one stream.
        `history_tolerance`: the relative difference of reciprocal eye depth up to which a reprojected pixel is the same surface.  `max_age`: a history
        pixel is reused while it is younger than this many frames (None: 2 scale^2).  `phase`: None for the Bayer sequence at the history's frame index.
        Returns (`out`, history)."""
        from . import temporal as TP

        if scale not in TP.SCALES:
            raise ValueError(f"scale must be 2 or 4, not {scale!r}")
        if composite and out is None:
            raise ValueError("composite=True blends into `out`, the scene colour buffer: it must be given")
        fn = TP.bind(self._lib).atmo_render_temporal_target
        state = {}

        def extra(cam, device):
            hist = history
            if hist is None or not hist.matches(cam, scale, device):
                hist = TP.TemporalHistory(cam.width, cam.height, scale, device)
            restart = bool(reset) or hist.fresh
            frame = self.make_frame(cam, time)
            opt = TP.options(scale, TP.phase_of_frame(scale, hist.frame_index) if phase is None else phase, depth_tolerance, history_tolerance, max_age,
                             restart, None if restart else TP.prev_clip_from_view(frame, hist.prev_camera),
                             None if restart else hist.prev_camera.inv_projection_cm)
            state["opt"], state["history"] = opt, hist      # (the structure outlives the call)
            return (C.byref(opt), C.c_void_p(self._reduced_scratch(cam, scale, scratch, device).data_ptr()),
                    C.c_void_p(None if restart else hist.previous.data_ptr()), C.c_void_p(hist.current.data_ptr()))

        out = self._render_one(camera, depth, out, None, stream, time, target, composite, None, split_depth_errors=True, reduced=(fn, extra))
        state["history"].advance(camera)
        return out, state["history"]

    # ---- caller-supplied rays (include/atmo_rays.h) --------------------------------------------------------------------------------
    def _entry(self, name: str):
        """An entry point of one of the optional headers (N.optional_headers); RuntimeError naming the header where the library lacks it."""
        return N.optional_entry(self._lib, name)

    def _serves_cloud_detail(self) -> bool:
        """Whether this node's rays and target draws are shaded with cloud detail (include/atmo_ray_detail.h, atmo_detail_target.h): `cloud_detail` on and
        a shader with clouds.  Without, the call goes where it went before (a node without clouds has no density to evaluate)."""
        return bool(getattr(self, "_cloud_detail", False) and getattr(self, "_shader", DefaultShader).cloud_steps)

    def shade_rays(self, rays, camera=None, *, width=None, first: int = 0, out=None, stream=None, time: float = 0.0, index=None):
        """Shades caller-supplied rays: what atmosphere_fragment returns for a fragment with each ray (atmo_shade_rays; include/atmo_rays.h states the
        arithmetic).  `rays`: a contiguous CUDA float32 tensor of shape (n, 8), one N.AtmoRay a row -- origin xyz, tmax (the distance to the first
        opaque hit, FLT_MAX for none), dir xyz (unit length, used as given), one unused float.  `camera` supplies inv_view, the map from ray space
        to world space; None: ray space is world space.  Ray i is image index first + i of an image `width` wide (default: n), which picks its
        blue-noise jitter.  Returns or fills `out`, a contiguous CUDA float32 (n, 4) tensor: ALBEDO.rgb and ALPHA per ray, zeros for a ray that misses
        the atmosphere.  The coverage cubemap is sampled at level 0; with `cloud_detail`, the detail fetch: the clouds are get_density_full's and move
        with `time` (atmo_shade_rays_detail; include/atmo_ray_detail.h), plain or through `index`.
        `index` (a contiguous CUDA int32 (m,) tensor, `ray_order`'s or any list of ray numbers): the rays it names are shaded, 64 consecutive entries a
        wavefront, each to its own row of `out` with the bits the plain call gives it (atmo_shade_rays_indexed; include/atmo_ray_order.h); rows it does
        not name are left as they are -- zeros where `out` is created here."""
        return self._shade_batch(1, rays, camera, width, first, out, stream, time, index)

    def _shade_batch(self, per, rays, camera, width, first, out, stream, time, index=None):
        """`shade_rays` (per = 1: a unit is a ray) and `shade_ray_quads` (per = 4: a unit is a quad): the checks in one order under each method's own
        names, `out` created where it is None -- zeros under an index list, whose unnamed rows are left as they are --, the bake, the `_RAY_ENTRIES` row."""
        what, first_name, units, out_shape, bits = _RAY_BATCH_NAMES[per]
        n = _check_rays(rays, what, 8)
        if n % per:
            raise ValueError("quads must have four rows per quad: shape (4 * n_quads, 8)")
        if index is not None:
            _check_index(index)
        try:
            width, first = max(n, 1) if width is None and per == 1 else operator.index(width), operator.index(first)
        except TypeError:
            raise TypeError(f"width and {first_name} must be integers") from None
        if width < 1 or first < 0 or first + n // per > 1 << bits:
            raise ValueError(f"width must be at least 1, {first_name} at least 0 and {first_name} + {units} at most 2^{bits}")
        if out is None:
            import torch

            out = (torch.empty if index is None else torch.zeros)((n, 4), dtype=torch.float32, device=rays.device)
        elif _check_rays(out, "out", 4) != n:
            raise ValueError(f"out must have one row per ray: shape {out_shape}")
        name = _RAY_ENTRIES[per == 4, self._serves_cloud_detail(), index is not None]
        fn = self._entry(name)
        stream = _stream_handle(stream, rays)
        self._bake_if_needed(stream)
        nf = self._ray_frame(camera, time)
        listed = _WHOLE_BATCH.get(name, ()) if index is None else (C.c_void_p(index.data_ptr()), int(index.shape[0]))
        N.check(self._ctx, fn(self._ctx, C.byref(nf), C.c_void_p(rays.data_ptr()), C.c_void_p(out.data_ptr()), n // per, width, first, *listed,
                              C.c_void_p(stream or 0)))
        return out

    def _ray_frame(self, camera, time: float) -> N.AtmoFrame:
        """The frame of a ray call: `camera` supplies inv_view, the map from ray space to world space; None: ray space is world space."""
        return _to_native_frame(self.make_frame(camera if camera is not None else _WORLD_RAY_SPACE, time))

    def _scratch(self, size_entry: str, count: int):
        """(bytes, int32 words) of the scratch a `*_scratch_bytes` entry point asks for `count` rays: the words fill whole 16-byte units."""
        need = C.c_size_t(0)
        N.check(self._ctx, self._entry(size_entry)(count, C.byref(need)))
        return need.value, (need.value + 15) // 16 * 4

    # ---- coherent ray queues (include/atmo_ray_order.h) ---------------------------------------------------------------------------
    def ray_order(self, rays, stream=None):
        """The coherence order of a ray queue, computed on the device (atmo_ray_order; include/atmo_ray_order.h states the key): a CUDA int32 (n,) tensor,
        the stable ascending sort of the rays' numbers by the octahedral cell of their directions -- godot_atmosphere_shader_amd.ray_order.ray_order is
        the same permutation in numpy.  `rays` as `shade_rays`'; hand the result to `shade_rays(index=...)`.  The scratch comes from torch's allocator."""
        import torch

        n = _check_rays(rays, "rays", 8)
        if n > 1 << 28:
            raise ValueError("at most 2^28 rays")
        order = torch.empty((n,), dtype=torch.int32, device=rays.device)
        if n == 0:
            return order
        fn = self._entry("atmo_ray_order")
        need, words = self._scratch("atmo_ray_order_scratch_bytes", n)
        handle, on_stream = _on_stream(stream, rays.device)
        with on_stream:
            scratch = torch.empty((words,), dtype=torch.int32, device=rays.device)
        N.check(self._ctx, fn(self._ctx, C.c_void_p(rays.data_ptr()), n, C.c_void_p(order.data_ptr()), C.c_void_p(scratch.data_ptr()), need,
                              C.c_void_p(handle or 0)))
        return order

    # ---- ray lists: counted queues and the sure-miss cull (include/atmo_ray_list.h) ------------------------------------------------
    def ray_list(self, rays, count=None, order=True, cull=False, camera=None, out=None, stream=None):
        """An index list for `shade_rays(index=...)` built on the device (atmo_ray_list; include/atmo_ray_list.h): `(index, listed)`, a CUDA int32
        (capacity,) tensor -- the listed rays, then -1 (ATMO_RAY_LIST_END) entries, which the indexed call skips -- and a CUDA int32 (1,) tensor, their
        number.  `rays` as `shade_rays`'; its rows are the queue's CAPACITY.  `count`: a one-element CUDA int32 tensor holding the queue's live length,
        read by the kernels when they run and never by the host (None: every row is live); rows behind it are not looked at.  `order`: the listed rays in
        `ray_order`'s order, else in queue order.  `cull`: rays that surely miss the shell seen through `camera` (None: ray space is world space) are
        left out and their rows of `out` are set to zero -- pass the same `out` to `shade_rays(index=...)`; None: a tensor of zeros, as that call's own
        default is.  The scratch comes from torch's allocator, on the call's stream.  godot_atmosphere_shader_amd.ray_list.ray_list is the same list
        in numpy."""
        import torch

        capacity = _check_rays(rays, "rays", 8)
        if capacity > 1 << 28:
            raise ValueError("at most 2^28 rays")
        if count is not None:
            _check_kind(count, "count must be a contiguous CUDA int32 tensor", "int32")
            if count.numel() != 1:
                raise ValueError("count must have one element")
        flags = (N.RAY_LIST_ORDER if order else 0) | (N.RAY_LIST_CULL if cull else 0)
        if cull and out is not None and _check_rays(out, "out", 4) != capacity:
            raise ValueError("out must have one row per ray: shape (n, 4)")
        if capacity == 0:
            return torch.empty((0,), dtype=torch.int32, device=rays.device), torch.zeros((1,), dtype=torch.int32, device=rays.device)
        fn = self._entry("atmo_ray_list")
        need, words = self._scratch("atmo_ray_list_scratch_bytes", capacity)
        handle, on_stream = _on_stream(stream, rays.device)
        with on_stream:   # what is allocated (and zeroed) here belongs to the call's stream, as the scratch does
            scratch = torch.empty((words,), dtype=torch.int32, device=rays.device)
            index = torch.empty((capacity,), dtype=torch.int32, device=rays.device)
            listed = torch.empty((1,), dtype=torch.int32, device=rays.device)
            if cull and out is None:
                out = torch.zeros((capacity, 4), dtype=torch.float32, device=rays.device)
        nf = self._ray_frame(camera, 0.0) if cull else None
        N.check(self._ctx, fn(self._ctx, C.byref(nf) if cull else None, C.c_void_p(rays.data_ptr()), C.c_void_p(count.data_ptr()) if count is not None else None,
                              capacity, flags, C.c_void_p(out.data_ptr()) if cull else None, C.c_void_p(index.data_ptr()), C.c_void_p(listed.data_ptr()),
                              C.c_void_p(scratch.data_ptr()), need, C.c_void_p(handle or 0)))
        return index, listed

    def camera_rays(self, camera, depth, rect=None, stream=None):
        """The rays the library's own prologue forms for `rect` (default: the whole viewport) of the camera's viewport, row-major: a CUDA float32
        (rect_h * rect_w, 8) tensor for `shade_rays` -- origin 0, the normalised view direction, tmax = the linear depth of the depth sample
        (atmo_debug_frame_rays).  `depth` as `render`'s float tensor."""
        import torch

        _check_depth(depth, camera, split=True)
        frame = self.make_frame(camera, 0.0, rect)
        x0, y0, x1, y1 = frame["rect"]
        rays = torch.empty(((y1 - y0) * (x1 - x0), 8), dtype=torch.float32, device=depth.device)
        fn = self._entry("atmo_debug_frame_rays")
        stream = _stream_handle(stream, depth)
        nf = _to_native_frame(frame)
        N.check(self._ctx, fn(self._ctx, C.byref(nf), C.c_void_p(depth.data_ptr()), C.c_void_p(rays.data_ptr()), C.c_void_p(stream or 0)))
        return rays

    # ---- rays in quads under the declared sampler (include/atmo_ray_quads.h) ------------------------------------------------------
    def shade_ray_quads(self, quads, camera=None, *, width, first_quad: int = 0, out=None, stream=None, time: float = 0.0):
        """Shades caller-supplied rays that arrive in 2 x 2 quads, the coverage cubemap sampled as the declared sampler samples it: each ray differences
        against the two partner rays of its quad (atmo_shade_ray_quads; include/atmo_ray_quads.h states the layout and the arithmetic).  `quads`: a
        contiguous CUDA float32 tensor of shape (4 * n_quads, 8), one N.AtmoRay a row in quad order (ray_quads.quad_order) -- slot 4 q + j is the ray of
        pixel (2 (Q % qpr) + (j & 1), 2 (Q // qpr) + (j >> 1)) with Q = first_quad + q and qpr = (width + 1) // 2; an all-zero direction marks an absent
        ray.  `camera` as in `shade_rays`.  Returns or fills `out`, a contiguous CUDA float32 (4 * n_quads, 4) tensor in the same order (zeros for an
        absent ray and for one that misses the atmosphere); ray_quads.quads_to_image puts a whole image's back into rows.  The declared sampler; with
        `cloud_detail`, the detail fetch as well, moving with `time` (atmo_shade_ray_quads_detail; include/atmo_ray_detail.h)."""
        return self._shade_batch(4, quads, camera, width, first_quad, out, stream, time)

    def camera_ray_quads(self, camera, depth, stream=None):
        """`camera_rays` of the whole viewport gathered into quad order (ray_quads.quad_order) for `shade_ray_quads(width=camera.width)`: a CUDA float32
        (4 * ceil(w / 2) * ceil(h / 2), 8) tensor, all-zero rows (absent rays) for the slots outside the image."""
        import torch

        from .ray_quads import quad_order

        rays = self.camera_rays(camera, depth, stream=stream)
        order = torch.as_tensor(quad_order(camera.width, camera.height), device=rays.device)
        with _on_stream(stream, depth.device)[1]:   # the gather behind the dump, on its stream
            return torch.where((order >= 0).unsqueeze(1), rays[order.clamp(min=0)], torch.zeros((), dtype=rays.dtype, device=rays.device)).contiguous()

    # ---- lens rays: panorama, fisheye, octahedral map, cube face (include/atmo_lens.h) ---------------------------------------------
    def lens_rays(self, lens, distance=None, quads: bool = False, tile_index: bool = False, stream=None):
        """The rays of a lens image, formed on the device (atmo_lens_rays; include/atmo_lens.h states the arithmetic, lens.lens_rays is the same statement
        in numpy): a CUDA float32 (n, 8) tensor for `shade_rays(width=lens.width, first=y0 * lens.width)` -- the rows `lens.rows` of the image, row-major
        -- or, with `quads`, in quad order for `shade_ray_quads(width=lens.width, first_quad=(y0 // 2) * ((lens.width + 1) // 2))`, slots outside the image
        and fisheye pixels outside the circle absent.  `lens`: a lens.Lens.  `distance`: a CUDA float32 (lens.height, >= lens.width) tensor whose rows may
        be further apart, every ray's tmax (default: lens.tmax).  `tile_index` (row-major only): returns `(rays, index)`, index the CUDA int32 tile index
        for `shade_rays(index=...)` -- the image's 16 x 4 tiles one after the other, -1 entries for the absent pixels and the ragged tiles' rest."""
        import torch

        if quads and tile_index:
            raise ValueError("the tile index is row-major only")
        pitch = 0
        if distance is not None:
            _check_kind(distance, "distance must be a CUDA float32 tensor", contiguous=False)
            if distance.dim() != 2 or distance.shape[0] != lens.height or distance.shape[1] < lens.width or distance.stride(1) != 1 or (
                    lens.height > 1 and distance.stride(0) < lens.width):
                raise ValueError("distance must have shape (lens.height, >= lens.width) with contiguous rows")
            pitch = int(distance.stride(0)) if lens.height > 1 else int(distance.shape[1])
        fn, counts = self._entry("atmo_lens_rays"), self._entry("atmo_lens_ray_counts")
        nl, flags = lens.native(), N.LENS_QUADS if quads else 0
        n_rays, n_index = C.c_uint32(0), C.c_uint32(0)
        N.check(self._ctx, counts(C.byref(nl), flags, C.byref(n_rays), C.byref(n_index)))
        device = distance.device if distance is not None else torch.device("cuda", self._device)
        handle, on_stream = _on_stream(stream, device)
        with on_stream:
            rays = torch.empty((n_rays.value, 8), dtype=torch.float32, device=device)
            index = torch.empty((n_index.value,), dtype=torch.int32, device=device) if tile_index else None
        N.check(self._ctx, fn(self._ctx, C.byref(nl), flags, C.c_void_p(distance.data_ptr()) if distance is not None else None, pitch,
                              C.c_void_p(rays.data_ptr()), C.c_void_p(index.data_ptr()) if tile_index else None, C.c_void_p(handle or 0)))
        return (rays, index) if tile_index else rays

    def _shades_ray_quads(self) -> bool:
        """Whether atmo_shade_ray_quads accepts this node (include/atmo_ray_quads.h): a cloud shader, a sampler mode other than 0, a mip chain bound."""
        if not getattr(self, "_shader", DefaultShader).cloud_steps or self._cubemap_lod is False:
            return False
        mips = C.c_int(0)
        N.check(self._ctx, self._lib.atmo_get_texture_size(self._ctx, b"u_cloud_coverage_cubemap", None, None, None, C.byref(mips)))
        return mips.value > 1

    def render_lens(self, lens, camera=None, distance=None, out=None, time: float = 0.0, stream=None, quads=None):
        """Draws the sky through a lens: the rows `lens.rows` of a panorama, a fisheye, an octahedral map or a cube face (lens.Lens), a CUDA float32
        (rows, lens.width, 4) image -- ALBEDO.rgb and ALPHA, zeros where a ray misses the atmosphere and outside a fisheye's circle.  The rays are
        formed on the device (`lens_rays`) and shaded by the ray entry points; `camera` as in `shade_rays` (None: ray space is world space), `distance`
        as in `lens_rays`.  `quads`: None picks the quad order -- the declared cubemap sampler, `shade_ray_quads` -- exactly when this node has one (a
        cloud shader, a sampler mode other than level 0, a mip chain bound); else the rays are row-major and shaded through the tile index, in 16 x 4
        blocks of the image, into a zeroed `out`.  With `cloud_detail` both paths go through the detail entry points.  An image drawn in several bands
        is the one-call image: `first` and `first_quad` carry the jitter."""
        import torch

        from .ray_quads import quads_to_image

        if quads is None:
            quads = self._shades_ray_quads()
        y0, y1 = lens.rows
        rows, w = y1 - y0, lens.width
        if out is not None:
            _check_kind(out, "out must be a contiguous CUDA float32 tensor")
            if tuple(out.shape) != (rows, w, 4):
                raise ValueError(f"out must have shape ({rows}, {w}, 4)")
        if rows == 0:
            return out if out is not None else torch.zeros((0, w, 4), dtype=torch.float32, device=torch.device("cuda", self._device))
        with _on_stream(stream, torch.device("cuda", self._device))[1]:   # the gather and the zeroed image beside the two calls, which enter it again
            _, shaded = self._shade_lens(lens, camera, distance, time, stream, quads, out)
            if quads:
                image = quads_to_image(shaded, w, rows)
                if out is None:
                    return image.contiguous()
                out.copy_(image)
                return out
            return out if out is not None else shaded.view(rows, w, 4)

    def _shade_lens(self, lens, camera, distance, time, stream, quads, image=None):
        """What `render_lens` and `ambient_sh9` share: `(rays, shaded)` of the lens's band in ray order, (n, 8) and (n, 4).  `quads`: the quad order through
        `shade_ray_quads`; else row-major through the tile index into zeros -- into `image` (rows, width, 4) where one is given -- so that the rows of
        absent pixels, which the indexed call leaves alone, are zero.  The band is not empty; the caller has entered the stream."""
        import torch

        y0, y1 = lens.rows
        rows, w = y1 - y0, lens.width
        if quads:
            rays = self.lens_rays(lens, distance=distance, quads=True, stream=stream)
            return rays, self.shade_ray_quads(rays, camera, width=w, first_quad=(y0 // 2) * ((w + 1) // 2), stream=stream, time=time)
        rays, index = self.lens_rays(lens, distance=distance, tile_index=True, stream=stream)
        if image is None:
            image = torch.zeros((rows, w, 4), dtype=torch.float32, device=rays.device)
        else:
            image.zero_()
        shaded = image.view(rows * w, 4)
        self.shade_rays(rays, camera, width=w, first=y0 * w, out=shaded, stream=stream, time=time, index=index)
        return rays, shaded

    # ---- the sky as light: solid angles and the SH9 projection (include/atmo_sky_sh.h) ---------------------------------------------
    def lens_solid_angles(self, lens, quads: bool = False, stream=None):
        """The solid angle, in steradians, of the pixel in every slot of `lens_rays(lens, quads=quads)`, computed on the device (atmo_lens_solid_angles;
        include/atmo_sky_sh.h states the arithmetic, sky_sh.solid_angles is the same statement in numpy): a CUDA float32 (n_rays,) tensor, +0 for an absent
        slot.  The weights `project_sh9` wants beside that lens's rays."""
        import torch

        from . import sky_sh as SH

        fn = SH.bind(self._lib).atmo_lens_solid_angles
        nl, flags = lens.native(), N.LENS_QUADS if quads else 0
        n_rays = C.c_uint32(0)
        N.check(self._ctx, self._entry("atmo_lens_ray_counts")(C.byref(nl), flags, C.byref(n_rays), None))
        device = torch.device("cuda", self._device)
        handle, on_stream = _on_stream(stream, device)
        with on_stream:
            weights = torch.empty((n_rays.value,), dtype=torch.float32, device=device)
        N.check(self._ctx, fn(self._ctx, C.byref(nl), flags, C.c_void_p(weights.data_ptr()), C.c_void_p(handle or 0)))
        return weights

    def project_sh9(self, rays, rgba, weights=None, out=None, accumulate: bool = False, stream=None):
        """Projects shaded rays onto the nine real spherical harmonics of bands 0 to 2, on the device and in one fixed order of summation (atmo_sky_sh9;
        include/atmo_sky_sh.h, sky_sh.sh9_project is the same sums in numpy, bit for bit).  `rays` as `shade_rays`' (their directions are used as given: the
        coefficients live in ray space), `rgba` what a shading call returned for them, `weights` a contiguous CUDA float32 (n,) tensor -- `lens_solid_angles`'
        -- or None: every ray weighs 1.  A ray whose weight is 0 is not read.  Returns or fills `out`, a contiguous CUDA float32 (40,) tensor:
        out[4 k + ch] the coefficient of Y_k in channel ch (rgb premultiplied by alpha, then alpha), out[36] the weights' sum, three zeros.  `accumulate`:
        the sums are added to what `out` holds (six cube faces: six calls, the five behind the first with it).  The scratch comes from torch's allocator,
        on the call's stream."""
        import torch

        from . import sky_sh as SH

        lib = SH.bind(self._lib)
        n = _check_rays(rays, "rays", 8)
        if _check_rays(rgba, "rgba", 4) != n:
            raise ValueError("rgba must have one row per ray: shape (n, 4)")
        if weights is not None:
            _check_kind(weights, "weights must be a contiguous CUDA float32 tensor")
            if tuple(weights.shape) != (n,):
                raise ValueError("weights must have one float per ray: shape (n,)")
        if n > SH.MAX_RAYS:
            raise ValueError("at most 2^28 rays")
        if out is not None:
            _check_kind(out, "out must be a contiguous CUDA float32 tensor")
            if tuple(out.shape) != (SH.FLOATS,):
                raise ValueError(f"out must have shape ({SH.FLOATS},)")
        elif accumulate:
            raise ValueError("accumulate needs the `out` it adds to")
        need = C.c_size_t(0)
        N.check(self._ctx, lib.atmo_sky_sh9_scratch_bytes(n, C.byref(need)))
        handle, on_stream = _on_stream(stream, rays.device)
        with on_stream:
            scratch = torch.empty((max(need.value // 4, 4),), dtype=torch.float32, device=rays.device)
            if out is None:
                out = torch.empty((SH.FLOATS,), dtype=torch.float32, device=rays.device)
        N.check(self._ctx, lib.atmo_sky_sh9(self._ctx, C.c_void_p(rays.data_ptr()), C.c_void_p(rgba.data_ptr()),
                                            C.c_void_p(weights.data_ptr()) if weights is not None else None, n, SH.ACCUMULATE if accumulate else 0,
                                            C.c_void_p(scratch.data_ptr()), need, C.c_void_p(out.data_ptr()), C.c_void_p(handle or 0)))
        return out

    def ambient_sh9(self, lenses, camera=None, time: float = 0.0, stream=None):
        """The sky's light through one lens or several (a lens.Lens or a sequence: an octahedral map, six cube faces) as nine spherical-harmonic
        coefficients per channel: each lens is shaded as `render_lens` shades it -- in quad order under the declared sampler where this node has one, else
        row-major through the tile index; with `cloud_detail` through the detail entry points --, weighed by `lens_solid_angles` and projected by
        `project_sh9` from the ray-ordered arrays, accumulating across the lenses.  `camera` as in `shade_rays`: the coefficients live in ray space.  Returns
        the CUDA float32 (40,) tensor of `project_sh9`; nothing is read back and nothing waits on the host.  sky_sh.sh9_irradiance turns it into the
        irradiance on a surface."""
        import torch

        from . import sky_sh as SH
        from .lens import Lens

        lenses = [lenses] if isinstance(lenses, Lens) else list(lenses)
        device = torch.device("cuda", self._device)
        quads = self._shades_ray_quads()
        with _on_stream(stream, device)[1]:
            out = None
            for lens in lenses:
                if lens.rows[0] == lens.rows[1]:
                    continue
                rays, shaded = self._shade_lens(lens, camera, None, time, stream, quads)
                out = self.project_sh9(rays, shaded, self.lens_solid_angles(lens, quads=quads, stream=stream), out=out, accumulate=out is not None,
                                       stream=stream)
            return out if out is not None else torch.zeros((SH.FLOATS,), dtype=torch.float32, device=device)

    # ---- the sky as an image: the resolve into a target and its mip chain (include/atmo_sky_image.h) -------------------------------
    def resolve_lens(self, lens, rgba, out, *, target=None, quads: bool = False, premultiplied: bool = False, composite: bool = False, stream=None):
        """Resolves what a shading call returned for `lens_rays(lens, quads=quads)` -- `rgba`, a contiguous CUDA float32 (n_rays, 4) tensor in ray order --
        into the rows `lens.rows` of the image `out` (atmo_sky_image_resolve; include/atmo_sky_image.h states it, sky_image.resolve is the same in numpy,
        bit for bit).  `out` is the WHOLE image: a CUDA float32, float16 or uint8 (lens.height, lens.width, 4) tensor whose rows may be further apart than
        a row, `target` naming a packed format, as in `render(..., target=)`; rows outside the band and bytes between rows are not written.  The rows of
        absent pixels (outside a fisheye's circle) are never read: a plain call stores zeros there, `composite` leaves them alone.  `premultiplied`: rgb
        times alpha is stored.  `composite`: blended into `out` where alpha > 0.  Returns `out`."""
        from . import sky_image as SI

        fn = SI.bind(self._lib).atmo_sky_image_resolve
        if premultiplied and composite:
            raise ValueError("premultiplied together with composite: the blend multiplies by alpha itself")
        n = _check_rays(rgba, "rgba", 4)
        if n != lens.counts(quads)[0]:
            raise ValueError(f"rgba must have one row per slot of the lens's ray array: shape ({lens.counts(quads)[0]}, 4)")
        tgt = _colour_target(out, lens.height, lens.width, "out", target)
        if tgt is None:
            tgt = N.AtmoTarget(out.data_ptr(), N.TARGET_RGBA32F, 0)
        flags = (SI.QUADS if quads else 0) | (SI.PREMULTIPLIED if premultiplied else 0) | (SI.COMPOSITE if composite else 0)
        nl = lens.native()
        N.check(self._ctx, fn(self._ctx, C.byref(nl), flags, C.c_void_p(rgba.data_ptr()), C.byref(tgt), C.c_void_p(_stream_handle(stream, rgba) or 0)))
        return out

    def sky_image_mips(self, levels, target=None, stream=None):
        """Fills the mip chain of an image (atmo_sky_image_mips; sky_image.mip_chain is the same in numpy, bit for bit): `levels[0]` is read, `levels[1:]`
        are written, each texel the average of the 2 x 2 stored texels above it.  `levels`: CUDA tensors (layers, h_l, w_l, 4) or (h_l, w_l, 4), float32,
        float16 or uint8 (`target` names a 4-byte format other than RGBA8_UNORM), h_l = max(1, h >> l), w_l = max(1, w >> l); row and layer pitches are
        taken from the strides.  All layers in one call, five levels a launch.  Returns `levels`."""
        import torch

        from . import sky_image as SI
        from . import targets as T

        fn = SI.bind(self._lib).atmo_sky_image_mips
        levels = list(levels)
        fmts = {torch.float32: T.RGBA32F, torch.float16: T.RGBA16F, torch.uint8: T.RGBA8}
        first = levels[0] if levels else None
        if not (isinstance(first, torch.Tensor) and first.is_cuda and first.dtype in fmts and first.dim() in (3, 4) and first.shape[-1] == 4):
            raise ValueError("levels must be CUDA float32, float16 or uint8 tensors of shape (layers, h, w, 4) or (h, w, 4)")
        fmt = fmts[first.dtype]
        if target is not None:
            fmt = T.format_id(target)
            if np.dtype(T.DTYPES[fmt]).name != str(first.dtype).replace("torch.", ""):
                raise ValueError(f"levels: target={target!r} is a {np.dtype(T.DTYPES[fmt]).name} format, the tensors are {first.dtype}")
        layers = int(first.shape[0]) if first.dim() == 4 else 1
        h, w = int(first.shape[-3]), int(first.shape[-2])
        if not 1 <= len(levels) <= SI.level_count(w, h):
            raise ValueError(f"a {w} x {h} image has 1 .. {SI.level_count(w, h)} levels")
        arr = (SI.AtmoSkyLevel * len(levels))()
        for l, t in enumerate(levels):
            wl, hl = SI.level_size(w, h, l)
            shape = (layers, hl, wl, 4) if first.dim() == 4 else (hl, wl, 4)
            if not (isinstance(t, torch.Tensor) and t.device == first.device and t.dtype == first.dtype and tuple(t.shape) == shape):
                raise ValueError(f"levels[{l}] must be a {first.dtype} tensor of shape {shape} on {first.device}")
            row = t.stride(-3) if hl > 1 else 4 * wl
            layer = t.stride(0) if (t.dim() == 4 and layers > 1) else 0
            if not (t.stride(-1) == 1 and t.stride(-2) == 4 and row >= 4 * wl and (layer == 0 or layer >= hl * row)):
                raise ValueError(f"levels[{l}]: the texels of a row must be contiguous, rows at least a row and layers at least a layer apart")
            arr[l] = SI.AtmoSkyLevel(t.data_ptr(), row * t.element_size(), 0, layer * t.element_size())
        N.check(self._ctx, fn(self._ctx, arr, len(levels), fmt, w, h, layers, C.c_void_p(_stream_handle(stream, first) or 0)))
        return levels

    def render_sky_image(self, lenses, target="rgba16f", *, mips: bool = True, premultiplied: bool = True, camera=None, time: float = 0.0, stream=None):
        """The sky through one lens or several of equal size (a lens.Lens or a sequence: an octahedral map, a panorama, six cube faces = six layers) as an
        image a renderer can bind: each lens is shaded as `render_lens` shades it -- in quad order under the declared sampler where this node has one,
        else row-major through the tile index --, resolved into its layer by `resolve_lens` (`premultiplied`: rgb times alpha, what filtering wants) and
        followed by ONE `sky_image_mips` call over all layers.  `target`: a format name of `render(..., target=)`.  Returns the list of level tensors,
        (layers, h_l, w_l, 4) each -- one tensor without `mips`; nothing is read back and nothing waits on the host."""
        import torch

        from . import sky_image as SI
        from .lens import Lens

        lenses = [lenses] if isinstance(lenses, Lens) else list(lenses)
        if not lenses or any((l.width, l.height) != (lenses[0].width, lenses[0].height) or l.rows != (0, l.height) for l in lenses):
            raise ValueError("render_sky_image takes one lens or several of equal size, each with its whole image as the band")
        w, h = lenses[0].width, lenses[0].height
        device = torch.device("cuda", self._device)
        quads = self._shades_ray_quads()
        with _on_stream(stream, device)[1]:
            n_levels = SI.level_count(w, h) if mips else 1
            levels = [_new_target(len(lenses) * hl, wl, target, device, zero=False).view(len(lenses), hl, wl, 4)
                      for wl, hl in (SI.level_size(w, h, l) for l in range(n_levels))]
            for layer, lens in enumerate(lenses):
                _, shaded = self._shade_lens(lens, camera, None, time, stream, quads)
                self.resolve_lens(lens, shaded, levels[0][layer], target=target, quads=quads, premultiplied=premultiplied, stream=stream)
            if n_levels > 1:
                self.sky_image_mips(levels, target=target, stream=stream)
            return levels

    def prepare_frame(self, camera, time: float = 0.0, rect=None) -> N.AtmoFrame:
        """The native per-frame argument block for `render_prepared` (build once per camera pose)."""
        return _to_native_frame(self.make_frame(camera, time, rect))

    def render_prepared(self, native_frame: N.AtmoFrame, depth_ptr: int, out_ptr: int, stream: int = 0):
        """Enqueue one draw with a frame from `prepare_frame` on raw device addresses: the per-step host cost is
        one ctypes call (what a render loop that re-draws an unchanged camera would do)."""
        self._bake_if_needed(stream)
        rc = self._lib.atmo_render(self._ctx, C.byref(native_frame), C.c_void_p(depth_ptr), C.c_void_p(out_ptr),
                                   C.c_void_p(stream or 0))
        N.check(self._ctx, rc)

    def render_composite(self, camera, depth, scene_rgba, rect=None, stream=None, time: float = 0.0, target=None):
        """The draw including the renderer's blend stage: shades `rect` and alpha-blends the result over
        `scene_rgba` (CUDA float32 (H, W, 4), the scene colour buffer) in place, as Godot's blend_mix does with
        ALBEDO/ALPHA; discarded fragments leave the scene untouched.  Returns `scene_rgba`.
        A float16 / uint8 `scene_rgba` (RGBA16F / RGBA8_UNORM, optionally with a row pitch) is blended in its own format: decoded, blended in fp32,
        encoded once (atmo_render_target).  `target` names the format of a uint8 buffer that is not RGBA8_UNORM, as in `render`."""
        return self._render_one(camera, depth, scene_rgba, rect, stream, time, target, True, None)

    # ---- several views in one launch (include/atmo_views.h) ------------------------------------------------------------------------
    def prepare_views(self, cameras, depth_ptrs, out_ptrs, rects=None, time: float = 0.0):
        """The native argument block of `render_views_prepared`: one N.AtmoView per camera, on raw device addresses."""
        return self._prepare_views(N.AtmoView, cameras, depth_ptrs, out_ptrs, rects, time)

    def render_views_prepared(self, views, n_views: int, composite: bool = False, stream: int = 0):
        """Enqueue one batch from `prepare_views`: one ctypes call, one launch for all views."""
        self._enqueue_views(self._lib.atmo_render_views, views, n_views, None, composite, stream)

    def prepare_views_target(self, cameras, depth_ptrs, targets, rects=None, time: float = 0.0):
        """The native argument block of `render_views_target_prepared`: one N.AtmoViewTarget per camera; targets[i] is an N.AtmoTarget (pixels, format,
        row pitch in bytes) addressed as `atmo_render_target` addresses it."""
        return self._prepare_views(N.AtmoViewTarget, cameras, depth_ptrs, targets, rects, time)

    def render_views_target_prepared(self, views, n_views: int, composite: bool = False, stream: int = 0):
        """Enqueue one batch from `prepare_views_target` (atmo_render_views_target): one ctypes call, one launch for all views."""
        self._enqueue_views(self._lib.atmo_render_views_target, views, n_views, None, composite, stream)

    def prepare_views_depth_target(self, cameras, depths, targets, rects=None, time: float = 0.0):
        """The native argument block of the depth-source batches (atmo_render_views_depth_target, atmo_render_views_proxy_depth_target): one
        N.AtmoViewDepthTarget per camera; depths[i] is an N.AtmoDepth, targets[i] an N.AtmoTarget."""
        return self._prepare_views(N.AtmoViewDepthTarget, cameras, depths, targets, rects, time)

    def _prepare_views(self, struct, cameras, depth_ptrs, colours, rects, time):
        field, name = ("rgba_dev", "outs") if struct is N.AtmoView else ("target", "targets")
        depth_field = "depth" if struct is N.AtmoViewDepthTarget else "depth_dev"
        n = len(cameras)
        if not (len(depth_ptrs) == n and len(colours) == n and (rects is None or len(rects) == n)):
            raise ValueError(f"cameras, depths, {name} and rects must have one entry per view")
        views = (struct * max(n, 1))()
        for i, cam in enumerate(cameras):
            views[i].frame = _to_native_frame(self.make_frame(cam, time, rects[i] if rects is not None else None))
            setattr(views[i], depth_field, depth_ptrs[i])
            setattr(views[i], field, colours[i])
        return views

    def _enqueue_views(self, fn, views, n_views, proxy, composite, stream):
        self._bake_if_needed(stream)
        box = () if proxy is None else (proxy[0], C.c_float(proxy[1]))
        N.check(self._ctx, fn(self._ctx, views, int(n_views), *box, int(bool(composite)), C.c_void_p(stream or 0)))

    def render_views(self, cameras, depths, outs=None, rects=None, composite: bool = False, stream=None, time: float = 0.0, target=None):
        """Several views of this planet in ONE launch (atmo_render_views): the two eyes of a stereo pass, a split screen, probe faces -- up to
        N.MAX_VIEWS.  View i is bit for bit `render(cameras[i], depths[i], outs[i], rects[i])` -- or, with composite=True,
        `render_composite(cameras[i], depths[i], outs[i], rects[i])`, where outs[i] is view i's (H_i, W_i, 4) scene buffer, blended in place --;
        viewport sizes and rects may differ between views.  The tensors are checked as those calls check theirs; outs=None allocates the plain
        outputs.  The tensors the views write must not overlap.  One native call; returns the list of output tensors.
        outs[i] may also be float16 (RGBA16F) or uint8 (RGBA8_UNORM) tensors, and their rows may be further apart than a row (a row pitch: the two
        halves of one double-wide image, say): the batch then stores or blends in that format (atmo_render_views_target; one format per batch).
        `target` allocates such outputs, or names the format of uint8 outs, as in `render`."""
        return self._render_views(cameras, depths, outs, rects, composite, stream, time, target, None)

    def _render_views(self, cameras, depths, outs, rects, composite, stream, time, target, proxy):
        """`render_views` (proxy None) and `render_views_proxy` (proxy = `_proxy`'s (model, box_size): zero-filled allocations, the proxy entry points)."""
        n = len(cameras)
        if n > N.MAX_VIEWS:
            raise ValueError(f"at most {N.MAX_VIEWS} views per batch")
        if len(depths) != n or (outs is not None and len(outs) != n) or (rects is not None and len(rects) != n):
            raise ValueError("cameras, depths, outs and rects must have one entry per view")
        if composite and outs is None:
            raise ValueError("composite=True blends into the views' scene buffers: pass them as outs")
        outs = list(outs) if outs is not None else [None] * n
        tgts = [None] * n
        sources = [isinstance(d, DepthSource) for d in depths]
        if any(sources) and not all(sources):
            raise TypeError("the depths of one batch are all tensors or all depth_source(...) objects")
        srcs = [None] * n
        for i, (cam, depth) in enumerate(zip(cameras, depths)):
            if sources[i]:
                srcs[i] = depth.native(cam, f"view {i}: ")
            else:
                _check_depth(depth, cam, f"view {i}: ", split=True)
            x0, y0, x1, y1 = rects[i] if rects is not None and rects[i] is not None else (0, 0, cam.width, cam.height)
            rows, cols = (cam.height, cam.width) if composite else (y1 - y0, x1 - x0)
            if outs[i] is None:
                outs[i] = _new_target(rows, cols, target, depth.device, zero=proxy is not None)
            # a contiguous float32 tensor (None), or the N.AtmoTarget of a float16 / uint8 / pitched one
            tgts[i] = _colour_target(outs[i], rows, cols, f"view {i}: {'scene_rgba' if composite else 'out'}", target)
        if n == 0:
            return outs
        stream = _stream_handle(stream, depths[0])
        depth_ptrs = [d.data_ptr() for d in depths] if not sources[0] else srcs
        packed = sources[0] or any(t is not None for t in tgts)   # (the depth-source batches take every colour tensor as an N.AtmoTarget)
        # cloud detail into targets (include/atmo_detail_target.h): the depth-source batch's structures, plain depth tensors as tight D32 sources.  The
        # float-only batch and the proxy batches have no detail form and refuse as before
        fn = self._entry("atmo_render_views_detail_target") if proxy is None and packed and self._serves_cloud_detail() else None
        if fn is not None and not sources[0]:
            depth_ptrs = [N.AtmoDepth(p, N.DEPTH_D32_SFLOAT, 0) for p in depth_ptrs]
        if packed:   # one batch, one struct: a contiguous float32 tensor among pitched ones is an RGBA32F target without a pitch
            tgts = [t if t is not None else N.AtmoTarget(o.data_ptr(), N.TARGET_RGBA32F, 0) for t, o in zip(tgts, outs)]
            prepare = self.prepare_views_depth_target if sources[0] or fn is not None else self.prepare_views_target
            views = prepare(cameras, depth_ptrs, tgts, rects, time)
        else:
            views = self.prepare_views(cameras, depth_ptrs, [o.data_ptr() for o in outs], rects, time)
        if fn is None:
            fn = getattr(self._lib, _BATCH_DRAWS[proxy is not None, packed, sources[0]])
        self._enqueue_views(fn, views, n, proxy, composite, stream)
        return outs

    # ---- several far-mode views in one launch (include/atmo_views_proxy.h) -----------------------------------------------------------
    def proxy_model(self):
        """The native model matrix of the proxy draws: global_transform, column-major."""
        return (C.c_float * 16)(*[float(x) for x in col_major(self.global_transform)])

    def render_views_proxy_prepared(self, views, n_views: int, model, box_size: float, composite: bool = False, stream: int = 0):
        """Enqueue one far-mode batch from `prepare_views` (atmo_render_views_proxy): `model` from `proxy_model`, one launch for all views."""
        self._enqueue_views(self._lib.atmo_render_views_proxy, views, n_views, (model, box_size), composite, stream)

    def render_views_proxy_target_prepared(self, views, n_views: int, model, box_size: float, composite: bool = False, stream: int = 0):
        """Enqueue one far-mode batch from `prepare_views_target` (atmo_render_views_proxy_target)."""
        self._enqueue_views(self._lib.atmo_render_views_proxy_target, views, n_views, (model, box_size), composite, stream)

    def render_views_proxy(self, cameras, depths, outs=None, rects=None, composite: bool = False, stream=None, time: float = 0.0,
                           box_size: float | None = None, target=None):
        """`render_views` through the far mode's BoxMesh: several views of this planet's proxy in ONE launch (atmo_render_views_proxy).  View i is bit
        for bit `render_proxy(cameras[i], depths[i], outs[i], rects[i], box_size=box_size)` -- or, with composite=True, `render_proxy_composite` --:
        only the box's passing front-face fragments are written.  One box per batch: edge `box_size` (default proxy_box_size(cameras[0])) centred on
        global_transform.  outs=None allocates zero-filled outputs, as `render_proxy` does; float16 / uint8 / pitched tensors go through
        atmo_render_views_proxy_target (one format per batch)."""
        proxy = self._proxy(cameras[0] if len(cameras) else None, box_size)
        return self._render_views(cameras, depths, outs, rects, composite, stream, time, target, proxy)

    def draw_views(self, cameras, depths, scene_rgbas, rects=None, stream=None, time: float = 0.0, target=None):
        """`draw` for several views in one launch: near mode `render_views(..., composite=True)`, far mode `render_views_proxy(..., composite=True)`
        with the BoxMesh of the reference's size.  Returns the list of scene buffers."""
        if self._mode == MODE_NEAR:
            return self.render_views(cameras, depths, scene_rgbas, rects=rects, composite=True, stream=stream, time=time, target=target)
        return self.render_views_proxy(cameras, depths, scene_rgbas, rects=rects, composite=True, stream=stream, time=time, target=target)

    # ---- the far-mode draw: the BoxMesh proxy (include/atmo_scene.h) ---------------------------------------------------------------
    def proxy_box_size(self, camera=None) -> float:
        """Edge of the far mode's BoxMesh: the reference's atmo_clip_distance (planet_atmosphere.gd:300-321), 1.75 (R + H + camera near) 1.1."""
        cam_near = 0.1 if camera is None else camera.near
        return 1.75 * (self._planet_radius + self._atmosphere_height + cam_near) * SWITCH_MARGIN_RATIO

    def _proxy(self, camera, box_size):
        """What the proxy entry points take beside a plain draw's arguments: (model matrix, the box's edge -- default proxy_box_size(camera))."""
        return self.proxy_model(), self.proxy_box_size(camera) if box_size is None else float(box_size)

    def render_proxy(self, camera, depth, out=None, rect=None, stream=None, time: float = 0.0, box_size: float | None = None, target=None):
        """`render` through the far mode's BoxMesh (default edge: proxy_box_size(camera)) centred on global_transform: only the box's front-face
        fragments that pass the depth test are shaded and written (atmo_render_proxy); every other pixel of `out` is left as it was (an `out` allocated
        here is zero-filled).  `out` / `target`: as `render` (float16 / uint8 tensors, a row pitch: atmo_render_proxy_target)."""
        return self._render_one(camera, depth, out, rect, stream, time, target, False, self._proxy(camera, box_size))

    def render_proxy_composite(self, camera, depth, scene_rgba, rect=None, stream=None, time: float = 0.0, box_size: float | None = None, target=None):
        """`render_composite` through the far mode's BoxMesh (atmo_render_proxy_composite; a float16 / uint8 / pitched `scene_rgba`:
        atmo_render_proxy_target; `target`: as `render_composite`).  Returns `scene_rgba`."""
        return self._render_one(camera, depth, scene_rgba, rect, stream, time, target, True, self._proxy(camera, box_size))

    def draw(self, camera, depth, scene_rgba, rect=None, stream=None, time: float = 0.0, target=None):
        """The draw Godot makes for this node in its current mode (set by `_process`): near mode the fullscreen quad (`render_composite`), far mode
        the BoxMesh of the reference's size (`render_proxy_composite`).  Returns `scene_rgba` (float32, float16 or uint8; a row pitch is taken from its row stride;
        `target` names the format of a uint8 buffer that is not RGBA8_UNORM)."""
        if self._mode == MODE_NEAR:
            return self.render_composite(camera, depth, scene_rgba, rect=rect, stream=stream, time=time, target=target)
        return self.render_proxy_composite(camera, depth, scene_rgba, rect=rect, stream=stream, time=time, target=target)

    def render_raw(self, frame: dict, depth_ptr: int, out_ptr: int, stream: int = 0):
        """`render` on raw device addresses (what a non-torch host would call)."""
        self._bake_if_needed(stream)
        nf = _to_native_frame(frame)
        rc = self._lib.atmo_render(self._ctx, C.byref(nf), C.c_void_p(depth_ptr), C.c_void_p(out_ptr), C.c_void_p(stream or 0))
        N.check(self._ctx, rc)

    def render_tiles_prepared(self, native_frame: N.AtmoFrame, depth_ptr: int, out_ptr: int, tiles_ptr: int, n_tiles: int, stream: int = 0,
                              n_heavy: int = 0):
        """atmo_render_tiles: draw only the listed tiles (uint32 indices in device memory, row-major in the grid of
        measure_tile_costs) of the frame's rect, in list order; `out_ptr` is addressed like render_prepared's.
        n_heavy > 0 (atmo_render_tiles_split): the list's first n_heavy tiles on two lanes per ray beside the rest (sharding.heavy_tiles)."""
        self._bake_if_needed(stream)
        if n_heavy:
            rc = self._lib.atmo_render_tiles_split(self._ctx, C.byref(native_frame), C.c_void_p(depth_ptr), C.c_void_p(out_ptr), C.c_void_p(tiles_ptr),
                                                   int(n_tiles), int(n_heavy), C.c_void_p(stream or 0))
        else:
            rc = self._lib.atmo_render_tiles(self._ctx, C.byref(native_frame), C.c_void_p(depth_ptr), C.c_void_p(out_ptr), C.c_void_p(tiles_ptr),
                                             int(n_tiles), C.c_void_p(stream or 0))
        N.check(self._ctx, rc)

    def measure_tile_costs(self, camera, depth, rect=None, stream=None, time: float = 0.0):
        """One draw through atmo_measure_tile_costs: ((tiles_y, tiles_x) uint32 costs -- every tile's longest wavefront in shader cycles --,
        tile_w, tile_h).  sharding.lpt_strips deals them to the GPUs of a node."""
        self.measure_row_costs(camera, depth, rect=rect, stream=stream, time=time)
        return self._last_tile_costs, self._last_tile_size[0], self._last_tile_size[1]

    def measure_row_costs(self, camera, depth, rect=None, stream=None, time: float = 0.0):
        """Measured cost of every pixel row of `rect` (default: the whole viewport): one draw through atmo_measure_tile_costs,
        each tile's cost (longest wavefront, shader cycles) spread over its pixel rows and summed along the row.  Feed it to
        sharding.balanced_row_bands to cut a viewport into row bands of equal WORK for several GPUs."""
        import torch

        frame = self.make_frame(camera, time, rect)
        x0, y0, x1, y1 = frame["rect"]
        nf = _to_native_frame(frame)
        stream = _stream_handle(stream, depth)
        self._bake_if_needed(stream)
        scratch = torch.empty((y1 - y0, x1 - x0, 4), dtype=torch.float32, device=depth.device)
        gx, gy, tw, th = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        args = (self._ctx, C.byref(nf), C.c_void_p(depth.data_ptr()), C.c_void_p(scratch.data_ptr()), C.c_void_p(stream or 0))
        N.check(self._ctx, self._lib.atmo_measure_tile_costs(*args, None, 0, C.byref(gx), C.byref(gy), C.byref(tw), C.byref(th)))
        cost = np.zeros((gy.value, gx.value), dtype=np.uint32)
        N.check(self._ctx, self._lib.atmo_measure_tile_costs(*args, cost.ctypes.data_as(C.c_void_p), cost.size, C.byref(gx), C.byref(gy),
                                                            C.byref(tw), C.byref(th)))
        self._last_tile_costs = cost  # (tiles_y, tiles_x) uint32, for diagnostics (tools/xcd_balance.py)
        self._last_tile_size = (tw.value, th.value)
        rows = np.repeat(cost.astype(np.float64).sum(axis=1) / th.value, th.value)[: y1 - y0]
        return rows

    def split_stats(self) -> dict:
        """atmo_get_split_stats: draws so far whose heaviest tiles were drawn with two lanes per ray beside the rest, and how many tiles the last
        such draw split (the raymarched-light kernel under the declared sampler, when a draw is as long as its heaviest wavefront)."""
        n, last = C.c_uint(0), C.c_uint(0)
        N.check(self._ctx, self._lib.atmo_get_split_stats(self._ctx, C.byref(n), C.byref(last)))
        return {"split_draws": int(n.value), "heavy_tiles_last": int(last.value)}

    def feedback_stats(self) -> dict:
        """atmo_get_feedback_stats (diagnostics of the tile-order feedback)."""
        st, od, so, rc = C.c_int(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
        N.check(self._ctx, self._lib.atmo_get_feedback_stats(self._ctx, C.byref(st), C.byref(od), C.byref(so), C.byref(rc)))
        return dict(states=st.value, ordered_draws=od.value, sorts=so.value, recycled=rc.value)

    # ---- kernel timing (HIP events on the launch stream) ---------------------------------------------
    def set_timing(self, enable, every: int = 1):
        """enable: False/0 off; True = bracket every `every`-th launch with HIP events."""
        k = 0 if not enable else max(1, int(every))
        N.check(self._ctx, self._lib.atmo_set_timing(self._ctx, k))

    def get_timing(self):
        n, ms = C.c_int(0), C.c_double(0.0)
        N.check(self._ctx, self._lib.atmo_get_timing(self._ctx, C.byref(n), C.byref(ms)))
        return n.value, ms.value


def _colour_target(t, rows: int, cols: int, what: str, target=None):
    """How a colour tensor is drawn into: None for a contiguous float32 (rows, cols, 4) tensor -- the float entry points --, else the N.AtmoTarget
    of a float16 (RGBA16F), uint8 (RGBA8_UNORM) or float32 tensor whose pixels are contiguous and whose rows may be further apart (the row pitch
    is the tensor's row stride): include/atmo_target.h.  `target` names the format of the tensor's bits where the dtype does not say it: a uint8
    tensor is RGBA8_UNORM unless `target` is another 4-byte format of `_new_target`'s list (the bytes as they lie in memory); a name that contradicts
    the dtype is a ValueError."""
    import torch

    from . import targets as T

    fmts = {torch.float32: T.RGBA32F, torch.float16: T.RGBA16F, torch.uint8: T.RGBA8}
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in fmts and tuple(t.shape) == (rows, cols, 4)):
        raise ValueError(f"{what} must be a CUDA float32, float16 or uint8 tensor of shape ({rows}, {cols}, 4)")
    fmt = fmts[t.dtype]
    if target is not None:
        fmt = T.format_id(target)
        if np.dtype(T.DTYPES[fmt]).name != str(t.dtype).replace("torch.", ""):
            raise ValueError(f"{what}: target={target!r} is a {np.dtype(T.DTYPES[fmt]).name} format, the tensor is {t.dtype}")
    if fmt == T.RGBA32F and t.is_contiguous():
        return None
    if not (t.stride(2) == 1 and t.stride(1) == 4 and (rows == 1 or t.stride(0) >= 4 * cols)):
        raise ValueError(f"{what}: the pixels of a row must be contiguous and the row stride at least a row (a row pitch is the only stride supported)")
    return N.AtmoTarget(t.data_ptr(), fmt, (t.stride(0) if rows > 1 else 4 * cols) * t.element_size())


def _new_target(rows: int, cols: int, target, device, zero: bool):
    """The tensor a draw allocates: float32, or the packed format named by target="rgba16f" | "rgba8" | "rgba8_srgb" | "bgra8" | "bgra8_srgb" |
    "a2b10g10r10" (uint8 (rows, cols, 4) for all but the first: the bytes as they lie in memory).  This is THE list of target names of every draw
    method: targets.FORMATS holds it, and a new format is one line there (plus its DTYPES / PIXEL_BYTES entries)."""
    import torch

    from . import targets as T

    np_dtype = T.DTYPES[T.format_id(target) if target is not None else T.RGBA32F]
    dtype = {np.float32: torch.float32, np.float16: torch.float16, np.uint8: torch.uint8}[np_dtype]
    return (torch.zeros if zero else torch.empty)((rows, cols, 4), dtype=dtype, device=device)


class _WorldRaySpace:
    """The camera of `shade_rays(camera=None)`: ray space is world space.  atmo_shade_rays reads the view matrices only."""
    width = height = 1
    view = inv_view = inv_projection = np.eye(4)


_WORLD_RAY_SPACE = _WorldRaySpace()


def _check_kind(t, message: str, dtype: str = "float32", contiguous: bool = True) -> None:
    """THE kind test of a tensor argument: a CUDA tensor of torch's `dtype`, contiguous where asked; TypeError(`message`, the site's own) otherwise."""
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, dtype) and (not contiguous or t.is_contiguous())):
        raise TypeError(message)


def _check_rays(t, what: str, cols: int) -> int:
    """`what` is a contiguous CUDA float32 tensor of shape (n, cols): TypeError for its kind, ValueError for its shape.  Returns n."""
    _check_kind(t, f"{what} must be a contiguous CUDA float32 tensor")
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{what} must have shape (n, {cols})")
    return int(t.shape[0])


def _check_index(t) -> int:
    """`index` is a contiguous CUDA int32 tensor of shape (m,): TypeError for its kind, ValueError for its shape.  Returns m."""
    _check_kind(t, "index must be a contiguous CUDA int32 tensor", "int32")
    if t.dim() != 1:
        raise ValueError("index must have shape (m,)")
    return int(t.shape[0])


def _stream_handle(stream, where) -> int:
    """The hipStream_t behind a draw's `stream` argument: a torch stream's, a raw handle as it is, None = torch's current stream on the device of `where`,
    a tensor or a device."""
    if stream is None:
        import torch

        return torch.cuda.current_stream(getattr(where, "device", where)).cuda_stream
    return getattr(stream, "cuda_stream", stream)


def _on_stream(stream, device):
    """(`_stream_handle`'s handle, the context in which a call allocates): torch's allocator reuses a tensor's memory in the order of the stream that was
    current when it was allocated, so the scratch and the results of a call on the caller's stream are allocated with that stream current.  None is
    torch's current stream already: a null context."""
    import torch

    handle = _stream_handle(stream, device)
    return handle, contextlib.nullcontext() if stream is None else torch.cuda.stream(torch.cuda.ExternalStream(handle, device=device))


def _check_depth(depth, camera, prefix: str = "", split: bool = False):
    """A depth buffer is a contiguous CUDA float32 (viewport_h, viewport_w) tensor.  split: `render` and the view batches raise TypeError for the tensor's
    kind and ValueError for its shape; the other single draws raise one TypeError that names both (kept as it was: NOTES.md)."""
    kind = "depth must be a contiguous CUDA float32 tensor"
    both = kind + " of shape (viewport_h, viewport_w)"
    _check_kind(depth, prefix + (kind if split else both))
    if tuple(depth.shape) != (camera.height, camera.width):
        raise ValueError(prefix + "depth must have shape (viewport_h, viewport_w)") if split else TypeError(prefix + both)


def draw_order(nodes, camera) -> list:
    """The order Godot draws alpha-blended instances of equal render priority in: back to front by the distance from the camera to the centre of
    each instance's AABB, farthest first (engine behaviour: the transparent render list's depth sort).  For both meshes of a PlanetAtmosphere that
    centre is the node's origin (the BoxMesh and the near-mode quad are centred on it).  Stable for equal distances."""
    cam_pos = np.asarray(camera.inv_view, dtype=np.float64)[:3, 3]
    dist = [float(np.linalg.norm(np.asarray(n.global_transform, dtype=np.float64)[:3, 3] - cam_pos)) for n in nodes]
    return [nodes[i] for i in sorted(range(len(nodes)), key=lambda i: -dist[i])]


def draw_atmospheres(nodes, camera, depth, scene_rgba, stream=None, time: float = 0.0, target=None):
    """Draws several PlanetAtmosphere nodes into one frame as Godot does: each node's draw for its current mode (`PlanetAtmosphere.draw`: the
    fullscreen quad near, the BoxMesh far), composited over `scene_rgba` in place, back to front (`draw_order`).  Returns `scene_rgba`, which may be the renderer's own RGBA16F / RGBA8_UNORM buffer
    (a float16 / uint8 tensor, optionally with a row pitch): every node then blends in that format.  `target` names the format of a uint8 buffer that is not
    RGBA8_UNORM, as in `PlanetAtmosphere.render`."""
    kw = {} if target is None else {"target": target}
    for node in draw_order(list(nodes), camera):
        node.draw(camera, depth, scene_rgba, stream=stream, time=time, **kw)
    return scene_rgba


def prepare_planets(draws, time: float = 0.0):
    """The native argument block of `render_planets_prepared` / `plan_planets`: one N.AtmoPlanetDraw per (node, camera, depth, scene_rgba, rect, box_size,
    target) entry, the tensors checked as `PlanetAtmosphere.render_proxy_composite` checks them."""
    draws = list(draws)
    if len(draws) > N.MAX_PLANET_DRAWS:
        raise ValueError(f"at most {N.MAX_PLANET_DRAWS} draws per call")
    arr = (N.AtmoPlanetDraw * max(len(draws), 1))()
    for i, (node, camera, depth, scene_rgba, rect, box_size, target) in enumerate(draws):
        if isinstance(depth, DepthSource):
            raise TypeError(f"draw {i}: atmo_render_planets takes float depth tensors only (AtmoPlanetDraw holds a float pointer), not a depth_source")
        _check_depth(depth, camera, f"draw {i}: ")
        tgt = _colour_target(scene_rgba, camera.height, camera.width, f"draw {i}: scene_rgba", target)
        model, size = node._proxy(camera, box_size)
        d = arr[i]
        d.ctx = node._ctx
        d.frame = _to_native_frame(node.make_frame(camera, time, rect))
        d.model_matrix = model
        d.box_size = size
        d.depth_dev = depth.data_ptr()
        d.target = tgt if tgt is not None else N.AtmoTarget(scene_rgba.data_ptr(), N.TARGET_RGBA32F, 0)
    return arr


def _check_planets(rc: int, arr, n: int, who: bytes) -> None:
    if rc != N.ATMO_OK:   # the message lies on the context of the draw it names, on the first draw's, or in the slot without a context
        lib = N.load()
        msgs = [lib.atmo_last_error_string(arr[i].ctx) for i in range(n) if arr[i].ctx] + [lib.atmo_last_error_string(None)]
        named = [m.decode() for m in msgs if m and m.startswith(who)]
        raise N.AtmoError(rc, named[0] if named else "")


def plan_planets(draws, time: float = 0.0):
    """atmo_plan_planets: (launch_of, n_launches) -- for every entry of `draws` the launch of `render_planets` that holds it, or -1 when its box leaves
    no tile on its rect.  Nothing is enqueued."""
    draws = list(draws)
    arr = prepare_planets(draws, time)
    launch_of, n_launches = (C.c_int * max(len(draws), 1))(), C.c_int(0)
    _check_planets(N.load().atmo_plan_planets(arr, len(draws), launch_of, C.byref(n_launches)), arr, len(draws), b"atmo_plan_planets")
    return list(launch_of)[:len(draws)], n_launches.value


def render_planets_prepared(arr, n_draws: int, stream: int = 0):
    """Enqueue one frame's far planets from `prepare_planets`: one ctypes call."""
    _check_planets(N.load().atmo_render_planets(arr, int(n_draws), C.c_void_p(stream or 0)), arr, int(n_draws), b"atmo_render_planets")


def render_planets(draws, stream=None, time: float = 0.0):
    """Several far-mode planets blended into their scene buffers in LIST ORDER by ONE native call (atmo_render_planets, include/atmo_planets.h): draws
    that cannot touch on screen share a launch, draws that may keep their order.  `draws` is a list of (node, camera, depth, scene_rgba, rect, box_size,
    target); entry i is bit for bit `node.render_proxy_composite(camera, depth, scene_rgba, rect=rect, box_size=box_size, target=target)` issued in that
    order: rect None is the whole viewport, box_size None is `node.proxy_box_size(camera)`, scene_rgba a float32, float16 or uint8 tensor with an
    optional row pitch, `target` the format name of a uint8 buffer that is not RGBA8_UNORM.  A node may appear more than once (stereo).  Bakes each
    node's optical depth first if that is pending.  At most N.MAX_PLANET_DRAWS entries."""
    draws = list(draws)
    if not draws:
        return
    arr = prepare_planets(draws, time)
    handle = _stream_handle(stream, draws[0][2])
    for d in draws:
        d[0]._bake_if_needed(handle)
    render_planets_prepared(arr, len(draws), handle)


def draw_atmospheres_batched(nodes, camera, depth, scene_rgba, stream=None, time: float = 0.0, target=None):
    """`draw_atmospheres` with the far nodes batched: the same order (`draw_order`), the same bytes, but every maximal run of far-mode nodes in that
    order goes through ONE `render_planets` call -- planets that do not overlap on screen share a launch -- and a near-mode node, whose fullscreen
    draw touches everything, is its own `node.draw` between the runs.  Returns `scene_rgba`."""
    if isinstance(depth, DepthSource):
        raise TypeError("draw_atmospheres_batched takes a float depth tensor only (atmo_render_planets), not a depth_source: use draw_atmospheres")
    kw = {} if target is None else {"target": target}
    run = []

    def flush():
        if run:
            render_planets([(n, camera, depth, scene_rgba, None, None, target) for n in run], stream=stream, time=time)
            run.clear()

    for node in draw_order(list(nodes), camera):
        if node._mode == MODE_FAR:
            run.append(node)
            continue
        flush()
        node.draw(camera, depth, scene_rgba, stream=stream, time=time, **kw)
    flush()
    return scene_rgba
