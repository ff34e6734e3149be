"""Host-side mirror of the `NoiseTexture3D` the reference's demo binds as `u_cloud_shape_texture`
(demo/planet_atmosphere_test.tscn:48-57,113): a seamless 3-D noise volume, generated on the GPU.

  NoiseTexture3D (engine resource)              here
  -------------------------------------------  ------------------------------------------------------------
  noise : Noise                                 `noise`: a `SeededValueNoise` (stands for the engine's FastNoiseLite)
  width, height, depth                          `width`, `height`, `depth`; `size` sets all three.  The context's shape texture is
                                                cubic, so unequal values raise when the volume is used
  seamless = false, invert = false              `seamless`, `invert`: the same defaults
  normalize = true                              `normalize`
  seamless_blend_skirt                          not needed: the seamless volume tiles by construction (periodic lattice)
  color_ramp                                    not mirrored (the shader reads one channel)
  update deferred to idle time                  `_request_update()`; the deferred `_update` runs on `process_deferred()` or on first
                                                access to the data
  get_data()                                    `get_data()`: the (n, n, n) uint8 array, [z, y, x]
  --                                            `offset`: noise-space offset in texels (lives here, not on the noise: the cubemap's
                                                meaning is unchanged); animate it for shapes that evolve over time
  --                                            `bind_to(node, stream=None)`: generate straight into a node's context, no read-back

The arithmetic is stated in include/atmo_noise_volume.h and lives in the device kernels only (`atmo_noise_volume_kernel`); a float32
numpy statement of it for the tests is tests/noise_volume_host.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .noise_cubemap import SeededValueNoise


class NoiseVolume:
    """See module docstring.  Generation runs on the GPU through `atmo_generate_noise_volume`."""

    def __init__(self, device: int = 0, noise: SeededValueNoise | None = None, size: int | None = None, width: int = 64, height: int = 64,
                 depth: int = 64, seamless: bool = False, invert: bool = False, normalize: bool = True, offset=(0.0, 0.0, 0.0)):
        self._lib = N.load()
        self._device = device
        self._ctx = None
        self._noise = None
        self._dims = [64, 64, 64]       # width, height, depth
        self._seamless, self._invert, self._normalize = False, False, True
        self._offset = (0.0, 0.0, 0.0)
        self._update_scheduled = False
        self._data = None
        self._changed = []
        if size is not None:
            width = height = depth = size
        self.width, self.height, self.depth = width, height, depth
        self.seamless, self.invert, self.normalize = seamless, invert, normalize
        self.offset = offset
        self.noise = noise if noise is not None else SeededValueNoise()
        self._request_update()

    # ---- properties ------------------------------------------------------------------------------------
    @property
    def noise(self):
        return self._noise

    @noise.setter
    def noise(self, value):
        if self._noise is not None:
            self._noise.disconnect_changed(self._on_noise_changed)
        self._noise = value
        if self._noise is not None:
            self._noise.connect_changed(self._on_noise_changed)
            self._request_update()

    def _set_dim(self, axis: int, value):
        v = int(value)
        if v != self._dims[axis]:
            self._dims[axis] = v
            self._request_update()

    width = property(lambda self: self._dims[0], lambda self, v: self._set_dim(0, v))
    height = property(lambda self: self._dims[1], lambda self, v: self._set_dim(1, v))
    depth = property(lambda self: self._dims[2], lambda self, v: self._set_dim(2, v))

    @property
    def size(self) -> int:
        """The side of the cubic volume; raises while width, height and depth differ."""
        w, h, d = self._dims
        if not (w == h == d):
            raise ValueError(f"NoiseVolume is {w} x {h} x {d}: width, height and depth must be equal, the context's shape texture is cubic "
                             "(u_cloud_shape_texture is n x n x n)")
        return w

    @size.setter
    def size(self, value):
        for axis in range(3):
            self._set_dim(axis, value)

    def _set_flag(self, name: str, value):
        value = bool(value)
        if value != getattr(self, name):
            setattr(self, name, value)
            self._request_update()

    seamless = property(lambda self: self._seamless, lambda self, v: self._set_flag("_seamless", v))
    invert = property(lambda self: self._invert, lambda self, v: self._set_flag("_invert", v))
    normalize = property(lambda self: self._normalize, lambda self, v: self._set_flag("_normalize", v))

    @property
    def offset(self):
        return self._offset

    @offset.setter
    def offset(self, value):
        value = tuple(float(v) for v in value)
        if len(value) != 3:
            raise ValueError("offset takes 3 floats (texels along x, y, z)")
        if value != self._offset:
            self._offset = value
            self._request_update()

    def connect_changed(self, cb):
        self._changed.append(cb)

    def _on_noise_changed(self):
        self._request_update()

    def _request_update(self):
        self._update_scheduled = True

    def process_deferred(self):
        """Runs the deferred `_update` if one is scheduled (Godot's call_deferred at idle time)."""
        if self._update_scheduled:
            self._update()

    def _update(self):
        if self._noise is None:
            self._update_scheduled = False
            return
        self._data = self._generate(self._descriptor())
        self._update_scheduled = False
        for cb in list(self._changed):
            cb()

    # ---- generation ------------------------------------------------------------------------------------
    def _descriptor(self) -> N.AtmoNoiseVolume:
        """The settings as the C ABI takes them (include/atmo_noise_volume.h)."""
        nz = self._noise
        if nz is None:
            raise ValueError("NoiseVolume has no noise")
        return N.AtmoNoiseVolume(self.size, int(nz.seed) & 0xFFFFFFFF, float(nz.frequency), int(nz.fractal_octaves), float(nz.fractal_gain),
                                 (C.c_float * 3)(*self._offset), int(self._seamless), int(self._invert), int(self._normalize))

    def _context(self):
        if self._ctx is None:
            ctx = C.c_void_p()
            N.check(None, self._lib.atmo_create(self._device, N.VARIANT_NO_CLOUDS, 0, 0, N.LIGHT_LUT, 0, C.byref(ctx)))
            self._ctx = ctx
        return self._ctx

    def _generate(self, desc: N.AtmoNoiseVolume) -> np.ndarray:  # on the device, read back through texels_host
        n = desc.size
        out = np.empty((n, n, n), dtype=np.uint8)
        ctx = self._context()
        N.check(ctx, self._lib.atmo_generate_noise_volume(ctx, C.byref(desc), 0, out.ctypes.data_as(C.c_void_p), None))
        return out

    def get_data(self) -> np.ndarray:
        """The (n, n, n) uint8 texels, [z, y, x]; runs the pending update."""
        self.process_deferred()
        return self._data

    def bind_to(self, node, stream=None):
        """Generates the volume, as it is set now, straight into `node`'s context and binds it as u_cloud_shape_texture: enqueued on `stream`
        (a torch stream or a raw handle; None = the null stream, where the node's other texture updates go), no read-back, no host wait.  Call it every
        frame in front of the draw, with `offset` moved, for shapes that evolve."""
        desc = self._descriptor()
        handle = getattr(stream, "cuda_stream", stream)
        N.check(node._ctx, node._lib.atmo_generate_noise_volume(node._ctx, C.byref(desc), 1, None, handle))

    def close(self):
        if self._ctx is not None:
            self._lib.atmo_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
