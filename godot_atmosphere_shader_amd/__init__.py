"""MI355X-native (gfx950) implementation of the per-pixel atmosphere / volumetric-cloud raymarch of
Zylann/godot_atmosphere_shader, behind the reference's `PlanetAtmosphere` / `shader_params` surface.

  csrc/                 hand-written HIP kernels + the C ABI of include/atmo.h (libatmo_hip.so)
  planet_atmosphere.py  host-side mirror of addons/zylann.atmosphere/planet_atmosphere.gd
  depth_formats.py      the depth sources' contract in numpy (include/atmo_depth.h; `depth_source` wraps a renderer's own depth buffer)
  noise_cubemap.py      host-side mirror of addons/zylann.atmosphere/noise_cubemap.gd (generation on the GPU)
  lens.py               lens rays in numpy: panorama, fisheye, octahedral map, cube face (include/atmo_lens.h; `Lens` describes one for `render_lens`)
  reduced.py            reduced-resolution draws in numpy and the header's ctypes declarations (include/atmo_reduced.h; `PlanetAtmosphere.render_reduced`)
  temporal.py           temporal draws in numpy -- phases, the phase frame, the history, the resolve -- and the header's ctypes declarations
                        (include/atmo_temporal.h; `PlanetAtmosphere.render_temporal`, `TemporalHistory`)
  sky_sh.py             the sky as light in numpy -- lens-pixel solid angles, the SH9 projection in its fixed order of summation, irradiance -- and the
                        header's ctypes declarations (include/atmo_sky_sh.h; `PlanetAtmosphere.lens_solid_angles`, `project_sh9`, `ambient_sh9`)
  sky_image.py          sky images in numpy -- the resolve of a lens's shaded rays into a target format, the mip chain -- and the header's ctypes
                        declarations (include/atmo_sky_image.h; `PlanetAtmosphere.resolve_lens`, `sky_image_mips`, `render_sky_image`)
  noise_volume.py       host-side mirror of the demo's NoiseTexture3D: the cloud shape volume, generated on the GPU (include/atmo_noise_volume.h)
  demo.py               the reference's demo scene + named shader configurations (tests, bench.py, smoke())
  scene.py              synthetic inputs (camera, depth, jitter, cloud textures) for tests and bench
  sharding.py           row-band / viewport sharding across the GPUs of a node + RCCL gather
"""
from .planet_atmosphere import (  # noqa: F401
    DefaultShader, DepthSource, PlanetAtmosphere, Shader, SHADERS, Transform2D, atmosphere_vertex, depth_source, load_shader, make_frame,
)

from .noise_cubemap import NoiseCubemap, SeededValueNoise  # noqa: F401,E402
from .noise_volume import NoiseVolume  # noqa: F401,E402
from .lens import Lens  # noqa: F401,E402

__all__ = ["NoiseCubemap", "NoiseVolume", "SeededValueNoise", "PlanetAtmosphere", "Shader", "SHADERS", "DefaultShader", "Transform2D", "load_shader",
           "atmosphere_vertex", "make_frame", "depth_source", "DepthSource", "Lens"]
