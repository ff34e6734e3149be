"""The sky as light in numpy (include/atmo_sky_sh.h states it; no GPU needed to import this), and the ctypes declarations of that header.

The solid angle of every pixel of a lens image (lens.Lens) and the projection of shaded rays onto the nine real spherical harmonics of bands 0 to 2, each
sum in the header's fixed order; tests/test_sky_sh_gpu.py holds the kernels to these functions, the projection and the two float32 lenses bit for bit:

    solid_angles(lens, quads=False)                    one float32 per slot of lens.lens_rays(lens, quads): steradians, +0 for an absent slot
    sh9_basis(dirs)                                    (n, 9) float32: the header's BASIS, operation for operation
    sh9_project(dirs, rgba, weights=None, prev=None)   the 40 floats of atmo_sky_sh9 in THE ORDER OF THE SUMS, tree included; prev: ACCUMULATE onto it
    sh9_project64(dirs, rgba, weights=None, prev=None) the same sums in float64 from the same float32 inputs, and sum |t| per output
    sh9_error_bound(n_rays, magnitude, calls=1)        how far sh9_project may lie from sh9_project64
    sh9_eval(sh, dirs)                                 the band-limited radiance along `dirs`, float64 (n, 4)
    sh9_irradiance(sh, normals)                        the irradiance on surfaces with these normals, float64 (n, 4)

LANES, RAYS_PER_LANE and FLOATS are read out of the header's text: the one place THE ORDER OF THE SUMS keeps its constants (the library asserts at compile
time that its kernels use the same).

The C side: `SKY_SH_ENTRY_POINTS`, `signatures` and `bind`, which declares the three entry points on the library `_native.load()` returns.  The header is
optional -- ATMO_ABI_VERSION stays 5 and the feature is detected by symbol: a library without the symbols makes `bind` raise a RuntimeError that names
the header (`PlanetAtmosphere.lens_solid_angles`, `project_sh9` and `ambient_sh9` then raise it).
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from . import lens as L

HEADER = "atmo_sky_sh.h"
# every symbol include/atmo_sky_sh.h declares
SKY_SH_ENTRY_POINTS = ("atmo_lens_solid_angles", "atmo_sky_sh9_scratch_bytes", "atmo_sky_sh9")
_F = np.float32


def _header_constants() -> dict:
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", HEADER)).read()
    return {name: int(value) for name, value in re.findall(r"^#define ATMO_SKY_SH_([A-Z_]+) (\d+)u?\b", text, flags=re.M)}


_K = _header_constants()
ACCUMULATE = _K["ACCUMULATE"]                # ATMO_SKY_SH_ACCUMULATE
LANES, RAYS_PER_LANE, FLOATS = _K["LANES"], _K["RAYS_PER_LANE"], _K["FLOATS"]
SEGMENT = LANES * RAYS_PER_LANE              # consecutive rays of one workgroup
SUMS = 37                                    # 9 coefficients x rgba, and the weights' sum
MAX_RAYS = 1 << 28
# BASIS: the floats nearest these decimals
Y0, C1, C2, C20, C22 = _F(0.28209479), _F(0.48860251), _F(1.0925484), _F(0.31539157), _F(0.54627422)
assert LANES & (LANES - 1) == 0 and FLOATS >= SUMS


def signatures() -> dict:
    """name -> (restype, argtypes) of SKY_SH_ENTRY_POINTS, in the tuple's order."""
    from . import _native as N

    vp, ip, u32 = C.c_void_p, C.c_int, C.c_uint32
    return {
        "atmo_lens_solid_angles": (ip, [vp, C.POINTER(N.AtmoLens), u32, vp, vp]),
        "atmo_sky_sh9_scratch_bytes": (ip, [u32, C.POINTER(C.c_size_t)]),
        "atmo_sky_sh9": (ip, [vp, vp, vp, vp, u32, u32, vp, C.c_size_t, vp, vp]),
    }


def bind(lib=None):
    """Declares the entry points of include/atmo_sky_sh.h on `lib` (default: the library `_native.load()` returns) and returns it; RuntimeError naming
    the header where the library lacks one of them."""
    if lib is None:
        from . import _native as N

        lib = N.load()
    table = signatures()
    assert tuple(table) == SKY_SH_ENTRY_POINTS
    for name, (res, args) in table.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError(f"libatmo_hip.so does not export {name} (include/{HEADER}): no sky ambient light; rebuild it")
        fn.restype = res
        fn.argtypes = args
    return lib


def segments(n_rays: int) -> int:
    return (int(n_rays) + SEGMENT - 1) // SEGMENT


def scratch_bytes(n_rays: int) -> int:
    """atmo_sky_sh9_scratch_bytes: FLOATS floats per segment."""
    if not 0 <= n_rays <= MAX_RAYS:
        raise ValueError("n_rays must lie in 0 .. 2^28")
    return 4 * FLOATS * segments(n_rays)


# ---- solid angles ---------------------------------------------------------------------------------------------------------------------------------------

def _octahedral(lens, x, y):
    with np.errstate(all="ignore"):   # n as lens._octahedral forms it
        u = (2 * x + 1).astype(_F) / _F(lens.width) - _F(1.0)
        v = (2 * y + 1).astype(_F) / _F(lens.height) - _F(1.0)
        z = (_F(1.0) - np.abs(u)) - np.abs(v)
        a = np.where(z < 0, np.copysign(_F(1.0) - np.abs(v), u), u)
        b = np.where(z < 0, np.copysign(_F(1.0) - np.abs(u), v), v)
        n = np.sqrt((a * a + b * b) + z * z)
        w = ((_F(4.0) / _F(lens.width)) / _F(lens.height)) / ((n * n) * n)
    assert w.dtype == np.float32
    return w


def _cube_face(lens, x, y):
    n = lens.width                     # h and len as lens._cube_face forms them
    half = _F(0.5) * _F(n)
    p = (x.astype(_F) + _F(0.5)) / half - _F(1.0)
    q = ((n - y - 1).astype(_F) + _F(0.5)) / half - _F(1.0)
    vx, vy, vz = np.ones_like(p), q, -p
    length = np.sqrt((vx * vx + vy * vy) + vz * vz)
    w = ((_F(1.0) / half) / half) / ((length * length) * length)
    assert w.dtype == np.float32
    return w


def _equirect(lens, x, y):
    theta = (0.5 - (y + 0.5) / float(lens.height)) * np.pi
    w = (((2.0 * np.pi) / float(lens.width)) * (np.pi / float(lens.height))) * np.cos(theta)
    return np.where(w > 0.0, w, 0.0).astype(_F)


def _fisheye(lens, x, y):
    w_, h_ = lens.width, lens.height
    px, py = (x + 0.5) - w_ / 2.0, h_ / 2.0 - (y + 0.5)
    rho = np.sqrt(px * px + py * py)
    k = (float(lens.fov) / 2.0) / (min(w_, h_) / 2.0)
    theta = (rho / (min(w_, h_) / 2.0)) * (float(lens.fov) / 2.0)
    w = np.where(rho == 0.0, k * k, (k * np.sin(theta)) / np.where(rho == 0.0, 1.0, rho))
    return np.where(w > 0.0, w, 0.0).astype(_F)


_SOLID_ANGLES = {L.EQUIRECT: _equirect, L.FISHEYE: _fisheye, L.OCTAHEDRAL: _octahedral, L.CUBE_FACE: _cube_face}


def solid_angles(lens, quads: bool = False) -> np.ndarray:
    """What atmo_lens_solid_angles writes for the lens's band: float32 (n_rays,), the solid angle in steradians of the pixel in each slot of
    lens.lens_rays(lens, quads), +0 for an absent slot.  OCTAHEDRAL and CUBE_FACE are float32 operation for operation; EQUIRECT and FISHEYE are float64
    numpy rounded once, which the device meets within 1 float32 ulp."""
    x, y, inside = L._pixels(lens, quads)
    xi, yi = np.where(inside, x, 0), np.where(inside, y, 0)
    _, absent = L.lens_directions(lens, xi, yi)
    w = _SOLID_ANGLES[lens.kind](lens, xi, yi)
    return np.where(inside & ~absent, w, _F(0.0)).astype(_F)


# ---- the projection -------------------------------------------------------------------------------------------------------------------------------------

def _dirs(dirs, dtype):
    d = np.asarray(dirs, dtype=np.float32)
    if d.ndim != 2 or d.shape[1] not in (3, 8):
        raise ValueError("dirs must have shape (n, 3), or (n, 8): AtmoRay rows")
    return (d[:, 4:7] if d.shape[1] == 8 else d).astype(dtype)


def _basis(d, c3):
    """BASIS on the columns of d, in d's dtype; c3 is that dtype's 3."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    k = d.dtype.type
    with np.errstate(all="ignore"):
        return np.stack([np.full_like(x, k(Y0)), k(C1) * y, k(C1) * z, k(C1) * x, k(C2) * (x * y), k(C2) * (y * z), k(C20) * (c3 * (z * z) - k(1.0)),
                         k(C2) * (x * z), k(C22) * (x * x - y * y)], axis=1)


def sh9_basis(dirs) -> np.ndarray:
    """The header's BASIS of the directions `dirs` ((n, 3), or AtmoRay rows (n, 8)) as given: float32 (n, 9), every operation rounded on its own."""
    out = _basis(_dirs(dirs, np.float32), _F(3.0))
    assert out.dtype == np.float32
    return out


def _terms(dirs, rgba, weights, dtype):
    """(n, SUMS) terms in `dtype` from the float32 inputs: t[k][ch] = (w Y_k) c_ch and w; zero rows where w == 0, whatever the other inputs hold."""
    d = _dirs(dirs, dtype)
    rgba = np.asarray(rgba, dtype=np.float32)
    n = d.shape[0]
    if rgba.shape != (n, 4):
        raise ValueError("rgba must have shape (n, 4)")
    w = np.ones(n, dtype=dtype) if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1).astype(dtype)
    if w.shape != (n,):
        raise ValueError("weights must have shape (n,)")
    live = w != 0
    with np.errstate(all="ignore"):
        px = rgba.astype(dtype)
        c = np.concatenate([px[:, :3] * px[:, 3:4], px[:, 3:4]], axis=1)
        wy = w[:, None] * _basis(d, dtype(3.0))
        t = np.concatenate([(wy[:, :, None] * c[:, None, :]).reshape(n, 36), w[:, None]], axis=1)
    assert t.dtype == dtype
    return np.where(live[:, None], t, dtype(0.0))


def _tree(v):
    """THE TREE over axis 1 (LANES values): v[t] = v[t] + v[t + s], s = LANES / 2 .. 1."""
    s = LANES // 2
    while s >= 1:
        v = v[:, :s] + v[:, s:2 * s]
        s //= 2
    return v[:, 0]


def _lane_sums(t, per_lane):
    """t: (groups * per_lane * LANES, SUMS), group-major; lane l of a group adds its rows l, l + LANES, ... in order, from +0."""
    t = t.reshape(-1, per_lane, LANES, SUMS)
    v = np.zeros((t.shape[0], LANES, SUMS), dtype=t.dtype)
    for j in range(per_lane):
        v = v + t[:, j]
    return v


def _pad(t, multiple):
    rows = -(-max(t.shape[0], 1) // multiple) * multiple
    return np.concatenate([t, np.zeros((rows - t.shape[0], SUMS), dtype=t.dtype)]) if rows != t.shape[0] else t


def sh9_project(dirs, rgba, weights=None, prev=None) -> np.ndarray:
    """The FLOATS floats atmo_sky_sh9 leaves in `out_dev`, in float32 and in THE ORDER OF THE SUMS: out[4 k + ch] the coefficient of Y_k in channel ch,
    out[36] the weights' sum, then +0.  `prev`: the floats `out_dev` held, under ATMO_SKY_SH_ACCUMULATE.  (A sum never holds -0, so the +0 this adds in the
    place of a ray that is skipped leaves every bit as it is.)"""
    dirs, rgba = np.asarray(dirs, dtype=np.float32), np.asarray(rgba, dtype=np.float32)
    weights = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
    n = _dirs(dirs, np.float32).shape[0]
    if rgba.shape != (n, 4) or (weights is not None and weights.shape != (n,)):
        raise ValueError("rgba must have shape (n, 4) and weights (n,)")
    out = np.zeros(FLOATS, dtype=np.float32)
    if n:
        with np.errstate(all="ignore"):
            partial = np.concatenate([_tree(_lane_sums(_pad(_terms(dirs[a:a + 64 * SEGMENT], rgba[a:a + 64 * SEGMENT],
                                                                   None if weights is None else weights[a:a + 64 * SEGMENT], np.float32), SEGMENT),
                                                       RAYS_PER_LANE)) for a in range(0, n, 64 * SEGMENT)])
            assert partial.shape == (segments(n), SUMS)
            padded = _pad(partial, LANES)
            out[:SUMS] = _tree(_lane_sums(padded, padded.shape[0] // LANES))[0]
    elif prev is not None:
        return np.array(prev, dtype=np.float32)
    if prev is not None:
        prev = np.asarray(prev, dtype=np.float32)
        with np.errstate(all="ignore"):
            out[:SUMS] = prev[:SUMS] + out[:SUMS]
    assert out.dtype == np.float32
    return out


def sh9_project64(dirs, rgba, weights=None, prev=None):
    """(the sums of sh9_project in float64 -- every term formed in float64 from the same float32 inputs and constants --, sum |t| per output), both float64
    (FLOATS,).  `prev`: an earlier call's pair, added to both."""
    t = _terms(dirs, rgba, weights, np.float64)
    total, magnitude = np.zeros(FLOATS), np.zeros(FLOATS)
    with np.errstate(all="ignore"):
        total[:SUMS], magnitude[:SUMS] = t.sum(axis=0), np.abs(t).sum(axis=0)
    if prev is not None:
        total, magnitude = total + np.asarray(prev[0], dtype=np.float64), magnitude + np.asarray(prev[1], dtype=np.float64)
    return total, magnitude


def sh9_error_bound(n_rays: int, magnitude, calls: int = 1) -> np.ndarray:
    """How far sh9_project may lie from sh9_project64, per output: (16 + 8 + ceil(S / 256) + 8 + calls + 6) * 2^-24 * sum |t| * 1.01, S the segments of
    the longest call.  Every addition of THE ORDER OF THE SUMS rounds a value that no partial sum of |t| exceeds: RAYS_PER_LANE in a lane, log2(LANES) in
    the tree, ceil(S / LANES) and the tree once more in the second launch, one per call under ACCUMULATE; a term carries six roundings (at most four in
    Y_k, w Y_k, the product with c) -- to first order, 1.01 holding the rest.  (RN(r a) is a seventh for the colour channels, and Y6 and Y8 round before
    they cancel; both are far inside what the additions' share leaves unused whenever a sum has more than a few terms.)"""
    depth = RAYS_PER_LANE + (LANES.bit_length() - 1) + -(-segments(n_rays) // LANES) + (LANES.bit_length() - 1) + int(calls) + 6
    return depth * 2.0 ** -24 * np.asarray(magnitude, dtype=np.float64) * 1.01


_BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
_COSINE_LOBE = np.array([np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0])       # the clamped cosine's zonal factors of bands 0, 1, 2


def _unit64(dirs):
    d = _dirs(dirs, np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def sh9_eval(sh, dirs) -> np.ndarray:
    """The band-limited function the coefficients `sh` (FLOATS or 36 floats) describe, along `dirs` (normalised here): float64 (n, 4)."""
    coeff = np.asarray(sh, dtype=np.float64)[:36].reshape(9, 4)
    return _basis(_unit64(dirs), 3.0) @ coeff


def sh9_irradiance(sh, normals) -> np.ndarray:
    """The irradiance (per channel; the alpha column: the covered share of the cosine lobe, times pi) on a surface with each of `normals`, float64
    (n, 4): the coefficients scaled by the cosine lobe's pi, 2 pi / 3 and pi / 4 per band, then evaluated."""
    coeff = np.asarray(sh, dtype=np.float64)[:36].reshape(9, 4) * _COSINE_LOBE[_BAND][:, None]
    return _basis(_unit64(normals), 3.0) @ coeff
