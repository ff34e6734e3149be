"""Sky images in numpy (include/atmo_sky_image.h states them; no GPU needed to import this), and the ctypes declarations of that header.

The resolve of a lens's shaded rays -- tight float4 rows in ray order -- into an image of a target format, and that image's mip chain, each operation in
the header's order; tests/test_sky_image_gpu.py holds the kernels to these functions bit for bit:

    resolve(lens, rgba, fmt, quads=False, premultiplied=False, dst=None)   the band's rows (rows, W, 4) as stored; dst: composite onto these rows
    mip_level(buf, fmt)                     the next level of (..., h, w, 4) stored texels: (..., max(1, h // 2), max(1, w // 2), 4)
    mip_chain(buf, fmt, n_levels)           [buf, its next level, ...]: n_levels arrays, each computed from the stored bits of the one before
    level_count(w, h)                       the full chain's length, 1 + floor(log2(max(w, h)))

Formats, encode, decode and blend are targets.py's (include/atmo_target.h); a lens's absent pixels lens.py's; the quad order ray_quads.quad_order.

The C side: `AtmoSkyLevel`, `SKY_IMAGE_ENTRY_POINTS`, `signatures` and `bind`, which declares the three entry points on the library `_native.load()`
returns.  The header is optional -- ATMO_ABI_VERSION stays 5 and the feature is detected by symbol: a library without the symbols makes `bind` raise a
RuntimeError that names the header (`PlanetAtmosphere.resolve_lens`, `sky_image_mips` and `render_sky_image` then raise it).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lens as L
from . import targets as T
from .ray_quads import quad_order

HEADER = "atmo_sky_image.h"
# every symbol include/atmo_sky_image.h declares
SKY_IMAGE_ENTRY_POINTS = ("atmo_sky_image_resolve", "atmo_sky_image_level_count", "atmo_sky_image_mips")
QUADS, PREMULTIPLIED, COMPOSITE = L.LENS_QUADS, 2, 4     # ATMO_LENS_QUADS, ATMO_SKY_IMAGE_PREMULTIPLIED, ATMO_SKY_IMAGE_COMPOSITE
MAX_SIDE, MAX_LAYERS, MAX_TEXELS = 65536, 4096, 1 << 30
LEVELS_PER_LAUNCH = 5                                    # a call is ceil((n_levels - 1) / 5) launches
_F = np.float32


class AtmoSkyLevel(C.Structure):   # include/atmo_sky_image.h: 24 bytes
    _fields_ = [
        ("pixels", C.c_void_p),
        ("row_pitch_bytes", C.c_int32),
        ("reserved", C.c_int32),
        ("layer_pitch_bytes", C.c_int64),
    ]


def signatures() -> dict:
    """name -> (restype, argtypes) of SKY_IMAGE_ENTRY_POINTS, in the tuple's order."""
    from . import _native as N

    vp, ip = C.c_void_p, C.c_int
    return {
        "atmo_sky_image_resolve": (ip, [vp, C.POINTER(N.AtmoLens), C.c_uint32, vp, C.POINTER(N.AtmoTarget), vp]),
        "atmo_sky_image_level_count": (ip, [ip, ip, C.POINTER(ip)]),
        "atmo_sky_image_mips": (ip, [vp, C.POINTER(AtmoSkyLevel), ip, ip, ip, ip, ip, vp]),
    }


def bind(lib=None):
    """Declares the entry points of include/atmo_sky_image.h on `lib` (default: the library `_native.load()` returns) and returns it; RuntimeError naming
    the header where the library lacks one of them."""
    if lib is None:
        from . import _native as N

        lib = N.load()
    table = signatures()
    assert tuple(table) == SKY_IMAGE_ENTRY_POINTS
    for name, (res, args) in table.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError(f"libatmo_hip.so does not export {name} (include/{HEADER}): no sky images; rebuild it")
        fn.restype = res
        fn.argtypes = args
    return lib


# ---- the statement ------------------------------------------------------------------------------------------------------------------------------------

def level_count(w: int, h: int) -> int:
    """atmo_sky_image_level_count: 1 + floor(log2(max(w, h)))."""
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError("width and height must lie in 1 .. 65536")
    return max(int(w), int(h)).bit_length()


def level_size(w: int, h: int, level: int):
    """(w_l, h_l) = (max(1, w >> l), max(1, h >> l))."""
    return max(1, int(w) >> level), max(1, int(h) >> level)


def slots(lens, quads: bool = False):
    """(slot, present): for every pixel of the lens's band, row-major (rows * W,), the ray slot THE RESOLVE reads, and whether the pixel is present."""
    y0, y1 = lens.rows
    rows, w = y1 - y0, lens.width
    i = np.arange(rows * w, dtype=np.int64)
    x, y = i % w, y0 + i // w
    _, absent = L.lens_directions(lens, x, y)
    if not quads:
        return i, ~absent
    lens.check_quads()
    order = quad_order(w, rows)                     # slot -> pixel of the band: Q is counted inside the band
    inside = np.nonzero(order >= 0)[0]
    slot = np.empty(rows * w, dtype=np.int64)
    slot[order[inside]] = inside
    return slot, ~absent


def resolve(lens, rgba, fmt, quads: bool = False, premultiplied: bool = False, dst=None) -> np.ndarray:
    """What atmo_sky_image_resolve leaves in the rows [y0, y1) of the target: (rows, W, 4) in the format's dtype.  `rgba`: float32 (n_rays, 4), the rows of
    lens.lens_rays(lens, quads)'s slots.  Plain (dst None): a present pixel is encode(rgba row), or of (r a, g a, b a, a) when `premultiplied`; an absent
    pixel is all-zero bits.  `dst` (the rows' stored texels before the call, (rows, W, 4)): ATMO_SKY_IMAGE_COMPOSITE -- a present pixel with a > 0 becomes
    targets.blend(row, dst pixel), every other pixel keeps dst's bytes.  The rows of absent pixels, and of slots outside the image, are not read."""
    f = T.format_id(fmt)
    if premultiplied and dst is not None:
        raise ValueError("premultiplied together with a composite (the blend multiplies by alpha itself)")
    rgba = np.asarray(rgba, dtype=np.float32)
    y0, y1 = lens.rows
    rows, w = y1 - y0, lens.width
    if rgba.shape != (lens.counts(quads)[0], 4):
        raise ValueError(f"rgba must have shape ({lens.counts(quads)[0]}, 4)")
    slot, present = slots(lens, quads)
    src = np.where(present[:, None], rgba[np.where(present, slot, 0)], _F(0.0)).astype(_F)
    with np.errstate(all="ignore"):
        if dst is None:
            if premultiplied:
                src = np.concatenate([src[:, :3] * src[:, 3:4], src[:, 3:4]], axis=1)
            assert src.dtype == np.float32
            out = T.encode(src, f).reshape(rows * w, 4)
            out[~present] = 0                       # (0, 0, 0, 0) is all-zero bits in every format
            return out.reshape(rows, w, 4)
        dst = np.asarray(dst)
        if dst.shape != (rows, w, 4) or dst.dtype != T.DTYPES[f]:
            raise ValueError(f"dst must be a ({rows}, {w}, 4) {np.dtype(T.DTYPES[f]).name} array")
        flat = dst.reshape(rows * w, 4)
        blend = present & (src[:, 3] > 0)           # a > 0 is false for 0, negatives and NaN
        out = flat.copy()
        out[blend] = T.blend(src[blend], flat[blend], f)
        return out.reshape(rows, w, 4)


def mip_level(buf, fmt) -> np.ndarray:
    """The next level of the stored texels `buf` (..., h, w, 4): per channel encode(((t00 + t10) + (t01 + t11)) * 0.25), every operation a float32 one, t_ab
    the decoded texel (min(2 i + a, w - 1), min(2 j + b, h - 1)).  Leading axes are layers, each on its own."""
    f = T.format_id(fmt)
    b = np.asarray(buf)
    if b.ndim < 3 or b.shape[-1] != 4:
        raise ValueError("a level is (..., h, w, 4) stored texels")
    h, w = b.shape[-3], b.shape[-2]
    t = T.decode(b, f)
    i, j = np.arange(max(1, w >> 1)), np.arange(max(1, h >> 1))
    xa, xb = np.minimum(2 * i, w - 1), np.minimum(2 * i + 1, w - 1)
    ya, yb = np.minimum(2 * j, h - 1)[:, None], np.minimum(2 * j + 1, h - 1)[:, None]
    with np.errstate(all="ignore"):
        v = ((t[..., ya, xa, :] + t[..., ya, xb, :]) + (t[..., yb, xa, :] + t[..., yb, xb, :])) * _F(0.25)
    assert v.dtype == np.float32
    return T.encode(v, f)


def mip_chain(buf, fmt, n_levels: int) -> list:
    """[level 0 = buf, level 1, ...], n_levels arrays: each level from the stored bits of the one before."""
    b = np.asarray(buf)
    if not 1 <= n_levels <= level_count(b.shape[-2], b.shape[-3]):
        raise ValueError("n_levels must lie in 1 .. level_count(w, h)")
    chain = [b]
    for _ in range(n_levels - 1):
        chain.append(mip_level(chain[-1], fmt))
    return chain
