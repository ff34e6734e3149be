"""Reduced-resolution draws in numpy (include/atmo_reduced.h states them; no GPU needed to import this), and the ctypes declarations of that header.

A cloud draw at 1 / scale of the resolution along each axis, put into the full-resolution colour buffer by a filter that respects depth edges.  Every
step is stated here in float32, unfused, in a fixed order, and tests/test_reduced_gpu.py holds the kernels to these functions bit for bit:

    low_size(w, h, s)                              (low_w, low_h) = (ceil(w / s), ceil(h / s))
    scratch_layout(w, h, s)                        (floats of the padded low depth, bytes of the whole scratch)
    low_frame(frame, s)                            the frame the low draw is atmo_render's of
    eye_q(frame, px, py, d)                        the reciprocal eye depth of depth d seen through pixel (px, py)
    reduce_depth(frame, depth, s)                  the low depth: one texel of each s x s block, farthest / nearest on a checkerboard
    upsample(frame, depth, low_depth, low_rgba, s, tol)   the full-resolution (rgb, alpha) pixels
    store(pixels, fmt, dst=None, composite=False)  those pixels in a target's format (targets.py), encoded or blended

`frame` is `make_frame`'s dict (inv_projection_matrix column-major, viewport_w, viewport_h); `depth` the DECODED depth (depth_formats.decode), float32
(viewport_h, viewport_w).

The C side: `AtmoReduced`, `REDUCED_ENTRY_POINTS` and `bind`, which declares the four entry points on the library `_native.load()` returns.  The header
is optional -- ATMO_ABI_VERSION stays 5 and the feature is detected by symbol: a library without the symbols makes `bind` raise a RuntimeError that
names the header (`PlanetAtmosphere.render_reduced` then raises it).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import targets as T

SCALES = (2, 4)
HEADER = "atmo_reduced.h"
# every symbol include/atmo_reduced.h declares
REDUCED_ENTRY_POINTS = ("atmo_reduced_size", "atmo_reduced_depth", "atmo_reduced_upsample", "atmo_render_reduced_target")
_F = np.float32


class AtmoReduced(C.Structure):   # include/atmo_reduced.h
    _fields_ = [
        ("scale", C.c_int32),
        ("depth_tolerance", C.c_float),
    ]


def signatures() -> dict:
    """name -> (restype, argtypes) of REDUCED_ENTRY_POINTS, in the tuple's order."""
    from . import _native as N

    vp, ip = C.c_void_p, C.c_int
    frame, depth, target, opt = C.POINTER(N.AtmoFrame), C.POINTER(N.AtmoDepth), C.POINTER(N.AtmoTarget), C.POINTER(AtmoReduced)
    return {
        "atmo_reduced_size": (ip, [ip, ip, ip, C.POINTER(ip), C.POINTER(ip), C.POINTER(C.c_size_t)]),
        "atmo_reduced_depth": (ip, [vp, frame, depth, ip, vp, vp]),
        "atmo_reduced_upsample": (ip, [vp, frame, depth, opt, vp, vp, target, ip, vp]),
        "atmo_render_reduced_target": (ip, [vp, frame, depth, opt, vp, target, ip, vp]),
    }


def bind(lib=None):
    """Declares the entry points of include/atmo_reduced.h on `lib` (default: the library `_native.load()` returns) and returns it; RuntimeError naming
    the header where the library lacks one of them."""
    if lib is None:
        from . import _native as N

        lib = N.load()
    table = signatures()
    assert tuple(table) == REDUCED_ENTRY_POINTS
    for name, (res, args) in table.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError(f"libatmo_hip.so does not export {name} (include/{HEADER}): no reduced-resolution draws; rebuild it")
        fn.restype = res
        fn.argtypes = args
    return lib


# ---- the statement ------------------------------------------------------------------------------------------------------------------------------------

def _scale(s) -> int:
    if s not in SCALES:
        raise ValueError(f"scale must be 2 or 4, not {s!r}")
    return int(s)


def low_size(w: int, h: int, s: int):
    """(low_w, low_h) = (ceil(w / s), ceil(h / s))."""
    s = _scale(s)
    return (int(w) + s - 1) // s, (int(h) + s - 1) // s


def scratch_layout(w: int, h: int, s: int):
    """(floats the low depth takes in the scratch -- low_w * low_h padded to whole 16-byte units --, bytes of the scratch: that, then low_w * low_h float4)."""
    lw, lh = low_size(w, h, s)
    depth_floats = (lw * lh + 3) & ~3
    return depth_floats, 4 * depth_floats + 16 * lw * lh


def low_frame(frame: dict, s: int) -> dict:
    """The low frame: viewport (low_w, low_h), all of it the rect, every other field the caller's but inv_projection_low = inv_projection * A -- A the
    identity with A[0][0] = kx, A[1][1] = ky and the translation column (kx - 1, ky - 1, 0, 1); kx = low_w s / W, ky = low_h s / H (quotients of doubles).
    The centre of low pixel i lies where the centre of its s x s block lies in the full frame.  The product is formed in double -- column 0 = kx M0,
    column 1 = ky M1, column 3 = (M0 (kx - 1) + M1 (ky - 1)) + M3 -- and rounded once per element; kx = ky = 1: the caller's bits untouched."""
    w, h = int(frame["viewport_w"]), int(frame["viewport_h"])
    lw, lh = low_size(w, h, s)
    low = dict(frame)
    low["viewport_w"], low["viewport_h"], low["rect"] = lw, lh, (0, 0, lw, lh)
    m = np.array(frame["inv_projection_matrix"], dtype=np.float32)
    kx, ky = float(lw * s) / float(w), float(lh * s) / float(h)
    if not (kx == 1.0 and ky == 1.0):
        with np.errstate(all="ignore"):
            m64 = m.astype(np.float64)
            out = m64.copy()
            out[0:4] = kx * m64[0:4]
            out[4:8] = ky * m64[4:8]
            out[12:16] = (m64[0:4] * (kx - 1.0) + m64[4:8] * (ky - 1.0)) + m64[12:16]
            m = out.astype(np.float32)
    low["inv_projection_matrix"] = m
    return low


def _ndc(p, size) -> np.ndarray:
    """The draws' NDC of a pixel centre: 2 ((p + 0.5) / size) - 1, one IEEE quotient."""
    return ((np.asarray(p).astype(np.float32) + _F(0.5)) / _F(size)) * _F(2.0) - _F(1.0)


def eye_q(frame: dict, px, py, d) -> np.ndarray:
    """q = w / z of depth `d` through pixel (px, py): z = m[2] nx + m[6] ny + m[10] d + m[14], w = m[3] nx + m[7] ny + m[11] d + m[15], summed left to
    right, m = inv_projection_matrix (column-major).  The reciprocal eye depth: 0 for a reverse-Z sky texel under an infinite far plane."""
    m = np.asarray(frame["inv_projection_matrix"], dtype=np.float32)
    nx, ny = _ndc(px, frame["viewport_w"]), _ndc(py, frame["viewport_h"])
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(all="ignore"):
        z = ((m[2] * nx + m[6] * ny) + m[10] * d) + m[14]
        w = ((m[3] * nx + m[7] * ny) + m[11] * d) + m[15]
        q = w / z
    assert q.dtype == np.float32
    return q


def reduce_depth(frame: dict, depth, s: int, return_index: bool = False):
    """The low depth, float32 (low_h, low_w): low texel (i, j) is the depth, bits untouched, of one texel of the block that exists -- where i + j is even
    the one with the smallest |q| (the farthest), where odd the largest (the nearest).  The block is scanned row-major from its first texel with a strict
    comparison: ties keep the earlier texel and a NaN never replaces the current choice.  return_index: also the chosen texels' (y, x), int (low_h, low_w)
    each."""
    s = _scale(s)
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    assert (w, h) == (int(frame["viewport_w"]), int(frame["viewport_h"]))
    lw, lh = low_size(w, h, s)
    j, i = np.meshgrid(np.arange(lh), np.arange(lw), indexing="ij")
    nearest = ((i + j) & 1) != 0
    best_d = best_q = best_y = best_x = None
    for dy in range(s):
        for dx in range(s):
            x, y = i * s + dx, j * s + dy
            exists = (x < w) & (y < h)
            xs, ys = np.minimum(x, w - 1), np.minimum(y, h - 1)
            d = depth[ys, xs]
            aq = np.abs(eye_q(frame, xs, ys, d))
            if best_d is None:   # the block's first texel always exists
                best_d, best_q, best_y, best_x = d.copy(), aq, ys.copy(), xs.copy()
                continue
            with np.errstate(invalid="ignore"):
                take = exists & np.where(nearest, aq > best_q, aq < best_q)
            best_d = np.where(take, d, best_d)
            best_q = np.where(take, aq, best_q)
            best_y, best_x = np.where(take, ys, best_y), np.where(take, xs, best_x)
    return (best_d, best_y, best_x) if return_index else best_d


def taps(w: int, s: int):
    """One axis of the bilinear footprint for the pixels 0 .. w - 1: (first neighbour clamped, second neighbour clamped, fraction float32).
    t = 2 x + 1 - s, i0 = floor(t / 2 s), f = (t - 2 s i0) / 2 s -- an odd multiple of 1 / 2 s."""
    s = _scale(s)
    n = (int(w) + s - 1) // s
    t = 2 * np.arange(int(w)) + 1 - s
    i0 = np.floor_divide(t, 2 * s)
    f = (t - 2 * s * i0).astype(np.float32) / _F(2 * s)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), f


def upsample(frame: dict, depth, low_depth, low_rgba, s: int, tol, details: bool = False):
    """The full-resolution pixels, float32 (H, W, 4) = (rgb, alpha), from the low frame `low_rgba` (low_h, low_w, 4) and its depth `low_depth`:
    include/atmo_reduced.h, item 5.  details: also a dict of the intermediate values -- `weights` (4, H, W) the bilinear weights in the order 00, 10, 01,
    11, `valid` (4, H, W) the neighbours accumulated (the fallback's one included), `agree` (4, H, W) the depth test alone, `alpha` (4, H, W) the
    neighbours' alphas, `index` (4, H, W, 2) their (j, i)."""
    s = _scale(s)
    depth = np.asarray(depth, dtype=np.float32)
    low_depth = np.asarray(low_depth, dtype=np.float32)
    low_rgba = np.asarray(low_rgba, dtype=np.float32)
    h, w = depth.shape
    lw, lh = low_size(w, h, s)
    assert low_depth.shape == (lh, lw) and low_rgba.shape == (lh, lw, 4)
    tol = _F(tol)
    ia, ib, fx = taps(w, s)
    ja, jb, fy = taps(h, s)
    fx, fy = np.broadcast_to(fx[None, :], (h, w)), np.broadcast_to(fy[:, None], (h, w))
    gx, gy = _F(1.0) - fx, _F(1.0) - fy
    weights = [gx * gy, fx * gy, gx * fy, fx * fy]
    index = [(ja, ia), (ja, ib), (jb, ia), (jb, ib)]
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(all="ignore"):
        q0 = eye_q(frame, x, y, depth)
        diff, agree, texel = [], [], []
        for jj, ii in index:
            qk = eye_q(frame, x, y, low_depth[jj[:, None], ii[None, :]])
            dk = np.abs(q0 - qk)
            diff.append(dk)
            agree.append(dk <= tol * np.fmax(np.abs(q0), np.abs(qk)))
            texel.append(low_rgba[jj[:, None], ii[None, :]])
        none = ~(agree[0] | agree[1] | agree[2] | agree[3])
        best = np.zeros((h, w), dtype=np.int64)       # the closest in depth: strict comparison, the first wins
        best_diff = diff[0]
        for k in range(1, 4):
            closer = diff[k] < best_diff
            best = np.where(closer, k, best)
            best_diff = np.where(closer, diff[k], best_diff)
        valid = [np.where(none, best == k, agree[k]) for k in range(4)]
        wk = [np.where(none, _F(1.0), weights[k]).astype(np.float32) for k in range(4)]
        wsum = np.zeros((h, w), dtype=np.float32)
        a = np.zeros((h, w), dtype=np.float32)
        c = np.zeros((h, w, 3), dtype=np.float32)
        for k in range(4):
            ak = texel[k][..., 3]
            wsum = np.where(valid[k], wsum + wk[k], wsum)
            a = np.where(valid[k], a + wk[k] * ak, a)
            c = np.where(valid[k][..., None], c + wk[k][..., None] * (ak[..., None] * texel[k][..., :3]), c)
        div = wsum != _F(1.0)
        a = np.where(div, a / wsum, a)
        c = np.where(div[..., None], c / wsum[..., None], c)
        has = a > _F(0.0)
        out = np.empty((h, w, 4), dtype=np.float32)
        out[..., :3] = np.where(has[..., None], c / a[..., None], _F(0.0))
        out[..., 3] = a
    assert wsum.dtype == a.dtype == c.dtype == np.float32
    if not details:
        return out
    jj = np.stack([np.broadcast_to(j_[:, None], (h, w)) for j_, _ in index])
    ii = np.stack([np.broadcast_to(i_[None, :], (h, w)) for _, i_ in index])
    return out, dict(weights=np.stack(weights), valid=np.stack(valid), agree=np.stack(agree), alpha=np.stack([t[..., 3] for t in texel]),
                     index=np.stack([jj, ii], axis=-1))


def store(pixels, fmt, dst=None, composite: bool = False) -> np.ndarray:
    """What the upsample leaves in a target of format `fmt` (targets.py's names or values), as a (H, W, 4) array of the format's dtype: plain, every pixel
    encoded; composite, `dst` with the pixels whose alpha > 0 blended in (decode, blend_mix, one encode) and all others untouched."""
    f = T.format_id(fmt)
    pixels = np.asarray(pixels, dtype=np.float32)
    if not composite:
        return T.encode(pixels, f)
    dst = np.asarray(dst)
    blended = T.blend(pixels, dst, f)
    return np.where((pixels[..., 3] > _F(0.0))[..., None], blended, dst)
