"""Temporal draws in numpy (include/atmo_temporal.h states them; no GPU needed to import this), and the ctypes declarations of that header.

One pixel of every scale x scale block is marched a frame; the others come from the last frame's result, reprojected, and from reduced.py's spatial
filter where that history is gone.  Every step is stated here in float32, unfused, in a fixed order, and tests/test_temporal_gpu.py holds the kernels to
these functions bit for bit:

    phase_offset(s, p)                     (ox, oy) = (p mod s, p div s)
    phase_sequence(s)                      the Bayer order of the phases: atmo_temporal_phase(s, f) for f = 0 .. s^2 - 1
    phase_frame(frame, s, p)               the frame the low draw of phase p is atmo_render's of
    phase_depth(depth, s, p)               the low depth: the texel under the phase's pixel of every block
    history_layout(w, h)                   (byte offset of q, byte offset of the ages, bytes of one history buffer)
    pack_history / unpack_history          (rgba, q, age) <-> the buffer's bytes
    prev_clip_from_view(frame, prev_camera)   previous projection x previous view x current inverse view, float64, rounded once
    resolve(...)                           the full-resolution pixels, their q and their ages; details=True: the path every pixel took

`frame` is `make_frame`'s dict; `depth` the DECODED depth, float32 (H, W); a history is the tuple (rgba (H, W, 4) float32, q (H, W) float32, age (H, W)
uint8).

The C side: `AtmoTemporal`, `TEMPORAL_ENTRY_POINTS`, `signatures` and `bind`, in reduced.py's pattern -- ATMO_ABI_VERSION stays 5, the feature is detected
by symbol, and a library without the symbols makes `bind` raise a RuntimeError that names the header.  `TemporalHistory` is what
`PlanetAtmosphere.render_temporal` keeps between frames."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import reduced as R
from .scene import col_major

SCALES = R.SCALES
HEADER = "atmo_temporal.h"
# every symbol include/atmo_temporal.h declares
TEMPORAL_ENTRY_POINTS = ("atmo_temporal_size", "atmo_temporal_phase", "atmo_temporal_depth", "atmo_temporal_resolve", "atmo_render_temporal_target")
FRESH, SNAP, BILINEAR, FALLBACK = 0, 1, 2, 3      # resolve's path labels
PATHS = ("fresh", "snap", "bilinear", "fallback")
NOT_HISTORY, OLDEST = 255, 254                    # the age of a pixel the spatial filter made; where a reused pixel's age saturates
SNAP_RADIUS = 1.0 / 64.0
_ORDER = {2: (0, 3, 1, 2), 4: (0, 10, 2, 8, 5, 15, 7, 13, 1, 11, 3, 9, 4, 14, 6, 12)}
_F = np.float32


class AtmoTemporal(C.Structure):   # include/atmo_temporal.h
    _fields_ = [
        ("scale", C.c_int32),
        ("phase", C.c_int32),
        ("depth_tolerance", C.c_float),
        ("history_tolerance", C.c_float),
        ("max_age", C.c_int32),
        ("reset", C.c_int32),
        ("prev_clip_from_view", C.c_float * 16),
        ("prev_inv_projection", C.c_float * 16),
    ]


def options(scale, phase, depth_tolerance=0.1, history_tolerance=0.1, max_age=None, reset=False, prev_clip=None, prev_inv_projection=None) -> AtmoTemporal:
    """An AtmoTemporal; max_age None: 2 scale^2; the matrices None: zeros (a reset reads neither)."""
    opt = AtmoTemporal(int(scale), int(phase), float(depth_tolerance), float(history_tolerance), int(2 * scale * scale if max_age is None else max_age),
                       int(bool(reset)))
    for name, m in (("prev_clip_from_view", prev_clip), ("prev_inv_projection", prev_inv_projection)):
        if m is not None:
            getattr(opt, name)[:] = [float(v) for v in np.asarray(m, dtype=np.float32).reshape(16)]
    return opt


def signatures() -> dict:
    """name -> (restype, argtypes) of TEMPORAL_ENTRY_POINTS, in the tuple's order."""
    from . import _native as N

    vp, ip = C.c_void_p, C.c_int
    frame, depth, target, opt = C.POINTER(N.AtmoFrame), C.POINTER(N.AtmoDepth), C.POINTER(N.AtmoTarget), C.POINTER(AtmoTemporal)
    return {
        "atmo_temporal_size": (ip, [ip, ip, ip, C.POINTER(ip), C.POINTER(ip), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "atmo_temporal_phase": (ip, [ip, ip]),
        "atmo_temporal_depth": (ip, [vp, frame, depth, ip, ip, vp, vp]),
        "atmo_temporal_resolve": (ip, [vp, frame, depth, opt, vp, vp, vp, vp, target, ip, vp]),
        "atmo_render_temporal_target": (ip, [vp, frame, depth, opt, vp, vp, vp, target, ip, vp]),
    }


def bind(lib=None):
    """Declares the entry points of include/atmo_temporal.h on `lib` (default: the library `_native.load()` returns) and returns it; RuntimeError naming
    the header where the library lacks one of them."""
    if lib is None:
        from . import _native as N

        lib = N.load()
    table = signatures()
    assert tuple(table) == TEMPORAL_ENTRY_POINTS
    for name, (res, args) in table.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError(f"libatmo_hip.so does not export {name} (include/{HEADER}): no temporal draws; rebuild it")
        fn.restype = res
        fn.argtypes = args
    return lib


# ---- the statement ------------------------------------------------------------------------------------------------------------------------------------

def _scale(s) -> int:
    if s not in SCALES:
        raise ValueError(f"scale must be 2 or 4, not {s!r}")
    return int(s)


def phase_offset(s: int, p: int):
    """(ox, oy) = (p mod s, p div s): the texel of every block that phase p marches."""
    s = _scale(s)
    if not 0 <= int(p) < s * s:
        raise ValueError(f"phase must be 0 .. {s * s - 1}, not {p!r}")
    return int(p) % s, int(p) // s


def phase_sequence(s: int):
    """The phases in the order of the s x s Bayer matrix: consecutive frames are far apart in the block; every phase once."""
    return _ORDER[_scale(s)]


def phase_of_frame(s: int, frame_index: int) -> int:
    """atmo_temporal_phase: the sequence at frame_index mod s^2 (the non-negative remainder)."""
    seq = phase_sequence(s)
    return seq[int(frame_index) % len(seq)]


def phase_frame(frame: dict, s: int, p: int) -> dict:
    """reduced.low_frame with one more term in the translation: the centre of low pixel i lies on the centre of full pixel i s + ox.  Column 0 = kx M0,
    column 1 = ky M1, column 3 = (M0 tx + M1 ty) + M3, tx = (kx - 1) + (2 ox + 1 - s) / W, ty = (ky - 1) + (2 oy + 1 - s) / H, in double, rounded once."""
    ox, oy = phase_offset(s, p)
    w, h = int(frame["viewport_w"]), int(frame["viewport_h"])
    lw, lh = R.low_size(w, h, s)
    low = dict(frame)
    low["viewport_w"], low["viewport_h"], low["rect"] = lw, lh, (0, 0, lw, lh)
    m64 = np.array(frame["inv_projection_matrix"], dtype=np.float32).astype(np.float64)
    kx, ky = float(lw * s) / float(w), float(lh * s) / float(h)
    tx = (kx - 1.0) + float(2 * ox + 1 - s) / float(w)
    ty = (ky - 1.0) + float(2 * oy + 1 - s) / float(h)
    with np.errstate(all="ignore"):
        out = m64.copy()
        out[0:4] = kx * m64[0:4]
        out[4:8] = ky * m64[4:8]
        out[12:16] = (m64[0:4] * tx + m64[4:8] * ty) + m64[12:16]
        low["inv_projection_matrix"] = out.astype(np.float32)
    return low


def phase_depth(depth, s: int, p: int) -> np.ndarray:
    """The low depth, float32 (low_h, low_w): low texel (i, j) is the depth, bits untouched, of texel (min(i s + ox, W - 1), min(j s + oy, H - 1))."""
    ox, oy = phase_offset(s, p)
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    lw, lh = R.low_size(w, h, s)
    x, y = np.minimum(np.arange(lw) * s + ox, w - 1), np.minimum(np.arange(lh) * s + oy, h - 1)
    return depth[y[:, None], x[None, :]].copy()


def _pad16(n: int) -> int:
    return (n + 15) & ~15


def history_layout(w: int, h: int):
    """(byte offset of the q part, byte offset of the ages, bytes of a history buffer): W H float4, W H float, W H uint8, each padded to 16 bytes."""
    n = int(w) * int(h)
    return 16 * n, 16 * n + _pad16(4 * n), 16 * n + _pad16(4 * n) + _pad16(n)


def pack_history(rgba, q, age, fill: int = 0) -> np.ndarray:
    """The bytes of a history buffer (padding = `fill`)."""
    h, w = np.asarray(q).shape
    oq, oa, total = history_layout(w, h)
    buf = np.full(total, fill, dtype=np.uint8)
    buf[:16 * w * h] = np.ascontiguousarray(rgba, dtype=np.float32).reshape(-1).view(np.uint8)
    buf[oq:oq + 4 * w * h] = np.ascontiguousarray(q, dtype=np.float32).reshape(-1).view(np.uint8)
    buf[oa:oa + w * h] = np.ascontiguousarray(age, dtype=np.uint8).reshape(-1)
    return buf


def unpack_history(buf, w: int, h: int):
    """(rgba, q, age) of a history buffer's bytes."""
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    oq, oa, total = history_layout(w, h)
    assert buf.size >= total
    n = w * h
    return (buf[:16 * n].copy().view(np.float32).reshape(h, w, 4), buf[oq:oq + 4 * n].copy().view(np.float32).reshape(h, w),
            buf[oa:oa + n].copy().reshape(h, w))


def prev_clip_from_view(frame: dict, prev_camera) -> np.ndarray:
    """AtmoTemporal::prev_clip_from_view for the current `frame` and the previous frame's camera: previous projection x previous view x current inverse
    view (the frame's float32 one), formed in float64 and rounded once; column-major float32 (16,)."""
    inv_view = np.asarray(frame["inv_view_matrix"], dtype=np.float32).astype(np.float64).reshape(4, 4).T
    return col_major(np.asarray(prev_camera.projection, dtype=np.float64) @ np.asarray(prev_camera.view, dtype=np.float64) @ inv_view)


def view_point(frame: dict, depth):
    """Item 5's V (4, H, W) = inv_projection (nx, ny, d0, 1), each row summed left to right, undivided, and q0 = V[3] / V[2]."""
    m = np.asarray(frame["inv_projection_matrix"], dtype=np.float32)
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    nx = np.broadcast_to(R._ndc(np.arange(w), w)[None, :], (h, w))
    ny = np.broadcast_to(R._ndc(np.arange(h), h)[:, None], (h, w))
    with np.errstate(all="ignore"):
        v = np.stack([((m[r] * nx + m[4 + r] * ny) + m[8 + r] * depth) + m[12 + r] for r in range(4)])
        q0 = v[3] / v[2]
    assert v.dtype == q0.dtype == np.float32
    return v, q0


def reproject(frame: dict, depth, prev_clip, prev_inv_projection):
    """Item 5b: (front, fpx, fpy, qe) of every pixel -- whether C[3] > 0, the previous frame's pixel position, the expected reciprocal eye depth."""
    p = np.asarray(prev_clip, dtype=np.float32).reshape(16)
    r_ = np.asarray(prev_inv_projection, dtype=np.float32).reshape(16)
    v, _ = view_point(frame, depth)
    h, w = v.shape[1:]
    with np.errstate(all="ignore"):
        c = [((p[r] * v[0] + p[4 + r] * v[1]) + p[8 + r] * v[2]) + p[12 + r] * v[3] for r in range(4)]
        front = c[3] > _F(0.0)
        u, vv, dp = c[0] / c[3], c[1] / c[3], c[2] / c[3]
        fpx = ((u + _F(1.0)) * _F(0.5)) * _F(w) - _F(0.5)
        fpy = ((vv + _F(1.0)) * _F(0.5)) * _F(h) - _F(0.5)
        qe = (((r_[3] * u + r_[7] * vv) + r_[11] * dp) + r_[15]) / (((r_[2] * u + r_[6] * vv) + r_[10] * dp) + r_[14])
    assert fpx.dtype == fpy.dtype == qe.dtype == np.float32
    return front, fpx, fpy, qe


def _blend(taps, weights, counts):
    """Items 5e / 5f: over the taps that count, in order, from zero: Wsum += w; A += w a; C += w (a rgb); the division where Wsum != 1; (C / A, A)."""
    shape = weights[0].shape
    wsum, a, c = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape + (3,), np.float32)
    with np.errstate(all="ignore"):
        for k in range(4):
            ak = taps[k][..., 3]
            wsum = np.where(counts[k], wsum + weights[k], wsum)
            a = np.where(counts[k], a + weights[k] * ak, a)
            c = np.where(counts[k][..., None], c + weights[k][..., None] * (ak[..., None] * taps[k][..., :3]), c)
        div = wsum != _F(1.0)
        a = np.where(div, a / wsum, a)
        c = np.where(div[..., None], c / wsum[..., None], c)
        has = a > _F(0.0)
        out = np.empty(shape + (4,), dtype=np.float32)
        out[..., :3] = np.where(has[..., None], c / a[..., None], _F(0.0))
        out[..., 3] = a
    assert wsum.dtype == a.dtype == c.dtype == np.float32
    return out


def fallback_taps(w: int, s: int, o: int):
    """One axis of 5f's footprint for the pixels 0 .. w - 1: (first neighbour, second neighbour, fraction float32).  i0 = floor((x - o) / s),
    f = ((x - o) - s i0) / s; the neighbours clamped to the low texels whose full pixel exists, 0 .. max(ceil((w - o) / s), 1) - 1."""
    s = _scale(s)
    last = max((int(w) - o + s - 1) // s, 1) - 1
    t = np.arange(int(w)) - o
    i0 = np.floor_divide(t, s)
    f = (t - s * i0).astype(np.float32) / _F(s)
    return np.clip(i0, 0, last), np.clip(i0 + 1, 0, last), f


def spatial_fallback(frame: dict, depth, low_depth, low_rgba, s: int, p: int, tol) -> np.ndarray:
    """Item 5f for every pixel: reduced.upsample's filter over the phase-positioned low samples; a neighbour counts when its depth agrees and its weight
    is > 0; none counts: the closest in depth of the four alone (strict comparison, the first wins), with weight 1."""
    ox, oy = phase_offset(s, p)
    depth = np.asarray(depth, dtype=np.float32)
    low_depth, low_rgba = np.asarray(low_depth, dtype=np.float32), np.asarray(low_rgba, dtype=np.float32)
    h, w = depth.shape
    tol = _F(tol)
    ia, ib, fx = fallback_taps(w, s, ox)
    ja, jb, fy = fallback_taps(h, s, oy)
    fx, fy = np.broadcast_to(fx[None, :], (h, w)), np.broadcast_to(fy[:, None], (h, w))
    gx, gy = _F(1.0) - fx, _F(1.0) - fy
    weights = [gx * gy, fx * gy, gx * fy, fx * fy]
    index = [(ja, ia), (ja, ib), (jb, ia), (jb, ib)]
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(all="ignore"):
        q0 = R.eye_q(frame, x, y, depth)
        diff, counts, taps = [], [], []
        for k, (jj, ii) in enumerate(index):
            qk = R.eye_q(frame, x, y, low_depth[jj[:, None], ii[None, :]])
            dk = np.abs(q0 - qk)
            diff.append(dk)
            counts.append((dk <= tol * np.fmax(np.abs(q0), np.abs(qk))) & (weights[k] > _F(0.0)))
            taps.append(low_rgba[jj[:, None], ii[None, :]])
        none = ~(counts[0] | counts[1] | counts[2] | counts[3])
        best = np.zeros((h, w), dtype=np.int64)
        best_diff = diff[0]
        for k in range(1, 4):
            closer = diff[k] < best_diff
            best = np.where(closer, k, best)
            best_diff = np.where(closer, diff[k], best_diff)
        counts = [np.where(none, best == k, counts[k]) for k in range(4)]
        weights = [np.where(none, _F(1.0), weights[k]).astype(np.float32) for k in range(4)]
    return _blend(taps, weights, counts)


def _texel_valid(front, qe, fi, fj, prev_q, prev_age, max_age, htol):
    """Item 5c for the history texels (fi, fj), float32 arrays: (valid, j, i, age) -- the indices 0 and the age 255 where the texel lies outside."""
    h, w = prev_q.shape
    with np.errstate(all="ignore"):
        inside = front & (fi >= _F(0.0)) & (fi < _F(w)) & (fj >= _F(0.0)) & (fj < _F(h))
        ii = np.where(inside, fi, _F(0.0)).astype(np.int64)
        jj = np.where(inside, fj, _F(0.0)).astype(np.int64)
        age = np.where(inside, prev_age[jj, ii].astype(np.int64), NOT_HISTORY)
        qk = prev_q[jj, ii]
        agree = np.abs(qe - qk) <= _F(htol) * np.fmax(np.abs(qe), np.abs(qk))
    return inside & (age < int(max_age)) & agree, jj, ii, age


def resolve(frame: dict, depth, low_depth, low_rgba, s: int, p: int, depth_tolerance, history_tolerance=0.1, max_age=None, prev=None, prev_clip=None,
            prev_inv_projection=None, reset: bool = False, details: bool = False):
    """Item 5: (pixels (H, W, 4) float32, q0 (H, W) float32, age (H, W) uint8) -- the current history's three parts; the target is
    `reduced.store(pixels, ...)`.  `prev`: the previous history's (rgba, q, age), never looked at under `reset`.  details: also a dict with `path` (H, W),
    one of FRESH / SNAP / BILINEAR / FALLBACK per pixel, and `fpx`, `fpy` (None under reset)."""
    ox, oy = phase_offset(s, p)
    depth = np.asarray(depth, dtype=np.float32)
    low_rgba = np.asarray(low_rgba, dtype=np.float32)
    h, w = depth.shape
    lw, lh = R.low_size(w, h, s)
    assert np.asarray(low_depth).shape == (lh, lw) and low_rgba.shape == (lh, lw, 4)
    max_age = 2 * s * s if max_age is None else int(max_age)
    if not 1 <= max_age <= 255:
        raise ValueError("max_age must be 1 .. 255")
    _, q0 = view_point(frame, depth)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pixels = spatial_fallback(frame, depth, low_depth, low_rgba, s, p, depth_tolerance)       # 5f, kept where nothing below takes the pixel
    age = np.full((h, w), NOT_HISTORY, dtype=np.int64)
    path = np.full((h, w), FALLBACK, dtype=np.int64)
    fresh = (x % s == ox) & (y % s == oy)
    fpx = fpy = None
    if not reset:
        if prev is None:
            raise ValueError("no previous history without reset")
        prev_rgba, prev_q, prev_age = (np.asarray(prev[0], dtype=np.float32), np.asarray(prev[1], dtype=np.float32), np.asarray(prev[2], dtype=np.uint8))
        assert prev_rgba.shape == (h, w, 4) and prev_q.shape == prev_age.shape == (h, w)
        front, fpx, fpy, qe = reproject(frame, depth, prev_clip, prev_inv_projection)
        with np.errstate(all="ignore"):
            jx, jy = np.floor(fpx + _F(0.5)), np.floor(fpy + _F(0.5))
            snap = (np.abs(fpx - jx) <= _F(SNAP_RADIUS)) & (np.abs(fpy - jy) <= _F(SNAP_RADIUS))
            # 5d
            ok, jj, ii, a = _texel_valid(front, qe, jx, jy, prev_q, prev_age, max_age, history_tolerance)
            take = snap & ok
            pixels = np.where(take[..., None], prev_rgba[jj, ii], pixels)
            age = np.where(take, np.minimum(a + 1, OLDEST), age)
            path = np.where(take, SNAP, path)
            # 5e
            i0, j0 = np.floor(fpx), np.floor(fpy)
            fx, fy = fpx - i0, fpy - j0
            gx, gy = _F(1.0) - fx, _F(1.0) - fy
            weights = [gx * gy, fx * gy, gx * fy, fx * fy]
            taps, counts = [], []
            oldest = np.full((h, w), -1, dtype=np.int64)
            for k in range(4):
                ok, jj, ii, a = _texel_valid(front, qe, i0 + _F(k & 1), j0 + _F(k >> 1), prev_q, prev_age, max_age, history_tolerance)
                ok = ok & (weights[k] > _F(0.0))
                counts.append(ok)
                taps.append(prev_rgba[jj, ii])
                oldest = np.where(ok, np.maximum(oldest, a), oldest)
            take = ~snap & (oldest >= 0)
            pixels = np.where(take[..., None], _blend(taps, weights, counts), pixels)
            age = np.where(take, np.minimum(oldest + 1, OLDEST), age)
            path = np.where(take, BILINEAR, path)
    # 5a
    pixels = np.where(fresh[..., None], np.asarray(low_rgba)[y // s, x // s], pixels)
    age = np.where(fresh, 0, age)
    path = np.where(fresh, FRESH, path)
    out = (pixels.astype(np.float32, copy=False), q0, age.astype(np.uint8))
    assert out[0].dtype == np.float32
    return out + (dict(path=path, fpx=fpx, fpy=fpy),) if details else out


# ---- what PlanetAtmosphere.render_temporal keeps between frames -----------------------------------------------------------------------------------------

class TemporalHistory:
    """The state of a sequence of temporal draws of one viewport: the two history buffers (CUDA uint8 tensors of `history_layout(w, h)[2]` bytes), which of
    them the next call reads, the previous call's camera matrices and the frame index.  `render_temporal` swaps the buffers on every call and starts over
    (`fresh` is True) when the viewport or the scale is not the one the buffers were made for."""

    def __init__(self, width: int, height: int, scale: int, device):
        import torch

        self.width, self.height, self.scale = int(width), int(height), _scale(scale)
        self.nbytes = history_layout(width, height)[2]
        self.buffers = [torch.zeros(self.nbytes, dtype=torch.uint8, device=device) for _ in range(2)]
        self.frame_index = 0
        self.fresh = True           # no call has written a history yet: the next one resets
        self.prev_camera = None     # the last call's projection, view and column-major float32 inv_projection

    def matches(self, camera, scale, device) -> bool:
        import torch

        return (self.width, self.height, self.scale) == (camera.width, camera.height, scale) and self.buffers[0].device == torch.device(device)

    @property
    def previous(self):
        """The buffer the last call wrote (the next call's previous history)."""
        return self.buffers[(self.frame_index + 1) & 1]

    @property
    def current(self):
        """The buffer the next call writes."""
        return self.buffers[self.frame_index & 1]

    def parts(self):
        """(rgba, q, age) of the history the last call wrote, as numpy arrays."""
        return unpack_history(self.previous.cpu().numpy(), self.width, self.height)

    def advance(self, camera):
        self.prev_camera = SimpleNamespace(projection=np.array(camera.projection, dtype=np.float64), view=np.array(camera.view, dtype=np.float64),
                                           inv_projection_cm=col_major(camera.inv_projection))
        self.frame_index += 1
        self.fresh = False
