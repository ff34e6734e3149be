"""The coherence order of a ray queue in numpy (include/atmo_ray_order.h states it; no GPU needed to import this): `ray_keys` is THE KEY operation for
operation in float32, `ray_order` the stable sort by it -- the permutation atmo_ray_order writes on the device (tests/test_ray_order_gpu.py holds the
kernels to these as integers)."""
from __future__ import annotations

import numpy as np

KEY_BITS = 18   # ATMO_RAY_KEY_BITS: 9 + 9 bits of an octahedral cell, Morton-interleaved
_F = np.float32


def _directions(rays) -> np.ndarray:
    """(n, 3) float32 directions from (n, 8) AtmoRay rows (columns 4..6) or from (n, 3) directions."""
    a = np.asarray(rays, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] not in (3, 8):
        raise ValueError("rays must have shape (n, 8) (AtmoRay rows) or (n, 3) (directions)")
    return a[:, 4:7] if a.shape[1] == 8 else a


def _spread(q: np.ndarray) -> np.ndarray:
    """Bit b of a 9-bit number to bit 2 b."""
    out = np.zeros_like(q)
    for b in range(9):
        out |= ((q >> np.uint32(b)) & np.uint32(1)) << np.uint32(2 * b)
    return out


def _cell(t: np.ndarray) -> np.ndarray:
    """clamp((int)floor(RN(RN(t * 256) + 256)), 0, 511)."""
    return np.clip(np.floor(t * _F(256.0) + _F(256.0)), 0.0, 511.0).astype(np.uint32)


def ray_keys(rays) -> np.ndarray:
    """The key of every ray, uint32 (n,): SUM, PLANE, FOLD, CELL and INTERLEAVE of the header, every operation a float32 one rounded on its own."""
    d = _directions(rays)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        bad = ~(s > _F(0.0)) | np.isinf(s)          # zero, NaN, infinite
        safe = np.where(bad, _F(1.0), s)
        u, v = dx / safe, dy / safe
        fold = np.signbit(dz)
        fu = np.where(fold, np.copysign(_F(1.0) - np.abs(v), u), u)
        fv = np.where(fold, np.copysign(_F(1.0) - np.abs(u), v), v)
        assert fu.dtype == np.float32 and fv.dtype == np.float32
        key = _spread(_cell(np.where(bad, _F(0.0), fu))) | (_spread(_cell(np.where(bad, _F(0.0), fv))) << np.uint32(1))
    return np.where(bad, np.uint32((1 << KEY_BITS) - 1), key).astype(np.uint32)


def ray_order(rays) -> np.ndarray:
    """The order atmo_ray_order writes: the stable ascending sort of 0 .. n-1 by key, int64 (n,)."""
    return np.argsort(ray_keys(rays), kind="stable")
