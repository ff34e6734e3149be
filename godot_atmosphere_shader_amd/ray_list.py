"""Ray lists in numpy (include/atmo_ray_list.h states them; no GPU needed to import this): `cull_mask` is THE CULL operation for operation in float32,
`ray_list` the list atmo_ray_list writes on the device -- the live rays the cull leaves, in queue order or in ray_order's, and the END tail
(tests/test_ray_list_gpu.py holds the kernels to these as integers)."""
from __future__ import annotations

import numpy as np

from .ray_order import ray_keys

ORDER, CULL = 1, 2      # ATMO_RAY_LIST_ORDER, ATMO_RAY_LIST_CULL
END = 0xFFFFFFFF        # ATMO_RAY_LIST_END
_F = np.float32


def _dot(a, b) -> np.ndarray:
    """Three rounded float32 products summed left to right."""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cull_mask(rays, consts) -> np.ndarray:
    """THE CULL: bool (n,), True where the ray surely misses the shell.  `rays`: (n, 8) AtmoRay rows; `consts`: the five floats of
    atmo_debug_ray_cull_constants -- c.x, c.y, c.z, R2, RN(R2 * 1.02f)."""
    r = np.asarray(rays, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError("rays must have shape (n, 8) (AtmoRay rows)")
    k = np.asarray(consts, dtype=np.float32)
    if k.shape != (5,):
        raise ValueError("consts must hold five floats: c.x, c.y, c.z, R2, RN(R2 * 1.02f)")
    with np.errstate(all="ignore"):
        c = [k[j] - r[:, j] for j in range(3)]
        d = [r[:, 4 + j] for j in range(3)]
        cc, b, dd = _dot(c, c), _dot(c, d), _dot(d, d)
        g = (b * b) * (_F(2.0) - dd)
        e = cc - k[3]
        assert g.dtype == np.float32 and e.dtype == np.float32
        return (cc >= k[4]) & (dd >= _F(0.25)) & (dd <= _F(1.75)) & (g < e * _F(0.998))


def list_from(keys, culled, n, flags):
    """`ray_list` on what is already worked out per ray: `keys` uint32 (capacity,), THE KEY of every ray; `culled` bool (capacity,), THE CULL of every ray
    (None without CULL).  Rows at and behind n take no part, whatever the two hold there."""
    capacity = len(keys)
    if flags & ~(ORDER | CULL):
        raise ValueError("unknown flag bits")
    n = capacity if n is None else min(int(n), capacity)
    zeros = np.zeros(capacity, dtype=bool)
    if flags & CULL:
        if culled is None:
            raise ValueError("CULL needs the cull constants")
        zeros[:n] = np.asarray(culled, dtype=bool)[:n]
    kept = np.nonzero(~zeros[:n])[0]
    if flags & ORDER:
        kept = kept[np.argsort(np.asarray(keys)[kept], kind="stable")]
    index = np.full(capacity, END, dtype=np.uint32)
    index[:kept.size] = kept
    return index, int(kept.size), zeros


def ray_list(rays, n, flags, consts=None):
    """(index, listed, zeros): what atmo_ray_list writes for a queue of capacity len(rays) whose count word holds `n` (None: no word, the capacity) --
    index uint32 (capacity,), the listed rays then END; listed = |L|; zeros bool (capacity,), the rows of rgba that receive zeros.  CULL needs `consts`,
    the five floats of atmo_debug_ray_cull_constants."""
    r = np.asarray(rays, dtype=np.float32)
    if flags & CULL and consts is None:
        raise ValueError("CULL needs the cull constants")
    return list_from(ray_keys(r), cull_mask(r, consts) if flags & CULL else None, n, flags)
