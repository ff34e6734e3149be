"""Lens rays in numpy (include/atmo_lens.h states them; no GPU needed to import this): the rays atmo_lens_rays writes on the device for a panorama, a
fisheye, an octahedral map and a cube face, row-major or in quad order, the 16 x 4 tile index beside the row-major ones, and the float64 inverse of every
lens.  OCTAHEDRAL, CUBE_FACE and the basis are float32, operation for operation; the two trigonometric lenses are float64 numpy rounded once, which the
device meets within 1 float32 ulp (tests/test_lens_gpu.py holds the kernels to these).

Lens space is a camera's view space: -Z forward, +Y up, +X right; image row 0 is the top row; pixel (x, y) has its centre at (x + 0.5, y + 0.5).
"""
from __future__ import annotations

import math

import numpy as np

EQUIRECT, FISHEYE, OCTAHEDRAL, CUBE_FACE = range(4)   # AtmoLensKind
KINDS = ("equirect", "fisheye", "octahedral", "cube_face")
LENS_QUADS = 1                                        # ATMO_LENS_QUADS
LIST_END = 0xFFFFFFFF                                 # ATMO_RAY_LIST_END: a tile-index entry without a ray
FLT_MAX = float(np.finfo(np.float32).max)
MAX_FOV = float(np.float32(6.2831855))
TILE_W, TILE_H = 16, 4                                # the tile index's tile: the draw kernels' block
_F = np.float32


class Lens:
    """An AtmoLens: the image, the band of rows this call writes, and where the lens stands in ray space.  `basis` is a 3 x 3 matrix (lens space -> ray
    space, `basis @ d`), `origin` every ray's origin, `tmax` every ray's distance limit where no distance buffer is given, `rows` = (y0, y1)."""

    def __init__(self, kind, width, height, *, rows=None, face=0, fov=0.0, tmax=FLT_MAX, origin=(0.0, 0.0, 0.0), basis=None):
        self.kind, self.width, self.height = int(kind), int(width), int(height)
        self.rows = (0, self.height) if rows is None else (int(rows[0]), int(rows[1]))
        self.face, self.fov, self.tmax = int(face), float(np.float32(fov)), float(np.float32(tmax))
        self.origin = np.asarray(origin, dtype=np.float32).reshape(3)
        self.basis = np.asarray(np.eye(3) if basis is None else basis, dtype=np.float32).reshape(3, 3)
        self.check()

    @classmethod
    def equirect(cls, width, height, **kw):
        """A panorama: longitude across, +-180 degrees at the edges and -Z in the middle; latitude down, +Y at the top."""
        return cls(EQUIRECT, width, height, **kw)

    @classmethod
    def fisheye(cls, width, height, fov=math.pi, **kw):
        """An equidistant fisheye looking along -Z: `fov` radians across the image circle, whose diameter is min(width, height)."""
        return cls(FISHEYE, width, height, fov=fov, **kw)

    @classmethod
    def octahedral(cls, width, height, **kw):
        """An octahedral map of the whole sphere, its centre looking along +Z: the inverse of the ray key's PLANE and FOLD (include/atmo_ray_order.h)."""
        return cls(OCTAHEDRAL, width, height, **kw)

    @classmethod
    def cube_face(cls, size, face, **kw):
        """Face 0 .. 5 = +X -X +Y -Y +Z -Z of a cubemap, `size` texels square, by the coverage cubemap's texel-to-direction table."""
        return cls(CUBE_FACE, size, size, face=face, **kw)

    def check(self):
        """atmo_lens_rays' checks on the lens alone, as ValueError."""
        y0, y1 = self.rows
        if self.kind not in (EQUIRECT, FISHEYE, OCTAHEDRAL, CUBE_FACE):
            raise ValueError(f"unknown lens kind {self.kind}")
        if self.width < 1 or self.height < 1 or self.width * self.height > 1 << 28:
            raise ValueError("width and height must be at least 1 and width * height at most 2^28")
        if y0 < 0 or y1 > self.height or y1 < y0:
            raise ValueError("rows = (y0, y1) must lie inside [0, height]")
        if self.kind == FISHEYE and not 0.0 < self.fov <= MAX_FOV:
            raise ValueError("a fisheye's fov must lie in (0, 6.2831855] radians")
        if self.kind == CUBE_FACE and (self.width != self.height or not 0 <= self.face <= 5):
            raise ValueError("a cube face is square and face is 0 .. 5")

    def band(self, rows) -> "Lens":
        """The same lens writing the rows [rows[0], rows[1])."""
        return Lens(self.kind, self.width, self.height, rows=rows, face=self.face, fov=self.fov, tmax=self.tmax, origin=self.origin, basis=self.basis)

    def check_quads(self):
        y0, y1 = self.rows
        if y0 % 2 or (y1 % 2 and y1 != self.height):
            raise ValueError("the quad order needs an even y0, and an even y1 or y1 == height")

    def counts(self, quads: bool = False):
        """(n_rays, n_index) of atmo_lens_ray_counts."""
        rows = self.rows[1] - self.rows[0]
        if rows == 0:
            return 0, 0
        if quads:
            self.check_quads()
        n_rays = 4 * ((self.width + 1) // 2) * ((rows + 1) // 2) if quads else self.width * rows
        return n_rays, 64 * ((self.width + TILE_W - 1) // TILE_W) * ((rows + TILE_H - 1) // TILE_H)

    def native(self):
        """The N.AtmoLens of this lens (the basis column-major)."""
        from . import _native as N

        s = N.AtmoLens()
        s.kind, s.width, s.height, s.y0, s.y1, s.face, s.fov, s.tmax = self.kind, self.width, self.height, self.rows[0], self.rows[1], self.face, self.fov, self.tmax
        s.origin[:] = [float(v) for v in self.origin]
        s.basis[:] = [float(v) for v in self.basis.T.reshape(9)]
        return s

    def __repr__(self):
        return f"Lens.{KINDS[self.kind]}({self.width} x {self.height}, rows={self.rows})"


def _octahedral(lens, x, y):
    with np.errstate(all="ignore"):
        u = (2 * x + 1).astype(_F) / _F(lens.width) - _F(1.0)
        v = (2 * y + 1).astype(_F) / _F(lens.height) - _F(1.0)
        z = (_F(1.0) - np.abs(u)) - np.abs(v)
        a = np.where(z < 0, np.copysign(_F(1.0) - np.abs(v), u), u)
        b = np.where(z < 0, np.copysign(_F(1.0) - np.abs(u), v), v)
        n = np.sqrt((a * a + b * b) + z * z)
        d = np.stack([a / n, b / n, z / n], axis=1)
    assert d.dtype == np.float32
    return d, np.zeros(x.shape, dtype=bool)


def _cube_face(lens, x, y):
    n = lens.width
    half = _F(0.5) * _F(n)
    p = (x.astype(_F) + _F(0.5)) / half - _F(1.0)
    q = ((n - y - 1).astype(_F) + _F(0.5)) / half - _F(1.0)
    vx, vy, vz = np.ones_like(p), q, -p
    length = np.sqrt((vx * vx + vy * vy) + vz * vz)
    vx, vy, vz = vx / length, vy / length, vz / length
    d = np.stack([(vx, vy, vz), (-vx, vy, -vz), (-vz, vx, -vy), (-vz, -vx, vy), (-vz, vy, vx), (vz, vy, -vx)][lens.face], axis=1)
    assert d.dtype == np.float32
    return d, np.zeros(x.shape, dtype=bool)


def _equirect(lens, x, y):
    phi = ((x + 0.5) / float(lens.width) - 0.5) * (2.0 * np.pi)
    theta = (0.5 - (y + 0.5) / float(lens.height)) * np.pi
    d = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta), -(np.cos(theta) * np.cos(phi))], axis=1)
    return d.astype(_F), np.zeros(x.shape, dtype=bool)


def _fisheye(lens, x, y):
    w, h = lens.width, lens.height
    absent = (2 * x + 1 - w) ** 2 + (h - 2 * y - 1) ** 2 > min(w, h) ** 2      # r > 1, in integers
    px, py = (x + 0.5) - w / 2.0, h / 2.0 - (y + 0.5)
    rho = np.sqrt(px * px + py * py)
    theta = (rho / (min(w, h) / 2.0)) * (float(lens.fov) / 2.0)
    safe = np.where(rho == 0.0, 1.0, rho)
    d = np.stack([np.sin(theta) * (px / safe), np.sin(theta) * (py / safe), -np.cos(theta)], axis=1)
    d[rho == 0.0] = (0.0, 0.0, -1.0)
    return d.astype(_F), absent


_DIRECTIONS = {EQUIRECT: _equirect, FISHEYE: _fisheye, OCTAHEDRAL: _octahedral, CUBE_FACE: _cube_face}


def lens_directions(lens, x, y):
    """The lens-space directions of the pixels (x, y) (int64 arrays): float32 (n, 3), and which of them are absent (their directions mean nothing)."""
    x, y = np.asarray(x, dtype=np.int64).reshape(-1), np.asarray(y, dtype=np.int64).reshape(-1)
    return _DIRECTIONS[lens.kind](lens, x, y)


def _pixels(lens, quads: bool):
    """(x, y, inside) of every slot of the band, in the order of the ray array."""
    y0, y1 = lens.rows
    if quads:
        lens.check_quads()
        qpr = (lens.width + 1) // 2
        slot = np.arange(lens.counts(True)[0], dtype=np.int64)
        q, j = slot >> 2, slot & 3
        x, y = 2 * (q % qpr) + (j & 1), y0 + 2 * (q // qpr) + (j >> 1)
    else:
        i = np.arange(lens.counts(False)[0], dtype=np.int64)
        x, y = i % lens.width, y0 + i // lens.width
    return x, y, (x < lens.width) & (y < y1)


def lens_rays(lens, quads: bool = False, distance=None) -> np.ndarray:
    """The AtmoRay rows atmo_lens_rays writes for the lens's band: float32 (n, 8) -- origin, tmax, dir, 0 -- row-major, or in quad order (`quads`; slots
    outside the image are absent).  An absent ray is eight +0.  `distance`: a (height, >= width) float32 array, every ray's tmax."""
    x, y, inside = _pixels(lens, quads)
    xi, yi = np.where(inside, x, 0), np.where(inside, y, 0)
    d, absent = lens_directions(lens, xi, yi)
    present = inside & ~absent
    B = lens.basis
    with np.errstate(all="ignore"):
        out_d = np.stack([(B[r, 0] * d[:, 0] + B[r, 1] * d[:, 1]) + B[r, 2] * d[:, 2] for r in range(3)], axis=1)
    assert out_d.dtype == np.float32
    rays = np.zeros((x.shape[0], 8), dtype=np.float32)
    rays[:, 0:3] = lens.origin
    if distance is None:
        rays[:, 3] = _F(lens.tmax)
    else:
        distance = np.asarray(distance, dtype=np.float32)
        if distance.ndim != 2 or distance.shape[0] != lens.height or distance.shape[1] < lens.width:
            raise ValueError("distance must have shape (height, pitch >= width)")
        rays[:, 3] = distance[yi, xi]
    rays[:, 4:7] = out_d
    rays[~present] = 0.0
    return rays


def lens_tile_index(lens) -> np.ndarray:
    """THE TILE INDEX of the band's row-major rays, uint32 (n_index,): 16 x 4 tiles in row-major order, lanes row-major inside a tile; the ray's number for a
    pixel inside the band that is not absent, else LIST_END."""
    y0, y1 = lens.rows
    k = np.arange(lens.counts(False)[1], dtype=np.int64)
    tpr = (lens.width + TILE_W - 1) // TILE_W
    t, l = k >> 6, k & 63
    x, y = TILE_W * (t % tpr) + (l & 15), y0 + TILE_H * (t // tpr) + (l >> 4)
    inside = (x < lens.width) & (y < y1)
    _, absent = lens_directions(lens, np.where(inside, x, 0), np.where(inside, y, 0))
    return np.where(inside & ~absent, (y - y0) * lens.width + x, LIST_END).astype(np.uint32)


def lens_pixel(lens, directions) -> np.ndarray:
    """The float64 inverse: ray-space directions (n, 3) (any length) to continuous pixel coordinates (n, 2), a pixel's centre at (x + 0.5, y + 0.5).  The
    basis is inverted as a matrix.  CUBE_FACE: directions outside the face's quadrant land outside [0, N]^2 or give NaN."""
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    d = d @ np.linalg.inv(lens.basis.astype(np.float64)).T        # back to lens space
    w, h = float(lens.width), float(lens.height)
    with np.errstate(all="ignore"):
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        if lens.kind == EQUIRECT:
            phi, theta = np.arctan2(dx, -dz), np.arcsin(np.clip(dy, -1.0, 1.0))
            return np.stack([(phi / (2.0 * np.pi) + 0.5) * w, (0.5 - theta / np.pi) * h], axis=1)
        if lens.kind == FISHEYE:
            theta, s = np.arccos(np.clip(-dz, -1.0, 1.0)), np.hypot(dx, dy)
            rho = theta / (float(lens.fov) / 2.0) * (min(w, h) / 2.0)
            s = np.where(s == 0.0, 1.0, s)
            return np.stack([w / 2.0 + rho * dx / s, h / 2.0 - rho * dy / s], axis=1)
        if lens.kind == OCTAHEDRAL:
            s = np.abs(dx) + np.abs(dy) + np.abs(dz)
            u, v = dx / s, dy / s
            fu = np.where(dz < 0, np.copysign(1.0 - np.abs(v), u), u)
            fv = np.where(dz < 0, np.copysign(1.0 - np.abs(u), v), v)
            return np.stack([(fu + 1.0) * w / 2.0, (fv + 1.0) * h / 2.0], axis=1)
        # CUBE_FACE: undo the face's permutation to v = (1, q, -p) / len, then the texel
        vx, vy, vz = [(dx, dy, dz), (-dx, dy, -dz), (dy, -dz, -dx), (-dy, dz, -dx), (dz, dy, -dx), (-dz, dy, dx)][lens.face]
        p, q = -vz / vx, vy / vx
        return np.stack([(p + 1.0) * w / 2.0, h - (q + 1.0) * h / 2.0], axis=1)
