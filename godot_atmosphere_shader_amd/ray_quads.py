"""Quad order: how PlanetAtmosphere.shade_ray_quads (atmo_shade_ray_quads; include/atmo_ray_quads.h) lays an image's rays out.

The quads of a `width` x `height` image in row-major order, the four pixels of a quad in row-major order: slot 4 q + j of quad q is pixel
x = 2 (q % qpr) + (j & 1), y = 2 (q // qpr) + (j >> 1) with qpr = (width + 1) // 2.  An odd width or height leaves slots outside the image: they hold
absent rays (an all-zero row).  Needs no GPU to import; `quads_to_image` takes numpy arrays and torch tensors alike.
"""
from __future__ import annotations

import numpy as np


def quad_order(width: int, height: int) -> np.ndarray:
    """Slot -> row-major pixel index y * width + x, int64, of length 4 * ceil(width / 2) * ceil(height / 2); -1 for a slot outside the image."""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("width and height must be at least 1")
    qpr, qrows = (width + 1) // 2, (height + 1) // 2
    slot = np.arange(4 * qpr * qrows, dtype=np.int64)
    q, j = slot >> 2, slot & 3
    x, y = 2 * (q % qpr) + (j & 1), 2 * (q // qpr) + (j >> 1)
    return np.where((x < width) & (y < height), y * width + x, -1)


def quads_to_image(values, width: int, height: int):
    """The inverse scatter: `values` has one row per slot of quad_order(width, height), shape (slots, ...); returns shape (height, width, ...) with pixel
    (x, y) taken from its slot.  The rows of the slots outside the image are dropped.  A numpy array gives a numpy array, a torch tensor a tensor on its
    device."""
    order = quad_order(width, height)
    if values.shape[0] != order.shape[0]:
        raise ValueError(f"values must have one row per slot: {order.shape[0]} for a {width} x {height} image, got {values.shape[0]}")
    inside = np.nonzero(order >= 0)[0]
    slot_of_pixel = np.empty(width * height, dtype=np.int64)
    slot_of_pixel[order[inside]] = inside
    if isinstance(values, np.ndarray):
        picked = values[slot_of_pixel]
    else:
        import torch

        picked = values[torch.as_tensor(slot_of_pixel, device=values.device)]
    return picked.reshape((height, width) + tuple(values.shape[1:]))
