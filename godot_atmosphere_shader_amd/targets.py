"""The numerical contract of the packed colour targets (include/atmo_target.h) in numpy: what atmo_render_target stores into, and blends with, an
RGBA16F or RGBA8_UNORM buffer.  Pure numpy, no device: the tests hold the kernels to these functions bit for bit, and a host can use them to
prepare or read a target.

    encode(rgba_f32, fmt)          fp32 channels -> the stored bits
    decode(buf, fmt)               stored bits -> fp32, exactly
    blend(src_f32, dst_buf, fmt)   decode(dst) -> the fp32 blend of atmo_render_composite (blend_mix) -> encode, once

fmt: "rgba32f" | "rgba16f" | "rgba8" (or the AtmoTargetFormat value 0 | 1 | 2).  Buffers are float32 / float16 / uint8 arrays of any shape for encode and
decode; blend takes (..., 4) arrays, RGBA last.
"""
from __future__ import annotations

import numpy as np

RGBA32F, RGBA16F, RGBA8 = 0, 1, 2
FORMATS = {"rgba32f": RGBA32F, "rgba16f": RGBA16F, "rgba8": RGBA8, "rgba8_unorm": RGBA8}
DTYPES = {RGBA32F: np.float32, RGBA16F: np.float16, RGBA8: np.uint8}
PIXEL_BYTES = {RGBA32F: 16, RGBA16F: 8, RGBA8: 4}
HALF_QNAN = 0x7E00   # the one NaN an RGBA16F store writes


def format_id(fmt) -> int:
    """"rgba16f" / "rgba8" / "rgba32f", a numpy or torch dtype, or an AtmoTargetFormat value -> the AtmoTargetFormat value."""
    if isinstance(fmt, str):
        if fmt.lower() not in FORMATS:
            raise ValueError(f"unknown target format {fmt!r}: one of {sorted(FORMATS)}")
        return FORMATS[fmt.lower()]
    if isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool):
        if int(fmt) not in DTYPES:
            raise ValueError(f"unknown target format {fmt}")
        return int(fmt)
    name = str(fmt).replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
    for key, val in (("float32", RGBA32F), ("float16", RGBA16F), ("uint8", RGBA8)):
        if name == key:
            return val
    raise ValueError(f"unknown target format {fmt!r}")


def encode(rgba_f32, fmt) -> np.ndarray:
    """fp32 -> stored bits.  RGBA16F: IEEE binary16, round-to-nearest-even, subnormals kept, overflow to infinity, every NaN -> the quiet NaN 0x7e00.
    RGBA8: (uint8) rint(clamp(x, 0, 1) * 255) with the product in fp32, ties to even, NaN -> 0."""
    f = format_id(fmt)
    x = np.asarray(rgba_f32, dtype=np.float32)
    if f == RGBA32F:
        return x.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        if f == RGBA16F:
            h = x.astype(np.float16)
            bits = h.view(np.uint16).copy()
            bits[np.isnan(x)] = HALF_QNAN
            return bits.view(np.float16)
        c = np.where(np.isnan(x), np.float32(0.0), x)
        c = np.minimum(np.maximum(c, np.float32(0.0)), np.float32(1.0)).astype(np.float32)
        return np.rint(c * np.float32(255.0)).astype(np.uint8)


def decode(buf, fmt) -> np.ndarray:
    """stored bits -> fp32, exactly: binary16 -> float (subnormals included); byte / 255.0f as an IEEE fp32 division."""
    f = format_id(fmt)
    b = np.asarray(buf)
    if b.dtype != DTYPES[f]:
        raise TypeError(f"a {fmt} buffer is {np.dtype(DTYPES[f]).name}, not {b.dtype.name}")
    if f == RGBA8:
        return b.astype(np.float32) / np.float32(255.0)
    return b.astype(np.float32)


def blend(src_f32, dst_buf, fmt) -> np.ndarray:
    """What a composite leaves in the target: the destination decoded, blended in fp32 by atmo_render_composite's unfused expressions (colour
    src * a + dst * (1 - a), alpha a + dst_a * (1 - a); a = the source's alpha), encoded once."""
    src = np.asarray(src_f32, dtype=np.float32)
    dst = decode(dst_buf, fmt)
    if src.shape != dst.shape or src.shape[-1] != 4:
        raise ValueError("blend: src and dst must have the same (..., 4) shape")
    with np.errstate(over="ignore", invalid="ignore"):
        a = src[..., 3:4]
        ia = (np.float32(1.0) - a).astype(np.float32)
        out = np.empty_like(src)
        out[..., :3] = (src[..., :3] * a).astype(np.float32) + (dst[..., :3] * ia).astype(np.float32)
        out[..., 3:4] = a + (dst[..., 3:4] * ia).astype(np.float32)
    return encode(out, fmt)
