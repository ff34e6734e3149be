"""The numerical contract of the depth sources (include/atmo_depth.h) in numpy: how atmo_render_depth_target and its siblings read a D32_SFLOAT,
D16_UNORM or X8_D24_UNORM depth buffer.  Pure numpy, no device: the tests hold the kernels to decode() bit for bit, and a host can use it to know the
depth a draw sees.

    decode(bits, fmt)            stored texels -> the fp32 depth the kernels read, exactly
    quantise(depth_f32, fmt)     for tests: fp32 depth -> texels, rint(clip(d, 0, 1) * max) in float64 (the library never encodes depth)

fmt: "d32f" | "d16" | "x8d24" (or the AtmoDepthFormat value 0 | 1 | 2).  Texels are float32 / uint16 / uint32 arrays of any shape (DTYPES; signed
arrays of the same width are taken by their bits).  X8_D24: depth in bits 0-23 of the little-endian word, bits 24-31 are ignored by decode and zero
from quantise.

Decode is Vulkan's UNORM rule as ONE IEEE fp32 division of the exactly converted code: code / 65535.0f, (word & 0xFFFFFF) / 16777215.0f.  Only the top
code decodes to 1.0 and only code 0 to 0.0.
"""
from __future__ import annotations

import numpy as np

D32F, D16, X8D24 = 0, 1, 2
FORMATS = {"d32f": D32F, "d16": D16, "x8d24": X8D24}
NAMES = {D32F: "d32f", D16: "d16", X8D24: "x8d24"}
TEXEL_BYTES = {D32F: 4, D16: 2, X8D24: 4}
DTYPES = {D32F: np.float32, D16: np.uint16, X8D24: np.uint32}
MAX_CODE = {D16: 65535, X8D24: 16777215}


def format_id(fmt) -> int:
    """The AtmoDepthFormat value of a name or a value; ValueError for anything else."""
    if isinstance(fmt, str):
        if fmt not in FORMATS:
            raise ValueError(f"unknown depth format {fmt!r}: one of {sorted(FORMATS)}")
        return FORMATS[fmt]
    if fmt not in NAMES:
        raise ValueError(f"unknown depth format {fmt!r}: one of {sorted(NAMES)}")
    return int(fmt)


def _texels(bits, f: int) -> np.ndarray:
    a = np.asarray(bits)
    want = np.dtype(DTYPES[f])
    if a.dtype == want:
        return a
    if a.dtype.kind in "iu" and f != D32F and a.dtype.itemsize == want.itemsize:
        return a.view(want)   # int16 / int32 carriers of the same bits
    raise ValueError(f"{NAMES[f]} texels are {want.name} arrays (or signed integers of the same width), not {a.dtype.name}")


def decode(bits, fmt) -> np.ndarray:
    """The fp32 depth of every texel, as the kernels read it."""
    f = format_id(fmt)
    a = _texels(bits, f)
    if f == D32F:
        return a.copy()
    code = a.astype(np.uint32) & np.uint32(MAX_CODE[f])
    return code.astype(np.float32) / np.float32(MAX_CODE[f])   # every code converts exactly; one IEEE fp32 division


def quantise(depth, fmt) -> np.ndarray:
    """Texels holding `depth` to the format's precision: rint(clip(d, 0, 1) * max) in float64, ties to even; d32f: the floats themselves."""
    f = format_id(fmt)
    d = np.asarray(depth, dtype=np.float32)
    if f == D32F:
        return d.copy()
    code = np.rint(np.clip(d.astype(np.float64), 0.0, 1.0) * float(MAX_CODE[f]))
    return code.astype(DTYPES[f])
