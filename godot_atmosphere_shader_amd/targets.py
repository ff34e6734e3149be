"""The numerical contract of the packed colour targets (include/atmo_target.h) in numpy: what atmo_render_target stores into, and blends with, an
RGBA16F, RGBA8_UNORM, RGBA8_SRGB, BGRA8_UNORM, BGRA8_SRGB or A2B10G10R10_UNORM buffer.  Pure numpy, no device: the tests hold the kernels to these
functions bit for bit, and a host can use them to prepare or read a target.

    encode(rgba_f32, fmt)          fp32 channels -> the stored bits
    decode(buf, fmt)               stored bits -> fp32, exactly
    blend(src_f32, dst_buf, fmt)   decode(dst) -> the fp32 blend of atmo_render_composite (blend_mix) -> encode, once

fmt: "rgba32f" | "rgba16f" | "rgba8" | "rgba8_srgb" | "bgra8" | "bgra8_srgb" | "a2b10g10r10" (or the AtmoTargetFormat value 0 | 1 | 2 | 16 .. 19).
Buffers are float32 / float16 / uint8 arrays.  The three formats of ATMO_ABI_VERSION 5's first header take any shape in encode and decode; the four
4-byte formats added later (values 16 .. 19) are (..., 4) uint8 arrays, the bytes as they lie in memory (A2B10G10R10: the four little-endian bytes of
the 32-bit word), and encode / decode take (..., 4) RGBA floats.  blend takes (..., 4) arrays, RGBA last.

The sRGB channels are two tables, and the tables are the contract (SRGB_DECODE, SRGB_THRESH; csrc/atmo_srgb_tables.h holds the same bits,
tools/make_srgb_tables.py writes them): decode is a look-up, encode counts the thresholds at or below the value.  No pow is evaluated anywhere.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

RGBA32F, RGBA16F, RGBA8 = 0, 1, 2
RGBA8_SRGB, BGRA8, BGRA8_SRGB, A2B10G10R10 = 16, 17, 18, 19   # 3 .. 15 and everything from 20 up are unknown formats
FORMATS = {"rgba32f": RGBA32F, "rgba16f": RGBA16F, "rgba8": RGBA8, "rgba8_unorm": RGBA8, "rgba8_srgb": RGBA8_SRGB, "bgra8": BGRA8, "bgra8_unorm": BGRA8,
           "bgra8_srgb": BGRA8_SRGB, "a2b10g10r10": A2B10G10R10, "rgb10a2": A2B10G10R10}
DTYPES = {RGBA32F: np.float32, RGBA16F: np.float16, RGBA8: np.uint8, RGBA8_SRGB: np.uint8, BGRA8: np.uint8, BGRA8_SRGB: np.uint8, A2B10G10R10: np.uint8}
PIXEL_BYTES = {RGBA32F: 16, RGBA16F: 8, RGBA8: 4, RGBA8_SRGB: 4, BGRA8: 4, BGRA8_SRGB: 4, A2B10G10R10: 4}
HALF_QNAN = 0x7E00   # the one NaN an RGBA16F store writes
_SRGB = (RGBA8_SRGB, BGRA8_SRGB)
_BGRA = (BGRA8, BGRA8_SRGB)


def _srgb_tables():
    """(SRGB_THRESH, SRGB_DECODE) by the rational procedure of include/atmo_target.h: the decimal constants of the sRGB curves as exact rationals,
    x^(12/5) <> c decided as x^5 <> c^12.  The fp64 formula proposes a float; exact comparisons move it to the defined one."""
    a, b, lin, jx, je = Fraction(55, 1000), Fraction(1055, 1000), Fraction(1292, 100), Fraction(31308, 10 ** 7), Fraction(4045, 10 ** 5)
    up, down = np.float32(2.0), np.float32(-1.0)

    def enc_ge(xf, c):   # E(x) >= c, exactly
        x = Fraction(float(xf))
        return lin * x >= c if x <= jx else x ** 5 >= ((c + a) / b) ** 12

    def dec_cmp(k, m):   # D(k / 255) >= m, exactly (m > 0)
        e = Fraction(k, 255)
        return e / lin >= m if e <= je else ((e + a) / b) ** 12 >= m ** 5

    thresh = np.zeros(256, dtype=np.float32)
    for k in range(1, 256):
        c = (k - 0.5) / 255.0
        t = np.float32(c / 12.92 if c <= 12.92 * 0.0031308 else ((c + 0.055) / 1.055) ** 2.4)
        exact = Fraction(2 * k - 1, 510)
        while enc_ge(np.nextafter(t, down), exact):
            t = np.nextafter(t, down)
        while not enc_ge(t, exact):
            t = np.nextafter(t, up)
        thresh[k] = t
    decode_ = np.zeros(256, dtype=np.float32)
    for k in range(1, 256):
        e = k / 255.0
        f = np.float32(e / 12.92 if e <= 0.04045 else ((e + 0.055) / 1.055) ** 2.4)
        while not dec_cmp(k, (Fraction(float(f)) + Fraction(float(np.nextafter(f, down)))) / 2):   # D below the lower midpoint
            f = np.nextafter(f, down)
        while dec_cmp(k, (Fraction(float(f)) + Fraction(float(np.nextafter(f, up)))) / 2) and f < np.float32(1.0):   # D at or above the upper one
            f = np.nextafter(f, up)
        decode_[k] = f
    return thresh, decode_


# SRGB_THRESH[k], k = 1 .. 255: the smallest fp32 x with E(x) >= (k - 0.5) / 255 (SRGB_THRESH[0] = 0.0 is a filler); SRGB_DECODE[k]: the fp32
# nearest to D(k / 255)
SRGB_THRESH, SRGB_DECODE = _srgb_tables()
SRGB_THRESH.setflags(write=False)
SRGB_DECODE.setflags(write=False)


def format_id(fmt) -> int:
    """A format's name, a numpy or torch dtype (uint8 means RGBA8_UNORM), or an AtmoTargetFormat value -> the AtmoTargetFormat value."""
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


def _unorm(x, scale) -> np.ndarray:
    """rint(clamp(x, 0, 1) * scale) with the product in fp32, ties to even, NaN -> 0; as uint32."""
    c = np.where(np.isnan(x), np.float32(0.0), x)
    c = np.minimum(np.maximum(c, np.float32(0.0)), np.float32(1.0)).astype(np.float32)
    return np.rint(c * np.float32(scale)).astype(np.uint32)


def srgb_encode(x) -> np.ndarray:
    """fp32 -> sRGB code: the number of k in 1 .. 255 with x >= SRGB_THRESH[k]; NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        code = np.searchsorted(SRGB_THRESH[1:], np.where(np.isnan(x), np.float32(0.0), x), side="right")
    return code.astype(np.uint8)


def encode(rgba_f32, fmt) -> np.ndarray:
    """fp32 -> stored bits.  RGBA16F: IEEE binary16, round-to-nearest-even, subnormals kept, overflow to infinity, every NaN -> the quiet NaN 0x7e00.
    RGBA8: (uint8) rint(clamp(x, 0, 1) * 255) with the product in fp32, ties to even, NaN -> 0.  BGRA8: the same with bytes 0 and 2 exchanged.
    RGBA8_SRGB / BGRA8_SRGB: R, G, B through srgb_encode, A as RGBA8's.  A2B10G10R10: the same rule with 1023 (R, G, B) and 3 (A), packed into
    one little-endian word, R in bits 0-9."""
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
        if f == RGBA8:
            return _unorm(x, 255.0).astype(np.uint8)
        if x.ndim == 0 or x.shape[-1] != 4:
            raise ValueError(f"encode: a {fmt} pixel is (..., 4) RGBA floats")
        if f == A2B10G10R10:
            word = _unorm(x[..., 0], 1023.0) | (_unorm(x[..., 1], 1023.0) << 10) | (_unorm(x[..., 2], 1023.0) << 20) | (_unorm(x[..., 3], 3.0) << 30)
            return np.ascontiguousarray(word.astype("<u4")).view(np.uint8).reshape(x.shape)
        out = np.empty(x.shape, dtype=np.uint8)
        out[..., :3] = srgb_encode(x[..., :3]) if f in _SRGB else _unorm(x[..., :3], 255.0)
        out[..., 3] = _unorm(x[..., 3], 255.0)
        if f in _BGRA:
            out = out[..., [2, 1, 0, 3]]
        return np.ascontiguousarray(out)


def decode(buf, fmt) -> np.ndarray:
    """stored bits -> fp32, exactly: binary16 -> float (subnormals included); byte / 255.0f as an IEEE fp32 division; an sRGB byte through
    SRGB_DECODE; a 10-bit (2-bit) field / 1023.0f (3.0f).  The formats 16 .. 19 return (..., 4) RGBA."""
    f = format_id(fmt)
    b = np.asarray(buf)
    if b.dtype != DTYPES[f]:
        raise TypeError(f"a {fmt} buffer is {np.dtype(DTYPES[f]).name}, not {b.dtype.name}")
    if f == RGBA8:
        return b.astype(np.float32) / np.float32(255.0)
    if f in (RGBA32F, RGBA16F):
        return b.astype(np.float32)
    if b.ndim == 0 or b.shape[-1] != 4:
        raise ValueError(f"decode: a {fmt} buffer is (..., 4) bytes")
    if f == A2B10G10R10:
        word = np.ascontiguousarray(b).view("<u4")[..., 0]
        rgb = np.stack([word & 1023, (word >> 10) & 1023, (word >> 20) & 1023], axis=-1).astype(np.float32) / np.float32(1023.0)
        return np.concatenate([rgb, ((word >> 30).astype(np.float32) / np.float32(3.0))[..., None]], axis=-1)
    if f in _BGRA:
        b = b[..., [2, 1, 0, 3]]
    out = np.empty(b.shape, dtype=np.float32)
    out[..., :3] = SRGB_DECODE[b[..., :3]] if f in _SRGB else b[..., :3].astype(np.float32) / np.float32(255.0)
    out[..., 3] = b[..., 3].astype(np.float32) / np.float32(255.0)
    return out


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
