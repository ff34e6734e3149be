"""CPU tests of the sRGB, BGRA and 10-bit colour targets (include/atmo_target.h, formats 16 .. 19): the two sRGB tables rebuilt from their definition with
exact rational arithmetic against targets.py and csrc/atmo_srgb_tables.h, the contract of targets.py on known answers, the capability query and the
constants, and every argument and state check of the draws on a host-only context.  (tests/test_target_formats_gpu.py holds the kernels to targets.py
bit for bit.)"""
import ctypes as C
import hashlib
import os
import re
from fractions import Fraction as Fr

import numpy as np
import pytest

from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T
from godot_atmosphere_shader_amd.scene import col_major

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = ("rgba8_srgb", "bgra8", "bgra8_srgb", "a2b10g10r10")
DEPTH = 0x1000


def _bits(x):
    return np.asarray(x, dtype=f32).view(np.uint32)


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------

A, B, LIN, JX, JE = Fr(55, 1000), Fr(1055, 1000), Fr(1292, 100), Fr(31308, 10 ** 7), Fr(4045, 10 ** 5)


def _enc_ge(x, c):
    """E(x) >= c, exactly: 1.055 x^(1/2.4) - 0.055 >= c  <=>  x^5 >= ((c + 0.055) / 1.055)^12."""
    x = Fr(float(x))
    return LIN * x >= c if x <= JX else x ** 5 >= ((c + A) / B) ** 12


@pytest.fixture(scope="module")
def exact_tables():
    """THRESH by bisection over the bit patterns of [0, 1] (which order as the floats do), DECODE as the float whose rounding interval holds D(k / 255)."""
    thresh = np.zeros(256, dtype=np.uint32)
    for k in range(1, 256):
        c = Fr(2 * k - 1, 510)
        lo, hi = 0, int(_bits(1.0))
        assert not _enc_ge(0.0, c) and _enc_ge(1.0, c)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _enc_ge(np.uint32(mid).view(f32), c):
                hi = mid
            else:
                lo = mid
        thresh[k] = hi
    decode = np.zeros(256, dtype=np.uint32)
    for k in range(1, 256):
        e = Fr(k, 255)
        guess = int(_bits(k / 255 / 12.92 if e <= JE else ((k / 255 + 0.055) / 1.055) ** 2.4))
        hits = []
        for b in range(guess - 2, guess + 3):
            v = [Fr(float(np.uint32(b + d).view(f32))) for d in (-1, 0, 1)]
            lo, hi = (v[0] + v[1]) / 2, (v[1] + v[2]) / 2
            if e <= JE:
                inside = lo <= e / LIN <= hi
            else:
                c12 = ((e + A) / B) ** 12
                inside = lo ** 5 <= c12 <= hi ** 5
            if inside:
                hits.append(b)
        assert len(hits) == 1, (k, hits)      # no value lies on a midpoint: the nearest float is unique
        decode[k] = hits[0]
    return thresh.view(f32), decode.view(f32)


def _header_tables():
    text = open(os.path.join(ROOT, "godot_atmosphere_shader_amd", "csrc", "atmo_srgb_tables.h")).read()
    out = {}
    for name in ("ATMO_SRGB_THRESH_BITS", "ATMO_SRGB_DECODE_BITS"):
        body = re.search(r"#define " + name + r" \\\n((?:.*\\\n)+)", text).group(1)
        out[name] = np.array([int(h, 16) for h in re.findall(r"0x([0-9a-f]{8})u", body)], dtype=np.uint32).view(f32)
    return out["ATMO_SRGB_THRESH_BITS"], out["ATMO_SRGB_DECODE_BITS"]


def test_srgb_tables_are_the_definition(exact_tables):
    thresh, decode = exact_tables
    assert T.SRGB_THRESH.dtype == f32 and T.SRGB_DECODE.dtype == f32 and T.SRGB_THRESH.shape == T.SRGB_DECODE.shape == (256,)
    assert np.array_equal(_bits(T.SRGB_THRESH), _bits(thresh)) and np.array_equal(_bits(T.SRGB_DECODE), _bits(decode))
    h_thresh, h_decode = _header_tables()
    assert h_thresh.shape == h_decode.shape == (256,)
    assert np.array_equal(_bits(h_thresh), _bits(thresh)) and np.array_equal(_bits(h_decode), _bits(decode))
    # the generator prints the committed header
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_srgb_tables", os.path.join(ROOT, "tools", "make_srgb_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.c_text() + "\n" == open(os.path.join(ROOT, "godot_atmosphere_shader_amd", "csrc", "atmo_srgb_tables.h")).read()
    # fingerprints and anchors
    assert hashlib.sha256(thresh.astype("<f4").tobytes()).hexdigest().startswith("6cbb4b361c72c797")
    assert hashlib.sha256(decode.astype("<f4").tobytes()).hexdigest().startswith("48a8f05136456237")
    assert thresh[0] == 0.0 and decode[0] == 0.0 and decode[255] == 1.0
    for got, want in ((thresh[1], "0.0001517635"), (thresh[11], "0.003188301"), (thresh[128], "0.21404114"), (thresh[255], "0.99554527"),
                      (decode[1], "0.000303527"), (decode[128], "0.2158605")):
        assert f32(want) == got, (got, want)
    assert np.all(np.diff(thresh[1:]) > 0) and thresh[1] > 0
    assert np.array_equal(T.srgb_encode(decode), np.arange(256))
    assert T.srgb_encode(f32(0.0031308)) == 10        # the junction of the two segments lies inside code 10, away from every threshold
    # the plain fp64 formulas, rounded as the definitions say, give the same tables
    k = np.arange(1, 256)
    c = (k - 0.5) / 255
    t64 = np.where(c <= 12.92 * 0.0031308, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    t32 = t64.astype(f32)
    t32 = np.where(t32.astype(np.float64) < t64, np.nextafter(t32, f32(2.0)), t32)
    e = np.arange(256) / 255
    d32 = np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4).astype(f32)
    assert np.array_equal(t32, thresh[1:]) and np.array_equal(d32, decode)


# ---- known answers ------------------------------------------------------------------------------------------------------------------------------

def test_srgb_encoding_on_known_answers():
    th = T.SRGB_THRESH
    k = np.arange(1, 256)
    assert np.array_equal(T.srgb_encode(th[1:]), k)
    assert np.array_equal(T.srgb_encode(np.nextafter(th[1:], f32(-1.0))), k - 1)
    sub = np.uint32(1).view(f32)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, sub, -sub, 2.0, 1.0, -1.0, 3e38], dtype=f32)
    assert list(T.srgb_encode(special)) == [0, 0, 255, 0, 0, 0, 0, 0, 255, 255, 0, 255]
    px = np.array([[0.5, np.nan, 2.0, 0.5], [th[128], np.nextafter(th[128], f32(0)), -0.0, np.nan]], dtype=f32)
    assert T.encode(px, "rgba8_srgb").tolist() == [[188, 0, 255, 128], [128, 127, 0, 0]]          # alpha is UNORM8: 0.5 * 255 = 127.5 -> 128 (even)
    assert T.encode(px, "bgra8_srgb").tolist() == [[255, 0, 188, 128], [0, 127, 128, 0]]
    assert T.encode(px[0], T.RGBA8_SRGB).dtype == np.uint8
    # decode is the table, alpha byte / 255
    b = np.array([[1, 128, 255, 51]], dtype=np.uint8)
    d = T.decode(b, "rgba8_srgb")
    assert d.dtype == f32 and d.tolist() == [[float(T.SRGB_DECODE[1]), float(T.SRGB_DECODE[128]), 1.0, float(f32(51) / f32(255))]]
    assert T.decode(b, "bgra8_srgb").tolist() == [[1.0, float(T.SRGB_DECODE[128]), float(T.SRGB_DECODE[1]), float(f32(51) / f32(255))]]


def test_a2b10g10r10_on_known_answers():
    enc = lambda px: int(T.encode(np.array(px, dtype=f32), "a2b10g10r10").view("<u4")[0])     # noqa: E731
    assert enc([1, 0, 0, 1]) == 0xC00003FF
    assert enc([0, 1, 0, 0]) == 0x000FFC00 and enc([0, 0, 1, 0]) == 0x3FF00000 and enc([0, 0, 0, 1 / 3]) == 0x40000000
    assert T.encode(np.array([1, 0, 0, 1], dtype=f32), "rgb10a2").tolist() == [0xFF, 0x03, 0x00, 0xC0]      # the word's little-endian bytes
    assert enc([np.nan, -1.0, np.inf, np.nan]) == 0x3FF00000 and enc([-0.0, -np.inf, 2.0, -np.nan]) == 0x3FF00000
    # ties of the fp32 product c * 1023.0f go to even: for k = 0, 1, 2, 510 the float nearest (k + 0.5) / 1023, times 1023.0f, rounds to k + 0.5 exactly
    c = np.array([0.5 / 1023, 1.5 / 1023, 2.5 / 1023, 510.5 / 1023], dtype=np.float64).astype(f32)
    prod = c * f32(1023.0)
    assert prod.tolist() == [0.5, 1.5, 2.5, 510.5]
    codes = T.encode(np.stack([c, c, c, np.zeros_like(c)], axis=-1), "a2b10g10r10").view("<u4")[:, 0] & 1023
    assert codes.tolist() == [0, 2, 2, 510]
    # ... and the fp32 neighbours of such a tie fall to either side
    x = c[-1]
    around = np.array([np.nextafter(x, f32(0)), x, np.nextafter(x, f32(1))], dtype=f32)
    got = T.encode(np.stack([around, around, around, around], axis=-1), "a2b10g10r10").view("<u4")[:, 0]
    assert np.array_equal(got & 1023, np.rint(around * f32(1023.0)).astype(np.uint32))
    assert np.array_equal(got >> 30, np.rint(around * f32(3.0)).astype(np.uint32))
    # 2-bit alpha: 0.5 * 3 = 1.5 -> 2 (even), 1 / 6 * 3 = 0.5 -> 0 (even) when the product is exactly the tie
    assert enc([0, 0, 0, 0.5]) >> 30 == 2
    sixth = f32(1 / 6)
    assert enc([0, 0, 0, sixth]) >> 30 == int(np.rint(sixth * f32(3.0)))
    # decode: field / 1023.0f, alpha / 3.0f, as IEEE fp32 divisions; decode inverts encode on every code
    word = (np.arange(1024, dtype=np.uint32) | ((1023 - np.arange(1024, dtype=np.uint32)) << 10) | (np.uint32(513) << 20)
            | ((np.arange(1024, dtype=np.uint32) & 3) << 30))
    buf = word.astype("<u4").view(np.uint8).reshape(1024, 4)
    d = T.decode(buf, "a2b10g10r10")
    assert d.dtype == f32 and d.shape == (1024, 4)
    assert np.array_equal(d[:, 0], np.arange(1024, dtype=f32) / f32(1023.0)) and np.array_equal(d[:, 1], d[::-1, 0])
    assert np.all(d[:, 2] == f32(513) / f32(1023.0)) and np.array_equal(d[:, 3], (np.arange(1024) & 3).astype(f32) / f32(3.0))
    assert np.array_equal(T.encode(d, "a2b10g10r10"), buf)


def test_bgra_is_rgba_with_bytes_0_and_2_exchanged():
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.25, 1.25, size=(4096, 4)).astype(f32)
    for rgba, bgra in (("rgba8", "bgra8"), ("rgba8_srgb", "bgra8_srgb")):
        a, b = T.encode(x, rgba), T.encode(x, bgra)
        assert a.dtype == b.dtype == np.uint8 and np.array_equal(b, a[:, [2, 1, 0, 3]]) and not np.array_equal(a, b)
        buf = rng.integers(0, 256, size=(4096, 4), dtype=np.uint8)
        assert np.array_equal(T.decode(buf, bgra), T.decode(buf[:, [2, 1, 0, 3]], rgba))
        src = np.concatenate([x[:, :3], rng.uniform(0, 1, size=(4096, 1)).astype(f32)], axis=1)
        assert np.array_equal(T.blend(src, buf, bgra), T.blend(src, buf[:, [2, 1, 0, 3]], rgba)[:, [2, 1, 0, 3]])
    assert np.array_equal(T.encode(x, "bgra8_unorm"), T.encode(x, "bgra8")) and T.format_id("bgra8_unorm") == 17
    assert T.decode(np.array([[255, 0, 51, 255]], dtype=np.uint8), "bgra8").tolist() == [[float(f32(51) / f32(255)), 0.0, 1.0, 1.0]]


def test_blend_is_decode_blend_encode_on_hand_computed_pixels():
    src = np.array([[1.0, 0.0, 0.25, 0.5]], dtype=f32)
    # RGBA8_SRGB over bytes (0, 255, 128, 255): R 1 * .5 + 0 * .5 = .5 -> 188; G 0 + 1 * .5 -> 188; B .125 + DECODE[128] * .5; A .5 + 1 * .5 = 1
    dst = np.array([[0, 255, 128, 255]], dtype=np.uint8)
    b = f32(0.25) * f32(0.5) + T.SRGB_DECODE[128] * f32(0.5)
    assert T.blend(src, dst, "rgba8_srgb").tolist() == [[188, 188, int(T.srgb_encode(b)), 255]]
    assert abs(float(b) - 0.23293) < 1e-5 and int(T.srgb_encode(b)) == 133
    # the same pixel as BGRA8_SRGB memory: bytes B, G, R, A
    assert T.blend(src, dst[:, [2, 1, 0, 3]], "bgra8_srgb").tolist() == [[133, 188, 188, 255]]
    # BGRA8_UNORM over memory (B 255, G 0, R 51, A 0): R 1 * .5 + .2 * .5 = .6 -> 153; G 0; B .125 + .5 = .625 -> 159.375 -> 159; A .5 -> 127.5 -> 128
    assert T.blend(src, np.array([[255, 0, 51, 0]], dtype=np.uint8), "bgra8").tolist() == [[159, 0, 153, 128]]
    # A2B10G10R10 over R 1023, G 0, B 511, A 3: R 1 -> 1023; G 0; B .125 + 511 / 1023 * .5 = 0.37475.. -> 383.37 -> 383; A .5 + .5 = 1 -> 3
    word = np.array([1023 | (0 << 10) | (511 << 20) | (3 << 30)], dtype="<u4")
    out = T.blend(src, word.view(np.uint8).reshape(1, 4), "a2b10g10r10").view("<u4")[0, 0]
    assert (int(out) & 1023, (int(out) >> 10) & 1023, (int(out) >> 20) & 1023, int(out) >> 30) == (1023, 0, 383, 3)
    # alpha 0 leaves the decoded destination, re-encoded: every code survives the round trip in all four formats
    rng = np.random.default_rng(5)
    dst = rng.integers(0, 256, size=(2048, 4), dtype=np.uint8)
    zero = np.zeros((2048, 4), dtype=f32)
    for fmt in NEW:
        assert np.array_equal(T.blend(zero, dst, fmt), dst), fmt
        with pytest.raises(TypeError):
            T.decode(dst.astype(np.float32), fmt)
        with pytest.raises(ValueError):
            T.encode(np.zeros((5, 3), dtype=f32), fmt)


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------------

def test_constants_and_the_capability_query():
    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.build import build_native

    build_native()
    lib = N.load()
    assert [lib.atmo_target_pixel_bytes(f) for f in (16, 17, 18, 19)] == [4, 4, 4, 4]
    assert [lib.atmo_target_pixel_bytes(f) for f in list(range(3, 16)) + [20]] == [0] * 14
    header = open(os.path.join(ROOT, "include", "atmo_target.h")).read()
    names = dict(re.findall(r"\b(ATMO_TARGET_[A-Z0-9_]+)\s*=\s*(\d+)", header))
    assert {k: int(v) for k, v in names.items()} == {"ATMO_TARGET_RGBA32F": 0, "ATMO_TARGET_RGBA16F": 1, "ATMO_TARGET_RGBA8_UNORM": 2, "ATMO_TARGET_RGBA8_SRGB": 16,
                                                     "ATMO_TARGET_BGRA8_UNORM": 17, "ATMO_TARGET_BGRA8_SRGB": 18, "ATMO_TARGET_A2B10G10R10_UNORM": 19}
    assert (N.TARGET_RGBA8_SRGB, N.TARGET_BGRA8_UNORM, N.TARGET_BGRA8_SRGB, N.TARGET_A2B10G10R10_UNORM) == (16, 17, 18, 19)
    assert (T.RGBA8_SRGB, T.BGRA8, T.BGRA8_SRGB, T.A2B10G10R10) == (16, 17, 18, 19)
    assert [T.format_id(n) for n in ("rgba8_srgb", "bgra8", "bgra8_unorm", "bgra8_srgb", "a2b10g10r10", "rgb10a2", "RGBA8_SRGB")] == [16, 17, 17, 18, 19, 19, 16]
    for f in (16, 17, 18, 19):
        assert T.PIXEL_BYTES[f] == lib.atmo_target_pixel_bytes(f) and T.DTYPES[f] is np.uint8 and T.format_id(f) == f
    assert T.format_id(np.uint8) == T.RGBA8 == 2                  # a uint8 buffer keeps meaning RGBA8_UNORM
    for bad in (3, 15, 20):
        with pytest.raises(ValueError):
            T.format_id(bad)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5


def _frame(cam, rect=None):
    from godot_atmosphere_shader_amd import _native as N

    f = N.AtmoFrame()
    f.inv_projection_matrix[:] = [float(x) for x in col_major(cam.inv_projection)]
    f.inv_view_matrix[:] = [float(x) for x in col_major(cam.inv_view)]
    f.viewport_w, f.viewport_h = cam.width, cam.height
    f.x0, f.y0, f.x1, f.y1 = rect if rect is not None else (0, 0, cam.width, cam.height)
    return f


def _host_ctx(variant, view_steps=0, light_mode=None, light_steps=0):
    from godot_atmosphere_shader_amd import _native as N

    ctx = C.c_void_p()
    lm = N.LIGHT_LUT if light_mode is None else light_mode
    assert N.load().atmo_debug_create_host_only(variant, view_steps, 0, lm, light_steps, C.byref(ctx)) == N.ATMO_OK
    return ctx


def _views(specs):
    from godot_atmosphere_shader_amd import _native as N

    arr = (N.AtmoViewTarget * max(len(specs), 1))()
    for i, (cam, rect, pixels, fmt, pitch) in enumerate(specs):
        arr[i].frame = _frame(cam, rect)
        arr[i].depth_dev = DEPTH
        arr[i].target = N.AtmoTarget(pixels, fmt, pitch)
    return arr


@pytest.mark.parametrize("fmt", [16, 17, 18, 19], ids=NEW)
def test_new_formats_pass_the_argument_checks_without_a_device(fmt):
    """Alignment (4 bytes), pitch (0, or at least the row -- the rect's, a composite's the viewport's -- and a multiple of 4): ATMO_E_ARG before anything
    touches a device, in the single draws and in the batches.  A well-formed call on a host-only context fails, but not for its arguments."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    err = lambda: lib.atmo_last_error_string(ctx)                                           # noqa: E731
    try:
        cam = S.Camera(64, 36, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
        f, sub = _frame(cam), _frame(cam, (8, 4, 40, 30))
        m = (C.c_float * 16)(*[float(x) for x in col_major(np.eye(4))])
        depth = C.c_void_p(DEPTH)

        def both(frame, target, composite):
            return (lib.atmo_render_target(ctx, C.byref(frame), depth, C.byref(target), composite, None),
                    lib.atmo_render_proxy_target(ctx, C.byref(frame), m, C.c_float(10.0), depth, C.byref(target), composite, None))

        E = (N.ATMO_E_ARG, N.ATMO_E_ARG)
        assert both(f, N.AtmoTarget(4096 + 2, fmt, 0), 0) == E and b"aligned" in err() and b"(4 bytes)" in err()
        assert both(f, N.AtmoTarget(4096 + 1, fmt, 0), 1) == E
        assert N.ATMO_E_ARG not in both(f, N.AtmoTarget(4096 + 4, fmt, 0), 0)
        assert both(f, N.AtmoTarget(None, fmt, 0), 0) == E
        assert both(f, N.AtmoTarget(4096, fmt, 64 * 4 - 4), 0) == E and b"row_pitch_bytes" in err()     # short
        assert both(f, N.AtmoTarget(4096, fmt, 64 * 4 + 2), 0) == E                                       # odd
        assert both(f, N.AtmoTarget(4096, fmt, -256), 0) == E
        assert both(sub, N.AtmoTarget(4096, fmt, 32 * 4), 1) == E and b"row_pitch_bytes" in err()        # a composite's row is the viewport's
        for frame, pitch, comp in ((f, 0, 0), (f, 0, 1), (f, 64 * 4, 0), (f, 71 * 4, 1), (sub, 32 * 4, 0)):
            for rc in both(frame, N.AtmoTarget(4096, fmt, pitch), comp):
                assert rc not in (N.ATMO_OK, N.ATMO_E_ARG), (pitch, comp)
        # the batches: the same checks per view, and one format per batch
        a, b = 0x100000, 0x200000
        for name, call in (("views", lambda v, comp=0: lib.atmo_render_views_target(ctx, v, 2, comp, None)),
                           ("proxy", lambda v, comp=0: lib.atmo_render_views_proxy_target(ctx, v, 2, m, C.c_float(10.0), comp, None))):
            assert call(_views([(cam, None, a, fmt, 0), (cam, None, b, fmt, 0)])) not in (N.ATMO_OK, N.ATMO_E_ARG), name
            assert call(_views([(cam, None, a, fmt, 71 * 4), (cam, (3, 3, 40, 30), b, fmt, 64 * 4)]), 1) not in (N.ATMO_OK, N.ATMO_E_ARG), name
            assert call(_views([(cam, None, a, fmt, 0), (cam, None, b + 2, fmt, 0)])) == N.ATMO_E_ARG and b"view 1" in err() and b"(4 bytes)" in err()
            assert call(_views([(cam, None, a, fmt, 0), (cam, None, b, fmt, 63 * 4)])) == N.ATMO_E_ARG and b"row_pitch_bytes" in err()
            assert call(_views([(cam, None, a, fmt, 0), (cam, None, b, fmt, 64 * 4 + 2)])) == N.ATMO_E_ARG and b"row_pitch_bytes" in err()
            assert call(_views([(cam, None, a, fmt, 0), (cam, (0, 0, 32, 36), b, fmt, 32 * 4)]), 1) == N.ATMO_E_ARG and b"row_pitch_bytes" in err()
            for other in (f for f in (0, 1, 2, 16, 17, 18, 19) if f != fmt):
                assert call(_views([(cam, None, a, fmt, 0), (cam, None, b, other, 0)])) == N.ATMO_E_ARG, (name, other)
                assert b"view 1" in err() and b"one format per batch" in err()
            assert call(_views([(cam, None, a, fmt, 0), (cam, None, b, 20, 0)])) == N.ATMO_E_ARG and b"unknown target format" in err()
            # the halves of one double-wide image, side by side: accepted
            assert call(_views([(cam, None, a, fmt, 128 * 4), (cam, None, a + 64 * 4, fmt, 128 * 4)]), 1) not in (N.ATMO_OK, N.ATMO_E_ARG), name
        # atmo_debug_store_target
        assert lib.atmo_debug_store_target(ctx, fmt, 0, None, depth, 16, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_store_target(ctx, fmt, 1, depth, None, 16, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_store_target(ctx, fmt, 0, depth, C.c_void_p(4098), 16, None) == N.ATMO_E_ARG and b"aligned" in err()
        assert lib.atmo_debug_store_target(ctx, fmt, 0, C.c_void_p(4104), depth, 16, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_store_target(ctx, fmt, 0, depth, depth, (1 << 31) + 1, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_store_target(ctx, 20, 0, depth, depth, 16, None) == N.ATMO_E_ARG and b"unknown target format" in err()
    finally:
        lib.atmo_destroy(ctx)


def test_a_batch_of_rgba8_srgb_and_bgra8_srgb_is_two_formats():
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    try:
        cam = S.Camera(64, 36, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
        v = _views([(cam, None, 0x100000, N.TARGET_RGBA8_SRGB, 0), (cam, None, 0x200000, N.TARGET_BGRA8_SRGB, 0)])
        assert lib.atmo_render_views_target(ctx, v, 2, 1, None) == N.ATMO_E_ARG
        assert b"view 1" in lib.atmo_last_error_string(ctx) and b"one format per batch" in lib.atmo_last_error_string(ctx)
    finally:
        lib.atmo_destroy(ctx)


@pytest.mark.parametrize("mode", ["precision0", "precision2", "view_steps64", "lane_split2"])
def test_new_formats_need_the_default_forms(mode):
    """The packed kernels exist for what a default context draws with: precision 0 / 2, 64 view steps, a forced lane split -> ATMO_E_STATE, with the
    message of the older packed formats."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    if mode == "precision0":
        ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
        assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK
    elif mode == "precision2":
        ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
        assert lib.atmo_set_precision(ctx, 2) == N.ATMO_OK
    elif mode == "view_steps64":
        ctx = _host_ctx(N.VARIANT_NO_CLOUDS, view_steps=64, light_mode=N.LIGHT_DIRECT, light_steps=8)
    else:
        ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
        assert lib.atmo_set_lane_split(ctx, 2) == N.ATMO_OK
    try:
        cam = S.Camera(64, 36, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
        f = _frame(cam)
        m = (C.c_float * 16)(*[float(x) for x in col_major(np.eye(4))])
        depth = C.c_void_p(DEPTH)
        for fmt in (16, 17, 18, 19):
            for composite in (0, 1):
                t = N.AtmoTarget(4096, fmt, 0)
                assert lib.atmo_render_target(ctx, C.byref(f), depth, C.byref(t), composite, None) == N.ATMO_E_STATE
                assert b"no RGBA16F / RGBA8 kernel" in lib.atmo_last_error_string(ctx)
                v = _views([(cam, None, 0x100000, fmt, 0), (cam, None, 0x200000, fmt, 0)])
                assert lib.atmo_render_views_target(ctx, v, 2, composite, None) == N.ATMO_E_STATE
                if mode != "precision0":   # (a cloud variant without its textures fails on those first, with ATMO_E_STATE all the same)
                    assert lib.atmo_render_proxy_target(ctx, C.byref(f), m, C.c_float(10.0), depth, C.byref(t), composite, None) == N.ATMO_E_STATE
                    assert b"no proxy kernel" in lib.atmo_last_error_string(ctx)
                    assert lib.atmo_render_views_proxy_target(ctx, v, 2, m, C.c_float(10.0), composite, None) == N.ATMO_E_STATE
    finally:
        lib.atmo_destroy(ctx)


# ---- the code bracket of a tolerance (tests/test_target_formats_kernels_gpu.py holds the kernels' frames to the CPU oracle with it) ------------------

def stored_fields(buf, fmt):
    """The stored codes of (..., 4) bytes of a format 16 .. 19 in R, G, B, A order, as int64: the bytes un-swizzled, or the word's 10- / 2-bit fields."""
    b = np.ascontiguousarray(buf, dtype=np.uint8)
    if T.format_id(fmt) == T.A2B10G10R10:
        w = b.view("<u4")[..., 0].astype(np.int64)
        return np.stack([w & 1023, (w >> 10) & 1023, (w >> 20) & 1023, w >> 30], axis=-1)
    return (b[..., [2, 1, 0, 3]] if T.format_id(fmt) in (T.BGRA8, T.BGRA8_SRGB) else b).astype(np.int64)


def code_bracket(o, fmt, tol):
    """(code(lo), code(hi)) for lo, hi = o -/+ tol * max(1, |o|), per field: code = targets.encode of that field (sRGB through SRGB_THRESH, UNORM with 255 /
    1023 / 3).  Every code function is monotone (non-decreasing) in its fp32 argument, and rounding lo and hi to fp32 is monotone too, so an fp32 x within the
    tolerance of o has code(lo) <= code(x) <= code(hi): the bracket carries no quantisation term."""
    o = np.asarray(o, dtype=np.float64)
    m = tol * np.maximum(1.0, np.abs(o))
    return stored_fields(T.encode(o - m, fmt), fmt), stored_fields(T.encode(o + m, fmt), fmt)


def _bracket_sources():
    th = T.SRGB_THRESH[1:]
    grid = (np.arange(2 ** 17 + 1, dtype=np.float64) * 2.0 ** -16 - 0.5).astype(f32)           # [-0.5, 1.5] in steps of 2^-16, exact in fp32
    return np.concatenate([th, np.nextafter(th, f32(-1.0)), np.nextafter(th, f32(2.0)), grid]).astype(f32)


@pytest.mark.parametrize("fmt", NEW)
def test_code_bracket_is_monotone_and_collapses_away_from_thresholds(fmt):
    """code_bracket at common.TOL on every sRGB threshold with its fp32 neighbours and on a 2^-16 grid of [-0.5, 1.5], the same value in all four fields:
    values within the tolerance encode inside the bracket; the bracket is one code wherever no threshold of the field lies within the tolerance (and never
    more than two codes: 2 TOL max(1, |o|) is below the narrowest code, 1 / 3295 at the foot of the sRGB curve and 1 / 1023 in a 10-bit field)."""
    from common import TOL

    o = _bracket_sources()
    lo, hi = code_bracket(np.stack([o] * 4, axis=-1), fmt, TOL)
    assert lo.shape == hi.shape == (o.size, 4) and np.all(lo <= hi) and np.all(hi - lo <= 1)
    m = TOL * np.maximum(1.0, np.abs(o.astype(np.float64)))
    rng = np.random.default_rng(5)
    for frac in (-1.0, -0.999, -0.5, 0.0, 0.5, 0.999, 1.0, None):
        d = rng.uniform(-1.0, 1.0, size=o.size) if frac is None else frac
        x64 = o.astype(np.float64) + d * m
        x = x64.astype(f32)
        # only fp32 values that do lie within the tolerance (the rounding of o + d m may step outside by half an ulp at d = +/-1)
        inside = np.abs(x.astype(np.float64) - o.astype(np.float64)) <= m
        assert inside.mean() > 0.4, frac
        c = stored_fields(T.encode(np.stack([x] * 4, axis=-1), fmt), fmt)
        assert np.all((lo <= c)[inside]) and np.all((c <= hi)[inside]), (fmt, frac)
    # the endpoints themselves
    assert np.array_equal(stored_fields(T.encode(np.stack([o.astype(np.float64) - m] * 4, axis=-1), fmt), fmt), lo)
    # away from thresholds: one code.  The thresholds of a field, as reals: SRGB_THRESH[k], or (k + 0.5) / N of a UNORM field (the fp32 product's own rounding
    # moves a UNORM threshold by less than 2^-22, allowed for below)
    srgb = T.format_id(fmt) in (T.RGBA8_SRGB, T.BGRA8_SRGB)
    tens = T.format_id(fmt) == T.A2B10G10R10
    for field in range(4):
        if srgb and field < 3:
            edges = T.SRGB_THRESH[1:].astype(np.float64)
        else:
            n = (3 if field == 3 else 1023) if tens else 255
            edges = (np.arange(n) + 0.5) / n
        i = np.clip(np.searchsorted(edges, o.astype(np.float64)), 1, edges.size - 1)
        dist = np.minimum(np.abs(o - edges[i - 1]), np.abs(o - edges[i]))
        away = dist > m + 2.0 ** -20
        assert away.mean() > 0.7, (fmt, field, away.mean())
        assert np.array_equal(lo[away, field], hi[away, field]), (fmt, field)
        wide = float((lo[:, field] != hi[:, field]).mean())
        print(f"{fmt} field {field}: the bracket holds two codes for {wide:.4f} of the sources")
        assert (lo[:, field] != hi[:, field]).any()              # ... and two next to one: the sources do straddle thresholds
    # known answers (SRGB_THRESH[188] = D(187.5 / 255) = 0.49991 lies between 0.4999 and 0.5001; alpha 0.5 * 255 = 127.5 between 127.47 and 127.53)
    assert [x.tolist() for x in code_bracket([[0.5, 0.0, 1.0, 0.5]], "rgba8_srgb", 1e-4)] == [[[187, 0, 255, 127]], [[188, 0, 255, 128]]]
    assert [x.tolist() for x in code_bracket([[0.5, 0.0, 2.0, 0.5]], "a2b10g10r10", 1e-4)] == [[[511, 0, 1023, 1]], [[512, 0, 1023, 2]]]
    assert stored_fields(np.array([[1, 2, 3, 4]], dtype=np.uint8), "bgra8").tolist() == [[3, 2, 1, 4]]
