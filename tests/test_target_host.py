"""CPU tests of the packed colour targets (include/atmo_target.h): the header's symbol set and the binding, the capability query, the argument and state
checks of atmo_render_target / atmo_render_proxy_target on a host-only context, and the numerical contract as godot_atmosphere_shader_amd/targets.py
states it, on chosen values.  (tests/test_target_gpu.py holds the kernels to that statement bit for bit.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T
from godot_atmosphere_shader_amd.scene import col_major

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(cam, rect=None):
    from godot_atmosphere_shader_amd import _native as N

    f = N.AtmoFrame()
    f.inv_projection_matrix[:] = [float(x) for x in col_major(cam.inv_projection)]
    f.inv_view_matrix[:] = [float(x) for x in col_major(cam.inv_view)]
    f.viewport_w, f.viewport_h = cam.width, cam.height
    f.x0, f.y0, f.x1, f.y1 = rect if rect is not None else (0, 0, cam.width, cam.height)
    return f


def test_binding_exposes_the_target_header():
    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.build import build_native

    build_native()
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "atmo_target.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(atmo_[a-z0-9_]+)\s*\(", header)) == set(N.TARGET_SYMBOLS)
    assert not set(N.TARGET_SYMBOLS) & set(N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS)
    for sym in N.TARGET_SYMBOLS + ("atmo_debug_store_target",):
        assert getattr(lib, sym) is not None and sym in N.EXPORTED_SYMBOLS
    assert "atmo_debug_store_target" in N.DEBUG_SYMBOLS
    # the feature is detected by its symbols and the query, not by the version: atmo.h and atmo_scene.h are what they were
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5
    assert [lib.atmo_target_pixel_bytes(f) for f in (N.TARGET_RGBA32F, N.TARGET_RGBA16F, N.TARGET_RGBA8_UNORM)] == [16, 8, 4]
    assert [lib.atmo_target_pixel_bytes(f) for f in (-1, 3, 1000)] == [0, 0, 0]
    assert (T.RGBA32F, T.RGBA16F, T.RGBA8) == (N.TARGET_RGBA32F, N.TARGET_RGBA16F, N.TARGET_RGBA8_UNORM)
    assert C.sizeof(N.AtmoTarget) == 16 and N.AtmoTarget.format.offset == 8 and N.AtmoTarget.row_pitch_bytes.offset == 12


def _host_ctx(variant, view_steps=0, light_mode=None, light_steps=0):
    from godot_atmosphere_shader_amd import _native as N

    ctx = C.c_void_p()
    lm = N.LIGHT_LUT if light_mode is None else light_mode
    assert N.load().atmo_debug_create_host_only(variant, view_steps, 0, lm, light_steps, C.byref(ctx)) == N.ATMO_OK
    return ctx


def test_target_entry_points_check_their_arguments_without_a_device():
    """Null target, unknown format, misaligned pixels, a pitch below the row or not a multiple of the pixel size: ATMO_E_ARG, before anything touches a
    device.  A host-only context never draws, so a well-formed call fails too -- but not with ATMO_E_ARG."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    try:
        cam = S.Camera(64, 36, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
        f = _frame(cam)
        sub = _frame(cam, (8, 4, 40, 30))   # 32 pixels wide
        m = (C.c_float * 16)(*[float(x) for x in col_major(np.eye(4))])
        depth = C.c_void_p(4096)

        def both(frame, target, composite):
            t = C.byref(target) if target is not None else None
            return (lib.atmo_render_target(ctx, C.byref(frame), depth, t, composite, None),
                    lib.atmo_render_proxy_target(ctx, C.byref(frame), m, C.c_float(10.0), depth, t, composite, None))

        E = (N.ATMO_E_ARG, N.ATMO_E_ARG)
        assert both(f, None, 0) == E and b"null target" in lib.atmo_last_error_string(ctx)
        assert both(f, N.AtmoTarget(4096, 3, 0), 0) == E and b"format" in lib.atmo_last_error_string(ctx)
        assert both(f, N.AtmoTarget(4096, -1, 0), 1) == E
        assert both(f, N.AtmoTarget(None, N.TARGET_RGBA16F, 0), 0) == E
        # alignment to the pixel size: 16 / 8 / 4 bytes
        for fmt, px in ((N.TARGET_RGBA32F, 16), (N.TARGET_RGBA16F, 8), (N.TARGET_RGBA8_UNORM, 4)):
            assert both(f, N.AtmoTarget(4096 + px // 2, fmt, 0), 0) == E and b"aligned" in lib.atmo_last_error_string(ctx)
            assert N.ATMO_E_ARG not in both(f, N.AtmoTarget(4096 + px, fmt, 0), 0)
            # pitch: 0 or >= the row's bytes -- the RECT's row for a plain draw, the VIEWPORT's for a composite -- and a multiple of the pixel size
            assert both(f, N.AtmoTarget(4096, fmt, 64 * px - px), 0) == E and b"row_pitch_bytes" in lib.atmo_last_error_string(ctx)
            assert both(f, N.AtmoTarget(4096, fmt, 64 * px + px // 2), 0) == E
            assert both(f, N.AtmoTarget(4096, fmt, -64 * px), 0) == E
            assert N.ATMO_E_ARG not in both(f, N.AtmoTarget(4096, fmt, 64 * px), 0)
            assert N.ATMO_E_ARG not in both(f, N.AtmoTarget(4096, fmt, 71 * px), 1)
            assert N.ATMO_E_ARG not in both(sub, N.AtmoTarget(4096, fmt, 32 * px), 0)    # a rect's rows are the rect's width ...
            assert both(sub, N.AtmoTarget(4096, fmt, 32 * px), 1) == E                    # ... a composite's the viewport's
        # a well-formed call on a context without a device fails, but never succeeds and never blames the arguments
        for rc in both(f, N.AtmoTarget(4096, N.TARGET_RGBA16F, 0), 0):
            assert rc not in (N.ATMO_OK, N.ATMO_E_ARG)
        bad = _frame(cam, (0, 0, 65, 36))
        assert both(bad, N.AtmoTarget(4096, N.TARGET_RGBA8_UNORM, 0), 0) == E
        assert lib.atmo_render_target(ctx, None, depth, C.byref(N.AtmoTarget(4096, 1, 0)), 0, None) == N.ATMO_E_ARG
        assert lib.atmo_render_target(None, C.byref(f), depth, C.byref(N.AtmoTarget(4096, 1, 0)), 0, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_store_target(ctx, 7, 0, depth, depth, 16, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_store_target(ctx, N.TARGET_RGBA16F, 0, None, depth, 16, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_store_target(ctx, N.TARGET_RGBA16F, 0, depth, C.c_void_p(4100), 16, None) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)


@pytest.mark.parametrize("mode", ["precision0", "precision2", "view_steps64", "lane_split2"])
def test_packed_targets_need_the_default_forms(mode):
    """The RGBA16F / RGBA8 kernels exist for what a default context draws with: precision 0 / 2, 64 view steps, a forced lane split -> ATMO_E_STATE."""
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
        depth = C.c_void_p(4096)
        for fmt in (N.TARGET_RGBA16F, N.TARGET_RGBA8_UNORM):
            for composite in (0, 1):
                t = N.AtmoTarget(4096, fmt, 0)
                assert lib.atmo_render_target(ctx, C.byref(f), depth, C.byref(t), composite, None) == N.ATMO_E_STATE
                assert b"no RGBA16F / RGBA8 kernel" in lib.atmo_last_error_string(ctx)
                if mode != "precision0":   # (a cloud variant without its textures fails on those first, with ATMO_E_STATE all the same)
                    assert lib.atmo_render_proxy_target(ctx, C.byref(f), m, C.c_float(10.0), depth, C.byref(t), composite, None) == N.ATMO_E_STATE
                    assert b"no proxy kernel" in lib.atmo_last_error_string(ctx)
    finally:
        lib.atmo_destroy(ctx)


def _h(bits):
    return np.array(bits, dtype=np.uint16).view(np.float16)


def test_half_encoding_on_chosen_values():
    f32 = np.float32
    enc = lambda x: T.encode(np.array(x, dtype=f32), "rgba16f").view(np.uint16)   # noqa: E731
    one = 0x3C00
    # ties to even: 1 + 2^-11 lies between 1 (even significand) and 1 + 2^-10; 1 + 3 * 2^-11 between 1 + 2^-10 (odd) and 1 + 2^-9 (even)
    assert list(enc([1.0, 1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, 1.0 + 2.0 ** -10])) == [one, one, one + 2, one + 1]
    assert float(_h([one + 2])[0]) == 1.0 + 2.0 ** -9
    # just off the ties: the fp32 neighbours of 1 + 2^-11
    assert list(enc([np.nextafter(f32(1.0 + 2.0 ** -11), f32(0.0)), np.nextafter(f32(1.0 + 2.0 ** -11), f32(2.0))])) == [one, one + 1]
    # overflow: 65504 is the largest half, 65520 = 65504 + 16 the tie that goes to the even side, infinity; the fp32 below it still rounds to 65504
    below = np.nextafter(f32(65520.0), f32(0.0))
    assert list(enc([65504.0, below, 65520.0, 1e9, np.inf, -below, -65520.0, -np.inf])) == [0x7BFF, 0x7BFF, 0x7C00, 0x7C00, 0x7C00, 0xFBFF, 0xFC00, 0xFC00]
    # subnormals: spacing 2^-24 below 2^-14; 2^-25 is the tie between 0 and the smallest subnormal (-> 0, even), its upper neighbour -> 1
    assert list(enc([2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, np.nextafter(f32(2.0 ** -25), f32(1.0)), 1e-10])) == [
        0x0400, 0x03FF, 0x0001, 0x0002, 0x0000, 0x0001, 0x0000]
    assert list(enc([511.5 * 2.0 ** -24, 512.5 * 2.0 ** -24])) == [0x0200, 0x0200]       # ties inside the subnormal range, both to the even pattern
    # signed zero is kept; every NaN becomes THE quiet NaN
    assert list(enc([0.0, -0.0, -(2.0 ** -26)])) == [0x0000, 0x8000, 0x8000]
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(f32)
    assert list(T.encode(nans, T.RGBA16F).view(np.uint16)) == [T.HALF_QNAN] * 4
    # decode is exact and inverts encode on every pattern that is not a NaN
    allh = np.arange(65536, dtype=np.uint16).view(np.float16)
    keep = ~np.isnan(allh)
    assert keep.sum() == 65536 - 2 * 1023
    dec = T.decode(allh[keep], "rgba16f")
    assert dec.dtype == np.float32 and np.array_equal(dec.astype(np.float64), allh[keep].astype(np.float64))
    assert np.array_equal(T.encode(dec, "rgba16f").view(np.uint16), allh[keep].view(np.uint16))
    assert float(T.decode(_h([0x0001]), 1)[0]) == 2.0 ** -24 and float(T.decode(_h([0x7BFF]), 1)[0]) == 65504.0


def test_unorm8_encoding_on_chosen_values():
    f32 = np.float32
    k = np.arange(256)
    assert np.array_equal(T.encode((k / 255.0).astype(f32), "rgba8"), k.astype(np.uint8))
    # (k + 0.5) / 255 in fp32, times 255 in fp32: where the product is exactly k + 0.5 the tie goes to the even byte; the statement is the fp32 product's rint
    x = ((k[:-1] + 0.5) / 255.0).astype(f32)
    prod = x * f32(255.0)
    assert prod.dtype == np.float32
    want = np.where(prod == k[:-1] + 0.5, k[:-1] + (k[:-1] & 1), np.where(prod > k[:-1] + 0.5, k[:-1] + 1, k[:-1]))
    got = T.encode(x, "rgba8")
    assert np.array_equal(got, want.astype(np.uint8))
    ties = prod == k[:-1] + 0.5
    assert (ties & (k[:-1] % 2 == 0)).any() and (ties & (k[:-1] % 2 == 1)).any()     # both parities are exercised by exact ties
    assert np.all(got[ties] % 2 == 0)
    # exact half-way products built directly: (k + 0.5) is representable, so rint's ties-to-even is visible without the division
    assert list(np.rint(np.array([0.5, 1.5, 2.5, 253.5, 254.5], dtype=f32)).astype(np.uint8)) == [0, 2, 2, 254, 254]
    # clamp and NaN
    assert list(T.encode(np.array([-0.0, -1e-3, -5.0, -np.inf, 1.0, 1.0 + 2.0 ** -20, 1.18, 65504.0, np.inf, np.nan, -np.nan], dtype=f32), T.RGBA8)) == [
        0, 0, 0, 0, 255, 255, 255, 255, 255, 0, 0]
    b = np.arange(256, dtype=np.uint8)
    dec = T.decode(b, "rgba8")
    assert dec.dtype == np.float32 and np.array_equal(dec, (b.astype(np.float64) / 255.0).astype(f32))   # the correctly rounded quotient
    assert np.array_equal(T.encode(dec, "rgba8"), b)
    with pytest.raises(TypeError):
        T.decode(b, "rgba16f")
    with pytest.raises(ValueError):
        T.encode(dec, "rgb10a2")


def test_blend_is_decode_blend_encode():
    f32 = np.float32
    src = np.array([[0.25, 0.5, 1.5, 0.5], [1.0, 2.0, 3.0, 0.0], [1.0, 2.0, 3.0, 1.0], [0.1, 0.2, 0.3, 1.0 / 3.0]], dtype=f32)
    dst16 = np.array([[1.0, 0.5, 0.25, 1.0], [1.0, 2.0, 4.0, 0.5], [7.0, 7.0, 7.0, 7.0], [0.3, 0.6, 0.9, 0.75]], dtype=np.float16)
    out = T.blend(src, dst16, "rgba16f")
    assert out.dtype == np.float16
    assert np.array_equal(out[1].view(np.uint16), dst16[1].view(np.uint16))                       # alpha 0 leaves the destination's bits
    assert np.array_equal(out[2].view(np.uint16), T.encode(src[2], 1).view(np.uint16))           # alpha 1 stores the source
    d = dst16[3].astype(f32)
    a = src[3, 3]
    ia = f32(1.0) - a
    want = np.array([src[3, 0] * a + d[0] * ia, src[3, 1] * a + d[1] * ia, src[3, 2] * a + d[2] * ia, a + d[3] * ia], dtype=f32)
    assert np.array_equal(out[3].view(np.uint16), want.astype(np.float16).view(np.uint16))
    dst8 = np.array([[255, 128, 0, 255], [1, 2, 3, 4], [9, 9, 9, 9], [10, 200, 30, 77]], dtype=np.uint8)
    out8 = T.blend(src, dst8, "rgba8")
    assert out8.dtype == np.uint8 and np.array_equal(out8[1], dst8[1]) and list(out8[2]) == [255, 255, 255, 255]
    d = dst8[0].astype(f32) / f32(255.0)
    want0 = np.rint(np.clip(np.array([f32(0.25) * f32(0.5) + d[0] * f32(0.5), f32(0.5) * f32(0.5) + d[1] * f32(0.5), f32(1.5) * f32(0.5) + d[2] * f32(0.5),
                                      f32(0.5) + d[3] * f32(0.5)], dtype=f32), 0, 1) * f32(255.0))
    assert list(out8[0]) == [int(v) for v in want0]
    # inf * 0 is born a NaN whose sign differs between machines: the stored bits do not
    weird = T.blend(np.array([[np.inf, -np.inf, 1.0, 0.0]], dtype=f32), np.array([[1.0, 1.0, np.inf, 1.0]], dtype=np.float16), 1).view(np.uint16)
    assert list(weird[0]) == [T.HALF_QNAN, T.HALF_QNAN, 0x7C00, 0x3C00]
    assert np.array_equal(T.blend(src, src.copy(), "rgba32f")[:, 3], src[:, 3] + src[:, 3] * (f32(1.0) - src[:, 3]))
