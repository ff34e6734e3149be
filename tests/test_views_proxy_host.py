"""CPU tests of the far-mode (proxy) view batches (include/atmo_views_proxy.h): the header's symbol set and the binding, every refusal of
atmo_render_views_proxy and atmo_render_views_proxy_target on a host-only context (nothing touches a device), the launch layout the host computes
(atmo_debug_views_proxy_layout) against the single proxy draw's launch rectangle and the float64 coverage of tests/proxy_geometry.py, and the families
the library was built with.  (tests/test_kernel_twins_host.py holds the static properties of the 36 kernels: tools/twin_resources.py.)
(tests/test_views_proxy_gpu.py holds the kernels to the single proxy draws' bytes bit for bit.)"""
import ctypes as C
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import proxy_geometry as G
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.scene import col_major
from test_proxy_host import _box_size, _poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, U8 = 0, 1, 2          # AtmoTargetFormat
PX = {F32: 16, F16: 8, U8: 4}
DEPTH = 0x1000
TILE_W, TILE_H = 16, 8
SIZE = _box_size(0.1)
FAR = S.Camera(64, 36, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))          # the demo planet's box (edge 208) in the middle of the picture
AWAY = S.Camera(64, 36, (0.0, 0.0, 400.0), (0.0, 0.0, 800.0))       # looking +z, the planet behind: no tile


def _frame(cam, rect=None):
    from godot_atmosphere_shader_amd import _native as N

    f = N.AtmoFrame()
    f.inv_projection_matrix[:] = [float(x) for x in col_major(cam.inv_projection)]
    f.inv_view_matrix[:] = [float(x) for x in col_major(cam.inv_view)]
    f.viewport_w, f.viewport_h = cam.width, cam.height
    f.x0, f.y0, f.x1, f.y1 = rect if rect is not None else (0, 0, cam.width, cam.height)
    return f


def _mat(m):
    return (C.c_float * 16)(*[float(x) for x in col_major(np.asarray(m, dtype=np.float64))])


def _fviews(specs):
    """specs: [(camera, rect or None, depth address, rgba address)] -> N.AtmoView array."""
    from godot_atmosphere_shader_amd import _native as N

    arr = (N.AtmoView * max(len(specs), 1))()
    for i, (cam, rect, depth, rgba) in enumerate(specs):
        arr[i].frame, arr[i].depth_dev, arr[i].rgba_dev = _frame(cam, rect), depth, rgba
    return arr


def _tviews(specs):
    """specs: [(camera, rect or None, depth address, pixels address, format, pitch in bytes)] -> N.AtmoViewTarget array."""
    from godot_atmosphere_shader_amd import _native as N

    arr = (N.AtmoViewTarget * max(len(specs), 1))()
    for i, (cam, rect, depth, pixels, fmt, pitch) in enumerate(specs):
        arr[i].frame, arr[i].depth_dev, arr[i].target = _frame(cam, rect), depth, N.AtmoTarget(pixels, fmt, pitch)
    return arr


def _host_ctx(variant, view_steps=0, light_mode=None, light_steps=0):
    from godot_atmosphere_shader_amd import _native as N

    ctx = C.c_void_p()
    lm = N.LIGHT_LUT if light_mode is None else light_mode
    assert N.load().atmo_debug_create_host_only(variant, view_steps, 0, lm, light_steps, C.byref(ctx)) == N.ATMO_OK
    return ctx


def _functions(header_name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header_name)).read(), flags=re.S)
    return set(re.findall(r"\b(atmo_[a-z0-9_]+)\s*\(", text))


def test_binding_exposes_the_views_proxy_header():
    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.build import build_native

    build_native()
    lib = N.load()
    assert _functions("atmo_views_proxy.h") == set(N.VIEWS_PROXY_SYMBOLS) == {"atmo_render_views_proxy", "atmo_render_views_proxy_target"}
    others = N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_TARGET_SYMBOLS
    assert not set(N.VIEWS_PROXY_SYMBOLS) & set(others)
    assert set(N.EXPORTED_SYMBOLS) == set(others) | set(N.VIEWS_PROXY_SYMBOLS) and len(N.EXPORTED_SYMBOLS) == len(set(N.EXPORTED_SYMBOLS))
    for sym in N.VIEWS_PROXY_SYMBOLS:
        assert getattr(lib, sym) is not None and sym in N.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "atmo_views_proxy.h")).read()
    assert '#include "atmo_views_target.h"' in header and '#include "atmo_scene.h"' in header
    # the five older headers keep their function sets, and the feature is detected by its symbols, not by the version
    assert _functions("atmo.h") == set(N.CORE_SYMBOLS) and len(N.CORE_SYMBOLS) == 22
    assert _functions("atmo_scene.h") == set(N.SCENE_SYMBOLS) == {"atmo_render_proxy", "atmo_render_proxy_composite"}
    assert _functions("atmo_target.h") == set(N.TARGET_SYMBOLS) == {"atmo_target_pixel_bytes", "atmo_render_target", "atmo_render_proxy_target"}
    assert _functions("atmo_views.h") == set(N.VIEWS_SYMBOLS) == {"atmo_render_views"}
    assert _functions("atmo_views_target.h") == set(N.VIEWS_TARGET_SYMBOLS) == {"atmo_render_views_target"}
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5
    assert "#define ATMO_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "atmo.h")).read()
    assert "atmo_debug_views_proxy_layout" in _functions("atmo_debug.h") and "atmo_debug_views_proxy_layout" in N.DEBUG_SYMBOLS
    assert lib.atmo_debug_views_proxy_layout is not None


def test_float_batch_checks_its_arguments_without_a_device():
    """Every refusal the header states for atmo_render_views_proxy, on a host-only context: the code comes back before anything touches a device, a
    well-formed batch never succeeds there, and a batch that has no tile is ATMO_OK."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    err = lambda: lib.atmo_last_error_string(ctx)                                                              # noqa: E731
    eye = _mat(np.eye(4))
    call = lambda v, k, comp=0, m=eye, size=SIZE: lib.atmo_render_views_proxy(ctx, v, k, m, C.c_float(size), comp, None)     # noqa: E731
    accepted = lambda rc: rc not in (N.ATMO_OK, N.ATMO_E_ARG)                                                  # noqa: E731
    try:
        a, b = 0x100000, 0x200000
        good = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, b)])
        # view count, null views, null context
        assert call(good, 0) == N.ATMO_OK and call(None, 0) == N.ATMO_OK
        assert call(good, -1) == N.ATMO_E_ARG and call(good, N.MAX_VIEWS + 1) == N.ATMO_E_ARG
        assert call(None, 2) == N.ATMO_E_ARG and b"null views" in err()
        assert lib.atmo_render_views_proxy(None, good, 2, eye, C.c_float(SIZE), 0, None) == N.ATMO_E_ARG
        # the box
        assert call(good, 2, m=None) == N.ATMO_E_ARG and b"null model_matrix" in err()
        for size in (0.0, -1.0, float("inf"), float("nan")):
            assert call(good, 2, size=size) == N.ATMO_E_ARG and b"box_size" in err(), size
        assert call(good, 2, m=_mat(np.zeros((4, 4)))) == N.ATMO_E_ARG and b"model_matrix is singular" in err()
        flat = np.eye(4)
        flat[1, 1] = 0.0
        assert call(good, 2, m=_mat(flat)) == N.ATMO_E_ARG and b"singular" in err()
        v = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, b)])
        v[1].frame.inv_projection_matrix[:] = [0.0] * 16
        assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"inv_projection_matrix is singular" in err()
        v = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, b)])
        v[0].frame.inv_view_matrix[:] = [0.0] * 16
        assert call(v, 2) == N.ATMO_E_ARG and b"view 0" in err() and b"inv_view_matrix is singular" in err()
        # a well-formed batch on a context without a device: refused, but not for its arguments -- plain and composite
        assert accepted(call(good, 2)) and accepted(call(good, 2, 1))
        moved = _mat(G.translation(12.0, -7.0, 30.0) @ G.rotation_y(30.0))
        assert accepted(call(good, 2, m=moved))
        # per-view checks: rect, viewport, null and misaligned pointers -- in any view, and the message names it
        for bad_rect in ((0, 0, 65, 36), (-1, 0, 64, 36), (10, 0, 5, 36), (0, 30, 64, 20)):
            v = _fviews([(FAR, None, DEPTH, a), (FAR, bad_rect, DEPTH, b)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err(), bad_rect
        v = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, b)])
        v[0].frame.viewport_w = 0
        assert call(v, 2) == N.ATMO_E_ARG and b"view 0" in err()
        v = _fviews([(FAR, None, None, a), (FAR, None, DEPTH, b)])
        assert call(v, 2) == N.ATMO_E_ARG and b"view 0" in err() and b"null device pointer" in err()
        v = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, None)])
        assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"null device pointer" in err()
        v = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, b + 8)])
        assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"16-byte aligned" in err()
        # ... also for a view whose box leaves no tile: it gets all its argument checks
        v = _fviews([(FAR, None, DEPTH, a), (AWAY, None, None, b)])
        assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"null device pointer" in err()
        # overlap: atmo_render_views' rule on the FRAME's rect (the box covers the middle of the picture only, the rects' bytes decide)
        size = 64 * 36 * 16
        v = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, a)])
        assert call(v, 2) == N.ATMO_E_ARG and b"views 0 and 1 write overlapping memory" in err()
        v = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, a + size - 16)])
        assert call(v, 2) == N.ATMO_E_ARG and b"overlapping" in err()
        v = _fviews([(FAR, None, DEPTH, a), (FAR, None, DEPTH, a + size)])
        assert accepted(call(v, 2))
        v = _fviews([(FAR, (0, 0, 64, 18), DEPTH, a), (FAR, (0, 18, 64, 36), DEPTH, a)])      # two row bands of one scene buffer
        assert accepted(call(v, 2, 1))
        v = _fviews([(FAR, (0, 0, 32, 36), DEPTH, a), (FAR, (32, 0, 64, 36), DEPTH, a)])      # side by side: interleaved rows, the float rule refuses
        assert call(v, 2, 1) == N.ATMO_E_ARG and b"overlapping" in err()
        v = _fviews([(FAR, None, DEPTH, a), (AWAY, None, DEPTH, a)])                          # ... whether the other view draws anything or not
        assert call(v, 2) == N.ATMO_E_ARG and b"overlapping" in err()
        # an empty view is skipped: its pointers are not looked at and it cannot overlap
        v = _fviews([(FAR, (5, 5, 5, 30), None, 3), (FAR, (0, 7, 64, 7), 1, None)])
        assert call(v, 2) == N.ATMO_OK
        v = _fviews([(FAR, (5, 5, 5, 30), None, 3), (FAR, None, DEPTH, a), (FAR, (0, 7, 64, 7), None, a)])
        assert accepted(call(v, 3))
        # the box behind every camera, beyond the far plane, off the rect: ATMO_OK, nothing to launch -- no device needed
        v = _fviews([(AWAY, None, DEPTH, a), (AWAY, (3, 3, 40, 30), DEPTH, b)])
        assert call(v, 2) == N.ATMO_OK and call(v, 2, 1) == N.ATMO_OK
        assert call(good, 2, m=_mat(G.translation(0.0, 0.0, -3000.0))) == N.ATMO_OK
        v = _fviews([(FAR, (0, 0, 4, 4), DEPTH, a), (AWAY, None, DEPTH, b)])
        assert call(v, 2) == N.ATMO_OK
    finally:
        lib.atmo_destroy(ctx)


def test_target_batch_checks_its_arguments_without_a_device():
    """The same for atmo_render_views_proxy_target, in all three formats: atmo_render_views_target's per-view checks, one format per batch, and its
    overlap rule -- the side-by-side halves of one image are accepted."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    err = lambda: lib.atmo_last_error_string(ctx)                                                              # noqa: E731
    eye = _mat(np.eye(4))
    call = lambda v, k, comp=0, m=eye, size=SIZE: lib.atmo_render_views_proxy_target(ctx, v, k, m, C.c_float(size), comp, None)     # noqa: E731
    accepted = lambda rc: rc not in (N.ATMO_OK, N.ATMO_E_ARG)                                                  # noqa: E731
    try:
        a, b = 0x100000, 0x200000
        for fmt in (F16, U8, F32):
            px = PX[fmt]
            good = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, b, fmt, 0)])
            assert call(good, 0) == N.ATMO_OK and call(None, 0) == N.ATMO_OK
            assert call(good, -1) == N.ATMO_E_ARG and call(good, N.MAX_VIEWS + 1) == N.ATMO_E_ARG
            assert call(None, 2) == N.ATMO_E_ARG and b"null views" in err()
            assert lib.atmo_render_views_proxy_target(None, good, 2, eye, C.c_float(SIZE), 0, None) == N.ATMO_E_ARG
            assert call(good, 2, m=None) == N.ATMO_E_ARG and b"null model_matrix" in err()
            for size in (0.0, -1.0, float("inf"), float("nan")):
                assert call(good, 2, size=size) == N.ATMO_E_ARG and b"box_size" in err(), size
            assert call(good, 2, m=_mat(np.zeros((4, 4)))) == N.ATMO_E_ARG and b"model_matrix is singular" in err()
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, b, fmt, 0)])
            v[1].frame.inv_view_matrix[:] = [0.0] * 16
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"singular" in err()
            # well-formed: plain, composite, pitched
            assert accepted(call(good, 2)) and accepted(call(good, 2, 1))
            v = _tviews([(FAR, None, DEPTH, a, fmt, (64 + 7) * px), (FAR, (3, 3, 40, 30), DEPTH, b, fmt, 64 * px)])
            assert accepted(call(v, 2))
            # per-view checks, the message names the view
            for bad_rect in ((0, 0, 65, 36), (-1, 0, 64, 36), (10, 0, 5, 36), (0, 30, 64, 20)):
                v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, bad_rect, DEPTH, b, fmt, 0)])
                assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err(), bad_rect
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, b, fmt, 0)])
            v[0].frame.viewport_h = 70000
            assert call(v, 2) == N.ATMO_E_ARG and b"view 0" in err()
            v = _tviews([(FAR, None, None, a, fmt, 0), (FAR, None, DEPTH, b, fmt, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 0" in err() and b"null device pointer" in err()
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, None, fmt, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"null target pixels" in err()
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, b + px // 2, fmt, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and f"({px} bytes)".encode() in err()
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, b + px, fmt, 0)])
            assert accepted(call(v, 2))
            for comp, rect, pitch in ((0, None, 63 * px), (0, None, 64 * px + px // 2), (1, (0, 0, 32, 36), 32 * px), (0, None, -px)):
                v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, rect, DEPTH, b, fmt, pitch)])
                assert call(v, 2, comp) == N.ATMO_E_ARG and b"view 1" in err() and b"row_pitch_bytes" in err(), (comp, rect, pitch)
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, b, 3, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"unknown target format" in err()
            other = {F16: U8, U8: F32, F32: F16}[fmt]
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, b, other, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"one format per batch" in err()
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (AWAY, None, DEPTH, b, other, 0)])      # ... for a view without a tile too
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"one format per batch" in err()
            # overlap: the same buffer; touching ranges; the side-by-side halves of ONE 128 x 36 image, plain and composite; halves one pixel too wide
            size = 64 * 36 * px
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, a, fmt, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"views 0 and 1 write overlapping memory" in err()
            v = _tviews([(FAR, None, DEPTH, a, fmt, 0), (FAR, None, DEPTH, a + size, fmt, 0)])
            assert accepted(call(v, 2))
            pitch = 128 * px
            v = _tviews([(FAR, None, DEPTH, a, fmt, pitch), (FAR, None, DEPTH, a + 64 * px, fmt, pitch)])
            assert accepted(call(v, 2)) and accepted(call(v, 2, 1))
            v = _tviews([(FAR, None, DEPTH, a, fmt, pitch), (FAR, None, DEPTH, a + 63 * px, fmt, pitch)])
            assert call(v, 2) == N.ATMO_E_ARG and b"overlapping" in err()
            v = _tviews([(FAR, (0, 0, 32, 36), DEPTH, a, fmt, 0), (FAR, (32, 0, 64, 36), DEPTH, a, fmt, 0)])      # two rects of one viewport, composite
            assert accepted(call(v, 2, 1))
            v = _tviews([(FAR, (0, 0, 33, 36), DEPTH, a, fmt, 0), (FAR, (32, 0, 64, 36), DEPTH, a, fmt, 0)])
            assert call(v, 2, 1) == N.ATMO_E_ARG and b"overlapping" in err()
            # an empty view is skipped: pointers, target and format are not looked at
            v = _tviews([(FAR, (5, 5, 5, 30), None, None, 7, 3), (FAR, (0, 7, 64, 7), None, 3, other, -1)])
            assert call(v, 2) == N.ATMO_OK
            v = _tviews([(FAR, (5, 5, 5, 30), None, None, other, 3), (FAR, None, DEPTH, a, fmt, 0), (FAR, (0, 7, 64, 7), None, a, 9, 1)])
            assert accepted(call(v, 3))
            # no view has a tile: ATMO_OK without a device
            v = _tviews([(AWAY, None, DEPTH, a, fmt, 0), (AWAY, (3, 3, 40, 30), DEPTH, b, fmt, 80 * px)])
            assert call(v, 2) == N.ATMO_OK and call(v, 2, 1) == N.ATMO_OK
    finally:
        lib.atmo_destroy(ctx)


@pytest.mark.parametrize("fmt", [None, F16, U8, F32], ids=["float", "rgba16f", "rgba8", "rgba32f"])
@pytest.mark.parametrize("mode", ["precision0", "precision2", "view_steps64", "lane_split2"])
def test_proxy_batches_need_the_default_forms(mode, fmt):
    """precision 0 / 2, 64 view steps, a forced lane split -> ATMO_E_STATE from both entry points, in every format; argument errors that need no matrix
    arithmetic come first."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH if mode == "precision0" else N.VARIANT_NO_CLOUDS, view_steps=64 if mode == "view_steps64" else 0,
                    light_mode=N.LIGHT_DIRECT, light_steps=8)
    try:
        if mode == "precision0":
            assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK
        elif mode == "precision2":
            assert lib.atmo_set_precision(ctx, 2) == N.ATMO_OK
        elif mode == "lane_split2":
            assert lib.atmo_set_lane_split(ctx, 2) == N.ATMO_OK
        eye = _mat(np.eye(4))
        if fmt is None:
            v = _fviews([(FAR, None, DEPTH, 0x100000), (FAR, None, DEPTH, 0x200000)])
            call = lambda k, comp, m=eye: lib.atmo_render_views_proxy(ctx, v, k, m, C.c_float(SIZE), comp, None)            # noqa: E731
        else:
            v = _tviews([(FAR, None, DEPTH, 0x100000, fmt, 0), (FAR, None, DEPTH, 0x200000, fmt, 80 * PX[fmt])])
            call = lambda k, comp, m=eye: lib.atmo_render_views_proxy_target(ctx, v, k, m, C.c_float(SIZE), comp, None)     # noqa: E731
        for composite in (0, 1):
            assert call(2, composite) == N.ATMO_E_STATE
            assert b"no proxy kernel" in lib.atmo_last_error_string(ctx)
        assert call(0, 0) == N.ATMO_OK                                    # no views: nothing to refuse
        assert call(2, 0, None) == N.ATMO_E_ARG                           # arguments are checked in front of the mode
        if fmt is None:
            v[1].depth_dev = None
        else:
            v[1].target.format = 5
        assert call(2, 0) == N.ATMO_E_ARG and b"view 1" in lib.atmo_last_error_string(ctx)
    finally:
        lib.atmo_destroy(ctx)


def _in_one_space(cam, model, common):
    """The camera of a (camera, model) pose carried into the space of the batch's one model: inv_view' = common inv(model) inv_view, so that
    inv(common) inv_view' inv_projection -- all the proxy geometry sees -- is the pose's inv(model) inv_view inv_projection."""
    return SimpleNamespace(width=cam.width, height=cam.height, inv_projection=cam.inv_projection, near=cam.near,
                           inv_view=common @ np.linalg.inv(model) @ np.asarray(cam.inv_view, dtype=np.float64))


def _layout_views():
    """Eight views of one box: the five poses of tests/test_proxy_host.py, a camera looking away, an empty rect, a 251 x 141 view with a partial rect."""
    common = G.translation(5.0, -3.0, 2.0) @ G.rotation_y(10.0)
    cams = [_in_one_space(cam, model, common) for _, cam, model in _poses()]
    rects = [None] * 5
    cams.append(_in_one_space(AWAY, np.eye(4), common))
    rects.append(None)
    cams.append(cams[0])
    rects.append((40, 20, 40, 50))
    cams.append(_in_one_space(S.Camera(251, 141, (31.0, 17.0, 420.0), (0.0, 0.0, 0.0)), np.eye(4), common))
    rects.append((17, 9, 250, 141))
    return common, cams, rects


@pytest.mark.parametrize("variant", ["no_clouds", "clouds_high_rm"])
def test_layout_is_the_single_draws_launch_per_view(variant):
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS if variant == "no_clouds" else N.VARIANT_CLOUDS_HIGH_RM)
    try:
        common, cams, rects = _layout_views()
        n = len(cams)
        assert n == N.MAX_VIEWS
        views = _fviews([(cam, rect, None, None) for cam, rect in zip(cams, rects)])       # the pointers are not looked at
        model = _mat(common)
        first, grid, out = (C.c_int * (n + 1))(), (C.c_int * (2 * n))(), (C.c_int * (4 * n))()
        rc = lib.atmo_debug_views_proxy_layout(ctx, views, n, model, C.c_float(SIZE), first, grid, out)
        assert rc == N.ATMO_OK, lib.atmo_last_error_string(ctx)
        first, grid = list(first), [(grid[2 * i], grid[2 * i + 1]) for i in range(n)]
        cut = [tuple(out[4 * i:4 * i + 4]) for i in range(n)]
        tiles = [gx * gy for gx, gy in grid]
        for i in range(n):
            x0, y0, x1, y1 = rects[i] or (0, 0, cams[i].width, cams[i].height)
            if x0 == x1 or y0 == y1:
                assert tiles[i] == 0 and grid[i] == (0, 0) and cut[i] == (x0, y0, x0, y0), i
                continue
            # the single proxy draw's launch of that view alone
            r1, t1 = (C.c_int * 4)(), C.c_int(-1)
            assert lib.atmo_debug_proxy_launch_rect(ctx, C.byref(views[i].frame), model, C.c_float(SIZE), r1, C.byref(t1)) == N.ATMO_OK
            assert cut[i] == tuple(r1) and tiles[i] == t1.value, (i, cut[i], tuple(r1), tiles[i], t1.value)
            cx0, cy0, cx1, cy1 = cut[i]
            assert x0 <= cx0 <= cx1 <= x1 and y0 <= cy0 <= cy1 <= y1, (i, cut[i])
            if tiles[i]:   # a host-only context has no mip chain: the level-0 sampler, the grid starts at the rectangle
                assert grid[i] == ((cx1 - cx0 + TILE_W - 1) // TILE_W, (cy1 - cy0 + TILE_H - 1) // TILE_H), (i, grid[i], cut[i])
            else:
                assert grid[i] == (0, 0) and (cx0 == cx1 or cy0 == cy1)
            # every covered pixel of the view's rect lies inside its rectangle
            ys, xs = np.meshgrid(np.arange(y0, y1, dtype=np.float64), np.arange(x0, x1, dtype=np.float64), indexing="ij")
            covered, _ = G.coverage(cams[i], common, SIZE, xs, ys)
            if covered.any():
                py, px = ys[covered], xs[covered]
                assert cx0 <= px.min() and px.max() < cx1 and cy0 <= py.min() and py.max() < cy1, (i, cut[i])
            else:
                assert i == 5
        assert tiles[5] == 0 and tiles[6] == 0 and all(tiles[i] > 0 for i in (0, 1, 2, 3, 4, 7)), tiles
        # first_block is the prefix of the grids; every block maps to exactly one (view, tile), as the kernels look it up
        assert first == [int(s) for s in np.concatenate([[0], np.cumsum(tiles)])]
        table = first + [first[-1]] * (N.MAX_VIEWS + 1 - len(first))
        seen = set()
        for blk in range(first[-1]):
            view = sum(1 for i in range(1, N.MAX_VIEWS) if blk >= table[i])
            local = blk - table[view]
            assert tiles[view] > 0 and 0 <= local < tiles[view], (blk, view, local)
            seen.add((view, local))
        assert len(seen) == first[-1] == sum(tiles)
        # the checks are the batch's
        assert lib.atmo_debug_views_proxy_layout(ctx, views, n, None, C.c_float(SIZE), (C.c_int * 9)(), (C.c_int * 16)(), (C.c_int * 32)()) == N.ATMO_E_ARG
        assert lib.atmo_debug_views_proxy_layout(ctx, views, n, model, C.c_float(SIZE), None, (C.c_int * 16)(), (C.c_int * 32)()) == N.ATMO_E_ARG
        assert lib.atmo_debug_views_proxy_layout(ctx, views, 9, model, C.c_float(SIZE), (C.c_int * 10)(), (C.c_int * 18)(), (C.c_int * 36)()) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)



def test_every_default_form_entry_point_has_the_same_families():
    """The proxy draws, the view batches, the packed-target draws and their combinations are all launched from ONE list of families (ATMO_DEFAULT_FAMILIES in
    csrc/atmo_kernels.hip): the thirteen default forms, five of them with the unrolled LSTEPS == 8 twin -- 18 (FLAGS, LSTEPS) pairs.  Read back from the
    library as built: each of the six kernels exists for exactly those pairs under its own family bits, and atmo_render_target_kernel for those with
    SPLIT 1, the KF_GEO twin of the direct-light family and the SPLIT 2 form of the two declared-sampler cloud families, and nothing else."""
    from godot_atmosphere_shader_amd.build import build_native

    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf of the ROCm toolchain not found")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import loop_phase
    finally:
        sys.path.pop(0)
    import tempfile

    CLOUDS, RM, DIRECT, LITE, PRECISE, LOD, GEO, PROXY, TARGET, VIEWS = 1, 2, 4, 8, 16, 32, 256, 512, 1024, 2048   # KernelFlags (csrc/atmo_device.h)
    plain = [0, PRECISE | CLOUDS, PRECISE | CLOUDS | RM, LOD | PRECISE | CLOUDS, LOD | PRECISE | CLOUDS | RM, PRECISE | LITE, PRECISE | LITE | CLOUDS,
             LOD | PRECISE | LITE | CLOUDS]
    direct = [DIRECT, PRECISE | CLOUDS | DIRECT, PRECISE | CLOUDS | RM | DIRECT, LOD | PRECISE | CLOUDS | DIRECT, LOD | PRECISE | CLOUDS | RM | DIRECT]
    want = {(f, 0) for f in plain + direct} | {(f, 8) for f in direct}
    assert len(plain) + len(direct) == 13 and len(want) == 18

    with tempfile.TemporaryDirectory(prefix="families_") as tmp:
        co = loop_phase.device_code_object(build_native(), os.path.join(tmp, "dev.co"))
        syms = subprocess.run([f"{loop_phase.LLVM}/llvm-readelf", "-sW", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for line in syms.splitlines():
        m = re.search(r"\d+(atmo_render_[a-z_]*kernel)ILi(\d+)ELi(\d+)E(?:Li(\d+)E)?E", line.split()[-1]) if " FUNC " in line else None
        if m:
            found.setdefault(m.group(1), set()).add(tuple(int(g) for g in m.groups()[1:] if g is not None))
    for kernel, bits in (("atmo_render_proxy_kernel", PROXY), ("atmo_render_views_kernel", VIEWS), ("atmo_render_proxy_target_kernel", PROXY | TARGET),
                         ("atmo_render_views_target_kernel", VIEWS | TARGET), ("atmo_render_views_proxy_kernel", VIEWS | PROXY),
                         ("atmo_render_views_proxy_target_kernel", VIEWS | PROXY | TARGET)):
        got = found[kernel]
        assert all(f & (PROXY | TARGET | VIEWS | GEO) == bits for f, _ in got), (kernel, sorted(got))
        assert {(f & ~bits, l) for f, l in got} == want, (kernel, sorted(got))
    got = found["atmo_render_target_kernel"]
    assert all(f & (PROXY | TARGET | VIEWS) == TARGET for f, _, _ in got), sorted(got)
    want_target = {(f, l, 1) for f, l in want} | {(DIRECT | GEO, 8, 1), (DIRECT | GEO, 0, 1)} | {(LOD | PRECISE | CLOUDS, 0, 2), (LOD | PRECISE | CLOUDS | RM, 0, 2)}
    assert {(f & ~TARGET, l, s) for f, l, s in got} == want_target, sorted(got)
