"""CPU tests of the multi-view draw (include/atmo_views.h): the header's symbol set and the binding, the argument and state checks of atmo_render_views on a
host-only context (nothing touches a device), the concatenated launch atmo_debug_views_layout reports -- every tile of every non-empty view exactly
once.  (tests/test_kernel_twins_host.py holds the static properties of the kernels: the headline twin's loop position; registers, stack and loads
against the atmo_render twins.)
(tests/test_views_gpu.py holds the kernels to atmo_render's pictures bit for bit.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.scene import col_major

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_W, TILE_H = 16, 8      # a workgroup's tile of the one-lane kernels


def _frame(cam, rect=None):
    from godot_atmosphere_shader_amd import _native as N

    f = N.AtmoFrame()
    f.inv_projection_matrix[:] = [float(x) for x in col_major(cam.inv_projection)]
    f.inv_view_matrix[:] = [float(x) for x in col_major(cam.inv_view)]
    f.viewport_w, f.viewport_h = cam.width, cam.height
    f.x0, f.y0, f.x1, f.y1 = rect if rect is not None else (0, 0, cam.width, cam.height)
    return f


def _views(specs):
    """specs: [(camera, rect or None, depth address, rgba address)] -> (N.AtmoView array, n)."""
    from godot_atmosphere_shader_amd import _native as N

    arr = (N.AtmoView * max(len(specs), 1))()
    for i, (cam, rect, depth, rgba) in enumerate(specs):
        arr[i].frame = _frame(cam, rect)
        arr[i].depth_dev = depth
        arr[i].rgba_dev = rgba
    return arr, len(specs)


def _host_ctx(variant, view_steps=0, light_mode=None, light_steps=0):
    from godot_atmosphere_shader_amd import _native as N

    ctx = C.c_void_p()
    lm = N.LIGHT_LUT if light_mode is None else light_mode
    assert N.load().atmo_debug_create_host_only(variant, view_steps, 0, lm, light_steps, C.byref(ctx)) == N.ATMO_OK
    return ctx


def test_binding_exposes_the_views_header():
    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.build import build_native

    build_native()
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "atmo_views.h")).read()
    assert "#define ATMO_MAX_VIEWS 8" in header and N.MAX_VIEWS == 8
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(atmo_[a-z0-9_]+)\s*\(", header)) == set(N.VIEWS_SYMBOLS) == {"atmo_render_views"}
    assert not set(N.VIEWS_SYMBOLS) & set(N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS)
    for sym in N.VIEWS_SYMBOLS + ("atmo_debug_views_layout",):
        assert getattr(lib, sym) is not None and sym in N.EXPORTED_SYMBOLS
    assert "atmo_debug_views_layout" in N.DEBUG_SYMBOLS
    debug_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "atmo_debug.h")).read(), flags=re.S)
    assert re.search(r"\batmo_debug_views_layout\s*\(", debug_header)
    # the feature is detected by its symbol, not by the version: atmo.h is what it was
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5 and len(N.CORE_SYMBOLS) == 22
    assert "#define ATMO_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "atmo.h")).read()


def test_atmoview_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of AtmoView as a C compiler sees the header against the ctypes structure."""
    from godot_atmosphere_shader_amd import _native as N

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "atmo_views.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(AtmoView), offsetof(AtmoView, frame), offsetof(AtmoView, depth_dev), '
                   'offsetof(AtmoView, rgba_dev), ATMO_MAX_VIEWS); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(N.AtmoView), N.AtmoView.frame.offset, N.AtmoView.depth_dev.offset, N.AtmoView.rgba_dev.offset, N.MAX_VIEWS]


def test_render_views_checks_its_arguments_without_a_device():
    """Every refusal the header states, on a host-only context: the code comes back before anything touches a device, and a well-formed batch never
    succeeds there."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    try:
        cam = S.Camera(64, 36, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
        px = 64 * 36 * 16
        a, b = 0x10000, 0x10000 + px            # two disjoint outputs
        good, n = _views([(cam, None, 0x1000, a), (cam, None, 0x1000, b)])
        call = lambda v, k, comp=0: lib.atmo_render_views(ctx, v, k, comp, None)   # noqa: E731
        # view count
        assert call(good, 0) == N.ATMO_OK and call(None, 0) == N.ATMO_OK
        assert call(good, -1) == N.ATMO_E_ARG and call(good, N.MAX_VIEWS + 1) == N.ATMO_E_ARG
        assert call(None, 2) == N.ATMO_E_ARG
        assert lib.atmo_render_views(None, good, 2, 0, None) == N.ATMO_E_ARG
        # per-view checks: rect, viewport, null pointers, alignment -- in any view
        for bad_rect in ((0, 0, 65, 36), (-1, 0, 64, 36), (10, 0, 5, 36), (0, 30, 64, 20)):
            v, _ = _views([(cam, None, 0x1000, a), (cam, bad_rect, 0x1000, b)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in lib.atmo_last_error_string(ctx), bad_rect
        v, _ = _views([(cam, None, 0x1000, a), (cam, None, 0x1000, b)])
        v[0].frame.viewport_w = 0
        assert call(v, 2) == N.ATMO_E_ARG and b"view 0" in lib.atmo_last_error_string(ctx)
        v, _ = _views([(cam, None, None, a), (cam, None, 0x1000, b)])
        assert call(v, 2) == N.ATMO_E_ARG and b"null device pointer" in lib.atmo_last_error_string(ctx)
        v, _ = _views([(cam, None, 0x1000, a), (cam, None, 0x1000, None)])
        assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in lib.atmo_last_error_string(ctx)
        v, _ = _views([(cam, None, 0x1000, a), (cam, None, 0x1000, b + 8)])
        assert call(v, 2) == N.ATMO_E_ARG and b"16-byte aligned" in lib.atmo_last_error_string(ctx)
        # overlap of the written byte ranges: the same buffer, a buffer starting inside another, one byte range touching the next is fine
        v, _ = _views([(cam, None, 0x1000, a), (cam, None, 0x1000, a)])
        assert call(v, 2) == N.ATMO_E_ARG and b"overlapping" in lib.atmo_last_error_string(ctx)
        v, _ = _views([(cam, None, 0x1000, a), (cam, None, 0x1000, b - 16)])
        assert call(v, 2) == N.ATMO_E_ARG and b"overlapping" in lib.atmo_last_error_string(ctx)
        v, _ = _views([(cam, (0, 0, 64, 18), 0x1000, a), (cam, (0, 18, 64, 36), 0x1000, a + 64 * 18 * 16 - 16)])
        assert call(v, 2) == N.ATMO_E_ARG and b"overlapping" in lib.atmo_last_error_string(ctx)
        # composite: two bands of ONE scene buffer are disjoint rows, the same band twice overlaps, side-by-side halves interleave (refused)
        v, _ = _views([(cam, (0, 0, 64, 18), 0x1000, a), (cam, (0, 18, 64, 36), 0x1000, a)])
        assert call(v, 2, 1) not in (N.ATMO_OK, N.ATMO_E_ARG)
        v, _ = _views([(cam, (0, 0, 64, 18), 0x1000, a), (cam, (0, 17, 64, 36), 0x1000, a)])
        assert call(v, 2, 1) == N.ATMO_E_ARG and b"overlapping" in lib.atmo_last_error_string(ctx)
        v, _ = _views([(cam, (0, 0, 32, 36), 0x1000, a), (cam, (32, 0, 64, 36), 0x1000, a)])
        assert call(v, 2, 1) == N.ATMO_E_ARG and b"overlapping" in lib.atmo_last_error_string(ctx)
        # an empty view is skipped: its pointers are not looked at, and it cannot overlap; a batch of empty views is ATMO_OK
        v, _ = _views([(cam, (5, 5, 5, 30), None, None), (cam, (0, 7, 64, 7), None, 3)])
        assert call(v, 2) == N.ATMO_OK
        # a well-formed batch on a context without a device: refused, but not for its arguments
        assert call(good, 2) not in (N.ATMO_OK, N.ATMO_E_ARG)
        v, _ = _views([(cam, (5, 5, 5, 30), None, None), (cam, None, 0x1000, a)])
        assert call(v, 2) not in (N.ATMO_OK, N.ATMO_E_ARG)
    finally:
        lib.atmo_destroy(ctx)


@pytest.mark.parametrize("mode", ["precision0", "precision2", "view_steps64", "lane_split2"])
def test_render_views_needs_the_default_forms(mode):
    """The multi-view kernels exist for what a default context draws with: precision 0 / 2, 64 view steps, a forced lane split -> ATMO_E_STATE, also from
    the layout query."""
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
        cam = S.Camera(64, 36, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
        v, n = _views([(cam, None, 0x1000, 0x10000), (cam, None, 0x1000, 0x90000)])
        assert lib.atmo_render_views(ctx, v, n, 0, None) == N.ATMO_E_STATE
        assert b"no multi-view kernel" in lib.atmo_last_error_string(ctx)
        first, grid = (C.c_int * 3)(), (C.c_int * 4)()
        assert lib.atmo_debug_views_layout(ctx, v, n, first, grid) == N.ATMO_E_STATE
        assert lib.atmo_render_views(ctx, v, 0, 0, None) == N.ATMO_OK      # no views: nothing to refuse
    finally:
        lib.atmo_destroy(ctx)


def _layout(ctx, specs):
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    v, n = _views(specs)
    first, grid = (C.c_int * (n + 1))(), (C.c_int * (2 * max(n, 1)))()
    rc = lib.atmo_debug_views_layout(ctx, v, n, first, grid)
    assert rc == N.ATMO_OK, lib.atmo_last_error_string(ctx)
    return list(first), [(grid[2 * i], grid[2 * i + 1]) for i in range(n)]


def _tiles_needed(rect, even_origin):
    """The tiles (in the view's own grid) that hold a pixel of the rect, given the grid's origin."""
    x0, y0, x1, y1 = rect
    gx0, gy0 = (x0 & ~1, y0 & ~1) if even_origin else (x0, y0)
    return {((x - gx0) // TILE_W, (y - gy0) // TILE_H) for y in range(y0, y1) for x in range(x0, x1)}, (gx0, gy0)


@pytest.mark.parametrize("even_origin", [False, True], ids=["rect_origin", "declared_sampler_origin"])
def test_views_layout_partitions_the_launch(even_origin):
    """Every tile of every non-empty view appears exactly once in the concatenated launch, an empty view contributes nothing; under the declared sampler
    each view's grid starts on an even pixel.  (A host-only context has no mip chain bound, so its own draws take the level-0 kernels, whose grid
    starts at the rect: the declared-sampler origin is checked as arithmetic on rects whose origin is even already, where both agree, and on odd
    origins against the rule itself.)"""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH_RM)
    try:
        big, small = S.Camera(251, 141, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0)), S.Camera(96, 64, (30.0, 0.0, 500.0), (0.0, 0.0, 0.0))
        rects = [None, (17, 9, 250, 141), (40, 20, 40, 60), (0, 0, 96, 64), (33, 7, 95, 63), (2, 2, 18, 10), (0, 5, 96, 5), (250, 140, 251, 141)]
        if even_origin:   # rects with an even origin: the level-0 grid (what the host-only context reports) IS the declared sampler's
            rects = [None if r is None else (r[0] & ~1, r[1] & ~1, r[2], r[3]) for r in rects]
        cams = [big, big, big, small, small, small, small, big]
        first, grids = _layout(ctx, [(c, r, 0x1000, 0x10000) for c, r in zip(cams, rects)])
        assert first[0] == 0 and len(first) == 9
        seen = set()
        for i, (cam, rect) in enumerate(zip(cams, rects)):
            rect = rect or (0, 0, cam.width, cam.height)
            gx, gy = grids[i]
            n_blocks = first[i + 1] - first[i]
            assert n_blocks == gx * gy >= 0
            if rect[0] == rect[2] or rect[1] == rect[3]:
                assert (gx, gy) == (0, 0) and n_blocks == 0, i     # an empty view contributes nothing
                continue
            needed, (gx0, gy0) = _tiles_needed(rect, even_origin)
            assert gx0 % 2 == 0 and gy0 % 2 == 0 or not even_origin
            # block b of the launch -> (view, local tile): every needed tile of this view is hit exactly once, and nothing else
            tiles = [((b - first[i]) % gx, (b - first[i]) // gx) for b in range(first[i], first[i + 1])]
            assert len(set(tiles)) == len(tiles) == n_blocks and set(tiles) == needed, i
            for b in range(first[i], first[i + 1]):
                assert b not in seen
                seen.add(b)
        assert seen == set(range(first[-1]))
        # n_views == 0: an empty launch; too many views: refused
        v, _ = _views([(big, None, 0x1000, 0x10000)] * 9)
        f0, g0 = (C.c_int * 10)(), (C.c_int * 18)()
        assert lib.atmo_debug_views_layout(ctx, v, 0, f0, g0) == N.ATMO_OK and f0[0] == 0
        assert lib.atmo_debug_views_layout(ctx, v, 9, f0, g0) == N.ATMO_E_ARG
        assert lib.atmo_debug_views_layout(ctx, v, 1, None, g0) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)
