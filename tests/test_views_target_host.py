"""CPU tests of the multi-view draw into packed and pitched colour targets (include/atmo_views_target.h): the header's symbol set and the binding, every
refusal of atmo_render_views_target on a host-only context (nothing touches a device) and the overlap rule against a brute-force byte-set comparison.
(tests/test_kernel_twins_host.py holds the static properties of the kernels: the headline twin's loop position; registers, stack and loads against the twins.)
(tests/test_views_target_gpu.py holds the kernels to atmo_render_target's bytes bit for bit.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.scene import col_major

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, U8 = 0, 1, 2          # AtmoTargetFormat
PX = {F32: 16, F16: 8, U8: 4}
DEPTH = 0x1000


def _frame(cam, rect=None):
    from godot_atmosphere_shader_amd import _native as N

    f = N.AtmoFrame()
    f.inv_projection_matrix[:] = [float(x) for x in col_major(cam.inv_projection)]
    f.inv_view_matrix[:] = [float(x) for x in col_major(cam.inv_view)]
    f.viewport_w, f.viewport_h = cam.width, cam.height
    f.x0, f.y0, f.x1, f.y1 = rect if rect is not None else (0, 0, cam.width, cam.height)
    return f


def _views(specs):
    """specs: [(camera, rect or None, depth address, pixels address, format, pitch in bytes)] -> (N.AtmoViewTarget array, n)."""
    from godot_atmosphere_shader_amd import _native as N

    arr = (N.AtmoViewTarget * max(len(specs), 1))()
    for i, (cam, rect, depth, pixels, fmt, pitch) in enumerate(specs):
        arr[i].frame = _frame(cam, rect)
        arr[i].depth_dev = depth
        arr[i].target = N.AtmoTarget(pixels, fmt, pitch)
    return arr, len(specs)


def _host_ctx(variant, view_steps=0, light_mode=None, light_steps=0):
    from godot_atmosphere_shader_amd import _native as N

    ctx = C.c_void_p()
    lm = N.LIGHT_LUT if light_mode is None else light_mode
    assert N.load().atmo_debug_create_host_only(variant, view_steps, 0, lm, light_steps, C.byref(ctx)) == N.ATMO_OK
    return ctx


def _functions(header_name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header_name)).read(), flags=re.S)
    return set(re.findall(r"\b(atmo_[a-z0-9_]+)\s*\(", text))


def test_binding_exposes_the_views_target_header():
    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.build import build_native

    build_native()
    lib = N.load()
    assert _functions("atmo_views_target.h") == set(N.VIEWS_TARGET_SYMBOLS) == {"atmo_render_views_target"}
    assert not set(N.VIEWS_TARGET_SYMBOLS) & set(N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS)
    assert N.EXPORTED_SYMBOLS[-len(N.VIEWS_TARGET_SYMBOLS):] == N.VIEWS_TARGET_SYMBOLS
    for sym in N.VIEWS_TARGET_SYMBOLS:
        assert getattr(lib, sym) is not None and sym in N.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "atmo_views_target.h")).read()
    assert '#include "atmo_views.h"' in header and '#include "atmo_target.h"' in header
    # the three older headers keep their function sets, and the feature is detected by its symbol, not by the version
    assert _functions("atmo_views.h") == set(N.VIEWS_SYMBOLS) == {"atmo_render_views"}
    assert _functions("atmo_target.h") == set(N.TARGET_SYMBOLS)
    assert _functions("atmo.h") == set(N.CORE_SYMBOLS) and len(N.CORE_SYMBOLS) == 22
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5
    assert "#define ATMO_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "atmo.h")).read()


def test_atmoviewtarget_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of AtmoViewTarget as a C compiler sees the header against the ctypes structure."""
    from godot_atmosphere_shader_amd import _native as N

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "atmo_views_target.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(AtmoViewTarget), offsetof(AtmoViewTarget, frame), '
                   'offsetof(AtmoViewTarget, depth_dev), offsetof(AtmoViewTarget, target), offsetof(AtmoViewTarget, target.pixels), '
                   'offsetof(AtmoViewTarget, target.format), offsetof(AtmoViewTarget, target.row_pitch_bytes)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    t = N.AtmoViewTarget.target.offset
    assert got == [C.sizeof(N.AtmoViewTarget), N.AtmoViewTarget.frame.offset, N.AtmoViewTarget.depth_dev.offset, t, t + N.AtmoTarget.pixels.offset,
                   t + N.AtmoTarget.format.offset, t + N.AtmoTarget.row_pitch_bytes.offset]


def test_render_views_target_checks_its_arguments_without_a_device():
    """Every refusal the header states, on a host-only context: the code comes back before anything touches a device, and a well-formed batch never
    succeeds there."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    err = lambda: lib.atmo_last_error_string(ctx)                                           # noqa: E731
    call = lambda v, k, comp=0: lib.atmo_render_views_target(ctx, v, k, comp, None)          # noqa: E731
    try:
        cam = S.Camera(64, 36, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
        a, b = 0x100000, 0x200000                  # two disjoint outputs, 1 MiB apart
        for fmt in (F16, U8, F32):
            good, n = _views([(cam, None, DEPTH, a, fmt, 0), (cam, None, DEPTH, b, fmt, 0)])
            # view count, null views, null context
            assert call(good, 0) == N.ATMO_OK and call(None, 0) == N.ATMO_OK
            assert call(good, -1) == N.ATMO_E_ARG and call(good, N.MAX_VIEWS + 1) == N.ATMO_E_ARG
            assert call(None, 2) == N.ATMO_E_ARG and b"null views" in err()
            assert lib.atmo_render_views_target(None, good, 2, 0, None) == N.ATMO_E_ARG
            # a well-formed batch on a context without a device: refused, but not for its arguments -- plain, composite, pitched
            assert call(good, 2) not in (N.ATMO_OK, N.ATMO_E_ARG)
            assert call(good, 2, 1) not in (N.ATMO_OK, N.ATMO_E_ARG)
            v, _ = _views([(cam, None, DEPTH, a, fmt, (64 + 7) * PX[fmt]), (cam, (3, 3, 40, 30), DEPTH, b, fmt, 64 * PX[fmt])])
            assert call(v, 2) not in (N.ATMO_OK, N.ATMO_E_ARG)
            # per-view checks: rect, viewport, null pointers -- in any view, and the message names it
            for bad_rect in ((0, 0, 65, 36), (-1, 0, 64, 36), (10, 0, 5, 36), (0, 30, 64, 20)):
                v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, bad_rect, DEPTH, b, fmt, 0)])
                assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err(), bad_rect
            v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, None, DEPTH, b, fmt, 0)])
            v[0].frame.viewport_w = 0
            assert call(v, 2) == N.ATMO_E_ARG and b"view 0" in err()
            v, _ = _views([(cam, None, None, a, fmt, 0), (cam, None, DEPTH, b, fmt, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 0" in err() and b"null device pointer" in err()
            v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, None, DEPTH, None, fmt, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"null target pixels" in err()
            # alignment to the pixel size: 8 for RGBA16F, 4 for RGBA8, 16 for RGBA32F -- half a pixel off is refused, a whole pixel is not
            v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, None, DEPTH, b + PX[fmt] // 2, fmt, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and f"({PX[fmt]} bytes)".encode() in err()
            v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, None, DEPTH, b + PX[fmt], fmt, 0)])
            assert call(v, 2) not in (N.ATMO_OK, N.ATMO_E_ARG)
            # a bad pitch: shorter than the row (plain: the rect's; composite: the viewport's), not a multiple of the pixel size
            for comp, rect, pitch in ((0, None, 63 * PX[fmt]), (0, None, 64 * PX[fmt] + PX[fmt] // 2), (1, (0, 0, 32, 36), 32 * PX[fmt]), (0, None, -PX[fmt])):
                v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, rect, DEPTH, b, fmt, pitch)])
                assert call(v, 2, comp) == N.ATMO_E_ARG and b"view 1" in err() and b"row_pitch_bytes" in err(), (comp, rect, pitch)
            v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, (0, 0, 32, 36), DEPTH, b, fmt, 32 * PX[fmt])])
            assert call(v, 2, 0) not in (N.ATMO_OK, N.ATMO_E_ARG)         # ... which is a fine pitch for the plain draw of that rect
            # an unknown format; mixed formats
            v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, None, DEPTH, b, 3, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"unknown target format" in err()
            other = {F16: U8, U8: F32, F32: F16}[fmt]
            v, _ = _views([(cam, None, DEPTH, a, fmt, 0), (cam, None, DEPTH, b, other, 0)])
            assert call(v, 2) == N.ATMO_E_ARG and b"view 1" in err() and b"one format per batch" in err()
            # an empty view is skipped: its pointers and its target are not looked at, it cannot overlap, its format does not count
            v, _ = _views([(cam, (5, 5, 5, 30), None, None, 7, 3), (cam, (0, 7, 64, 7), None, 3, other, -1)])
            assert call(v, 2) == N.ATMO_OK
            v, _ = _views([(cam, (5, 5, 5, 30), None, None, other, 3), (cam, None, DEPTH, a, fmt, 0), (cam, (0, 7, 64, 7), None, a, 9, 1)])
            assert call(v, 3) not in (N.ATMO_OK, N.ATMO_E_ARG)
    finally:
        lib.atmo_destroy(ctx)


def test_overlap_fixed_cases():
    """The overlap rule on the layouts a host builds: the same buffer, touching ranges, row bands, side-by-side halves of one pitched image."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    call = lambda v, k, comp=0: lib.atmo_render_views_target(ctx, v, k, comp, None)          # noqa: E731
    accepted = lambda rc: rc not in (N.ATMO_OK, N.ATMO_E_ARG)                               # noqa: E731  (host-only: refused later, for the missing device)

    def refused(rc):
        return rc == N.ATMO_E_ARG and b"overlapping" in lib.atmo_last_error_string(ctx)

    try:
        half, full = S.Camera(96, 64, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0)), S.Camera(192, 64, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
        img = 0x400000
        for fmt in (F16, U8, F32):
            px = PX[fmt]
            size = 96 * 64 * px
            # the same buffer; a buffer starting one pixel inside another; one range touching the next
            v, _ = _views([(half, None, DEPTH, img, fmt, 0), (half, None, DEPTH, img, fmt, 0)])
            assert refused(call(v, 2))
            v, _ = _views([(half, None, DEPTH, img, fmt, 0), (half, None, DEPTH, img + size - px, fmt, 0)])
            assert refused(call(v, 2))
            v, _ = _views([(half, None, DEPTH, img, fmt, 0), (half, None, DEPTH, img + size, fmt, 0)])
            assert accepted(call(v, 2))
            v, _ = _views([(half, None, DEPTH, img + size, fmt, 0), (half, None, DEPTH, img, fmt, 0)])     # ... in either order
            assert accepted(call(v, 2))
            # two row bands of one image: composite (rects of one viewport) and plain (pixels at the band's first row)
            v, _ = _views([(half, (0, 0, 96, 32), DEPTH, img, fmt, 0), (half, (0, 32, 96, 64), DEPTH, img, fmt, 0)])
            assert accepted(call(v, 2, 1))
            v, _ = _views([(half, (0, 0, 96, 32), DEPTH, img, fmt, 0), (half, (0, 31, 96, 64), DEPTH, img, fmt, 0)])
            assert refused(call(v, 2, 1))
            v, _ = _views([(half, (0, 0, 96, 32), DEPTH, img, fmt, 0), (half, (0, 32, 96, 64), DEPTH, img + 32 * 96 * px, fmt, 0)])
            assert accepted(call(v, 2))
            # side-by-side halves of ONE pitched 192 x 64 image: two 96 x 64 views, pixels = image and image + 96 pixels, pitch = the full row
            pitch = 192 * px
            v, _ = _views([(half, None, DEPTH, img, fmt, pitch), (half, None, DEPTH, img + 96 * px, fmt, pitch)])
            assert accepted(call(v, 2)) and accepted(call(v, 2, 1))
            v, _ = _views([(half, None, DEPTH, img + 96 * px, fmt, pitch), (half, None, DEPTH, img, fmt, pitch)])
            assert accepted(call(v, 2)) and accepted(call(v, 2, 1))
            # ... as two rects of ONE viewport, composite: what atmo_render_views refuses
            v, _ = _views([(full, (0, 0, 96, 64), DEPTH, img, fmt, 0), (full, (96, 0, 192, 64), DEPTH, img, fmt, 0)])
            assert accepted(call(v, 2, 1))
            if fmt == F32:
                fv = (N.AtmoView * 2)()
                for i, rect in enumerate(((0, 0, 96, 64), (96, 0, 192, 64))):
                    fv[i].frame, fv[i].depth_dev, fv[i].rgba_dev = _frame(full, rect), DEPTH, img
                assert lib.atmo_render_views(ctx, fv, 2, 1, None) == N.ATMO_E_ARG and b"overlapping" in lib.atmo_last_error_string(ctx)
            # halves that overlap by one pixel
            v, _ = _views([(half, None, DEPTH, img, fmt, pitch), (half, None, DEPTH, img + 95 * px, fmt, pitch)])
            assert refused(call(v, 2)) and refused(call(v, 2, 1))
            v, _ = _views([(full, (0, 0, 97, 64), DEPTH, img, fmt, 0), (full, (96, 0, 192, 64), DEPTH, img, fmt, 0)])
            assert refused(call(v, 2, 1))
            # a wrapping row: the right half pushed one pixel further, so that its rows end in the next row of the left half
            v, _ = _views([(half, None, DEPTH, img, fmt, pitch), (half, None, DEPTH, img + 97 * px, fmt, pitch)])
            assert refused(call(v, 2)) and refused(call(v, 2, 1))
            # the halves with a pitch each of its own size: interleaved rows of different pitches are refused (the rule is conservative there)
            v, _ = _views([(half, None, DEPTH, img, fmt, pitch), (half, None, DEPTH, img + 96 * px, fmt, 2 * pitch)])
            assert refused(call(v, 2))
            # three views: the overlapping pair is found wherever it sits
            v, _ = _views([(half, None, DEPTH, img, fmt, pitch), (half, None, DEPTH, img + 96 * px, fmt, pitch), (half, (0, 0, 8, 8), DEPTH, img + 5 * pitch, fmt, 0)])
            assert refused(call(v, 3)) and b"views 0 and 2" in lib.atmo_last_error_string(ctx)
    finally:
        lib.atmo_destroy(ctx)


def _byte_set(base, rows, row_bytes, pitch):
    return {base + r * pitch + k for r in range(rows) for k in range(row_bytes)}


def _rule(a, b):
    """The header's rule on (base, rows, row_bytes, pitch) of two views."""
    if a[0] > b[0]:
        a, b = b, a
    (base_a, rows_a, rb_a, p_a), (base_b, rows_b, rb_b, p_b) = a, b
    if base_a + (rows_a - 1) * p_a + rb_a <= base_b:
        return True                                                   # (a)
    if p_a == p_b:
        q, r = divmod(base_b - base_a, p_a)
        return q >= rows_a or (r >= rb_a and r + rb_b <= p_a)         # (b)
    return False


def test_overlap_random_pairs_against_brute_force():
    """2 400 seeded pairs of small pitched rectangles, plain and composite, in all three formats: the library's verdict equals the header's rule, and the
    rule never accepts two views that share a byte (the brute-force comparison of the byte sets)."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    rng = np.random.default_rng(20240607)
    counts = dict(accepted=0, refused=0, accepted_b_only=0, refused_disjoint=0, same_pitch=0)
    try:
        for trial in range(2400):
            fmt = (F16, U8, F32)[trial % 3]
            px = PX[fmt]
            composite = int(rng.integers(0, 2))
            same_pitch = bool(rng.integers(0, 2))
            shapes = []
            for k in range(2):
                vw, vh = int(rng.integers(1, 9)), int(rng.integers(1, 7))
                x0 = int(rng.integers(0, vw))
                x1 = int(rng.integers(x0 + 1, vw + 1))
                y0 = int(rng.integers(0, vh))
                y1 = int(rng.integers(y0 + 1, vh + 1))
                shapes.append((vw, vh, x0, y0, x1, y1, vw if composite else x1 - x0))      # the last: the pixels a pitch must hold
            common = (max(sh[6] for sh in shapes) + int(rng.integers(0, 10))) * px
            specs, geo = [], []
            for vw, vh, x0, y0, x1, y1, row_px in shapes:
                pitch = common if same_pitch else (row_px + int(rng.integers(0, 6))) * px
                pixels = 0x800000 + int(rng.integers(0, 40)) * px
                cam = S.Camera(vw, vh, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))
                tight = pitch == row_px * px and bool(rng.integers(0, 2))                  # 0 means the tight pitch
                specs.append((cam, (x0, y0, x1, y1), DEPTH, pixels, fmt, 0 if tight else pitch))
                geo.append((pixels + (y0 * pitch + x0 * px if composite else 0), y1 - y0, (x1 - x0) * px, pitch))
            v, _ = _views(specs)
            rc = lib.atmo_render_views_target(ctx, v, 2, composite, None)
            got_accept = rc != N.ATMO_E_ARG
            assert rc != N.ATMO_OK
            if not got_accept:
                assert b"overlapping" in lib.atmo_last_error_string(ctx), (trial, lib.atmo_last_error_string(ctx))
            disjoint = not (_byte_set(*geo[0]) & _byte_set(*geo[1]))
            want_accept = _rule(geo[0], geo[1])
            assert got_accept == want_accept, (trial, geo, composite)                 # every pair satisfying (a) or (b) is accepted, nothing else
            assert disjoint or not got_accept, (trial, geo, composite)                # no overlapping pair is ever accepted
            if geo[0][3] == geo[1][3] and all(g[2] <= g[3] for g in geo):
                counts["same_pitch"] += 1
                lo, hi = sorted(geo)
                wraps = any((g[0] - lo[0]) % g[3] + g[2] > g[3] for g in geo)
                if not wraps:
                    assert got_accept == disjoint, (trial, geo, composite)            # exact for equal pitches whose rows do not wrap
            counts["accepted" if got_accept else "refused"] += 1
            lo, hi = sorted(geo)
            if got_accept and not lo[0] + (lo[1] - 1) * lo[3] + lo[2] <= hi[0]:
                counts["accepted_b_only"] += 1
            if disjoint and not got_accept:
                counts["refused_disjoint"] += 1
        print(counts)
        # the sample exercises every branch: both verdicts, acceptances that only (b) grants, and the conservative refusals
        assert counts["accepted"] >= 300 and counts["refused"] >= 300 and counts["accepted_b_only"] >= 30 and counts["same_pitch"] >= 300
    finally:
        lib.atmo_destroy(ctx)


@pytest.mark.parametrize("fmt", [F16, U8, F32], ids=["rgba16f", "rgba8", "rgba32f"])
@pytest.mark.parametrize("mode", ["precision0", "precision2", "view_steps64", "lane_split2"])
def test_render_views_target_needs_the_default_forms(mode, fmt):
    """The intersection of the batch's modes and the packed target's: precision 0 / 2, 64 view steps, a forced lane split -> ATMO_E_STATE."""
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
        v, n = _views([(cam, None, DEPTH, 0x100000, fmt, 0), (cam, None, DEPTH, 0x200000, fmt, 80 * PX[fmt])])
        for composite in (0, 1):
            assert lib.atmo_render_views_target(ctx, v, n, composite, None) == N.ATMO_E_STATE
            assert b"no multi-view kernel" in lib.atmo_last_error_string(ctx)
        assert lib.atmo_render_views_target(ctx, v, 0, 0, None) == N.ATMO_OK      # no views: nothing to refuse
        # arguments are checked in front of the mode
        v[1].target.format = 5
        assert lib.atmo_render_views_target(ctx, v, n, 0, None) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)
