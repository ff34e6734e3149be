"""CPU tests of the ray entry points (include/atmo_rays.h): the header's symbol set and the binding, the AtmoRay layout on both sides, every refusal of
atmo_shade_rays on host-only contexts in the header's order (nothing touches a device), and the tensor checks of PlanetAtmosphere.shade_rays /
camera_rays with the recorder and the fake tensors of tests/test_binding_calls_host.py.
(tests/test_rays_gpu.py holds the kernels to atmo_render and to the oracle.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import test_binding_calls_host as B
from test_views_proxy_host import FAR, ROOT, _frame, _functions, _host_ctx

RAYS, RGBA, DEPTH = 0x10000, 0x20000, 0x30000   # addresses no refusal dereferences
ABI = {
    "atmo_shade_rays": ("ctx", "frame", "rays", "rgba", "n", "width", "first", "stream"),
    "atmo_debug_frame_rays": ("ctx", "frame", "depth", "rays", "stream"),
}


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, N.load()


def _said(lib, ctx, rc):
    return rc, (lib.atmo_last_error_string(ctx) or b"").decode()


def _shade(lib, ctx, frame=True, rays=RAYS, rgba=RGBA, n=64, width=8, first=0):
    f = _frame(FAR)
    return _said(lib, ctx, lib.atmo_shade_rays(ctx, C.byref(f) if frame else None, rays, rgba, n, width, first, None))


def test_binding_exposes_the_rays_header():
    N, lib = _lib()
    assert _functions("atmo_rays.h") == set(N.RAYS_SYMBOLS) == {"atmo_shade_rays", "atmo_debug_frame_rays"}
    for sym in N.RAYS_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS
    # a tuple of its own beside EXPORTED_SYMBOLS, which stays the union of the seven older headers' tuples; the feature is detected by symbol
    assert N.EXPORTED_SYMBOLS == (N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_PROXY_SYMBOLS +
                                  N.VIEWS_TARGET_SYMBOLS)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5


def test_every_header_s_signatures_are_its_tuple_and_every_symbol_is_bound():
    """N.HEADERS is the one table of signatures: a block a header, each block's names its `*_SYMBOLS` tuple in the tuple's order, the nineteen tuples
    pairwise disjoint, and after load() no name of any tuple is left with ctypes' default signature (argtypes None: an int for every pointer)."""
    N, lib = _lib()
    tuples = {k: v for k, v in vars(N).items() if k.endswith("_SYMBOLS") and k != "EXPORTED_SYMBOLS"}
    assert len(tuples) == len(N.HEADERS) == 19 and all(_functions(h) >= set(block[0]) for h, block in N.HEADERS.items())      # under its own header's name
    assert sorted(map(id, tuples.values())) == sorted(id(symbols) for symbols, _, _, _ in N.HEADERS.values())      # every tuple heads one block
    for header, (symbols, required, suffix, signatures) in N.HEADERS.items():
        assert tuple(signatures) == symbols and len(set(symbols)) == len(symbols), header
        assert required or header in N.optional_headers() and N.optional_headers()[header] == (symbols, suffix, signatures), header
        for name in symbols:
            assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(signatures[name][1]), name
    names = [name for symbols in tuples.values() for name in symbols]
    assert len(names) == len(set(names)) == 88      # pairwise disjoint
    assert [h for h, block in N.HEADERS.items() if not block[1]] == list(N.optional_headers()) == [
        "atmo_cloud_detail.h", "atmo_rays.h", "atmo_ray_quads.h", "atmo_ray_order.h", "atmo_ray_list.h", "atmo_ray_detail.h", "atmo_detail_target.h",
        "atmo_lens.h"]


def test_an_atmo_ray_is_32_bytes_on_both_sides(tmp_path):
    N, _ = _lib()
    assert C.sizeof(N.AtmoRay) == 32
    assert [(name, getattr(N.AtmoRay, name).offset) for name, _ in N.AtmoRay._fields_] == [("origin", 0), ("tmax", 12), ("dir", 16), ("reserved", 28)]
    # the C side: the header as a C99 compiler lays it out (atmo_api.hip holds sizeof(AtmoRay) == 32 with a static_assert of its own at every build)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or shutil.which("hipcc")
    assert cc is not None, "no C compiler, and the library was built here?"
    if os.path.basename(cc) == "hipcc":
        cc = os.path.join(os.path.dirname(os.path.realpath(cc)), "..", "lib", "llvm", "bin", "clang")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "atmo_rays.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(AtmoRay), offsetof(AtmoRay, origin), offsetof(AtmoRay, tmax), offsetof(AtmoRay, dir),'
                   ' offsetof(AtmoRay, reserved)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["32", "0", "12", "16", "28"]


def test_no_rays_is_ok_whatever_else_is_passed():
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    try:
        assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK   # a mode that refuses every other call
        assert lib.atmo_shade_rays(ctx, None, None, None, 0, 0, 0, None) == N.ATMO_OK
        assert _shade(lib, ctx, n=0, width=0, rays=RAYS + 4)[0] == N.ATMO_OK
    finally:
        lib.atmo_destroy(ctx)
    assert lib.atmo_shade_rays(None, None, None, None, 0, 0, 0, None) == N.ATMO_E_ARG


def test_argument_refusals_come_first_and_name_the_entry_point():
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    try:
        assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK   # the first mode refusal stands behind every argument check
        for kw in (dict(frame=False), dict(rays=None), dict(rgba=None), dict(rays=RAYS + 4), dict(rays=RAYS + 8), dict(rgba=RGBA + 4), dict(width=0),
                   dict(first=2 ** 32 - 63), dict(first=2 ** 32 - 1, n=2), dict(first=2, n=2 ** 32 - 1)):
            rc, msg = _shade(lib, ctx, **kw)
            assert rc == N.ATMO_E_ARG and msg.startswith("atmo_shade_rays: "), (kw, rc, msg)
        # the largest batch that is accepted gets as far as the mode
        for kw in (dict(first=2 ** 32 - 64), dict(first=0, n=2 ** 32 - 1), dict(first=2 ** 32 - 1, n=1)):
            rc, msg = _shade(lib, ctx, **kw)
            assert rc == N.ATMO_E_STATE and "atmo_set_precision 0" in msg, (kw, rc, msg)
        # null pointers in front of alignment, alignment in front of width, width in front of the range
        assert "null" in _shade(lib, ctx, rays=None, rgba=RGBA + 4, width=0)[1]
        assert "aligned" in _shade(lib, ctx, rays=RAYS + 4, width=0, first=2 ** 32 - 1)[1]
        assert "width" in _shade(lib, ctx, width=0, first=2 ** 32 - 1)[1]
        assert "2^32" in _shade(lib, ctx, first=2 ** 32 - 1)[1]
    finally:
        lib.atmo_destroy(ctx)


def _mode_ctx(N, lib, variant, view_steps=0, light_mode=None, light_steps=0, precision=None, lane_split=None, detail=False, sampler=None):
    ctx = _host_ctx(variant, view_steps, light_mode, light_steps)
    if precision is not None:
        assert lib.atmo_set_precision(ctx, precision) == N.ATMO_OK
    if lane_split is not None:
        assert lib.atmo_set_lane_split(ctx, lane_split) == N.ATMO_OK
    if detail:
        assert lib.atmo_set_cloud_detail(ctx, 1) == N.ATMO_OK
    if sampler is not None:
        assert lib.atmo_set_sampler_lod(ctx, sampler) == N.ATMO_OK
    return ctx


def _mode_cases(N):
    D = N.LIGHT_DIRECT
    # (what the message must name, the variant, the context's settings): each context has ONE thing wrong
    return [
        ("atmo_set_precision 0", N.VARIANT_CLOUDS_HIGH, dict(precision=0)),
        ("atmo_set_precision 0", N.VARIANT_V1_NO_CLOUDS, dict(precision=0)),
        ("atmo_set_precision 2", N.VARIANT_NO_CLOUDS, dict(precision=2)),
        ("atmo_set_precision 2", N.VARIANT_CLOUDS_HIGH_RM, dict(precision=2)),
        ("32 view steps", N.VARIANT_NO_CLOUDS, dict(view_steps=64)),
        ("32 view steps", N.VARIANT_CLOUDS, dict(view_steps=33)),
        ("atmo_set_lane_split 2", N.VARIANT_NO_CLOUDS, dict(lane_split=2)),
        ("atmo_set_lane_split 2", N.VARIANT_CLOUDS_HIGH, dict(lane_split=2)),
        ("direct light", N.VARIANT_CLOUDS_HIGH, dict(light_mode=D, light_steps=8)),
        ("direct light", N.VARIANT_CLOUDS_HIGH_RM, dict(light_mode=D, light_steps=5)),
        ("cloud detail (atmo_set_cloud_detail 1)", N.VARIANT_CLOUDS_HIGH, dict(detail=True)),
        ("cloud detail (atmo_set_cloud_detail 1)", N.VARIANT_V1_CLOUDS, dict(detail=True)),
    ]


def test_every_mode_refusal_names_its_mode():
    N, lib = _lib()
    for needle, variant, kw in _mode_cases(N):
        ctx = _mode_ctx(N, lib, variant, **kw)
        try:
            rc, msg = _shade(lib, ctx)
            assert rc == N.ATMO_E_STATE and msg.startswith("atmo_shade_rays: ") and needle in msg, (needle, kw, rc, msg)
        finally:
            lib.atmo_destroy(ctx)


def test_mode_refusals_come_in_the_header_s_order():
    """A context with everything wrong is refused for the first item of the list; taking the items away one by one walks the list."""
    N, lib = _lib()
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH, view_steps=64, light_mode=N.LIGHT_DIRECT, light_steps=8, precision=0, lane_split=2, detail=True)
    try:
        assert "atmo_set_precision 0" in _shade(lib, ctx)[1]
        assert lib.atmo_set_precision(ctx, 2) == N.ATMO_OK
        assert "atmo_set_precision 2" in _shade(lib, ctx)[1]
        assert lib.atmo_set_precision(ctx, 1) == N.ATMO_OK
        assert "32 view steps" in _shade(lib, ctx)[1]
    finally:
        lib.atmo_destroy(ctx)
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH, light_mode=N.LIGHT_DIRECT, light_steps=8, lane_split=2, detail=True)
    try:
        assert "atmo_set_lane_split 2" in _shade(lib, ctx)[1]
        assert lib.atmo_set_lane_split(ctx, 1) == N.ATMO_OK
        assert "direct light" in _shade(lib, ctx)[1]
    finally:
        lib.atmo_destroy(ctx)
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH, detail=True, sampler=1)
    try:
        assert "cloud detail" in _shade(lib, ctx)[1]
        assert lib.atmo_set_cloud_detail(ctx, 0) == N.ATMO_OK
        # (sampler mode 1 refuses only with a mip chain bound, which needs a device: tests/test_rays_gpu.py) -- next, the textures' check
        rc, msg = _shade(lib, ctx)
        assert rc == N.ATMO_E_STATE and "u_optical_depth_texture not set" in msg, (rc, msg)
    finally:
        lib.atmo_destroy(ctx)


def test_no_device_comes_behind_every_check():
    N, lib = _lib()
    # the direct-light variant without clouds needs no texture: a well-formed call gets as far as the device
    ctx = _mode_ctx(N, lib, N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)
    try:
        rc, msg = _shade(lib, ctx)
        assert rc == N.ATMO_E_NO_DEVICE and msg.startswith("atmo_shade_rays: "), (rc, msg)
        assert _shade(lib, ctx, width=0)[0] == N.ATMO_E_ARG
        assert lib.atmo_set_lane_split(ctx, 2) == N.ATMO_OK
        assert _shade(lib, ctx)[0] == N.ATMO_E_STATE
        assert lib.atmo_set_lane_split(ctx, 0) == N.ATMO_OK
        f = _frame(FAR)
        rc, msg = _said(lib, ctx, lib.atmo_debug_frame_rays(ctx, C.byref(f), DEPTH, RAYS, None))
        assert rc == N.ATMO_E_NO_DEVICE and msg.startswith("atmo_debug_frame_rays: "), (rc, msg)
        for args in ((None, DEPTH, RAYS), (C.byref(f), None, RAYS), (C.byref(f), DEPTH, None), (C.byref(f), DEPTH, RAYS + 4)):
            rc, msg = _said(lib, ctx, lib.atmo_debug_frame_rays(ctx, *args, None))
            assert rc == N.ATMO_E_ARG and msg.startswith("atmo_debug_frame_rays: "), (args, rc, msg)
        empty = _frame(FAR, (5, 5, 5, 9))
        assert lib.atmo_debug_frame_rays(ctx, C.byref(empty), None, None, None) == N.ATMO_OK
    finally:
        lib.atmo_destroy(ctx)


# ---- the binding, without a device ---------------------------------------------------------------------------------------------------------------
def _calls(node):
    return [(name, dict(zip(ABI[name], args))) for name, args in node._lib.calls if name != "atmo_destroy"]


def test_shade_rays_reaches_its_entry_point():
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    node, cam = B._node(), B._cam()
    rays, out = B._fake((70, 8)), B._fake((70, 4))
    assert node.shade_rays(rays, cam, width=10, first=30, out=out, stream=B._Stream(), time=B.TIME) is out
    (name, a), = _calls(node)
    assert name == "atmo_shade_rays"
    assert a == dict(ctx=B.CTX, frame=bytes(PA._to_native_frame(node.make_frame(cam, B.TIME))), rays=rays.data_ptr(), rgba=out.data_ptr(), n=70, width=10,
                     first=30, stream=B.STREAM)
    # width defaults to n; the output is allocated; no camera: ray space is world space (an identity inv_view, the planet where the node is)
    node = B._node()
    with B._AllocateAsCuda():
        out = node.shade_rays(rays, stream=B.STREAM)
    assert tuple(out.shape) == (70, 4) and out.dtype == torch.float32
    (name, a), = _calls(node)
    assert (a["n"], a["width"], a["first"], a["rgba"]) == (70, 70, 0, out.data_ptr())
    f = B.N.AtmoFrame.from_buffer_copy(a["frame"])
    assert list(f.inv_view_matrix) == [float(x) for x in np.eye(4).reshape(-1)]
    assert list(f.planet_center_viewspace) == [float(np.float32(x)) for x in B.TRANSFORM[:3, 3]]


def test_camera_rays_reaches_its_entry_point():
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    node, cam = B._node(), B._cam()
    depth = B._depth(cam)
    with B._AllocateAsCuda():
        rays = node.camera_rays(cam, depth, rect=B.RECT, stream=B.STREAM)
    x0, y0, x1, y1 = B.RECT
    assert tuple(rays.shape) == ((y1 - y0) * (x1 - x0), 8) and rays.dtype == torch.float32 and rays.is_contiguous()
    (name, a), = _calls(node)
    assert name == "atmo_debug_frame_rays"
    assert a == dict(ctx=B.CTX, frame=bytes(PA._to_native_frame(node.make_frame(cam, 0.0, B.RECT))), depth=depth.data_ptr(), rays=rays.data_ptr(),
                     stream=B.STREAM)


def test_bad_tensors_raise_before_anything_reaches_the_library():
    node, cam = B._node(), B._cam()
    good, out = B._fake((12, 8)), B._fake((12, 4))
    cpu = torch.zeros((12, 8))
    for bad in (cpu, B._fake((12, 8), torch.float16), B._fake((12, 16))[:, ::2], np.zeros((12, 8), dtype=np.float32), None):
        with pytest.raises(TypeError, match="rays must be a contiguous CUDA float32 tensor"):
            node.shade_rays(bad, cam, stream=B.STREAM)
    for bad in (B._fake((12, 7)), B._fake((96,)), B._fake((12, 8, 1))):
        with pytest.raises(ValueError, match=r"rays must have shape \(n, 8\)"):
            node.shade_rays(bad, cam, stream=B.STREAM)
    for bad in (torch.zeros((12, 4)), B._fake((12, 4), torch.float64), B._fake((12, 8))[:, ::2]):
        with pytest.raises(TypeError, match="out must be a contiguous CUDA float32 tensor"):
            node.shade_rays(good, cam, out=bad, stream=B.STREAM)
    for bad in (B._fake((12, 3)), B._fake((11, 4)), B._fake((48,))):
        with pytest.raises(ValueError, match="out must have"):
            node.shade_rays(good, cam, out=bad, stream=B.STREAM)
    for kw in (dict(width=0), dict(width=-3), dict(first=-1), dict(first=2 ** 32 - 11)):
        with pytest.raises(ValueError, match="width must be at least 1"):
            node.shade_rays(good, cam, out=out, stream=B.STREAM, **kw)
    for kw in (dict(width=2.5), dict(first="0")):
        with pytest.raises(TypeError, match="width and first must be integers"):
            node.shade_rays(good, cam, out=out, stream=B.STREAM, **kw)
    with pytest.raises(TypeError, match="depth must be a contiguous CUDA float32 tensor"):
        node.camera_rays(cam, torch.zeros((cam.height, cam.width)), stream=B.STREAM)
    with pytest.raises(ValueError, match=r"depth must have shape \(viewport_h, viewport_w\)"):
        node.camera_rays(cam, B._fake((cam.height, cam.width + 1)), stream=B.STREAM)
    assert _calls(node) == []


def test_a_library_without_the_symbols_says_so():
    node, cam = B._node(lib=B.library_without("atmo_shade_rays", "atmo_debug_frame_rays")), B._cam()
    with pytest.raises(RuntimeError, match="atmo_shade_rays"):
        node.shade_rays(B._fake((4, 8)), cam, out=B._fake((4, 4)), stream=B.STREAM)
    with pytest.raises(RuntimeError, match="atmo_debug_frame_rays"), B._AllocateAsCuda():
        node.camera_rays(cam, B._depth(cam), stream=B.STREAM)
