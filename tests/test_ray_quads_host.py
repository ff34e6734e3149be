"""CPU tests of the ray-quad entry point (include/atmo_ray_quads.h): the header's symbol set and the binding, every refusal of atmo_shade_ray_quads on
host-only contexts in the header's order (nothing touches a device), the quad order helpers, the tensor checks of PlanetAtmosphere.shade_ray_quads with
the recorder and the fake tensors of tests/test_binding_calls_host.py, and the three new kernels in the compiled assembly (one compile, shared with
tests/test_kernel_twins_host.py).  (tests/test_ray_quads_gpu.py holds the kernels to atmo_render and to the oracle.)"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import test_binding_calls_host as B
import test_kernel_twins_host as T
from test_rays_host import RAYS, RGBA, _mode_cases, _mode_ctx, _said
from test_views_proxy_host import FAR, ROOT, _frame, _functions, _host_ctx

WHO = "atmo_shade_ray_quads: "
ABI = {"atmo_shade_ray_quads": ("ctx", "frame", "rays", "rgba", "n_quads", "width", "first_quad", "stream"),
       "atmo_debug_frame_rays": ("ctx", "frame", "depth", "rays", "stream")}
# the three new kernels and their pixel twins under the declared sampler: atmo_shade_rays_kernel<FLAGS | 16384, 0> beside atmo_render_kernel<FLAGS, 0, 1>
KERNELS = {49: "clouds_high", 51: "clouds_high_rm", 57: "v1_clouds"}


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, N.load()


def _shade(lib, ctx, frame=True, rays=RAYS, rgba=RGBA, n=16, width=8, first=0):
    f = _frame(FAR)
    return _said(lib, ctx, lib.atmo_shade_ray_quads(ctx, C.byref(f) if frame else None, rays, rgba, n, width, first, None))


def test_binding_exposes_the_ray_quads_header():
    N, lib = _lib()
    assert _functions("atmo_ray_quads.h") == set(N.RAY_QUADS_SYMBOLS) == {"atmo_shade_ray_quads"}
    assert lib.atmo_shade_ray_quads is not None and "atmo_shade_ray_quads" not in N.EXPORTED_SYMBOLS
    assert not set(N.RAY_QUADS_SYMBOLS) & set(N.RAYS_SYMBOLS)
    assert N.EXPORTED_SYMBOLS == (N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_PROXY_SYMBOLS +
                                  N.VIEWS_TARGET_SYMBOLS)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5


def test_no_quads_is_ok_whatever_else_is_passed():
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS)
    try:
        assert lib.atmo_set_precision(ctx, 2) == N.ATMO_OK   # a variant and a mode that refuse every other call
        assert lib.atmo_shade_ray_quads(ctx, None, None, None, 0, 0, 0, None) == N.ATMO_OK
        assert _shade(lib, ctx, n=0, width=0, rays=RAYS + 4, first=2 ** 31)[0] == N.ATMO_OK
    finally:
        lib.atmo_destroy(ctx)
    assert lib.atmo_shade_ray_quads(None, None, None, None, 0, 0, 0, None) == N.ATMO_E_ARG


def test_argument_refusals_come_first_and_name_the_entry_point():
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    try:
        assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK   # the first mode refusal stands behind every argument check
        for kw in (dict(frame=False), dict(rays=None), dict(rgba=None), dict(rays=RAYS + 4), dict(rays=RAYS + 8), dict(rgba=RGBA + 4), dict(width=0),
                   dict(first=2 ** 30 - 15), dict(first=2 ** 30, n=1), dict(first=1, n=2 ** 30), dict(first=2 ** 32 - 1, n=2 ** 32 - 1)):
            rc, msg = _shade(lib, ctx, **kw)
            assert rc == N.ATMO_E_ARG and msg.startswith(WHO), (kw, rc, msg)
        # the largest batch that is accepted gets as far as the mode
        for kw in (dict(first=2 ** 30 - 16), dict(first=0, n=2 ** 30), dict(first=2 ** 30 - 1, n=1)):
            rc, msg = _shade(lib, ctx, **kw)
            assert rc == N.ATMO_E_STATE and msg.startswith(WHO) and "atmo_set_precision 0" in msg, (kw, rc, msg)
        # null pointers in front of alignment, alignment in front of width, width in front of the range
        assert "null" in _shade(lib, ctx, rays=None, rgba=RGBA + 4, width=0)[1]
        assert "aligned" in _shade(lib, ctx, rays=RAYS + 4, width=0, first=2 ** 30)[1]
        assert "width" in _shade(lib, ctx, width=0, first=2 ** 30)[1]
        assert "2^30" in _shade(lib, ctx, first=2 ** 30)[1]
    finally:
        lib.atmo_destroy(ctx)


def test_every_mode_refusal_names_its_mode():
    """atmo_shade_rays' refusals (its table of cases), then this entry point's own: a variant without clouds, sampler mode 0.  Each context has one thing wrong."""
    N, lib = _lib()
    own = [("without clouds", N.VARIANT_NO_CLOUDS, {}), ("without clouds", N.VARIANT_V1_NO_CLOUDS, {}),
           ("without clouds", N.VARIANT_NO_CLOUDS, dict(light_mode=N.LIGHT_DIRECT, light_steps=8)),
           ("atmo_set_sampler_lod 0", N.VARIANT_CLOUDS_HIGH, dict(sampler=0)), ("atmo_set_sampler_lod 0", N.VARIANT_V1_CLOUDS, dict(sampler=0))]
    for needle, variant, kw in _mode_cases(N) + own:
        ctx = _mode_ctx(N, lib, variant, **kw)
        try:
            rc, msg = _shade(lib, ctx)
            assert rc == N.ATMO_E_STATE and msg.startswith(WHO) and needle in msg, (needle, kw, rc, msg)
            if (needle, variant, kw) in own:
                assert "atmo_shade_rays" in msg.replace(WHO, ""), msg     # the message points to the entry point that does serve this context
        finally:
            lib.atmo_destroy(ctx)


def test_mode_refusals_come_in_the_header_s_order():
    """A context with everything wrong is refused for the first item of the list; taking the items away one by one walks the list."""
    N, lib = _lib()
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH, view_steps=64, light_mode=N.LIGHT_DIRECT, light_steps=8, precision=0, lane_split=2, detail=True, sampler=0)
    try:
        assert "atmo_set_precision 0" in _shade(lib, ctx)[1]
        assert lib.atmo_set_precision(ctx, 2) == N.ATMO_OK
        assert "atmo_set_precision 2" in _shade(lib, ctx)[1]
        assert lib.atmo_set_precision(ctx, 1) == N.ATMO_OK
        assert "32 view steps" in _shade(lib, ctx)[1]
    finally:
        lib.atmo_destroy(ctx)
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH, light_mode=N.LIGHT_DIRECT, light_steps=8, lane_split=2, detail=True, sampler=0)
    try:
        assert "atmo_set_lane_split 2" in _shade(lib, ctx)[1]
        assert lib.atmo_set_lane_split(ctx, 1) == N.ATMO_OK
        assert "direct light" in _shade(lib, ctx)[1]
    finally:
        lib.atmo_destroy(ctx)
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH, detail=True, sampler=0)
    try:
        assert "cloud detail" in _shade(lib, ctx)[1]
        assert lib.atmo_set_cloud_detail(ctx, 0) == N.ATMO_OK
        assert "atmo_set_sampler_lod 0" in _shade(lib, ctx)[1]
        assert lib.atmo_set_sampler_lod(ctx, 1) == N.ATMO_OK
        # behind the sampler mode: the textures' check, as every draw (the mip chain's needs a device: tests/test_ray_quads_gpu.py)
        rc, msg = _shade(lib, ctx)
        assert rc == N.ATMO_E_STATE and msg.startswith(WHO) and "u_optical_depth_texture not set" in msg, (rc, msg)
    finally:
        lib.atmo_destroy(ctx)
    # a variant without clouds is refused in front of the sampler mode and behind atmo_shade_rays' list
    ctx = _mode_ctx(N, lib, N.VARIANT_NO_CLOUDS, lane_split=2, sampler=0)
    try:
        assert "atmo_set_lane_split 2" in _shade(lib, ctx)[1]
        assert lib.atmo_set_lane_split(ctx, 1) == N.ATMO_OK
        assert "without clouds" in _shade(lib, ctx)[1]
    finally:
        lib.atmo_destroy(ctx)


def test_a_host_only_context_never_gets_past_the_checks():
    """ATMO_E_NO_DEVICE stands behind every check.  Every variant this call accepts needs u_cloud_shape_texture, which only a device context can hold, so a
    host-only context's last answer is that texture's refusal (the header says so) -- for a v1 cloud variant, which needs no optical-depth texture, the
    one check in front of the device -- and never ATMO_OK; argument and mode refusals still come in front of it."""
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_V1_CLOUDS)
    try:
        rc, msg = _shade(lib, ctx)
        assert rc == N.ATMO_E_STATE and msg.startswith(WHO) and "u_cloud_shape_texture not set" in msg, (rc, msg)
        assert _shade(lib, ctx, width=0)[0] == N.ATMO_E_ARG
        assert lib.atmo_set_lane_split(ctx, 2) == N.ATMO_OK
        assert "atmo_set_lane_split 2" in _shade(lib, ctx)[1]
    finally:
        lib.atmo_destroy(ctx)


# ---- quad order --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 3), (113, 67), (300, 5)])
def test_quad_order_and_its_inverse(w, h):
    from godot_atmosphere_shader_amd.ray_quads import quad_order, quads_to_image

    order = quad_order(w, h)
    qpr = (w + 1) // 2
    assert order.dtype == np.int64 and order.shape == (4 * qpr * ((h + 1) // 2),)
    for slot in range(order.size):       # the header's formula, slot by slot
        q, j = divmod(slot, 4)
        x, y = 2 * (q % qpr) + (j & 1), 2 * (q // qpr) + (j >> 1)
        assert order[slot] == (y * w + x if x < w and y < h else -1), (slot, x, y)
    inside = order[order >= 0]
    assert np.array_equal(np.sort(inside), np.arange(w * h))        # a bijection onto the pixels
    # the round trip, with a trailing shape, on numpy arrays and on tensors
    image = np.arange(w * h * 3, dtype=np.float32).reshape(h, w, 3) + 1.0
    values = np.where((order >= 0)[:, None], image.reshape(-1, 3)[np.clip(order, 0, None)], 0.0).astype(np.float32)
    assert np.array_equal(quads_to_image(values, w, h), image)
    back = quads_to_image(torch.from_numpy(values), w, h)
    assert isinstance(back, torch.Tensor) and np.array_equal(back.numpy(), image)
    assert np.array_equal(quads_to_image(values[:, 0], w, h), image[:, :, 0])
    with pytest.raises(ValueError, match="one row per slot"):
        quads_to_image(values[:-1], w, h)
    with pytest.raises(ValueError, match="at least 1"):
        quad_order(0, h)


# ---- the binding, without a device ---------------------------------------------------------------------------------------------------------------
def _calls(node):
    return [(name, dict(zip(ABI[name], args))) for name, args in node._lib.calls if name != "atmo_destroy"]


def test_shade_ray_quads_reaches_its_entry_point():
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    node, cam = B._node(), B._cam()
    quads, out = B._fake((72, 8)), B._fake((72, 4))
    assert node.shade_ray_quads(quads, cam, width=11, first_quad=30, out=out, stream=B._Stream(), time=B.TIME) is out
    (name, a), = _calls(node)
    assert name == "atmo_shade_ray_quads"
    assert a == dict(ctx=B.CTX, frame=bytes(PA._to_native_frame(node.make_frame(cam, B.TIME))), rays=quads.data_ptr(), rgba=out.data_ptr(), n_quads=18,
                     width=11, first_quad=30, stream=B.STREAM)
    node = B._node()
    with B._AllocateAsCuda():
        out = node.shade_ray_quads(quads, width=11, stream=B.STREAM)   # the output is allocated; no camera: ray space is world space
    assert tuple(out.shape) == (72, 4) and out.dtype == torch.float32
    (name, a), = _calls(node)
    assert (a["n_quads"], a["width"], a["first_quad"], a["rgba"]) == (18, 11, 0, out.data_ptr())
    f = B.N.AtmoFrame.from_buffer_copy(a["frame"])
    assert list(f.inv_view_matrix) == [float(x) for x in np.eye(4).reshape(-1)]


def test_bad_tensors_raise_before_anything_reaches_the_library():
    node, cam = B._node(), B._cam()
    good, out = B._fake((12, 8)), B._fake((12, 4))
    for bad in (torch.zeros((12, 8)), B._fake((12, 8), torch.float16), B._fake((12, 16))[:, ::2], np.zeros((12, 8), dtype=np.float32), None):
        with pytest.raises(TypeError, match="quads must be a contiguous CUDA float32 tensor"):
            node.shade_ray_quads(bad, cam, width=6, stream=B.STREAM)
    for bad in (B._fake((12, 7)), B._fake((96,)), B._fake((12, 8, 1))):
        with pytest.raises(ValueError, match=r"quads must have shape \(n, 8\)"):
            node.shade_ray_quads(bad, cam, width=6, stream=B.STREAM)
    for bad in (B._fake((13, 8)), B._fake((6, 8)), B._fake((1, 8))):
        with pytest.raises(ValueError, match="four rows per quad"):
            node.shade_ray_quads(bad, cam, width=6, stream=B.STREAM)
    for bad in (torch.zeros((12, 4)), B._fake((12, 4), torch.float64), B._fake((12, 8))[:, ::2]):
        with pytest.raises(TypeError, match="out must be a contiguous CUDA float32 tensor"):
            node.shade_ray_quads(good, cam, width=6, out=bad, stream=B.STREAM)
    for bad in (B._fake((12, 3)), B._fake((8, 4)), B._fake((48,))):
        with pytest.raises(ValueError, match="out must have"):
            node.shade_ray_quads(good, cam, width=6, out=bad, stream=B.STREAM)
    for kw in (dict(width=0), dict(width=-3), dict(width=6, first_quad=-1), dict(width=6, first_quad=2 ** 30 - 2)):
        with pytest.raises(ValueError, match="width must be at least 1"):
            node.shade_ray_quads(good, cam, out=out, stream=B.STREAM, **kw)
    for kw in (dict(width=2.5), dict(width=6, first_quad="0")):
        with pytest.raises(TypeError, match="width and first_quad must be integers"):
            node.shade_ray_quads(good, cam, out=out, stream=B.STREAM, **kw)
    with pytest.raises(TypeError):      # width has no default: quad order means nothing without it
        node.shade_ray_quads(good, cam, out=out, stream=B.STREAM)
    with pytest.raises(TypeError, match="depth must be a contiguous CUDA float32 tensor"):
        node.camera_ray_quads(cam, torch.zeros((cam.height, cam.width)), stream=B.STREAM)
    assert _calls(node) == []


def test_a_library_without_the_symbol_says_so():
    node, cam = B._node(lib=B.library_without("atmo_shade_ray_quads")), B._cam()
    with pytest.raises(RuntimeError, match=r"atmo_shade_ray_quads \(include/atmo_ray_quads.h\)"):
        node.shade_ray_quads(B._fake((4, 8)), cam, width=2, out=B._fake((4, 4)), stream=B.STREAM)
    assert node.shade_rays(B._fake((4, 8)), cam, out=B._fake((4, 4)), stream=B.STREAM) is not None   # the older entry points of such a library still serve


# ---- the three kernels in the compiled assembly ---------------------------------------------------------------------------------------------------------------
def _mangled(kernel, flags, split=None):
    return f"_ZN4atmo{len(kernel)}{kernel}ILi{flags}ELi0E" + (f"Li{split}E" if split else "") + "E"


def test_the_new_kernels_cost_what_their_pixel_twins_cost(capsys):
    """atmo_shade_rays_kernel<16433 / 16435 / 16441, 0>: present under their mangled names, no stack frame, a VGPR count on the occupancy step of the pixel
    twin atmo_render_kernel<49 / 51 / 57, 0, 1> or a better one, and tools/check_quad_regs.py's `: ok;` line for each (the whole-quad exchange registers
    private, the march position written by the position update alone)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_quad_regs
    finally:
        sys.path.pop(0)
    text = T._asm()
    numbers = T.twin_resources.kernels(text)
    by_prefix = lambda p: [k for name, k in numbers.items() if name.startswith(p)]   # noqa: E731  (the mangled name, then the argument types)
    waves = T.twin_resources.vgpr_waves
    for flags, label in KERNELS.items():
        (new,), (twin,) = by_prefix(_mangled("atmo_shade_rays_kernel", flags | 16384)), by_prefix(_mangled("atmo_render_kernel", flags, 1))
        print(f"{label}: atmo_shade_rays_kernel<{flags | 16384}, 0> {new}; atmo_render_kernel<{flags}, 0, 1> {twin}")
        assert new["scratch"] == 0, label
        assert waves(new["vgprs"]) >= waves(twin["vgprs"]), (label, new["vgprs"], twin["vgprs"])
        assert new["loop_vector"] == twin["loop_vector"], label      # the texture fetches; no constant arrives through a vector load
    seen = capsys.readouterr().out
    assert check_quad_regs.report(text) == 0
    lines = capsys.readouterr().out.splitlines()
    print(seen)
    for flags in KERNELS:
        mine = [ln for ln in lines if ln.startswith(f"atmo_shade_rays_kernel<{flags | 16384}, 0> ")]
        assert len(mine) == 1 and ": ok;" in mine[0] and "only the position update writes them" in mine[0], (flags, mine)
    assert re.search(r"^\d+ kernels, 0 with a stack frame, 0 scratch instructions$", lines[-1]), lines[-1]
