"""CPU tests of cloud detail for rays (include/atmo_ray_detail.h): the header's symbol set and the binding, every refusal of the two entry points on
host-only contexts in their siblings' order and with their siblings' text (nothing touches a device), the cloud contexts with detail on that now pass the
mode checks while the older entry points still refuse them, the nine kernels in the compiled assembly (one compile, shared with
tests/test_kernel_twins_host.py), and the routing of PlanetAtmosphere.shade_rays / shade_ray_quads on the recorder of tests/test_binding_calls_host.py.
(tests/test_ray_detail_gpu.py holds the kernels to the detail draws, bit for bit.)"""
import ctypes as C

import pytest
import torch

import test_binding_calls_host as B
import test_kernel_twins_host as T
from test_rays_host import RAYS, RGBA, _mode_cases, _mode_ctx, _said
from test_views_proxy_host import FAR, _frame, _functions, _host_ctx

INDEX = 0x40000   # an address no refusal dereferences
RAYS_WHO, QUADS_WHO = "atmo_shade_rays_detail: ", "atmo_shade_ray_quads_detail: "
NAMES = {"atmo_shade_rays_detail", "atmo_shade_ray_quads_detail"}


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, N.load()


def _rays(lib, ctx, frame=True, rays=RAYS, rgba=RGBA, n=64, width=8, first=0, index=None, n_index=0, entry="atmo_shade_rays_detail"):
    """atmo_shade_rays_detail, or one of its two siblings with the same arguments (the plain one takes no list)."""
    f = _frame(FAR)
    listed = () if entry == "atmo_shade_rays" else (index, n_index)
    return _said(lib, ctx, getattr(lib, entry)(ctx, C.byref(f) if frame else None, rays, rgba, n, width, first, *listed, None))


def _quads(lib, ctx, frame=True, rays=RAYS, rgba=RGBA, n=16, width=8, first=0, entry="atmo_shade_ray_quads_detail"):
    f = _frame(FAR)
    return _said(lib, ctx, getattr(lib, entry)(ctx, C.byref(f) if frame else None, rays, rgba, n, width, first, None))


def _listed(lib, ctx, **kw):
    return _rays(lib, ctx, index=INDEX, n_index=33, **kw)


def _listed_old(lib, ctx, **kw):
    return _rays(lib, ctx, index=INDEX, n_index=33, entry="atmo_shade_rays_indexed", **kw)


# (the new call, its sibling, the new name, the sibling's name)
PAIRS = [(_rays, lambda lib, ctx, **kw: _rays(lib, ctx, entry="atmo_shade_rays", **kw), RAYS_WHO, "atmo_shade_rays: "),
         (_listed, _listed_old, RAYS_WHO, "atmo_shade_rays_indexed: "),
         (_quads, lambda lib, ctx, **kw: _quads(lib, ctx, entry="atmo_shade_ray_quads", **kw), QUADS_WHO, "atmo_shade_ray_quads: ")]


def _same_but_for_the_name(new, old, who_new, who_old):
    """The sibling's answer and the new entry point's are equal once the names are removed (a message may name the sibling as the call to use instead)."""
    assert new[0] == old[0], (new, old)
    assert new[1].startswith(who_new) and old[1].startswith(who_old), (new, old)
    assert new[1][len(who_new):] == old[1][len(who_old):], (new, old)


def test_binding_exposes_the_ray_detail_header():
    N, lib = _lib()
    assert _functions("atmo_ray_detail.h") == set(N.RAY_DETAIL_SYMBOLS) == NAMES
    for sym in N.RAY_DETAIL_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS
    assert N.EXPORTED_SYMBOLS == (N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_PROXY_SYMBOLS +
                                  N.VIEWS_TARGET_SYMBOLS)
    for other in (N.RAYS_SYMBOLS, N.RAY_QUADS_SYMBOLS, N.RAY_ORDER_SYMBOLS, N.RAY_LIST_SYMBOLS, N.CLOUD_DETAIL_SYMBOLS):
        assert not set(N.RAY_DETAIL_SYMBOLS) & set(other)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5


def test_nothing_to_shade_is_ok_whatever_else_is_passed():
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    try:
        assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK   # a mode that refuses every other call
        assert lib.atmo_shade_rays_detail(ctx, None, None, None, 0, 0, 0, None, 0, None) == N.ATMO_OK
        assert lib.atmo_shade_rays_detail(ctx, None, None, None, 64, 0, 0, INDEX + 1, 0, None) == N.ATMO_OK      # a list of no entries
        assert _rays(lib, ctx, n=0, width=0, rays=RAYS + 4)[0] == N.ATMO_OK
        assert lib.atmo_shade_ray_quads_detail(ctx, None, None, None, 0, 0, 0, None) == N.ATMO_OK
        assert _quads(lib, ctx, n=0, width=0, rays=RAYS + 4, first=2 ** 31)[0] == N.ATMO_OK
        # index_dev == NULL: n_index is not looked at -- the call gets as far as the mode, as atmo_shade_rays does
        rc, msg = _rays(lib, ctx, index=None, n_index=0)
        assert rc == N.ATMO_E_STATE and "atmo_set_precision 0" in msg
    finally:
        lib.atmo_destroy(ctx)
    assert lib.atmo_shade_rays_detail(None, None, None, None, 0, 0, 0, None, 0, None) == N.ATMO_E_ARG
    assert lib.atmo_shade_ray_quads_detail(None, None, None, None, 0, 0, 0, None) == N.ATMO_E_ARG


def test_argument_refusals_come_in_the_siblings_order_under_the_new_names():
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    try:
        assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK   # the first mode refusal stands behind every argument check
        ray_cases = (dict(frame=False), dict(rays=None), dict(rgba=None), dict(rays=RAYS + 4), dict(rays=RAYS + 8), dict(rgba=RGBA + 4), dict(width=0),
                     dict(first=2 ** 32 - 63), dict(first=2 ** 32 - 1, n=2), dict(first=2, n=2 ** 32 - 1))
        quad_cases = (dict(frame=False), dict(rays=None), dict(rgba=None), dict(rays=RAYS + 4), dict(rgba=RGBA + 4), dict(width=0),
                      dict(first=2 ** 30 - 15), dict(first=2 ** 30, n=1), dict(first=1, n=2 ** 30))
        for (new, old, who_new, who_old), cases in zip(PAIRS, (ray_cases, ray_cases, quad_cases)):
            for kw in cases:
                got = new(lib, ctx, **kw)
                assert got[0] == N.ATMO_E_ARG, (kw, got)
                _same_but_for_the_name(got, old(lib, ctx, **kw), who_new, who_old)
            got = new(lib, ctx)          # a well-formed call gets as far as the mode
            assert got[0] == N.ATMO_E_STATE and "atmo_set_precision 0" in got[1]
        # the list's own two, behind the pointers' alignment and in front of width
        for kw in (dict(index=INDEX + 2, n_index=5), dict(index=INDEX + 1, n_index=5, width=0)):
            rc, msg = _rays(lib, ctx, **kw)
            assert rc == N.ATMO_E_ARG and msg.startswith(RAYS_WHO) and "index_dev must be 4-byte aligned" in msg, (kw, rc, msg)
            _same_but_for_the_name((rc, msg), _rays(lib, ctx, entry="atmo_shade_rays_indexed", **kw), RAYS_WHO, "atmo_shade_rays_indexed: ")
        assert "aligned" in _listed(lib, ctx, rays=RAYS + 4, width=0)[1] and "width" in _listed(lib, ctx, width=0, first=2 ** 32 - 1)[1]
        assert "null" in _quads(lib, ctx, rays=None, rgba=RGBA + 4, width=0)[1] and "2^30" in _quads(lib, ctx, first=2 ** 30)[1]
    finally:
        lib.atmo_destroy(ctx)


def test_every_mode_refusal_is_the_sibling_s_under_the_new_name():
    """test_rays_host's table minus its two cloud-detail rows; for the quads, their own two as well."""
    N, lib = _lib()
    cases = [c for c in _mode_cases(N) if "cloud detail" not in c[0]]
    assert len(cases) == len(_mode_cases(N)) - 2
    own = [("without clouds", N.VARIANT_NO_CLOUDS, {}), ("atmo_set_sampler_lod 0", N.VARIANT_CLOUDS_HIGH, dict(sampler=0))]
    for new, old, who_new, who_old in PAIRS:
        for needle, variant, kw in cases + (own if who_new == QUADS_WHO else []):
            for detail in (False, True):       # the switch changes none of these answers
                ctx = _mode_ctx(N, lib, variant, **dict(kw, detail=detail))
                try:
                    got = new(lib, ctx)
                    assert got[0] == N.ATMO_E_STATE and got[1].startswith(who_new) and needle in got[1], (needle, kw, detail, got)
                    if not detail:
                        _same_but_for_the_name(got, old(lib, ctx), who_new, who_old)
                finally:
                    lib.atmo_destroy(ctx)


def test_cloud_contexts_with_detail_on_pass_the_mode_checks():
    """... and reach the textures' check; the OLD entry points still name cloud detail on the very same contexts; the quad entry's sampler rule stands."""
    N, lib = _lib()
    for variant in (N.VARIANT_CLOUDS_HIGH, N.VARIANT_CLOUDS_HIGH_RM, N.VARIANT_V1_CLOUDS):
        # (a v1 cloud variant needs no optical-depth texture: its first missing texture is the shape volume)
        missing = "u_cloud_shape_texture not set" if variant == N.VARIANT_V1_CLOUDS else "u_optical_depth_texture not set"
        ctx = _mode_ctx(N, lib, variant, detail=True)
        try:
            for new, old, who_new, who_old in PAIRS:
                rc, msg = new(lib, ctx)
                assert rc == N.ATMO_E_STATE and msg.startswith(who_new) and missing in msg, (variant, rc, msg)
                rc, msg = old(lib, ctx)
                assert rc == N.ATMO_E_STATE and msg.startswith(who_old) and "cloud detail (atmo_set_cloud_detail 1)" in msg, (variant, rc, msg)
            assert lib.atmo_set_sampler_lod(ctx, 0) == N.ATMO_OK
            rc, msg = _quads(lib, ctx)
            assert rc == N.ATMO_E_STATE and msg.startswith(QUADS_WHO) and "atmo_set_sampler_lod 0" in msg, (variant, rc, msg)
            assert missing in _rays(lib, ctx)[1]        # level 0 is the plain rays' sampler
        finally:
            lib.atmo_destroy(ctx)


def test_the_clouds_high_context_names_the_optical_depth_texture():
    """The v2 cloud variants through all three call shapes: detail on, the mode checks passed, `u_optical_depth_texture not set`."""
    N, lib = _lib()
    for variant in (N.VARIANT_CLOUDS_HIGH, N.VARIANT_CLOUDS_HIGH_RM):
        ctx = _mode_ctx(N, lib, variant, detail=True)
        try:
            for call in (_rays, _listed, _quads):
                assert "u_optical_depth_texture not set" in call(lib, ctx)[1]
        finally:
            lib.atmo_destroy(ctx)


def test_with_detail_off_the_answers_are_the_siblings():
    N, lib = _lib()
    for variant in (N.VARIANT_CLOUDS_HIGH, N.VARIANT_V1_CLOUDS, N.VARIANT_NO_CLOUDS):
        ctx = _mode_ctx(N, lib, variant)
        try:
            for new, old, who_new, who_old in PAIRS:
                _same_but_for_the_name(new(lib, ctx), old(lib, ctx), who_new, who_old)
        finally:
            lib.atmo_destroy(ctx)
    # the direct-light variant without clouds needs no texture: a well-formed call gets as far as the device, switch on or off
    for detail in (False, True):
        ctx = _mode_ctx(N, lib, N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8, detail=detail)
        try:
            for call in (_rays, _listed):
                rc, msg = call(lib, ctx)
                assert rc == N.ATMO_E_NO_DEVICE and msg.startswith(RAYS_WHO), (rc, msg)
            assert "without clouds" in _quads(lib, ctx)[1]
            assert _rays(lib, ctx, width=0)[0] == N.ATMO_E_ARG
        finally:
            lib.atmo_destroy(ctx)


# ---- the nine kernels in the compiled assembly ----------------------------------------------------------------------------------------------------------------
LEVEL0 = {17: "clouds_high", 19: "clouds_high_rm", 25: "v1_clouds"}
KF_DETAIL, KF_RAYS, KF_INDEX = 8192, 16384, 32768


def _mangled(kernel, flags):
    return f"_ZN4atmo{len(kernel)}{kernel}ILi{flags}ELi0EE"


def test_the_nine_kernels_cost_what_their_detail_twins_cost():
    """Present under their mangled names, no stack frame, a VGPR count on the occupancy step of the atmo_render_detail_kernel twin or a better one; the
    indexed kernels with as many vector loads inside loops as their plain detail-ray twins; names of their own."""
    text = T._asm()
    numbers = T.twin_resources.kernels(text)
    by_prefix = lambda p: [k for name, k in numbers.items() if name.startswith(p)]   # noqa: E731  (the mangled name, then the argument types)
    waves = T.twin_resources.vgpr_waves

    def base(mangled):     # _ZN4atmo<length><name>...
        m = T.re.match(r"_ZN4atmo(\d+)", mangled)
        return mangled[m.end():m.end() + int(m.group(1))]

    assert len([n for n in numbers if base(n) == "atmo_detail_rays_kernel"]) == 6
    assert len([n for n in numbers if "atmo_detail_rays_kernel" in n]) == 6
    assert len([n for n in numbers if "atmo_detail_rays_indexed_kernel" in n]) == 3
    for family, label in LEVEL0.items():
        for kernel, flags in (("atmo_detail_rays_kernel", family | KF_DETAIL | KF_RAYS), ("atmo_detail_rays_kernel", family | 32 | KF_DETAIL | KF_RAYS),
                              ("atmo_detail_rays_indexed_kernel", family | KF_DETAIL | KF_RAYS | KF_INDEX)):
            (new,), (twin,) = by_prefix(_mangled(kernel, flags)), by_prefix(_mangled("atmo_render_detail_kernel", flags & ~(KF_RAYS | KF_INDEX)))
            print(f"{label}: {kernel}<{flags}, 0> {new}; atmo_render_detail_kernel<{flags & ~(KF_RAYS | KF_INDEX)}, 0> {twin}")
            assert new["scratch"] == 0, (label, kernel, flags)
            assert waves(new["vgprs"]) >= waves(twin["vgprs"]), (label, kernel, flags, new["vgprs"], twin["vgprs"])
            if flags & KF_INDEX:
                (plain,) = by_prefix(_mangled("atmo_detail_rays_kernel", flags & ~KF_INDEX))
                assert new["loop_vector"] == plain["loop_vector"], label      # the index entry is loaded once, in front of everything
    names = {base(n) for n in numbers}
    new_names = {"atmo_detail_rays_kernel", "atmo_detail_rays_indexed_kernel"}
    assert new_names <= names, names
    for a in new_names:
        for b in names - {a}:
            assert a not in b and b not in a, (a, b)


# ---- the binding, without a device -----------------------------------------------------------------------------------------------------------------------------
RAY_NAMES = ("ctx", "frame", "rays", "rgba", "n", "width", "first", "index", "n_index", "stream")
QUAD_NAMES = ("ctx", "frame", "rays", "rgba", "n_quads", "width", "first_quad", "stream")


def _detail_node(shader="planet_atmosphere_clouds_high", on=True, lib=None):
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    node = B._node(lib=lib)
    node._cloud_detail, node._shader = on, PA.SHADERS[shader]
    return node


def _calls(node):
    return [c for c in node._lib.calls if c[0] != "atmo_destroy"]


def test_a_cloud_node_with_cloud_detail_reaches_the_new_entry_points():
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    cam = B._cam()
    rays, out, index = B._fake((72, 8)), B._fake((72, 4)), B._fake((33,), torch.int32)
    for shader in ("planet_atmosphere_clouds_high", "planet_atmosphere_clouds_high_rm", "planet_atmosphere_v1_clouds"):
        node = _detail_node(shader)
        frame = bytes(PA._to_native_frame(node.make_frame(cam, B.TIME)))      # `time` goes into the frame
        assert node.shade_rays(rays, cam, width=10, first=30, out=out, stream=B._Stream(), time=B.TIME) is out
        assert node.shade_rays(rays, cam, width=10, first=30, out=out, stream=B._Stream(), time=B.TIME, index=index) is out
        assert node.shade_ray_quads(rays, cam, width=11, first_quad=30, out=out, stream=B._Stream(), time=B.TIME) is out
        (n0, a0), (n1, a1), (n2, a2) = _calls(node)
        assert n0 == n1 == "atmo_shade_rays_detail" and n2 == "atmo_shade_ray_quads_detail"
        assert dict(zip(RAY_NAMES, a0)) == dict(ctx=B.CTX, frame=frame, rays=rays.data_ptr(), rgba=out.data_ptr(), n=72, width=10, first=30, index=None,
                                                n_index=0, stream=B.STREAM)
        assert dict(zip(RAY_NAMES, a1)) == dict(ctx=B.CTX, frame=frame, rays=rays.data_ptr(), rgba=out.data_ptr(), n=72, width=10, first=30,
                                                index=index.data_ptr(), n_index=33, stream=B.STREAM)
        assert dict(zip(QUAD_NAMES, a2)) == dict(ctx=B.CTX, frame=frame, rays=rays.data_ptr(), rgba=out.data_ptr(), n_quads=18, width=11, first_quad=30,
                                                 stream=B.STREAM)
        assert C.c_float.from_buffer_copy(frame, B.N.AtmoFrame.time.offset).value == C.c_float(B.TIME).value != 0.0


def test_with_it_off_or_without_clouds_the_old_entry_points_serve():
    cam = B._cam()
    rays, out, index = B._fake((72, 8)), B._fake((72, 4)), B._fake((33,), torch.int32)
    for node in (_detail_node(on=False), _detail_node("planet_atmosphere_no_clouds"), _detail_node("planet_atmosphere_v1_no_clouds"), B._node()):
        node.shade_rays(rays, cam, out=out, stream=B.STREAM)
        node.shade_rays(rays, cam, out=out, stream=B.STREAM, index=index)
        node.shade_ray_quads(rays, cam, width=11, out=out, stream=B.STREAM)
        assert [name for name, _ in _calls(node)] == ["atmo_shade_rays", "atmo_shade_rays_indexed", "atmo_shade_ray_quads"]
        assert [len(args) for _, args in _calls(node)] == [8, 10, 8]


def test_a_library_without_the_symbols_says_so():
    cam = B._cam()
    rays, out = B._fake((8, 8)), B._fake((8, 4))
    node = _detail_node(lib=B.library_without(*NAMES))
    with pytest.raises(RuntimeError, match=r"atmo_shade_rays_detail \(include/atmo_ray_detail.h\)"):
        node.shade_rays(rays, cam, out=out, stream=B.STREAM)
    with pytest.raises(RuntimeError, match=r"atmo_shade_ray_quads_detail \(include/atmo_ray_detail.h\)"):
        node.shade_ray_quads(rays, cam, width=4, out=out, stream=B.STREAM)
    assert _calls(node) == []
    # with the switch off, or on a node without clouds, such a library serves as before
    for node in (_detail_node(on=False, lib=B.library_without(*NAMES)), _detail_node("planet_atmosphere_no_clouds", lib=B.library_without(*NAMES))):
        assert node.shade_rays(rays, cam, out=out, stream=B.STREAM) is out and node.shade_ray_quads(rays, cam, width=4, out=out, stream=B.STREAM) is out
        assert [name for name, _ in _calls(node)] == ["atmo_shade_rays", "atmo_shade_ray_quads"]
