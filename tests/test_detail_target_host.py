"""CPU tests of cloud detail into colour targets through a depth source (include/atmo_detail_target.h): the header's symbol set and the binding, every
refusal of the two entry points on host-only contexts in their siblings' order (nothing touches a device), with the switch off the siblings' answers under
the new names, the older entry points' unchanged refusals, the twelve kernels in the compiled assembly (one compile, shared with
tests/test_kernel_twins_host.py), and the routing of PlanetAtmosphere's draws on the recorder of tests/test_binding_calls_host.py.
(tests/test_detail_target_gpu.py holds the kernels to the detail draws, bit for bit, and the kernel names atmo_kernel_name reports after a draw: a
host-only context cannot draw, and before the first draw the name is atmo_render's.)"""
import ctypes as C

import pytest
import torch

import test_binding_calls_host as B
import test_kernel_twins_host as T
from test_rays_host import _mode_ctx, _said
from test_views_proxy_host import FAR, _frame, _functions, _host_ctx

IMG, TEX, STEP = 0x100000, 0x800000, 0x10000   # addresses no refusal dereferences
F32, F16, U8, SRGB = 0, 1, 2, 16
D32, D16, D24 = 0, 1, 2
W, H = FAR.width, FAR.height
ONE, ONE_OLD = "atmo_render_detail_target: ", "atmo_render_depth_target: "
BATCH, BATCH_OLD = "atmo_render_views_detail_target: ", "atmo_render_views_depth_target: "
NAMES = {"atmo_render_detail_target", "atmo_render_views_detail_target"}
CLOUD_VARIANTS = ("VARIANT_CLOUDS", "VARIANT_CLOUDS_HIGH", "VARIANT_CLOUDS_HIGH_RM", "VARIANT_V1_CLOUDS", "VARIANT_V1_CLOUDS_HIGH")


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, N.load()


def _one(lib, ctx, frame=True, rect=None, depth=True, texels=TEX, dfmt=D32, dpitch=0, target=True, pixels=IMG, fmt=F16, pitch=0, composite=0,
         entry="atmo_render_detail_target"):
    """atmo_render_detail_target, or atmo_render_depth_target with the same arguments."""
    N, _ = _lib()
    f, d, t = _frame(FAR, rect), N.AtmoDepth(texels, dfmt, dpitch), N.AtmoTarget(pixels, fmt, pitch)
    return _said(lib, ctx, getattr(lib, entry)(ctx, C.byref(f) if frame else None, C.byref(d) if depth else None, C.byref(t) if target else None,
                                                composite, None))


def _one_old(lib, ctx, **kw):
    return _one(lib, ctx, entry="atmo_render_depth_target", **kw)


def _views(specs):
    """specs: [dict(rect, texels, dfmt, dpitch, pixels, fmt, pitch)] -> N.AtmoViewDepthTarget array; the defaults are two disjoint tight views."""
    N, _ = _lib()
    arr = (N.AtmoViewDepthTarget * max(len(specs), 1))()
    for i, s in enumerate(specs):
        arr[i].frame = _frame(FAR, s.get("rect"))
        arr[i].depth = N.AtmoDepth(s.get("texels", TEX + i * STEP), s.get("dfmt", D16), s.get("dpitch", 0))
        arr[i].target = N.AtmoTarget(s.get("pixels", IMG + i * STEP), s.get("fmt", F16), s.get("pitch", 0))
    return arr


def _batch(lib, ctx, specs=({}, {}), n=None, null=False, composite=0, entry="atmo_render_views_detail_target"):
    arr = None if null else _views(list(specs))
    return _said(lib, ctx, getattr(lib, entry)(ctx, arr, len(specs) if n is None else n, composite, None))


def _batch_old(lib, ctx, **kw):
    return _batch(lib, ctx, entry="atmo_render_views_depth_target", **kw)


PAIRS = [(_one, _one_old, ONE, ONE_OLD), (_batch, _batch_old, BATCH, BATCH_OLD)]


def _same_but_for_the_name(new, old, who_new, who_old):
    """The sibling's answer and the new entry point's are equal once the names in front are exchanged.  (What atmo_render_depth_target hears from
    render_impl -- the textures' check -- names atmo_render; the new entry point's every message names the new entry point.)"""
    assert new[0] == old[0], (new, old)
    if who_old == ONE_OLD and old[1].startswith("atmo_render: "):
        who_old = "atmo_render: "
    assert new[1].startswith(who_new) and old[1].startswith(who_old), (new, old)
    assert new[1][len(who_new):] == old[1][len(who_old):], (new, old)


# ---- the header and the binding ----------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_the_detail_target_header():
    """Fails on a library without the feature: the header does not exist and the symbols are not exported."""
    N, lib = _lib()
    assert _functions("atmo_detail_target.h") == set(N.DETAIL_TARGET_SYMBOLS) == NAMES
    for sym in N.DETAIL_TARGET_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS
    assert N.EXPORTED_SYMBOLS == (N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_PROXY_SYMBOLS +
                                  N.VIEWS_TARGET_SYMBOLS)
    for other in (N.DEPTH_SYMBOLS, N.CLOUD_DETAIL_SYMBOLS, N.RAY_DETAIL_SYMBOLS, N.RAYS_SYMBOLS, N.PLANETS_SYMBOLS):
        assert not set(N.DETAIL_TARGET_SYMBOLS) & set(other)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5
    text = open(T.os.path.join(T.ROOT, "include", "atmo_detail_target.h")).read()
    for inc in ("atmo_depth.h", "atmo_views_target.h", "atmo_cloud_detail.h"):
        assert f'#include "{inc}"' in text
    # the older headers do not know the new one
    for name in ("atmo.h", "atmo_target.h", "atmo_depth.h", "atmo_views_target.h", "atmo_ray_detail.h"):
        assert "atmo_detail_target" not in open(T.os.path.join(T.ROOT, "include", name)).read(), name


# ---- nothing to draw -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("detail", [False, True])
def test_an_empty_rect_and_no_views_are_ok(detail):
    N, lib = _lib()
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH_RM, detail=detail)
    try:
        assert _one(lib, ctx, rect=(5, 5, 5, 30), depth=False)[0] == N.ATMO_OK          # behind the target's checks and the mode; the depth is not looked at
        assert _one(lib, ctx, rect=(5, 7, 30, 7), texels=0, composite=1)[0] == N.ATMO_OK
        assert _one(lib, ctx, rect=(5, 5, 5, 30), target=False)[0] == N.ATMO_E_ARG      # ... the target is
        assert lib.atmo_render_views_detail_target(ctx, None, 0, 0, None) == N.ATMO_OK  # n_views == 0: nothing else is looked at
        assert _batch(lib, ctx, n=0)[0] == N.ATMO_OK
        assert _batch(lib, ctx, specs=(dict(rect=(5, 5, 5, 30), texels=0, pixels=0), dict(rect=(0, 9, 64, 9))))[0] == N.ATMO_OK   # every rect empty
        assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK                               # a mode that refuses every draw
        assert lib.atmo_render_views_detail_target(ctx, None, 0, 0, None) == N.ATMO_OK
        assert _one(lib, ctx, rect=(5, 5, 5, 30))[0] == N.ATMO_E_STATE                   # the single draw's mode check stands in front of the empty rect, as its sibling's
        assert _one_old(lib, ctx, rect=(5, 5, 5, 30))[0] == N.ATMO_E_STATE
    finally:
        lib.atmo_destroy(ctx)
    assert lib.atmo_render_detail_target(None, None, None, None, 0, None) == N.ATMO_E_ARG
    assert lib.atmo_render_views_detail_target(None, None, 0, 0, None) == N.ATMO_E_ARG


# ---- the argument checks: the siblings', in their order, under the new names ---------------------------------------------------------------------------
ONE_ARGS = [dict(frame=False), dict(target=False), dict(fmt=3), dict(fmt=20), dict(pixels=0), dict(pixels=IMG + 4), dict(fmt=U8, pixels=IMG + 2),
            dict(rect=(0, 0, W + 1, H)), dict(rect=(9, 0, 8, H)), dict(pitch=W * 8 - 8), dict(pitch=W * 8 + 4), dict(composite=1, rect=(8, 8, 16, 16), pitch=64),
            # the depth source, behind everything of the target and behind the mode
            dict(depth=False), dict(dfmt=3), dict(dfmt=-1), dict(texels=0), dict(texels=TEX + 2), dict(dfmt=D16, texels=TEX + 1),
            dict(dpitch=W * 4 - 4), dict(dpitch=W * 4 + 2), dict(dfmt=D16, dpitch=W * 2 + 1)]
ONE_ORDER = [dict(frame=False, target=False), dict(target=False, fmt=3), dict(fmt=3, pixels=0), dict(pixels=0, rect=(9, 0, 8, H)),
             dict(pixels=IMG + 4, pitch=4), dict(rect=(9, 0, 8, H), pitch=4), dict(pitch=4, depth=False), dict(depth=False, dfmt=3),
             dict(dfmt=3, texels=0), dict(texels=0, dpitch=4), dict(texels=TEX + 2, dpitch=4)]
BATCH_ARGS = [dict(n=-1), dict(n=9), dict(null=True), dict(specs=({}, dict(rect=(0, 0, W + 1, H)))), dict(specs=(dict(fmt=3), {})),
              dict(specs=({}, dict(pixels=0))), dict(specs=({}, dict(pixels=IMG + STEP + 4))), dict(specs=({}, dict(pitch=8))),
              dict(specs=({}, dict(texels=0))), dict(specs=({}, dict(dfmt=7))), dict(specs=(dict(texels=TEX + 1), {})), dict(specs=({}, dict(dpitch=W * 2 - 2))),
              dict(specs=({}, dict(fmt=SRGB))), dict(specs=({}, dict(pixels=IMG))), dict(specs=({}, dict(pixels=IMG + 64))),
              dict(specs=(dict(fmt=3), dict(texels=0))), dict(specs=(dict(texels=0), dict(fmt=3))), dict(specs=(dict(pitch=8, texels=0), {}))]


@pytest.mark.parametrize("detail", [False, True])
def test_argument_refusals_are_the_siblings_under_the_new_names(detail):
    """Every ATMO_E_ARG of atmo_render_depth_target / atmo_render_views_depth_target, alone and in pairs that show the order, with the switch off and on
    (a cloud context: on, the older calls refuse at their mode check -- behind every argument check of the target, so those answers are compared with
    the switch-off sibling on a second context)."""
    N, lib = _lib()
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH, detail=detail)
    ref = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH)
    try:
        for (new, old, who_new, who_old), cases in zip(PAIRS, (ONE_ARGS + ONE_ORDER, BATCH_ARGS)):
            for kw in cases:
                got = new(lib, ctx, **kw)
                assert got[0] == N.ATMO_E_ARG and got[1].startswith(who_new), (kw, got)
                _same_but_for_the_name(got, old(lib, ref, **kw), who_new, who_old)
            got = new(lib, ctx)          # a well-formed call gets as far as the textures
            assert got[0] == N.ATMO_E_STATE and got[1] == who_new + "u_optical_depth_texture not set (call atmo_bake_optical_depth or atmo_set_texture)", got
        # a view's refusal names the view; the side-by-side halves of one image and one depth image are accepted
        assert _batch(lib, ctx, specs=({}, dict(texels=0)))[1].startswith(BATCH + "view 1: ")
        halves = (dict(rect=None, pixels=IMG, pitch=2 * W * 8, texels=TEX, dpitch=2 * W * 2), dict(pixels=IMG + W * 8, pitch=2 * W * 8, texels=TEX + W * 2, dpitch=2 * W * 2))
        assert _batch(lib, ctx, specs=halves)[0] == N.ATMO_E_STATE and "texture not set" in _batch(lib, ctx, specs=halves)[1]
        assert "overlapping" in _batch(lib, ctx, specs=({}, dict(pixels=IMG + 64)))[1]
    finally:
        lib.atmo_destroy(ctx)
        lib.atmo_destroy(ref)


# ---- the mode checks -----------------------------------------------------------------------------------------------------------------------------------
MODES = {
    "precision 0": dict(precision=0),
    "precision 2": dict(precision=2),
    "lane split 2": dict(lane_split=2),
    "direct light": dict(light_mode=1, light_steps=8),
    "64 view steps": dict(view_steps=64),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_with_detail_on_the_modes_without_a_detail_kernel_are_refused(mode):
    """cloud_detail_mode's refusal, under the new names, behind every argument check of the target and in front of the depth source, the textures and the
    device; with the switch off the answer is the sibling's (its own mode refusal, or -- direct light -- the textures')."""
    N, lib = _lib()
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH_RM, **MODES[mode])
    try:
        for new, old, who_new, who_old in PAIRS:
            _same_but_for_the_name(new(lib, ctx), old(lib, ctx), who_new, who_old)
        assert lib.atmo_set_cloud_detail(ctx, 1) == N.ATMO_OK
        for new, old, who_new, who_old in PAIRS:
            rc, msg = new(lib, ctx)
            assert rc == N.ATMO_E_STATE and msg.startswith(who_new + "no cloud-detail kernel for this context's mode (atmo_set_cloud_detail 1"), (rc, msg)
            rc, msg = old(lib, ctx)      # the older entry points: their refusal of cloud detail, as before
            assert rc == N.ATMO_E_STATE and msg.startswith(who_old) and "cloud detail (atmo_set_cloud_detail 1)" in msg, (rc, msg)
        # order: the target's argument checks in front, the depth source behind
        assert _one(lib, ctx, pixels=0)[0] == N.ATMO_E_ARG and _one(lib, ctx, texels=0)[0] == N.ATMO_E_STATE
        assert _batch(lib, ctx, specs=({}, dict(texels=0)))[0] == N.ATMO_E_ARG      # (the batch checks every view's depth with its target, as its sibling)
    finally:
        lib.atmo_destroy(ctx)


def test_cloud_contexts_with_detail_on_pass_the_mode_checks_and_the_older_calls_still_refuse():
    N, lib = _lib()
    for name in CLOUD_VARIANTS:
        variant = getattr(N, name)
        missing = "u_cloud_shape_texture not set" if "V1" in name else "u_optical_depth_texture not set"
        ctx = _mode_ctx(N, lib, variant, detail=True)
        try:
            for fmt in (F32, F16, U8, SRGB, 17, 18, 19):
                rc, msg = _one(lib, ctx, fmt=fmt)
                assert rc == N.ATMO_E_STATE and msg.startswith(ONE) and missing in msg and "detail" not in msg[len(ONE):], (name, fmt, rc, msg)
            for new, old, who_new, who_old in PAIRS:
                rc, msg = new(lib, ctx)
                assert rc == N.ATMO_E_STATE and msg.startswith(who_new) and missing in msg, (name, rc, msg)
                rc, msg = old(lib, ctx)
                assert rc == N.ATMO_E_STATE and msg.startswith(who_old) and "cloud detail (atmo_set_cloud_detail 1)" in msg, (name, rc, msg)
            # two more of the entry points atmo_cloud_detail.h lists, re-asserted: unchanged
            f, t = _frame(FAR), N.AtmoTarget(IMG, F16, 0)
            rc, msg = _said(lib, ctx, lib.atmo_render_target(ctx, C.byref(f), 0x1000, C.byref(t), 0, None))
            assert rc == N.ATMO_E_STATE and msg.startswith("atmo_render_target: cloud detail (atmo_set_cloud_detail 1)"), (rc, msg)
            tv = (N.AtmoViewTarget * 1)()
            tv[0].frame, tv[0].depth_dev, tv[0].target = _frame(FAR), 0x1000, N.AtmoTarget(IMG, F16, 0)
            rc, msg = _said(lib, ctx, lib.atmo_render_views_target(ctx, tv, 1, 0, None))
            assert rc == N.ATMO_E_STATE and msg.startswith("atmo_render_views_target: cloud detail (atmo_set_cloud_detail 1)"), (rc, msg)
            # ... and atmo_render itself answers a target that reaches it as before: its own name, "tile lists, cost measurements or targets"
            rc, msg = _said(lib, ctx, lib.atmo_render_tiles(ctx, C.byref(f), 0x1000, 0x2000, 0x3000, 4, None))
            assert rc == N.ATMO_E_STATE and "cloud detail" in msg, (rc, msg)
        finally:
            lib.atmo_destroy(ctx)


def test_with_detail_off_or_without_clouds_the_answers_are_the_siblings():
    N, lib = _lib()
    for variant, kw in ((N.VARIANT_CLOUDS_HIGH, {}), (N.VARIANT_V1_CLOUDS, {}), (N.VARIANT_NO_CLOUDS, {}), (N.VARIANT_CLOUDS_HIGH, dict(precision=0)),
                        (N.VARIANT_NO_CLOUDS, dict(precision=2)), (N.VARIANT_NO_CLOUDS, dict(view_steps=64)), (N.VARIANT_NO_CLOUDS, dict(lane_split=2, detail=True)),
                        (N.VARIANT_NO_CLOUDS, dict(detail=True)), (N.VARIANT_V1_NO_CLOUDS, dict(detail=True))):
        ctx = _mode_ctx(N, lib, variant, **kw)
        try:
            for new, old, who_new, who_old in PAIRS:
                for fmt in (F32, F16):
                    args = dict(fmt=fmt) if new is _one else dict(specs=(dict(fmt=fmt), dict(fmt=fmt)))
                    got = new(lib, ctx, **args)
                    if variant == N.VARIANT_V1_NO_CLOUDS:      # it needs no texture: as far as the device, below
                        assert got[0] == N.ATMO_E_NO_DEVICE and got[1].startswith(who_new), got
                        continue
                    assert got[0] == N.ATMO_E_STATE, got
                    _same_but_for_the_name(got, old(lib, ctx, **args), who_new, who_old)
        finally:
            lib.atmo_destroy(ctx)
    # the direct-light variant without clouds needs no texture: a well-formed call gets as far as the device, switch on or off
    for detail in (False, True):
        ctx = _mode_ctx(N, lib, N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8, detail=detail)
        try:
            for new, old, who_new, who_old in PAIRS:
                rc, msg = new(lib, ctx)
                assert rc == N.ATMO_E_NO_DEVICE and msg == who_new + "a host-only context has no device to draw on", (rc, msg)
                assert old(lib, ctx)[0] not in (N.ATMO_OK, N.ATMO_E_ARG, N.ATMO_E_STATE)      # the sibling got as far, too
            assert lib.atmo_kernel_name(ctx) == b"atmo_render_kernel<4, 8, 1>"      # nothing was drawn
        finally:
            lib.atmo_destroy(ctx)


# ---- the twelve kernels in the compiled assembly --------------------------------------------------------------------------------------------------------
FAMILIES = (17, 19, 25, 49, 51, 57)
KF_TARGET, KF_VIEWS, KF_DEPTH, KF_DETAIL = 1024, 2048, 4096, 8192
DETAIL_WAVES = {17: 6, 19: 6, 25: 6, 49: 5, 51: 5, 57: 5}      # profiles/cloud_detail/README.md, section 4: atmo_render_detail_kernel's occupancy steps


def _mangled(kernel, flags):
    return f"_ZN4atmo{len(kernel)}{kernel}ILi{flags}ELi0EE"


def test_the_twelve_kernels_cost_what_their_detail_twins_cost():
    """Present under their mangled names and in tools/twin_resources.py's table (tests/test_kernel_twins_host.py holds its rules: no stack frame, the
    detail twin's vector loads inside loops -- no constant through a vector load --, the occupancy step of the lower twin); here: six of each, the
    written flag sums, each on the occupancy step of its atmo_render_detail_kernel twin, names of their own."""
    text = T._asm()
    numbers = T.twin_resources.kernels(text)
    waves = T.twin_resources.vgpr_waves
    by_prefix = lambda p: [k for name, k in numbers.items() if name.startswith(p)]   # noqa: E731

    def base(mangled):
        m = T.re.match(r"_ZN4atmo(\d+)", mangled)
        return mangled[m.end():m.end() + int(m.group(1))]

    new_names = {"atmo_detail_target_kernel": KF_DETAIL | KF_DEPTH | KF_TARGET, "atmo_detail_views_target_kernel": KF_DETAIL | KF_DEPTH | KF_VIEWS | KF_TARGET}
    assert [13312 + f for f in FAMILIES] == [13329, 13331, 13337, 13361, 13363, 13369] and KF_DETAIL | KF_DEPTH | KF_TARGET == 13312
    for kernel, bits in new_names.items():
        assert len([n for n in numbers if base(n) == kernel]) == 6, kernel
        for f in FAMILIES:
            (new,), (twin,) = by_prefix(_mangled(kernel, f | bits)), by_prefix(_mangled("atmo_render_detail_kernel", f | KF_DETAIL))
            print(f"{kernel}<{f | bits}, 0> {new}; atmo_render_detail_kernel<{f | KF_DETAIL}, 0> {twin}")
            assert new["scratch"] == 0, (kernel, f)
            assert waves(twin["vgprs"]) == DETAIL_WAVES[f] and waves(new["vgprs"]) >= DETAIL_WAVES[f], (kernel, f, new["vgprs"], twin["vgprs"])
            assert new["loop_vector"] == twin["loop_vector"], (kernel, f, new["loop_vector"], twin["loop_vector"])
    rows = [r for r in T._rows() if r.family.kernel in new_names]
    assert len(rows) == 12 and not any(r.bad for r in rows), [(r.name, r.bad) for r in rows if r.bad]
    names = {base(n) for n in numbers}
    assert set(new_names) <= names, names
    for a in new_names:
        for b in names - {a}:
            assert a not in b and b not in a, (a, b)


# ---- the binding, without a device ----------------------------------------------------------------------------------------------------------------------
def _detail_node(shader="planet_atmosphere_clouds_high", on=True, lib=None, mode=None):
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    node = B._node(mode=PA.MODE_NEAR if mode is None else mode, lib=lib)
    node._cloud_detail, node._shader = on, PA.SHADERS[shader]
    return node


def _calls(node):
    return [c for c in node._lib.calls if c[0] not in ("atmo_destroy", "atmo_bake_optical_depth")]


def _depth_struct(raw):
    N = B.N
    d = N.AtmoDepth.from_buffer_copy(raw)
    return d.texels, d.format, d.row_pitch_bytes


def _target_struct(raw):
    N = B.N
    t = N.AtmoTarget.from_buffer_copy(raw)
    return t.pixels, t.format, t.row_pitch_bytes


def test_a_cloud_node_with_cloud_detail_reaches_the_new_entry_points():
    """render / render_composite / draw whenever the colour is packed or pitched or the depth a depth_source; a plain depth tensor travels as D32 tight;
    float colour with float depth stays atmo_render."""
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    N = B.N
    cam = B._cam()
    depth = B._depth(cam)
    h, w = cam.height, cam.width
    for shader in ("planet_atmosphere_clouds_high", "planet_atmosphere_clouds_high_rm", "planet_atmosphere_v1_clouds"):
        node = _detail_node(shader)
        f16, u8 = B._fake((h, w, 4), torch.float16), B._fake((h, w, 4), torch.uint8)
        wide = B._fake((h, 2 * w, 4), torch.float16)[:, w:]                 # pitched
        f32 = B._fake((h, w, 4))
        d16 = PA.DepthSource(B._fake((h, w), torch.int16), N.DEPTH_D16_UNORM, 2 * w)
        node.render(cam, depth, f16, stream=B.STREAM, time=B.TIME)
        node.render_composite(cam, depth, u8, stream=B.STREAM, time=B.TIME, target="bgra8_srgb")
        node.draw(cam, depth, wide, stream=B.STREAM, time=B.TIME)
        node.render(cam, d16, f32, stream=B.STREAM, time=B.TIME)
        node.render(cam, depth, f32, stream=B.STREAM, time=B.TIME)          # float / float: atmo_render
        node.render_composite(cam, depth, f32, stream=B.STREAM, time=B.TIME)
        calls = _calls(node)
        assert [c[0] for c in calls] == ["atmo_render_detail_target"] * 4 + ["atmo_render", "atmo_render_composite"], [c[0] for c in calls]
        want = [((depth.data_ptr(), N.DEPTH_D32_SFLOAT, 0), (f16.data_ptr(), N.TARGET_RGBA16F, w * 8), 0),
                ((depth.data_ptr(), N.DEPTH_D32_SFLOAT, 0), (u8.data_ptr(), N.TARGET_BGRA8_SRGB, w * 4), 1),
                ((depth.data_ptr(), N.DEPTH_D32_SFLOAT, 0), (wide.data_ptr(), N.TARGET_RGBA16F, 2 * w * 8), 1),
                ((d16.tensor.data_ptr(), N.DEPTH_D16_UNORM, 2 * w), (f32.data_ptr(), N.TARGET_RGBA32F, 0), 0)]
        for (_, args), (dep, tgt, comp) in zip(calls[:4], want):
            assert len(args) == 6 and args[0] == B.CTX and args[5] == B.STREAM
            got_t = _target_struct(args[3])
            assert _depth_struct(args[2]) == dep and got_t[:2] == tgt[:2] and got_t[2] in (tgt[2], 0) and args[4] == comp, (args, dep, tgt)
            assert C.c_float.from_buffer_copy(args[1], N.AtmoFrame.time.offset).value == C.c_float(B.TIME).value != 0.0


def test_target_batches_of_such_a_node_reach_the_new_batch_entry_point():
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    N = B.N
    cams = [B._cam(), B._cam()]
    h, w = cams[0].height, cams[0].width
    depths = [B._depth(c) for c in cams]
    node = _detail_node("planet_atmosphere_clouds_high_rm")
    image = B._fake((h, 2 * w, 4), torch.uint8)
    outs = [image[:, :w], image[:, w:]]
    node.render_views(cams, depths, outs, stream=B.STREAM, time=B.TIME, target="rgba8_srgb")
    node.draw_views(cams, depths, outs, stream=B.STREAM, time=B.TIME, target="rgba8_srgb")
    srcs = [PA.DepthSource(B._fake((h, w), torch.int16), N.DEPTH_D16_UNORM, 2 * w) for _ in cams]
    node.render_views(cams, srcs, [B._fake((h, w, 4)) for _ in cams], stream=B.STREAM, time=B.TIME)
    calls = _calls(node)
    assert [c[0] for c in calls] == ["atmo_render_views_detail_target"] * 3, [c[0] for c in calls]
    for (_, args), comp, deps in zip(calls, (0, 1, 0), (depths, depths, None)):
        views, n = args[1], args[2]
        assert args[0] == B.CTX and n == 2 and args[3] == comp and args[4] == B.STREAM
        arr = (N.AtmoViewDepthTarget * 2).from_buffer_copy(views)
        for i in range(2):
            if deps is not None:
                assert (arr[i].depth.texels, arr[i].depth.format, arr[i].depth.row_pitch_bytes) == (deps[i].data_ptr(), N.DEPTH_D32_SFLOAT, 0)
                assert (arr[i].target.pixels, arr[i].target.format, arr[i].target.row_pitch_bytes) == (outs[i].data_ptr(), N.TARGET_RGBA8_SRGB, 2 * w * 4)
            else:
                assert (arr[i].depth.texels, arr[i].depth.format) == (srcs[i].tensor.data_ptr(), N.DEPTH_D16_UNORM) and arr[i].target.format == N.TARGET_RGBA32F
            assert arr[i].frame.time == C.c_float(B.TIME).value
    # the float-only batch and the proxy methods go where they went: the library refuses them on a device
    node = _detail_node("planet_atmosphere_clouds_high")
    node.render_views(cams, depths, [B._fake((h, w, 4)) for _ in cams], stream=B.STREAM)
    node.render_proxy(cams[0], depths[0], B._fake((h, w, 4), torch.float16), stream=B.STREAM)
    node.render_views_proxy(cams, depths, outs, stream=B.STREAM, target="rgba8_srgb")
    assert [c[0] for c in _calls(node)] == ["atmo_render_views", "atmo_render_proxy_target", "atmo_render_views_proxy_target"]


def test_with_it_off_or_without_clouds_the_old_entry_points_serve():
    cam = B._cam()
    depth = B._depth(cam)
    h, w = cam.height, cam.width
    for node in (_detail_node(on=False), _detail_node("planet_atmosphere_no_clouds"), _detail_node("planet_atmosphere_v1_no_clouds")):
        node.render(cam, depth, B._fake((h, w, 4), torch.float16), stream=B.STREAM)
        node.render_views([cam], [depth], [B._fake((h, w, 4), torch.float16)], stream=B.STREAM)
        assert [c[0] for c in _calls(node)] == ["atmo_render_target", "atmo_render_views_target"]


def test_a_library_without_the_symbols_says_so():
    cam = B._cam()
    depth = B._depth(cam)
    h, w = cam.height, cam.width
    node = _detail_node(lib=B.library_without(*NAMES))
    with pytest.raises(RuntimeError, match=r"atmo_render_detail_target \(include/atmo_detail_target.h\)"):
        node.render(cam, depth, B._fake((h, w, 4), torch.float16), stream=B.STREAM)
    with pytest.raises(RuntimeError, match=r"atmo_render_views_detail_target \(include/atmo_detail_target.h\)"):
        node.render_views([cam], [depth], [B._fake((h, w, 4), torch.float16)], stream=B.STREAM)
    assert _calls(node) == []
    node.render(cam, depth, B._fake((h, w, 4)), stream=B.STREAM)          # float / float needs no new symbol
    assert [c[0] for c in _calls(node)] == ["atmo_render"]
    for node in (_detail_node(on=False, lib=B.library_without(*NAMES)), _detail_node("planet_atmosphere_no_clouds", lib=B.library_without(*NAMES))):
        node.render(cam, depth, B._fake((h, w, 4), torch.float16), stream=B.STREAM)
        assert [c[0] for c in _calls(node)] == ["atmo_render_target"]
