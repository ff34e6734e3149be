"""CPU tests of atmo_render_planets / atmo_plan_planets (include/atmo_planets.h) on host-only contexts, where nothing touches a device: the header's
symbol set and the binding, every refusal the header states -- its code, its message and the context that holds it --, and the plan against a Python
restatement written from the header's text (levels, family keys, chunks, the pair test of atmo_views_target.h), on hand cases and 200 seeded random scenes.
(tests/test_planets_gpu.py holds the pixels to the sequential single draws bit for bit; tools/planets_plan_check.cpp runs the planner alone under the host
sanitizers.)"""
import ctypes as C
import os

import numpy as np
import pytest

import proxy_geometry as G
from godot_atmosphere_shader_amd import scene as S
from test_views_proxy_host import DEPTH, ROOT, _frame, _functions, _host_ctx, _mat

F32, F16, U8, SRGB8, A2B10 = 0, 1, 2, 16, 19          # AtmoTargetFormat
PX = {F32: 16, F16: 8, U8: 4, SRGB8: 4, A2B10: 4}
MAX_VIEWS = 8
W, H = 384, 216
CAM = S.Camera(W, H, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0))            # looks down -z: 1 pixel is about 4.3 units in the plane z = 0
AWAY = S.Camera(W, H, (0.0, 0.0, 400.0), (0.0, 0.0, 800.0))         # looks +z: everything near the origin is behind it
IMG = 0x10000000
# KernelFlags (csrc/atmo_device.h) a default host-only context resolves for a proxy draw (no mip chain: never KF_CUBE_LOD)
CLOUDS, RM, DIRECT, LITE, PRECISE = 1, 2, 4, 8, 16
KINDS = {
    "no_clouds": ("VARIANT_NO_CLOUDS", None, 0, 0),
    "direct8": ("VARIANT_NO_CLOUDS", "direct", 8, DIRECT),
    "direct5": ("VARIANT_NO_CLOUDS", "direct", 5, DIRECT),
    "clouds_high": ("VARIANT_CLOUDS_HIGH", None, 0, PRECISE | CLOUDS),
    "clouds": ("VARIANT_CLOUDS", None, 0, PRECISE | CLOUDS),
    "clouds_high_rm": ("VARIANT_CLOUDS_HIGH_RM", None, 0, PRECISE | CLOUDS | RM),
    "v1_no_clouds": ("VARIANT_V1_NO_CLOUDS", None, 0, PRECISE | LITE),
}


class _Contexts:
    """Host-only contexts by (kind, instance); destroyed together."""

    def __init__(self):
        from godot_atmosphere_shader_amd import _native as N

        self.N, self.lib, self.made = N, N.load(), {}

    def get(self, kind, instance=0):
        N = self.N
        if (kind, instance) not in self.made:
            variant, light, steps, _ = KINDS[kind]
            self.made[kind, instance] = _host_ctx(getattr(N, variant), light_mode=N.LIGHT_DIRECT if light else None, light_steps=steps)
        return self.made[kind, instance]

    def close(self):
        for ctx in self.made.values():
            self.lib.atmo_destroy(ctx)


@pytest.fixture()
def ctxs():
    c = _Contexts()
    yield c
    c.close()


def _draws(specs):
    """specs: [dict(ctx, cam, rect, model, size, depth, pixels, fmt, pitch)] -> N.AtmoPlanetDraw array."""
    from godot_atmosphere_shader_amd import _native as N

    arr = (N.AtmoPlanetDraw * max(len(specs), 1))()
    for i, s in enumerate(specs):
        arr[i].ctx = s["ctx"]
        arr[i].frame = _frame(s.get("cam", CAM), s.get("rect"))
        arr[i].model_matrix[:] = list(_mat(s.get("model", np.eye(4))))
        arr[i].box_size = s.get("size", 60.0)
        arr[i].depth_dev = s.get("depth", DEPTH)
        arr[i].target = N.AtmoTarget(s.get("pixels", IMG), s.get("fmt", F16), s.get("pitch", 0))
    return arr


def _plan(lib, draws, n):
    from godot_atmosphere_shader_amd import _native as N

    launch_of, n_launches = (C.c_int * max(n, 1))(*([-7] * max(n, 1))), C.c_int(-7)
    rc = lib.atmo_plan_planets(draws, n, launch_of, C.byref(n_launches))
    assert rc == N.ATMO_OK, (rc, lib.atmo_last_error_string(draws[0].ctx))
    return list(launch_of)[:n], n_launches.value


# ---- the plan, restated from the text of include/atmo_planets.h -----------------------------------------------------------------------------------------
def _footprint(lib, d):
    """(base, rows, row_bytes, pitch) of the draw's launch rectangle in its target, or None when it has no tile."""
    from godot_atmosphere_shader_amd import _native as N

    f = d.frame
    if f.x0 == f.x1 or f.y0 == f.y1:
        return None
    rect, tiles = (C.c_int * 4)(), C.c_int(-1)
    model = (C.c_float * 16)(*d.model_matrix)
    assert lib.atmo_debug_proxy_launch_rect(d.ctx, C.byref(f), model, C.c_float(d.box_size), rect, C.byref(tiles)) == N.ATMO_OK
    if tiles.value == 0:
        return None
    cx0, cy0, cx1, cy1 = rect
    px = PX[d.target.format]
    pitch = d.target.row_pitch_bytes or f.viewport_w * px
    return (d.target.pixels + cy0 * pitch + cx0 * px, cy1 - cy0, (cx1 - cx0) * px, pitch)


def _proved_disjoint(x, y):
    """Rules (a) and (b) of include/atmo_views_target.h."""
    a, b = (x, y) if x[0] <= y[0] else (y, x)
    (base_a, rows_a, row_a, pitch_a), (base_b, _, row_b, pitch_b) = a, b
    if base_a + (rows_a - 1) * pitch_a + row_a <= base_b:
        return True
    if pitch_a == pitch_b:
        q, r = divmod(base_b - base_a, pitch_a)
        return q >= rows_a or (r >= row_a and r + row_b <= pitch_a)
    return False


def _restated_plan(lib, draws, n, kinds):
    fps = [_footprint(lib, draws[i]) for i in range(n)]
    keys = []
    for i in range(n):
        _, light, steps, flags = KINDS[kinds[i]]
        fmt = draws[i].target.format
        keys.append((flags, bool(flags & DIRECT) and steps == 8, "float" if fmt == F32 else fmt))
    level = [None] * n
    touching = 0
    for j in range(n):
        if fps[j] is None:
            continue
        before = [level[i] for i in range(j) if fps[i] is not None and not _proved_disjoint(fps[i], fps[j])]
        touching += len(before)
        level[j] = 1 + max(before) if before else 0
    launch_of, launches = [-1] * n, 0
    for lv in sorted({v for v in level if v is not None}):
        members = [i for i in range(n) if level[i] == lv]
        order = []
        for i in members:
            if keys[i] not in order:
                order.append(keys[i])
        for key in order:
            same = [i for i in members if keys[i] == key]
            for c in range(0, len(same), MAX_VIEWS):
                for i in same[c:c + MAX_VIEWS]:
                    launch_of[i] = launches
                launches += 1
    return launch_of, launches, touching


def test_binding_exposes_the_planets_header():
    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.build import build_native

    build_native()
    lib = N.load()
    assert _functions("atmo_planets.h") == set(N.PLANETS_SYMBOLS) == {"atmo_render_planets", "atmo_plan_planets"}
    for sym in N.PLANETS_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "atmo_planets.h")).read()
    assert '#include "atmo_views_proxy.h"' in header and "#define ATMO_MAX_PLANET_DRAWS 64" in header and N.MAX_PLANET_DRAWS == 64
    # the older headers keep their function sets (atmo_debug.h: tests/test_host_logic.py), EXPORTED_SYMBOLS is the older tuples' union, and the feature is detected by symbol, not by the version
    assert N.EXPORTED_SYMBOLS == (N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_PROXY_SYMBOLS +
                                  N.VIEWS_TARGET_SYMBOLS)
    for name, want in (("atmo.h", N.CORE_SYMBOLS), ("atmo_scene.h", N.SCENE_SYMBOLS), ("atmo_target.h", N.TARGET_SYMBOLS),
                       ("atmo_views.h", N.VIEWS_SYMBOLS), ("atmo_views_target.h", N.VIEWS_TARGET_SYMBOLS), ("atmo_views_proxy.h", N.VIEWS_PROXY_SYMBOLS)):
        assert _functions(name) == set(want), name
    assert len(N.CORE_SYMBOLS) == 22 and lib.atmo_abi_version() == N.ABI_VERSION == 5
    assert "#define ATMO_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "atmo.h")).read()
    # the struct is the header's: ctx, frame, 16 + 1 floats, depth, target
    assert C.sizeof(N.AtmoPlanetDraw) == 8 + ((C.sizeof(N.AtmoFrame) + 17 * 4 + 7) // 8) * 8 + 8 + 16


def test_every_refusal_its_code_its_message_and_its_context(ctxs):
    """Both entry points, the same checks: the code, the message, and the context that holds it -- the context of the draw the message names; draws[0]'s for
    a message that names no draw; the slot atmo_last_error_string(NULL) reads where there is no such context."""
    N, lib = ctxs.N, ctxs.lib
    a, b = ctxs.get("direct8"), ctxs.get("clouds_high_rm")
    err = lambda ctx: lib.atmo_last_error_string(ctx) or b""                                                    # noqa: E731
    left, right = G.translation(-300.0, 0.0, 0.0), G.translation(300.0, 0.0, 0.0)
    good = lambda: [dict(ctx=a, model=left), dict(ctx=b, model=right, pixels=IMG + 0x1000000, fmt=U8, pitch=(W + 3) * 4)]      # noqa: E731
    for fn_name in ("atmo_plan_planets", "atmo_render_planets"):
        fn = getattr(lib, fn_name)
        call = (lambda d, k: fn(d, k, None, None)) if fn_name == "atmo_plan_planets" else (lambda d, k: fn(d, k, None))
        who = fn_name.encode()

        def refused(specs, code, where, *words, n=None):
            d = _draws(specs)
            for ctx in (a, b):      # (another message in every slot first, so that an old one cannot pass)
                assert lib.atmo_get_param_f32(ctx, b"no such parameter", None, 0) != N.ATMO_OK
            assert lib.atmo_debug_create_host_only(99, 0, 0, 0, 0, C.byref(C.c_void_p())) != N.ATMO_OK
            rc = call(d, len(specs) if n is None else n)
            msg = err(where)
            assert rc == code and msg.startswith(who) and all(w in msg for w in words), (fn_name, rc, msg, words)

        # the count, null draws, a null context
        assert call(_draws(good()), 0) == N.ATMO_OK and call(None, 0) == N.ATMO_OK
        refused(good(), N.ATMO_E_ARG, a, b"n_draws must be 0 .. 64", n=65)
        refused(good(), N.ATMO_E_ARG, None, b"n_draws must be 0 .. 64", n=-1)
        assert call(None, 2) == N.ATMO_E_ARG and b"null draws" in err(None)
        refused([dict(ctx=a, model=left), dict(ctx=None, model=right)], N.ATMO_E_ARG, None, b"draw 1", b"null ctx")
        refused([dict(ctx=None), dict(ctx=a)], N.ATMO_E_ARG, None, b"draw 0", b"null ctx")
        # every per-draw check of atmo_render_proxy_target, in either draw, the message on THAT draw's context and naming it
        for i, ctx in ((0, a), (1, b)):
            def bad(**kw):
                specs = good()
                specs[i].update(kw)
                return specs

            name = b"draw %d" % i
            for size in (0.0, -1.0, float("inf"), float("nan")):
                refused(bad(size=size), N.ATMO_E_ARG, ctx, name, b"box_size must be positive and finite")
            for rect in ((0, 0, W + 1, H), (-1, 0, W, H), (10, 0, 5, H), (0, 30, W, 20)):
                refused(bad(rect=rect), N.ATMO_E_ARG, ctx, name, b"rect outside the viewport")
            refused(bad(depth=None), N.ATMO_E_ARG, ctx, name, b"null device pointer")
            refused(bad(pixels=None), N.ATMO_E_ARG, ctx, name, b"null target pixels")
            refused(bad(fmt=3), N.ATMO_E_ARG, ctx, name, b"unknown target format 3")
            refused(bad(fmt=F16, pixels=IMG + 4, pitch=0), N.ATMO_E_ARG, ctx, name, b"aligned to the pixel size (8 bytes)")
            refused(bad(fmt=F32, pixels=IMG + 8, pitch=0), N.ATMO_E_ARG, ctx, name, b"aligned to the pixel size (16 bytes)")
            refused(bad(fmt=U8, pitch=(W - 1) * 4), N.ATMO_E_ARG, ctx, name, b"row_pitch_bytes")      # composite addressing: the VIEWPORT's row
            refused(bad(fmt=U8, pitch=W * 4 + 2), N.ATMO_E_ARG, ctx, name, b"row_pitch_bytes")
            refused(bad(fmt=U8, rect=(0, 0, 8, 8), pitch=8 * 4), N.ATMO_E_ARG, ctx, name, b"row_pitch_bytes")
            refused(bad(model=np.zeros((4, 4))), N.ATMO_E_ARG, ctx, name, b"model_matrix is singular")
            d = _draws(good())
            d[i].frame.viewport_w = 70000
            assert call(d, 2) == N.ATMO_E_ARG and name in err(ctx) and b"bad viewport size" in err(ctx)
            d = _draws(good())
            d[i].frame.inv_projection_matrix[:] = [0.0] * 16
            assert call(d, 2) == N.ATMO_E_ARG and name in err(ctx) and b"inv_projection_matrix is singular" in err(ctx)
            # ... also for a draw whose box leaves no tile
            refused(bad(cam=AWAY, depth=None), N.ATMO_E_ARG, ctx, name, b"null device pointer")
        # a draw with an empty rect has no tile, but (as the single proxy draw's) all its checks
        refused([dict(ctx=a, model=left, rect=(5, 5, 5, 30), depth=None)], N.ATMO_E_ARG, a, b"draw 0", b"null device pointer")
        # nothing to draw: ATMO_OK without a device -- behind the camera, off the rect, an empty rect
        nothing = [dict(ctx=a, cam=AWAY), dict(ctx=b, model=right, rect=(0, 0, 40, 40), pixels=IMG + 0x1000000), dict(ctx=a, rect=(7, 7, 7, 90))]
        if fn_name == "atmo_plan_planets":
            assert _plan(lib, _draws(nothing), 3) == ([-1, -1, -1], 0)
            assert _plan(lib, _draws(good()), 2) == ([0, 1], 2)      # two families
        else:   # the render call checks the textures of every draw's context, as the single draw does whether it has a tile or not: none is set here
            assert call(_draws([nothing[0], nothing[2]]), 2) == N.ATMO_OK           # (the direct-light atmosphere needs no texture)
            assert call(_draws(nothing), 3) == N.ATMO_E_STATE and b"draw 1" in err(b) and b"u_optical_depth_texture not set" in err(b)
            assert call(_draws(good()[:1]), 1) not in (N.ATMO_OK, N.ATMO_E_ARG, N.ATMO_E_STATE)   # well-formed: it is the missing device that stops it


@pytest.mark.parametrize("mode", ["precision0", "precision2", "view_steps64", "lane_split2"])
def test_planets_need_the_default_forms(mode, ctxs):
    """A context outside the default forms anywhere in the list: ATMO_E_STATE with the single draw's message, on that draw's context; argument errors of
    ANY draw that need no matrix arithmetic come first, a singular matrix may come behind."""
    N, lib = ctxs.N, ctxs.lib
    ok = ctxs.get("direct8")
    odd = _host_ctx(N.VARIANT_CLOUDS_HIGH if mode == "precision0" else N.VARIANT_NO_CLOUDS, view_steps=64 if mode == "view_steps64" else 0,
                    light_mode=N.LIGHT_DIRECT, light_steps=8)
    try:
        if mode.startswith("precision"):
            assert lib.atmo_set_precision(odd, int(mode[-1])) == N.ATMO_OK
        elif mode == "lane_split2":
            assert lib.atmo_set_lane_split(odd, 2) == N.ATMO_OK
        left, right = G.translation(-300.0, 0.0, 0.0), G.translation(300.0, 0.0, 0.0)
        for fmt in (F32, F16, SRGB8):
            specs = [dict(ctx=ok, model=left, fmt=fmt), dict(ctx=odd, model=right, fmt=fmt), dict(ctx=ok, cam=AWAY, fmt=fmt)]
            for call in (lambda d, k: lib.atmo_plan_planets(d, k, None, None), lambda d, k: lib.atmo_render_planets(d, k, None)):
                assert call(_draws(specs), 3) == N.ATMO_E_STATE
                msg = lib.atmo_last_error_string(odd)
                assert b"draw 1" in msg and b"no proxy kernel for this context's mode" in msg and b"atmo_set_precision 1" in msg
                if mode != "precision0":    # the single draw's message, but for the name in front (a cloud context without textures: those come first there)
                    single, f = N.AtmoTarget(IMG, fmt, 0), _frame(CAM)
                    assert lib.atmo_render_proxy_target(odd, C.byref(f), _mat(right), C.c_float(60.0), DEPTH, C.byref(single), 1, None) == N.ATMO_E_STATE
                    assert lib.atmo_last_error_string(odd).split(b": ", 1)[1] == msg.split(b"draw 1: ", 1)[1]
                specs2 = [dict(s) for s in specs]
                specs2[2]["depth"] = None
                assert call(_draws(specs2), 3) == N.ATMO_E_ARG and b"draw 2" in lib.atmo_last_error_string(ok)
                assert call(_draws(specs[:1]), 0) == N.ATMO_OK
    finally:
        lib.atmo_destroy(odd)


def test_hand_cases_of_the_plan(ctxs):
    lib = ctxs.lib
    a, a2, b = ctxs.get("clouds_high"), ctxs.get("clouds_high", 1), ctxs.get("direct8")
    at = lambda x, y, z=0.0: G.translation(float(x), float(y), float(z))                                   # noqa: E731

    def plan(specs, kinds):
        d = _draws(specs)
        got = _plan(lib, d, len(specs))
        want = _restated_plan(lib, d, len(specs), kinds)
        assert got == want[:2], (got, want)
        return got

    # nine disjoint boxes of one family (two contexts of it): 8 + 1
    grid = [dict(ctx=(a, a2)[k % 2], model=at(250 * (k % 3 - 1), 250 * (k // 3 - 1))) for k in range(9)]
    assert plan(grid, ["clouds_high"] * 9) == ([0] * 8 + [1], 2)
    # a chain: A under B under C
    chain = [dict(ctx=a, model=at(-80, 0), size=120.0), dict(ctx=a2, model=at(0, 0, 50), size=120.0), dict(ctx=a, model=at(80, 0, 100), size=120.0)]
    assert plan(chain, ["clouds_high"] * 3) == ([0, 1, 2], 3)
    # two families, disjoint: two launches in level 0, the keys in order of appearance
    two = [dict(ctx=b, model=at(-300, 0)), dict(ctx=a, model=at(0, 0)), dict(ctx=b, model=at(300, 0))]
    assert plan(two, ["direct8", "clouds_high", "direct8"]) == ([0, 1, 0], 2)
    # ... and the format of a packed target is part of the key, the float kernel another one
    fmts = [dict(ctx=a, model=at(-300, 0), fmt=F16), dict(ctx=a, model=at(0, 0), fmt=U8), dict(ctx=a, model=at(300, 0), fmt=F16),
            dict(ctx=a, model=at(0, 300), fmt=F32), dict(ctx=a, model=at(0, -300), fmt=SRGB8)]
    for k, s in enumerate(fmts):
        s["pixels"] = IMG + 0x1000000 * s["fmt"]
    assert plan(fmts, ["clouds_high"] * 5) == ([0, 1, 0, 2, 3], 4)
    # the 8-step twin of a direct-light family is a key of its own; clouds and clouds_high (32 and 64 cloud steps) are one family
    twins = [dict(ctx=b, model=at(-300, 0)), dict(ctx=ctxs.get("direct5"), model=at(0, 0)), dict(ctx=ctxs.get("clouds"), model=at(300, 0)),
             dict(ctx=a, model=at(0, 300))]
    assert plan(twins, ["direct8", "direct5", "clouds", "clouds_high"]) == ([0, 1, 2, 2], 3)
    # a box behind the camera: -1, and it touches nothing
    behind = [dict(ctx=a, model=at(0, 0)), dict(ctx=a, cam=AWAY, model=at(0, 0)), dict(ctx=a, model=at(10, 0, 60))]
    assert plan(behind, ["clouds_high"] * 3) == ([0, -1, 1], 2)
    # the halves of one double-wide image never touch, whatever is drawn in them: the same box for both eyes, then a moon in front for both
    half = lambda eye, **kw: dict(pixels=IMG + eye * W * 8, pitch=2 * W * 8, fmt=F16, **kw)                # noqa: E731
    stereo = [half(0, ctx=a, model=at(0, 0)), half(1, ctx=a, model=at(0, 0)), half(0, ctx=a2, model=at(30, 0, 80)), half(1, ctx=a2, model=at(30, 0, 80))]
    assert plan(stereo, ["clouds_high"] * 4) == ([0, 0, 1, 1], 2)
    #  ... but two windows of that image ten pixels apart do: the box's rectangles overlap
    wide = [half(0, ctx=a, model=at(0, 0)), dict(pixels=IMG + 10 * 8, pitch=2 * W * 8, fmt=F16, ctx=a, model=at(0, 0))]
    assert plan(wide, ["clouds_high"] * 2) == ([0, 1], 2)
    # the same context twice: apart -- one launch; the same box into the same pixels -- two
    assert plan([dict(ctx=a, model=at(-300, 0)), dict(ctx=a, model=at(300, 0))], ["clouds_high"] * 2) == ([0, 0], 1)
    assert plan([dict(ctx=a, model=at(0, 0)), dict(ctx=a, model=at(0, 0))], ["clouds_high"] * 2) == ([0, 1], 2)
    # two rects of one viewport cut one box in two: the footprints are the CUT rectangles', which do not touch
    cut = [dict(ctx=a, model=at(0, 0), size=200.0, rect=(0, 0, W // 2, H)), dict(ctx=a, model=at(0, 0), size=200.0, rect=(W // 2, 0, W, H))]
    assert plan(cut, ["clouds_high"] * 2) == ([0, 0], 1)
    # 64 draws: all one box -- 64 launches; 65 are refused
    from godot_atmosphere_shader_amd import _native as N
    assert plan([dict(ctx=a, model=at(0, 0))] * 64, ["clouds_high"] * 64) == (list(range(64)), 64)
    assert lib.atmo_plan_planets(_draws([dict(ctx=a)] * 65), 65, None, None) == N.ATMO_E_ARG


SEEDS = range(200)


def _random_scene(seed, ctxs):
    """1 .. 24 boxes at random positions; three variants mixed in (two contexts of one of them); one of two target layouts: every draw into ONE tight RGBA16F
    image, or the two halves of a double-wide RGBA8 image beside a float image of its own pitch."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 25))
    layout = seed % 2
    spread = (900.0, 500.0) if n > 6 else (500.0, 280.0)     # (few boxes stay near the middle, so that small scenes have touching pairs too)
    pool = [("clouds_high", 0), ("clouds_high", 1), ("direct8", 0), ("v1_no_clouds", 0)]
    specs, kinds = [], []
    for _ in range(n):
        kind, instance = pool[int(rng.integers(0, len(pool)))]
        s = dict(ctx=ctxs.get(kind, instance), size=float(rng.uniform(20.0, 110.0)),
                 model=G.translation(rng.uniform(-spread[0], spread[0]), rng.uniform(-spread[1], spread[1]), rng.uniform(-400.0, 300.0)) @
                 G.rotation_y(rng.uniform(0.0, 90.0)))
        if rng.integers(0, 8) == 0:
            s["cam"] = AWAY
        if layout == 0:
            s.update(pixels=IMG, fmt=F16, pitch=0)
        else:
            where = int(rng.integers(0, 3))
            if where == 2:
                s.update(pixels=IMG + 0x4000000, fmt=F32, pitch=(W + 5) * 16)
            else:
                s.update(pixels=IMG + where * W * 4, fmt=U8, pitch=2 * W * 4)
        specs.append(s)
        kinds.append(kind)
    return specs, kinds


def test_plan_equals_its_restatement_on_random_scenes(ctxs):
    lib = ctxs.lib
    with_touch = without_touch = launches = drawn = 0
    for seed in SEEDS:
        specs, kinds = _random_scene(seed, ctxs)
        d = _draws(specs)
        got = _plan(lib, d, len(specs))
        want_launch_of, want_launches, touching = _restated_plan(lib, d, len(specs), kinds)
        assert got == (want_launch_of, want_launches), (seed, got, want_launch_of, want_launches)
        with_touch += touching > 0
        without_touch += touching == 0
        launches += got[1]
        drawn += sum(1 for v in got[0] if v >= 0)
    print(f"{len(SEEDS)} scenes: {with_touch} with a touching pair, {without_touch} without; {drawn} draws with a tile in {launches} launches")
    # the scenes exercise both sides of the rule
    assert with_touch * 4 >= len(SEEDS) and without_touch * 4 >= len(SEEDS)
