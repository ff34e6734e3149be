"""GPU tests of atmo_render_planets (include/atmo_planets.h): a frame's far planets -- several contexts -- in as few launches as blending allows, against
the sequential atmo_render_proxy_target / atmo_render_proxy_composite draws in list order.  Every picture comparison is BIT-EXACT on whole
sentinel-guarded buffers (no tolerance); one test goes to the CPU oracle at common.TOL, so that the file is not only self-comparison.

The scene: one 480 x 270 viewport, the camera at (0, 0, 700) looking at the origin, and three planets.  P (the demo planet, radius 100 + 8) and Q (83 + 12)
are apart on screen; M (45 + 5) stands in front of P, 450 from the camera.  Their launch rectangles are P (163, 95, 232, 161), Q (267, 119, 324, 168) and
M (183, 99, 232, 145): each at least 3 x 3 tiles of 16 x 8, a width and a height that are no multiple of the tile (partial tiles at the right and the
bottom) and an origin that is odd in x and y (under the declared sampler the grid starts one pixel in front of it: helper lanes at the left and the top).
tests/proxy_geometry.py's float64 statement gives 2998 / 2356 / 1880 passing fragments and no unstable pixel; `_geometry` asserts all of that."""
import ctypes as C

import numpy as np
import pytest
import torch

import proxy_geometry as G
from common import CONFIGS, TOL, demo_params, demo_textures, kernel_flags, make_node, oracle_inputs
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import planet_atmosphere as PA
from godot_atmosphere_shader_amd import scene as S
from test_views_gpu import FAMILY_CASES, _bits, _guarded, _guards_intact, _scene
from test_views_proxy_gpu import IDS, KF_VIEWS
from test_views_target_gpu import PAD, Buf, _random_dst

pytestmark = pytest.mark.gpu

W, H = 480, 270
TILE_W, TILE_H = 16, 8
PLANETS = {"P": ((-150.0, 24.0, 0.0), 100.0, 8.0), "Q": ((237.0, -35.0, -100.0), 83.0, 12.0), "M": ((-77.0, 30.0, 250.0), 45.0, 5.0)}
RECTS = {"P": (163, 95, 232, 161), "Q": (267, 119, 324, 168), "M": (183, 99, 232, 145)}


def _cam(dx=0.0):
    return S.Camera(W, H, (dx, 0.0, 700.0), (dx, 0.0, 0.0), far=5000.0)


def _depth_np(cam):
    """The three planets' ground spheres (reverse-Z: the nearest wins)."""
    return np.maximum.reduce([S.depth_ground_sphere(cam, pos, r) for pos, r, _ in PLANETS.values()])


def _place(node, name, cam):
    pos, radius, height = PLANETS[name]
    node.planet_radius, node.atmosphere_height = radius, height
    node.global_transform = G.translation(*pos)
    node._process(camera=cam, time=0.0)
    return node


def _nodes(configs, cam, tex, **kw):
    """{"P": .., "Q": .., "M": ..}: configs is one name for all three, or a dict per planet of (config, make_node keywords)."""
    out = {}
    for name in PLANETS:
        config, extra = configs[name] if isinstance(configs, dict) else (configs, kw)
        out[name] = _place(make_node(config, tex, **extra), name, cam)
    return out


def _geometry(nodes, cam, depth_np, label, names=("P", "Q", "M"), rects=RECTS):
    """Asserts the scene's premises for `nodes` as they stand (their real contexts) and prints the counts."""
    lib = N.load()
    for name in names:
        node = nodes[name]
        size = node.proxy_box_size(cam)
        f = node.prepare_frame(cam)
        rect, tiles = (C.c_int * 4)(), C.c_int(-1)
        assert lib.atmo_debug_proxy_launch_rect(node._ctx, C.byref(f), node.proxy_model(), C.c_float(size), rect, C.byref(tiles)) == N.ATMO_OK
        x0, y0, x1, y1 = rect
        if rects is not None:
            assert tuple(rect) == rects[name], (label, name, tuple(rect))
        assert x1 - x0 > 2 * TILE_W and y1 - y0 > 2 * TILE_H and (x1 - x0) % TILE_W and (y1 - y0) % TILE_H, (label, name, tuple(rect))
        if rects is not None:
            assert x0 % 2 == 1 and y0 % 2 == 1, (label, name, tuple(rect))
        covered, passing, unstable = G.frame_masks(cam, node.global_transform, size, depth_np)
        print(f"{label} {name}: launch rectangle {tuple(rect)}, {tiles.value} tiles, {int(passing.sum())} passing fragments, {int(unstable.sum())} unstable")
        assert passing.sum() >= 300 and unstable.sum() == 0, (label, name, int(passing.sum()), int(unstable.sum()))


def _changed(after, before):
    return (np.asarray(after).reshape(before.shape) != before).any(axis=-1)


def _sequential(draws):
    for node, cam, depth, scene, rect, size, target in draws:
        node.render_proxy_composite(cam, depth, scene, rect=rect, box_size=size, **({} if target is None else {"target": target}))


def _views_proxy_name_of(single_name, node):
    """`node` last drew through the views-proxy kernel of the family its single proxy draw (`single_name`) uses."""
    packed = "_target" if "_target_" in single_name else ""
    assert single_name.startswith(f"atmo_render_proxy{packed}_kernel<"), single_name
    assert node.kernel_name.startswith(f"atmo_render_views_proxy{packed}_kernel<"), (node.kernel_name, single_name)
    assert kernel_flags(node) == int(single_name.split("<")[1].split(",")[0]) + KF_VIEWS, (node.kernel_name, single_name)
    assert node.kernel_name.split(",")[1].strip(" >") == single_name.split(",")[1].strip(" >"), (node.kernel_name, single_name)


# ---- 1. every kernel family -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config,kw,sampler", FAMILY_CASES, ids=IDS)
def test_planets_equal_the_sequential_composites(config, kw, sampler):
    tex = demo_textures(cube_n=64, shape_n=32)
    cam = _cam()
    depth_np = _depth_np(cam)
    depth = torch.from_numpy(depth_np).cuda()
    nodes = _nodes(config, cam, tex, sampler=sampler, **kw)
    _geometry(nodes, cam, depth_np, f"{config} {sampler}")
    fill = _scene(cam, 41)
    pictures, singles = {}, {}
    for order in ("PQM", "MQP"):
        want, want_whole = _guarded(H, W, fill=fill)
        _sequential([(nodes[k], cam, depth, want, None, None, None) for k in order])
        torch.cuda.synchronize()
        singles = {k: nodes[k].kernel_name for k in order}
        got, got_whole = _guarded(H, W, fill=fill)
        draws = [(nodes[k], cam, depth, got, None, None, None) for k in order]
        launch_of, n_launches = PA.plan_planets(draws)
        assert (launch_of, n_launches) == ([0, 0, 1], 2), (order, launch_of)       # P and Q beside each other; M over P, or P over M
        PA.render_planets(draws)
        torch.cuda.synchronize()
        assert _guards_intact(got_whole, H * W) and _guards_intact(want_whole, H * W)
        assert np.array_equal(_bits(got_whole), _bits(want_whole)), (config, sampler, order)
        for k in order:
            _views_proxy_name_of(singles[k], nodes[k])
        pictures[order] = _bits(got).copy()
    # the order is visible: P and M share pixels that both composites change, and the exchanged list gives another picture
    alone = {}
    for k in "PM":
        buf = torch.from_numpy(fill).cuda()
        _sequential([(nodes[k], cam, depth, buf, None, None, None)])
        alone[k] = _changed(_bits(buf), fill.view(np.uint32))
    both = int((alone["P"] & alone["M"]).sum())
    print(f"{config} {sampler}: P changes {int(alone['P'].sum())} pixels, M {int(alone['M'].sum())}, both {both}")
    assert both >= 100
    assert not np.array_equal(pictures["PQM"], pictures["MQP"])
    for node in nodes.values():
        node.close()


# ---- 2. mixed families and formats --------------------------------------------------------------------------------------------------------------------

MIXED = {"P": ("clouds_high", dict(sampler="declared")), "Q": ("no_clouds_8", {}), "M": ("v1_no_clouds", {})}


@pytest.mark.parametrize("fmt,pad", [("rgba32f", 0), ("rgba16f", 0), ("rgba8_srgb", PAD)], ids=["float", "rgba16f", "rgba8_srgb_pitched"])
def test_mixed_families_in_one_frame(fmt, pad):
    tex = demo_textures(cube_n=64, shape_n=32)
    cam = _cam()
    depth_np = _depth_np(cam)
    depth = torch.from_numpy(depth_np).cuda()
    nodes = _nodes(MIXED, cam, tex)
    _geometry(nodes, cam, depth_np, f"mixed {fmt}")
    fill = _random_dst((H, W, 4), fmt, 43)
    target = fmt if fmt == "rgba8_srgb" else None
    want, got = Buf(H, W, fmt, pad, fill), Buf(H, W, fmt, pad, fill)
    _sequential([(nodes[k], cam, depth, want.view, None, None, target) for k in "PQM"])
    torch.cuda.synchronize()
    singles = {k: nodes[k].kernel_name for k in "PQM"}
    draws = [(nodes[k], cam, depth, got.view, None, None, target) for k in "PQM"]
    assert PA.plan_planets(draws) == ([0, 1, 2], 3)          # three families: P and Q in level 0, one launch each; M behind P
    PA.render_planets(draws)
    torch.cuda.synchronize()
    assert want.outside_intact() and got.outside_intact(), "padding or guards"
    assert np.array_equal(got.bits(), want.bits())
    assert int(_changed(got.picture(), fill).sum()) > 1000
    for k in "PQM":      # each node's kernel_name names the views-proxy kernel of ITS OWN flags
        _views_proxy_name_of(singles[k], nodes[k])
    assert len({kernel_flags(n) for n in nodes.values()}) == 3 and kernel_flags(nodes["P"]) & 32
    for node in nodes.values():
        node.close()


# ---- 3. stereo halves of one image ----------------------------------------------------------------------------------------------------------------------

def test_stereo_halves_of_one_rgba16f_image():
    """Two eyes times (P, M): four draws into the halves of one 960 x 270 RGBA16F image, two launches, bit-equal to the four single draws."""
    tex = demo_textures(cube_n=64, shape_n=32)
    eyes = [_cam(-3.0), _cam(3.0)]
    depths_np = [_depth_np(c) for c in eyes]
    depths = [torch.from_numpy(d).cuda() for d in depths_np]
    nodes = _nodes({"P": ("clouds_high_rm", {}), "Q": ("no_clouds_8", {}), "M": ("clouds_high_rm", {})}, _cam(), tex)
    for e in range(2):
        _geometry(nodes, eyes[e], depths_np[e], f"eye {e}", names=("P", "M"), rects=None)
    fill = _random_dst((H, 2 * W, 4), "rgba16f", 47)
    images = [Buf(H, 2 * W, "rgba16f", PAD, fill) for _ in range(2)]
    halves = [[img.view[:, :W], img.view[:, W:]] for img in images]
    order = [(k, e) for k in "PM" for e in range(2)]
    _sequential([(nodes[k], eyes[e], depths[e], halves[0][e], None, None, None) for k, e in order])
    draws = [(nodes[k], eyes[e], depths[e], halves[1][e], None, None, None) for k, e in order]
    assert PA.plan_planets(draws) == ([0, 0, 1, 1], 2)
    PA.render_planets(draws)
    torch.cuda.synchronize()
    assert images[0].outside_intact() and images[1].outside_intact()
    assert np.array_equal(images[1].bits(), images[0].bits())
    for half in (slice(0, W), slice(W, 2 * W)):
        assert int(_changed(images[1].picture()[:, half], fill[:, half]).sum()) > 1000
    for node in nodes.values():
        node.close()


# ---- 4. every entry from its own context ----------------------------------------------------------------------------------------------------------------

def test_planets_differ_in_uniforms_and_textures():
    """P and Q are one family and share a launch, but Q has another radius (the scene's), density, cubemap and shape volume: an entry filled from the
    wrong context shows."""
    tex = demo_textures(cube_n=64, shape_n=32)
    other = dict(tex, cubemap=np.ascontiguousarray(tex["cubemap"][::-1, ::-1, :]), shape=np.ascontiguousarray(255 - tex["shape"][::-1]))
    cam = _cam()
    depth_np = _depth_np(cam)
    depth = torch.from_numpy(depth_np).cuda()
    nodes = {"P": _place(make_node("clouds_high", tex), "P", cam),
             "Q": _place(make_node("clouds_high", other, params=demo_params(u_density=0.35, u_cloud_density_scale=80.0)), "Q", cam)}
    fill = _scene(cam, 53)
    bufs = {}
    for which in ("sequential", "batched", "q_as_p"):
        bufs[which] = _guarded(H, W, fill=fill)
    _sequential([(nodes[k], cam, depth, bufs["sequential"][0], None, None, None) for k in "PQ"])
    draws = [(nodes[k], cam, depth, bufs["batched"][0], None, None, None) for k in "PQ"]
    assert PA.plan_planets(draws) == ([0, 0], 1)
    PA.render_planets(draws)
    # what a frame looks like when Q is drawn with P's textures and density: not this one
    twin = _place(make_node("clouds_high", tex), "Q", cam)
    _sequential([(nodes["P"], cam, depth, bufs["q_as_p"][0], None, None, None), (twin, cam, depth, bufs["q_as_p"][0], None, None, None)])
    torch.cuda.synchronize()
    assert _guards_intact(bufs["batched"][1], H * W)
    assert np.array_equal(_bits(bufs["batched"][1]), _bits(bufs["sequential"][1]))
    assert not np.array_equal(_bits(bufs["batched"][1]), _bits(bufs["q_as_p"][1]))
    x0, y0, x1, y1 = RECTS["Q"]
    assert int(_changed(_bits(bufs["batched"][0])[y0:y1, x0:x1], fill.view(np.uint32)[y0:y1, x0:x1]).sum()) >= 300
    for node in list(nodes.values()) + [twin]:
        node.close()


# ---- 5. draws that draw nothing --------------------------------------------------------------------------------------------------------------------------

def test_draws_that_draw_nothing():
    tex = demo_textures(cube_n=64, shape_n=32)
    cam, away = _cam(), S.Camera(W, H, (0.0, 0.0, 700.0), (0.0, 0.0, 1400.0), far=5000.0)
    depth_np = _depth_np(cam)
    depth = torch.from_numpy(depth_np).cuda()
    nodes = _nodes("clouds_high", cam, tex)
    fill = _scene(cam, 59)
    want, want_whole = _guarded(H, W, fill=fill)
    got, got_whole = _guarded(H, W, fill=fill)
    off = (0, 0, 100, 60)          # no box reaches this rect
    _sequential([(nodes["P"], cam, depth, want, None, None, None), (nodes["M"], cam, depth, want, None, None, None)])
    draws = [(nodes["Q"], away, depth, got, None, None, None), (nodes["P"], cam, depth, got, None, None, None), (nodes["Q"], cam, depth, got, off, None, None),
             (nodes["M"], cam, depth, got, None, None, None), (nodes["P"], cam, depth, got, (7, 7, 7, 90), None, None)]
    assert PA.plan_planets(draws) == ([-1, 0, -1, 1, -1], 2)
    PA.render_planets(draws)
    torch.cuda.synchronize()
    assert _guards_intact(got_whole, H * W) and np.array_equal(_bits(got_whole), _bits(want_whole))
    assert int(_changed(_bits(got), fill.view(np.uint32)).sum()) > 1000
    # nothing at all: ATMO_OK, the scene untouched, no launch (the last kernel's name stays)
    names = {k: n.kernel_name for k, n in nodes.items()}
    before = _bits(got_whole).copy()
    nothing = [draws[0], draws[2], draws[4]]
    assert PA.plan_planets(nothing) == ([-1, -1, -1], 0)
    PA.render_planets(nothing)
    PA.render_planets([])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got_whole), before) and names == {k: n.kernel_name for k, n in nodes.items()}
    for node in nodes.values():
        node.close()


# ---- 6. a texture update on another stream between two frames ---------------------------------------------------------------------------------------------

def test_texture_update_on_another_stream_between_two_frames():
    """Frame, update of Q's cubemap on a side stream, frame -- with no host synchronisation in between: Q is not its launch's first context, and still
    the update waits for the first frame and the second frame for the update, on the device."""
    tex = demo_textures(cube_n=64, shape_n=32)
    cube2 = np.ascontiguousarray(tex["cubemap"][::-1, :, ::-1])
    cam = _cam()
    depth = torch.from_numpy(_depth_np(cam)).cuda()
    nodes = _nodes("clouds_high", cam, tex)
    fill = _scene(cam, 61)
    frames = [_guarded(H, W, fill=fill) for _ in range(2)]
    side = torch.cuda.Stream()
    lib = N.load()
    torch.cuda.synchronize()
    PA.render_planets([(nodes[k], cam, depth, frames[0][0], None, None, None) for k in "PQM"])
    rc = lib.atmo_set_texture(nodes["Q"]._ctx, b"u_cloud_coverage_cubemap", N.TEX_CUBE_R8, 64, 64, 6, 0, cube2.ctypes.data_as(C.c_void_p), N.MEM_HOST,
                              C.c_void_p(side.cuda_stream))
    assert rc == N.ATMO_OK, lib.atmo_last_error_string(nodes["Q"]._ctx)
    PA.render_planets([(nodes[k], cam, depth, frames[1][0], None, None, None) for k in "PQM"])
    torch.cuda.synchronize()
    want = []
    for cube in (tex["cubemap"], cube2):
        ref = _nodes({"P": ("clouds_high", {}), "Q": ("clouds_high", {}), "M": ("clouds_high", {})}, cam, dict(tex, cubemap=cube))
        buf, whole = _guarded(H, W, fill=fill)
        _sequential([(nodes["P"], cam, depth, buf, None, None, None), (ref["Q"], cam, depth, buf, None, None, None),
                     (nodes["M"], cam, depth, buf, None, None, None)])
        torch.cuda.synchronize()
        want.append(_bits(whole).copy())
        for node in ref.values():
            node.close()
    assert np.array_equal(_bits(frames[0][1]), want[0]) and np.array_equal(_bits(frames[1][1]), want[1])
    assert not np.array_equal(want[0], want[1])
    for node in nodes.values():
        node.close()


# ---- 7. against the CPU oracle -----------------------------------------------------------------------------------------------------------------------------

def test_two_planet_frame_matches_the_oracle(oracle32):
    """P (clouds_high_rm) and Q (no_clouds_8) in one call into zero-filled float scenes -- one per planet, so that each picture is the planet's own
    premultiplied-free composite over nothing -- against the oracle's plain render of the passing fragments: rgb * a over zero."""
    tex = demo_textures(cube_n=64, shape_n=32)
    cam = _cam()
    depth_np = _depth_np(cam)
    depth = torch.from_numpy(depth_np).cuda()
    configs = {"P": "clouds_high_rm", "Q": "no_clouds_8"}
    params = {k: demo_params(u_planet_radius=PLANETS[k][1], u_atmosphere_height=PLANETS[k][2]) for k in configs}
    nodes = {k: _place(make_node(c, tex, params=params[k]), k, cam) for k, c in configs.items()}
    scenes = {k: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for k in configs}
    draws = [(nodes[k], cam, depth, scenes[k], None, None, None) for k in "PQ"]
    assert PA.plan_planets(draws) == ([0, 1], 2)
    PA.render_planets(draws)
    torch.cuda.synchronize()
    for k, config in configs.items():
        node = nodes[k]
        cfg = CONFIGS[config][1]
        ocfg, otex = oracle_inputs(oracle32, cfg, tex, node.read_optical_depth())
        covered, passing, unstable = G.frame_masks(cam, node.global_transform, node.proxy_box_size(cam), depth_np)
        m = passing & ~unstable
        ys, xs = np.nonzero(passing)
        x0, y0, x1, y1 = int(xs.min()) & ~1, int(ys.min()) & ~1, min((int(xs.max()) + 2) & ~1, W), min((int(ys.max()) + 2) & ~1, H)
        # (as the node stands behind `_process`: the planet's own model space, the cloud layer not yet rotated)
        oparams = dict(params[k], u_world_to_model_matrix=S.col_major(np.linalg.inv(node.global_transform)), u_cloud_coverage_rotation=(1.0, 0.0, 0.0, 1.0))
        plain = np.zeros((H, W, 4), dtype=np.float32)
        plain[y0:y1, x0:x1], hits = oracle32.render(oparams, otex, ocfg, node.make_frame(cam), depth_np, rect=(x0, y0, x1, y1), nthreads=8)
        assert hits > 0
        # blend_mix over a zero scene: rgb = src.rgb * a, alpha = a (include/atmo.h: atmo_render_composite)
        want = plain.copy()
        want[..., :3] *= plain[..., 3:4]
        got = scenes[k].cpu().numpy()
        err = float(np.abs(got[m] - want[m]).max())
        print(f"\n{k} {config}: {int(m.sum())} fragments, max abs err vs oracle {err:.3e}")
        assert err <= TOL, (k, config, err)
        assert not got[~passing & ~unstable].any()
        node.close()


# ---- 8. capture is refused; ahead of the device --------------------------------------------------------------------------------------------------------------

def test_capture_is_refused_and_forty_calls_run_ahead():
    tex = demo_textures(cube_n=64, shape_n=32)
    cam = _cam()
    depth = torch.from_numpy(_depth_np(cam)).cuda()
    nodes = _nodes({"P": ("clouds_high", {}), "Q": ("no_clouds_8", {}), "M": ("clouds_high", {})}, cam, tex)
    fill = _scene(cam, 67)
    scene = torch.from_numpy(fill).cuda()
    PA.render_planets([(nodes[k], cam, depth, torch.from_numpy(fill).cuda(), None, None, None) for k in "PQM"])      # (bakes the optical depths)
    arr = PA.prepare_planets([(nodes[k], cam, depth, scene, None, None, None) for k in "PQM"])
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(N.AtmoError) as ei:
                PA.render_planets_prepared(arr, 3, side.cuda_stream)
            assert ei.value.code == N.ATMO_E_STATE and "cannot be captured" in str(ei.value)
            scene.add_(0.0)      # (the capture is still usable)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(scene), fill.view(np.uint32))
    # 40 frames with a new pose each, back to back without a host synchronisation (two or three launches a call; the staging rings have 16 slots)
    poses = [S.Camera(W, H, (2.0 * k - 40.0, 0.5 * k, 700.0), (2.0 * k - 40.0, 0.0, 0.0), far=5000.0) for k in range(40)]
    depths = [torch.from_numpy(_depth_np(c)).cuda() for c in poses]
    outs = [torch.from_numpy(fill).cuda() for _ in poses]
    torch.cuda.synchronize()
    for k, c in enumerate(poses):              # no synchronisation in here
        PA.render_planets([(nodes[n], c, depths[k], outs[k], None, None, None) for n in "PQM"])
    torch.cuda.synchronize()
    for k in (0, 7, 8, 15, 16, 17, 38, 39):
        want = torch.from_numpy(fill).cuda()
        _sequential([(nodes[n], poses[k], depths[k], want, None, None, None) for n in "PQM"])
        torch.cuda.synchronize()
        assert np.array_equal(_bits(outs[k]), _bits(want)), k
        assert int(_changed(_bits(want), fill.view(np.uint32)).sum()) > 1000
    assert not np.array_equal(_bits(outs[38]), _bits(outs[39]))
    for node in nodes.values():
        node.close()


# ---- 9. the node-level form ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", [None, "rgba16f"])
def test_draw_atmospheres_batched_equals_draw_atmospheres(target):
    """The near-plus-far scene of tests/test_proxy_gpu.py::test_several_planets_draw_back_to_front: far, planet (far mode), then the moon's fullscreen draw."""
    from test_proxy_gpu import H as PH, W as PW

    tex = demo_textures(cube_n=64, shape_n=32)
    cam = S.Camera(PW, PH, (0.0, 0.0, 500.0), (0.0, 0.0, 0.0), far=5000.0)
    planet, moon, far = make_node("clouds", tex), make_node("no_clouds_8", tex), make_node("v1_no_clouds", tex)
    moon.planet_radius, moon.atmosphere_height = 27.0, 3.0
    placed = [(planet, (0.0, 0.0, 0.0)), (moon, (6.0, 4.0, 455.0)), (far, (-700.0, 150.0, -1500.0))]
    for node, pos in placed:
        node.global_transform = G.translation(*pos)
        node._process(camera=cam, time=0.0)
    assert planet._mode == 1 and far._mode == 1 and moon._mode == 0
    depth = torch.from_numpy(S.depth_far(cam)).cuda()
    fmt = target or "rgba32f"
    fill = _random_dst((PH, PW, 4), fmt, 71)
    want, got = Buf(PH, PW, fmt, 0, fill), Buf(PH, PW, fmt, 0, fill)
    assert PA.draw_atmospheres([planet, moon, far], cam, depth, want.view) is want.view
    assert PA.draw_atmospheres_batched([planet, moon, far], cam, depth, got.view) is got.view
    torch.cuda.synchronize()
    assert planet.kernel_name.startswith("atmo_render_views_proxy") and far.kernel_name.startswith("atmo_render_views_proxy")
    assert got.outside_intact() and np.array_equal(got.bits(), want.bits())
    assert int(_changed(got.picture(), fill).sum()) > 1000
    for node, _ in placed:
        node.close()
