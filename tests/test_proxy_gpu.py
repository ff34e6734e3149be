"""GPU tests of the far-mode proxy draw (include/atmo_scene.h: atmo_render_proxy / atmo_render_proxy_composite, PlanetAtmosphere.draw,
draw_atmospheres): every passing fragment is atmo_render's pixel bit for bit, every other pixel is left alone, the passing set is the float64
statement of the fragment test (tests/proxy_geometry.py), and the cases where Godot draws nothing leave the frame untouched."""
import numpy as np
import pytest
import torch

import proxy_geometry as G
from common import CONFIGS, TOL, demo_frame, demo_params, demo_textures, make_node, oracle_inputs
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.planet_atmosphere import draw_atmospheres, draw_order

pytestmark = pytest.mark.gpu

W, H = 96, 54
# the seven shader variants under default settings (the declared sampler where there are clouds), the direct-light atmosphere, and the one-lane
# level-0 and direct-light cloud families
VARIANTS = [("no_clouds_8", {}), ("no_clouds_32x8_direct", {}), ("clouds", {}), ("clouds_high", {}), ("clouds_high_rm", {}), ("v1_no_clouds", {}),
            ("v1_clouds", {}), ("v1_clouds_high", {}), ("clouds_high_rm", dict(sampler="lod0")), ("clouds_high", dict(light_mode="direct", light_steps=8))]


def _far_cam(w=W, h=H):
    return S.Camera(w, h, (31.0, 17.0, 420.0), (0.0, 0.0, 0.0))


def _node(config, tex, **kw):
    node = make_node(config, tex, **kw)
    node.global_transform = np.eye(4)
    return node


def _pattern(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32).cuda()


def _same_bits(a, b):
    return (a.view(torch.int32) == b.view(torch.int32)).all(dim=-1)


def _check_composite(node, cam, depth_np, seed=1):
    depth = torch.from_numpy(depth_np).cuda()
    scene = _pattern((cam.height, cam.width, 4), seed)
    full = node.render_composite(cam, depth, scene.clone())
    got = node.render_proxy_composite(cam, depth, scene.clone())
    torch.cuda.synchronize()
    covered, passing, unstable = G.frame_masks(cam, node.global_transform, node.proxy_box_size(cam), depth_np)
    passing_t, stable_t = torch.from_numpy(passing).cuda(), torch.from_numpy(~unstable).cuda()
    as_full, as_scene = _same_bits(got, full), _same_bits(got, scene)
    assert bool((as_full | as_scene).all())
    assert bool(as_full[passing_t & stable_t].all()), "a passing fragment differs from atmo_render_composite"
    assert bool(as_scene[~passing_t & stable_t].all()), "a pixel outside the passing set was written"
    assert unstable.sum() < 1e-3 * max(covered.sum(), 1), (unstable.sum(), covered.sum())
    return full, got, scene, passing


@pytest.mark.parametrize("config,kw", VARIANTS, ids=[c + ("@" + "_".join(f"{v}" for v in k.values()) if k else "") for c, k in VARIANTS])
def test_proxy_is_atmo_render_on_its_fragments(config, kw):
    tex = demo_textures(cube_n=64, shape_n=32)
    node = _node(config, tex, **kw)
    cam = _far_cam()
    depth_np = S.depth_ground_sphere(cam)
    full, got, scene, passing = _check_composite(node, cam, depth_np)
    assert passing.sum() > 300 and bool((got != scene).any())
    assert "proxy" in node.kernel_name
    # the plain call into a pre-filled buffer: passing pixels are atmo_render's (covered discards (0,0,0,0)), the rest keeps the fill
    depth = torch.from_numpy(depth_np).cuda()
    ref = node.render(cam, depth)
    fill = _pattern((H, W, 4), 7)
    out = node.render_proxy(cam, depth, out=fill.clone())
    torch.cuda.synchronize()
    _, passing, unstable = G.frame_masks(cam, node.global_transform, node.proxy_box_size(cam), depth_np)
    p, s = torch.from_numpy(passing).cuda(), torch.from_numpy(~unstable).cuda()
    assert bool(_same_bits(out, ref)[p & s].all()) and bool(_same_bits(out, fill)[~p & s].all())
    node.close()


@pytest.mark.parametrize("config", ["no_clouds_8", "clouds_high_rm"])
def test_proxy_fragments_match_the_oracle(config):
    from oracle.oracle import Oracle

    oracle = Oracle("f32")
    tex = demo_textures(cube_n=64, shape_n=32)
    node = _node(config, tex)
    cam = _far_cam()
    depth_np = S.depth_ground_sphere(cam)
    depth = torch.from_numpy(depth_np).cuda()
    out = node.render_proxy(cam, depth, out=torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")).cpu().numpy()
    cfg = CONFIGS[config][1]
    lut = node.read_optical_depth() if not cfg.get("lite") else None
    ocfg, otex = oracle_inputs(oracle, cfg, tex, lut)
    want, _ = oracle.render(demo_params(), otex, ocfg, demo_frame(cam), depth_np, nthreads=4)
    _, passing, unstable = G.frame_masks(cam, node.global_transform, node.proxy_box_size(cam), depth_np)
    m = passing & ~unstable
    assert m.sum() > 300
    assert float(np.abs(out[m] - want[m]).max()) <= TOL
    node.close()


def test_nothing_is_drawn_where_godot_draws_nothing():
    """Planet behind the camera, planet beyond the far plane: the proxy leaves the scene bit-unchanged; the fullscreen draw does not."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = _node("no_clouds_8", tex)
    cams = [S.Camera(64, 36, (0.0, 0.0, 400.0), (0.0, 0.0, 800.0))]                        # looking +z, away from the planet
    cams += [S.Camera(64, 36, (0.0, 0.0, z), (0.0, 0.0, z - 1.0)) for z in (1000.0, 1500.0, 3000.0)]     # the planet 1000 / 1500 / 3000 ahead, far = 800
    changed_by_full = 0
    for cam in cams:
        depth = torch.from_numpy(S.depth_far(cam)).cuda()
        scene = _pattern((cam.height, cam.width, 4), 3)
        got = node.render_proxy_composite(cam, depth, scene.clone())
        full = node.render_composite(cam, depth, scene.clone())
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), scene.view(torch.int32))
        changed_by_full += int((~_same_bits(full, scene)).sum())
    assert changed_by_full > 0
    node.close()


def test_occluder_in_front_of_the_box_keeps_its_pixels():
    tex = demo_textures(cube_n=64, shape_n=32)
    node = _node("clouds_high", tex)
    cam = _far_cam()
    depth_np = S.depth_ground_sphere(cam)
    # a ship 150 units in front of the camera over the middle of the planet (the box's front face is ~ 300 away): its reverse-Z depth
    p = cam.projection
    z_ship = (p[2, 2] * -150.0 + p[2, 3]) / (p[3, 2] * -150.0 + p[3, 3])
    depth_np[22:32, 42:54] = np.float32(z_ship)
    full, got, scene, passing = _check_composite(node, cam, depth_np, seed=5)
    covered, _, _ = G.frame_masks(cam, node.global_transform, node.proxy_box_size(cam), depth_np)
    assert covered[22:32, 42:54].all() and not passing[22:32, 42:54].any()
    assert torch.equal(got[22:32, 42:54].view(torch.int32), scene[22:32, 42:54].view(torch.int32))
    node.close()


def test_telephoto_view_shows_the_rim_clip():
    """The reference's quirk: the box's half-edge 0.9625 (R + H + near) < R + H, so face-on from ~40 (R + H) the box cuts the halo's rim."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = _node("no_clouds_8", tex)
    cam = S.Camera(256, 144, (0.0, 0.0, 4320.0), (0.0, 0.0, 0.0), fovy_deg=2.0, far=10000.0)
    depth_np = S.depth_far(cam)   # (no ground: from 4320 away the ground's depth is within 1e-8 of the box face's)
    full, got, scene, passing = _check_composite(node, cam, depth_np, seed=9)
    covered, _, unstable = G.frame_masks(cam, node.global_transform, node.proxy_box_size(cam), depth_np)
    halo_outside = ~_same_bits(full, scene).cpu().numpy() & ~covered & ~unstable
    assert halo_outside.sum() > 10   # halo pixels the fullscreen draw shades and the box does not
    assert bool(_same_bits(got, scene).cpu().numpy()[halo_outside].all())
    node.close()


def test_rect_crop_is_the_crop_of_the_full_proxy_draw():
    tex = demo_textures(cube_n=64, shape_n=32)
    node = _node("clouds_high", tex)   # declared sampler: pixels outside the rect are helpers
    cam = _far_cam()
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    scene = _pattern((H, W, 4), 11)
    full = node.render_proxy_composite(cam, depth, scene.clone())
    x0, y0, x1, y1 = 37, 13, 71, 40
    crop = node.render_proxy_composite(cam, depth, scene.clone(), rect=(x0, y0, x1, y1))
    torch.cuda.synchronize()
    want = scene.clone()
    want[y0:y1, x0:x1] = full[y0:y1, x0:x1]
    assert torch.equal(crop.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(full[y0:y1, x0:x1], scene[y0:y1, x0:x1])
    node.close()


def test_proxy_draw_replays_from_a_hip_graph():
    tex = demo_textures(cube_n=64, shape_n=32)
    node = _node("clouds_high_rm", tex)
    cam = _far_cam()
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    scene = _pattern((H, W, 4), 13)
    ref = node.render_proxy_composite(cam, depth, scene.clone())
    torch.cuda.synchronize()
    target = scene.clone()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            node.render_proxy_composite(cam, depth, target, stream=side)
    torch.cuda.synchronize()
    target.copy_(scene)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(target.view(torch.int32), ref.view(torch.int32))
    node.close()


@pytest.mark.parametrize("config,kw", [("clouds_high", dict(precise_clouds=False)), ("no_clouds_8", dict(precise_atmosphere=True)),
                                       ("no_clouds_8", dict(view_steps=64)), ("clouds_high_rm", dict(lane_split=2))],
                         ids=["precision0", "precision2", "view_steps64", "lane_split2"])
def test_unsupported_modes_fail_with_state_error(config, kw):
    from godot_atmosphere_shader_amd import _native as N

    tex = demo_textures(cube_n=64, shape_n=32)
    node = _node(config, tex, **kw) if "precise_clouds" not in kw else _node(config, tex, sampler="lod0", **kw)
    cam = _far_cam()
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    scene = _pattern((H, W, 4), 17)
    with pytest.raises(N.AtmoError) as e:
        node.render_proxy_composite(cam, depth, scene)
    assert e.value.code == N.ATMO_E_STATE and "no proxy kernel" in str(e.value)
    node.render_composite(cam, depth, scene)   # the fullscreen draw of the same context still works
    node.close()


def test_several_planets_draw_back_to_front():
    tex = demo_textures(cube_n=64, shape_n=32)
    cam = S.Camera(W, H, (0.0, 0.0, 500.0), (0.0, 0.0, 0.0), far=5000.0)
    planet = make_node("clouds", tex)
    moon = make_node("no_clouds_8", tex)
    far = make_node("v1_no_clouds", tex)
    moon.planet_radius, moon.atmosphere_height = 27.0, 3.0
    placed = [(planet, (0.0, 0.0, 0.0)), (moon, (6.0, 4.0, 455.0)), (far, (-700.0, 150.0, -1500.0))]
    for node, pos in placed:
        node.global_transform = G.translation(*pos)
        node._process(camera=cam, time=0.0)
    assert planet._mode == 1 and far._mode == 1 and moon._mode == 0   # far, far, near (the moon is 45 away: inside its 57.9 switch distance)
    depth = torch.from_numpy(S.depth_far(cam)).cuda()
    scene = _pattern((H, W, 4), 19)
    got = draw_atmospheres([planet, moon, far], cam, depth, scene.clone())
    assert [n for n in draw_order([planet, moon, far], cam)] == [far, planet, moon]
    want = scene.clone()
    far.render_proxy_composite(cam, depth, want, box_size=far.proxy_box_size(cam))
    planet.render_proxy_composite(cam, depth, want, box_size=planet.proxy_box_size(cam))
    moon.render_composite(cam, depth, want)
    swapped = scene.clone()
    far.render_proxy_composite(cam, depth, swapped)
    moon.render_composite(cam, depth, swapped)
    planet.render_proxy_composite(cam, depth, swapped)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got.view(torch.int32), swapped.view(torch.int32))
    for node, _ in placed:
        node.close()
