"""GPU tests of the multi-view draw (include/atmo_views.h): atmo_render_views against atmo_render / atmo_render_composite of every view on its own.
Every picture comparison is BIT-EXACT (np.array_equal on the raw 32-bit patterns; no tolerance): the header's contract is that a view's pixels do not
depend on the views drawn with it nor on the order the tiles of the batch run in.  One test goes to the CPU oracle, at common.TOL, so that the file is
not only self-comparison."""
import numpy as np
import pytest
import torch

from common import CONFIGS, TOL, demo_frame, demo_params, demo_textures, has_clouds, kernel_flags, make_node, oracle_inputs
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import scene as S

pytestmark = pytest.mark.gpu

KF_VIEWS = 2048
GUARD = 64                       # sentinel pixels in front of and behind every output
SENTINEL = 0x7FC5A5A5            # a NaN pattern no kernel produces
BIG, SMALL = (251, 141), (96, 64)            # an odd size (partial tiles on both edges, odd rows of quads) and a small one
SMALL_RECT = (33, 7, 95, 63)                 # odd origin, partial: under the declared sampler its grid starts at (32, 6), helper lanes in front


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _guarded(rows, cols, fill=None):
    """A contiguous (rows, cols, 4) float32 CUDA tensor inside a sentinel-filled buffer: (view, whole buffer as uint32 bits accessor)."""
    n = rows * cols
    whole = torch.from_numpy(np.full(((2 * GUARD + n) * 4,), SENTINEL, dtype=np.uint32).view(np.float32)).cuda()
    view = whole[GUARD * 4:(GUARD + n) * 4].view(rows, cols, 4)
    if fill is not None:
        view.copy_(torch.from_numpy(fill).cuda())
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return view, whole


def _guards_intact(whole, n):
    b = _bits(whole)
    return bool(np.all(b[:GUARD * 4] == SENTINEL) and np.all(b[(GUARD + n) * 4:] == SENTINEL))


def _scene(cam, seed):
    """A pseudo-random scene colour buffer (finite values, alphas in [0, 1])."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.25, 2.0, size=(cam.height, cam.width, 4)).astype(np.float32)
    a[..., 3] = rng.uniform(0.0, 1.0, size=(cam.height, cam.width)).astype(np.float32)
    return a


def _depth(cam):
    return torch.from_numpy(S.depth_ground_sphere(cam)).cuda()


def _check_batch(node, cams, depths, rects, label):
    """Plain and composite: every view of one batch == its own atmo_render / atmo_render_composite, memory around the outputs untouched."""
    n = len(cams)
    full = [r or (0, 0, c.width, c.height) for c, r in zip(cams, rects)]
    # the separate draws
    want_plain, want_comp, scenes = [], [], []
    for i, (cam, depth, rect) in enumerate(zip(cams, depths, rects)):
        x0, y0, x1, y1 = full[i]
        if x0 == x1 or y0 == y1:
            want_plain.append(None)
        else:
            want_plain.append(_bits(node.render(cam, depth, rect=rect)).copy())
        scene = _scene(cam, 100 + i)
        scenes.append(scene)
        want_comp.append(_bits(node.render_composite(cam, depth, torch.from_numpy(scene).cuda(), rect=rect)).copy())
    torch.cuda.synchronize()
    single_name = node.kernel_name
    # the batch, plain
    outs, wholes = [], []
    for (x0, y0, x1, y1) in full:
        v, w = _guarded(max(y1 - y0, 0), max(x1 - x0, 0))
        outs.append(v)
        wholes.append(w)
    got = node.render_views(cams, depths, outs=outs, rects=rects)
    torch.cuda.synchronize()
    assert node.kernel_name.startswith("atmo_render_views_kernel<"), node.kernel_name
    assert kernel_flags(node) == int(single_name.split("<")[1].split(",")[0]) + KF_VIEWS, (node.kernel_name, single_name)
    assert node.kernel_name.split(",")[1].strip(" >") == single_name.split(",")[1].strip(), (node.kernel_name, single_name)
    for i in range(n):
        x0, y0, x1, y1 = full[i]
        assert _guards_intact(wholes[i], (y1 - y0) * (x1 - x0)), (label, "plain: memory outside view", i)
        if want_plain[i] is None:
            continue
        assert got[i] is outs[i]
        assert np.array_equal(_bits(got[i]), want_plain[i]), (label, "plain", i)
        assert (want_plain[i] != 0).any(), (label, i, "the view shades nothing")
    # the batch, composite: the whole scene buffer of every view (the pixels outside its rect included) == atmo_render_composite's
    outs, wholes = [], []
    for cam, scene in zip(cams, scenes):
        v, w = _guarded(cam.height, cam.width, fill=scene)
        outs.append(v)
        wholes.append(w)
    node.render_views(cams, depths, outs=outs, rects=rects, composite=True)
    torch.cuda.synchronize()
    for i, cam in enumerate(cams):
        assert _guards_intact(wholes[i], cam.height * cam.width), (label, "composite: memory outside view", i)
        assert np.array_equal(_bits(outs[i]), want_comp[i]), (label, "composite", i)
        x0, y0, x1, y1 = full[i]
        if x1 > x0 and y1 > y0:
            assert not np.array_equal(want_comp[i], scenes[i].view(np.uint32)), (label, i, "the composite changes nothing")


# every multi-view kernel: (config, PlanetAtmosphere keywords, sampler) -> <FLAGS, LSTEPS>
DIRECT4 = dict(light_mode="direct", light_steps=4)
DIRECT8 = dict(light_mode="direct", light_steps=8)
FAMILY_CASES = [
    ("no_clouds_8", {}, "declared"),                      # <0, 0>
    ("no_clouds_32x8_direct", {}, "declared"),            # <4, 8>
    ("no_clouds_8", DIRECT4, "declared"),                 # <4, 0>
    ("v1_no_clouds", {}, "declared"),                     # <24, 0>
] + [(c, kw, s) for s in ("declared", "lod0") for c, kw in (
    ("clouds_high", {}), ("clouds_high_rm", {}),          # <17 | 49, 0>, <19 | 51, 0>
    ("clouds_high", DIRECT8), ("clouds_high_rm", DIRECT8),    # <21 | 53, 8>, <23 | 55, 8>
    ("clouds_high", DIRECT4), ("clouds_high_rm", DIRECT4),    # <21 | 53, 0>, <23 | 55, 0>
    ("v1_clouds", {}),                                    # <25 | 57, 0>
)]


@pytest.mark.parametrize("config,kw,sampler", FAMILY_CASES, ids=[f"{c}{'_direct%d' % kw['light_steps'] if kw else ''}_{s}" for c, kw, s in FAMILY_CASES])
def test_views_equal_their_own_draws(config, kw, sampler):
    """Two views with different poses and sizes -- 251 x 141 whole, 96 x 64 with an odd-origin partial rect -- in one launch, for every kernel of the
    family, plain and composite over pseudo-random scene buffers; memory outside the outputs is untouched."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node(config, tex, sampler=sampler, **kw)
    cams = [S.Camera.from_pose(*BIG, "P_space"), S.Camera.from_pose(*SMALL, "P_limb")]
    depths = [_depth(c) for c in cams]
    _check_batch(node, cams, depths, [None, SMALL_RECT], f"{config} {sampler}")
    if has_clouds(config):
        assert bool(kernel_flags(node) & 32) == (sampler == "declared")
    node.close()


def test_stereo_pair_with_a_visible_baseline():
    """The two eyes of a stereo pass: the same size, eyes 4 units apart looking at the same point -- different pictures, one launch."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    pose = S.POSES["P_space"]
    cams = [S.Camera.from_pose(320, 180, dict(eye=(pose["eye"][0] + dx, pose["eye"][1], pose["eye"][2]), target=pose["target"])) for dx in (-2.0, 2.0)]
    depths = [_depth(c) for c in cams]
    left = _bits(node.render(cams[0], depths[0])).copy()
    right = _bits(node.render(cams[1], depths[1])).copy()
    assert not np.array_equal(left, right)
    _check_batch(node, cams, depths, [None, None], "stereo")
    node.close()


def test_view_counts():
    """n_views = 1 is atmo_render; n_views = 8 with one empty view; n_views = 0 draws nothing; 9 views are refused."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    cam = S.Camera.from_pose(*BIG, "P_space")
    _check_batch(node, [cam], [_depth(cam)], [(17, 9, 250, 141)], "one view")
    poses = ["P_space", "P_ground", "P_limb", "P_clouds", "P_night", "P_space", "P_limb", "P_night"]
    sizes = [(96, 64), (80, 48), (64, 40), (112, 56), (96, 64), (48, 32), (72, 72), (96, 54)]
    cams = [S.Camera.from_pose(w, h, p) for (w, h), p in zip(sizes, poses)]
    rects = [None, (1, 3, 79, 47), None, (40, 20, 40, 50), None, (3, 3, 47, 31), None, (0, 1, 96, 53)]   # view 3 is empty
    _check_batch(node, cams, [_depth(c) for c in cams], rects, "eight views")
    assert node.render_views([], []) == []
    with pytest.raises(ValueError):
        node.render_views([cam] * 9, [_depth(cam)] * 9)
    node.close()


def test_layout_starts_even_under_the_declared_sampler():
    """atmo_debug_views_layout on contexts that do have a mip chain bound: under the declared sampler every view's grid starts on an even pixel (an odd
    origin adds a column / row of tiles where the rect ends on a tile edge), under the level-0 sampler at the rect."""
    import ctypes as C

    tex = demo_textures(cube_n=64, shape_n=32)
    cams = [S.Camera.from_pose(*BIG, "P_space"), S.Camera.from_pose(*SMALL, "P_limb"), S.Camera.from_pose(*SMALL, "P_limb")]
    rects = [(1, 1, 241, 137), SMALL_RECT, (8, 8, 8, 40)]          # 240 x 136 from an odd origin; 62 x 56 from (33, 7); empty
    for sampler, origin in (("declared", lambda v: v & ~1), ("lod0", lambda v: v)):
        node = make_node("clouds_high", tex, sampler=sampler)
        views = node.prepare_views(cams, [16] * 3, [32] * 3, rects)
        first, grid = (C.c_int * 4)(), (C.c_int * 6)()
        assert node._lib.atmo_debug_views_layout(node._ctx, views, 3, first, grid) == N.ATMO_OK
        want = [((x1 - origin(x0) + 15) // 16, (y1 - origin(y0) + 7) // 8) if x1 > x0 and y1 > y0 else (0, 0) for x0, y0, x1, y1 in rects]
        assert [(grid[2 * i], grid[2 * i + 1]) for i in range(3)] == want, (sampler, list(grid), want)
        assert list(first) == [0, want[0][0] * want[0][1], want[0][0] * want[0][1] + want[1][0] * want[1][1]] + [want[0][0] * want[0][1] + want[1][0] * want[1][1]]
        node.close()
    # the two samplers differ on the first rect: (1, 1, 241, 137) is 15 x 17 tiles from (1, 1) and 16 x 18 from (0, 0)
    assert ((241 - 1 + 15) // 16, (137 - 1 + 7) // 8) == (15, 17) and ((241 + 15) // 16, (137 + 7) // 8) == (16, 18)


def _two_views(w, h):
    return [S.Camera.from_pose(w, h, "P_space"), S.Camera.from_pose(w, h, "P_limb")]


def test_pictures_do_not_depend_on_the_tile_order():
    """Two 640 x 360 clouds_high_rm views, a still camera, 16 batches: every one is bit for bit the separate draws, the learnt order is in use by the
    end (feedback_stats), and the same run with atmo_set_tile_feedback(0) gives the same bits."""
    tex = demo_textures(cube_n=64, shape_n=32)
    cams = _two_views(640, 360)
    depths = [_depth(c) for c in cams]
    ref_node = make_node("clouds_high_rm", tex, tile_feedback=0)
    want = [_bits(ref_node.render(c, d)).copy() for c, d in zip(cams, depths)]
    ref_node.close()
    for feedback in (-1, 0):
        node = make_node("clouds_high_rm", tex, tile_feedback=feedback)
        before = node.feedback_stats()
        for k in range(16):
            outs = node.render_views(cams, depths)
            torch.cuda.synchronize()
            for i in range(2):
                assert np.array_equal(_bits(outs[i]), want[i]), (feedback, k, i)
        st = node.feedback_stats()
        print(f"\ntile_feedback {feedback}: {st}")
        if feedback == 0:
            assert st["ordered_draws"] == before["ordered_draws"] and st["sorts"] == before["sorts"]
        else:
            assert st["ordered_draws"] - before["ordered_draws"] >= 4 and st["sorts"] - before["sorts"] >= 1 and st["states"] == 1
        node.close()


def test_batches_can_be_enqueued_ahead():
    """16 batches with a new pose each, back to back without a host synchronisation, into 16 output sets: each equals its separate draws -- a staging slot
    of the per-view constants reused too early would shade a batch with a later batch's cameras.  Then 24 more the same way: the ring of 16 slots wraps."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    w, h = 320, 180

    def cams_of(k):
        a = 0.05 * k
        return [S.Camera(w, h, (160.0 * np.sin(a), 10.0 + k, 160.0 * np.cos(a)), (0.0, 0.0, 0.0)),
                S.Camera(w, h, (160.0 * np.sin(a) + 3.0, 10.0 + k, 160.0 * np.cos(a)), (0.0, 0.0, 0.0))]

    depth_of = {}
    for first, count in ((0, 16), (16, 24)):
        batches = [cams_of(k) for k in range(first, first + count)]
        for k, cams in enumerate(batches):
            depth_of[first + k] = [_depth(c) for c in cams]
        outs = [[torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2)] for _ in range(count)]
        torch.cuda.synchronize()
        for k, cams in enumerate(batches):              # no synchronisation in here
            node.render_views(cams, depth_of[first + k], outs=outs[k])
        torch.cuda.synchronize()
        got = [[_bits(o).copy() for o in pair] for pair in outs]
        for k, cams in enumerate(batches):
            for i in range(2):
                want = _bits(node.render(cams[i], depth_of[first + k][i]))
                assert np.array_equal(got[k][i], want), (first + k, i)
        assert not np.array_equal(got[0][0], got[1][0])   # the poses differ
    node.close()


@pytest.mark.parametrize("config", ["clouds_high_rm", "no_clouds_32x8_direct"])
def test_views_against_the_oracle(config, oracle32):
    """One cloud and one cloudless family: both views of a batch against the CPU oracle, at common.TOL."""
    tex = demo_textures(cube_n=64, shape_n=32)
    params = demo_params()
    node = make_node(config, tex, params)
    cfg = CONFIGS[config][1]
    lut = node.read_optical_depth() if not (cfg.get("lite") or cfg.get("light_steps")) else None
    ocfg, otex = oracle_inputs(oracle32, cfg, tex, lut)
    cams = [S.Camera.from_pose(128, 72, "P_space"), S.Camera.from_pose(*SMALL, "P_limb")]
    rects = [None, (32, 6, 96, 64)]
    depths_np = [S.depth_ground_sphere(c) for c in cams]
    outs = node.render_views(cams, [torch.from_numpy(d).cuda() for d in depths_np], rects=rects)
    torch.cuda.synchronize()
    for i, (cam, rect) in enumerate(zip(cams, rects)):
        want, hits = oracle32.render(params, otex, ocfg, demo_frame(cam), depths_np[i], nthreads=8)
        assert hits > 0
        if rect is not None:
            want = want[rect[1]:rect[3], rect[0]:rect[2]]
        got = outs[i].cpu().numpy()
        err = float(np.abs(got - want).max())
        print(f"\n{config} view {i}: {hits} hit rays, max abs err vs oracle {err:.3e}")
        assert err <= TOL, (config, i, err)
    node.close()


@pytest.mark.parametrize("mode,kw", [("precision0", dict(precise_clouds=False)), ("precision2", dict(precise_atmosphere=True)),
                                     ("view_steps64", dict(view_steps=64)), ("lane_split2", dict(lane_split=2))])
def test_views_refuse_the_other_modes(mode, kw):
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high", tex, **kw)
    cams = _two_views(96, 64)
    depths = [_depth(c) for c in cams]
    with pytest.raises(N.AtmoError) as ei:
        node.render_views(cams, depths)
    assert ei.value.code == N.ATMO_E_STATE and "no multi-view kernel" in str(ei.value)
    node.render(cams[0], depths[0])     # the context still draws single views
    torch.cuda.synchronize()
    node.close()


def test_views_refuse_graph_capture():
    """The per-view constants live in context-owned device memory the next batch overwrites: on a capturing stream atmo_render_views returns ATMO_E_STATE
    and leaves the capture usable (atmo_render into the same graph still works); outside a capture the batch works as before."""
    tex = demo_textures(cube_n=64, shape_n=32)
    cams = _two_views(320, 180)
    depths = [_depth(c) for c in cams]
    node = make_node("clouds_high", tex)
    refs = [node.render(c, d).clone() for c, d in zip(cams, depths)]
    torch.cuda.synchronize()
    outs = [torch.zeros_like(r) for r in refs]
    views = node.prepare_views(cams, [d.data_ptr() for d in depths], [o.data_ptr() for o in outs])
    frame = node.prepare_frame(cams[0])
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(N.AtmoError) as ei:
                node.render_views_prepared(views, 2, False, side.cuda_stream)
            assert ei.value.code == N.ATMO_E_STATE
            node.render_prepared(frame, depths[0].data_ptr(), outs[0].data_ptr(), side.cuda_stream)
    torch.cuda.synchronize()
    outs[0].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], refs[0]) and not outs[1].any()
    node.render_views_prepared(views, 2, False, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], refs[0]) and torch.equal(outs[1], refs[1])
    node.close()


@pytest.mark.parametrize("config", ["clouds_high", "no_clouds_8"])
def test_cleared_target_leaves_discarded_pixels_untouched(config):
    """atmo_set_target_cleared(1): a discarded fragment stores nothing, per view, as in atmo_render."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node(config, tex, target_cleared=True)
    cams = [S.Camera.from_pose(*BIG, "P_space"), S.Camera.from_pose(*SMALL, "P_space")]
    depths = [_depth(c) for c in cams]
    fill = lambda c: torch.from_numpy(np.full((c.height, c.width, 4), SENTINEL, dtype=np.uint32).view(np.float32)).cuda()   # noqa: E731
    want = [_bits(node.render(c, d, out=fill(c))).copy() for c, d in zip(cams, depths)]
    got = node.render_views(cams, depths, outs=[fill(c) for c in cams])
    torch.cuda.synchronize()
    for i in range(2):
        kept = (want[i] != SENTINEL).any(axis=-1)
        assert 0.1 <= kept.mean() <= 0.9, kept.mean()            # both branches are exercised
        assert np.array_equal(_bits(got[i]), want[i]), (config, i)
    # ... and with the double-precision origin convention (atmo_set_host_double_precision): per view as atmo_render
    node2 = make_node(config, tex, double_precision=True)
    want = [_bits(node2.render(c, d)).copy() for c, d in zip(cams, depths)]
    got = node2.render_views(cams, depths)
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(_bits(got[i]), want[i]), (config, "double_precision", i)
    node2.close()
    node.close()
