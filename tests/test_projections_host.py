"""The cameras of tests/cameras.py on the CPU: off-axis (stereo eye) frusta, a sub-pixel jitter, an infinite far plane and an orthographic projection,
each under a rolled view -- inputs that put non-zero values into the elements of inv_projection_matrix and inv_view_matrix that the host code reads
one by one.  Proved here, without a GPU, so that no case of tests/test_projections_gpu.py passes on nothing:

(a) every frame that file draws is finite on the fp32 oracle and shades between 10 % and 90 % of its pixels (`ortho`: at least 10 %);
(b) the sure-miss test of shade_pixel, restated in numpy from the constants a draw would use (atmo_debug_frame_constants on a host-only context), only
    ever fires where the oracle discards; it is live (miss_k > 0) for every depth-free kind from outside the shell and off (miss_k == 0) for `ortho`;
(c) the proxy's launch rectangle holds every pixel the float64 fragment test (tests/proxy_geometry.py) calls covered and is no larger than their
    bounding box grown by 3 pixels -- for `ortho` that is proxy_setup's branch for an eye that is a direction;
(d) atmo_plan_planets under the left eye's frustum and every other kind: planets that overlap on screen get different launches, planets clear of each other share one."""
import ctypes as C

import numpy as np
import pytest

import cameras as K
import proxy_geometry as G
from common import CONFIGS, demo_frame, demo_params, demo_textures, oracle_inputs
from godot_atmosphere_shader_amd import depth_formats as D
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame, make_frame
from test_planets_host import _draws, _plan
from test_views_proxy_host import _frame, _host_ctx, _mat

R, H = S.DEMO_PLANET_RADIUS, S.DEMO_ATMOSPHERE_HEIGHT
MIN_DEPTH_SHOWS = 0.10       # the share of an `ortho` frame's shaded pixels that D16 quantisation of its depth pattern must change


def shaded_share(frame):
    return float(np.any(frame != 0.0, axis=-1).mean())


@pytest.fixture(scope="module")
def lut(oracle32):
    return oracle32.bake_optical_depth(R, H, S.DEMO_SHADER_PARAMS["u_density"])


def oracle_frame(oracle, config, sampler, cam, depth, lut, factor=0.0):
    ocfg = CONFIGS[config][1]
    uses_lut = not ocfg.get("lite") and not ocfg.get("light_steps")
    cfg, tex = oracle_inputs(oracle, ocfg, demo_textures(), lut if uses_lut else None, declared=sampler == "declared")
    return oracle.render(demo_params(u_sphere_depth_factor=factor), tex, cfg, demo_frame(cam), depth, nthreads=8)[0]


# ---- the cameras themselves ---------------------------------------------------------------------------------------------------------------------------

def test_the_kinds_fill_the_elements_the_symmetric_camera_leaves_zero():
    """Column-major elements of the inverses, as include/atmo.h numbers them: what each kind is for."""
    plain = K.from_pose("plain", 96, 54, "P_space", up=(0.0, 1.0, 0.0))
    e = S.col_major(plain.inv_projection)
    assert e[8] == e[9] == e[10] == e[12] == e[13] == 0.0 and e[15] != 0.0 and e[11] != 0.0
    for kind in K.KINDS + ("rolled",):
        cam = K.from_pose(kind, 96, 54, "P_space", **(dict(ortho_size=300.0) if kind == "ortho" else {}))
        e = S.col_major(cam.inv_projection)
        assert np.allclose(cam.projection @ cam.inv_projection, np.eye(4), atol=1e-9) and np.allclose(cam.view @ cam.inv_view, np.eye(4), atol=1e-9)
        assert abs(cam.inv_view[0, 1]) > 0.05, kind                              # rolled: the camera's up vector leans out of the world's y
        if kind in ("eye_left", "eye_right", "jitter"):
            assert e[12] != 0.0 and e[13] != 0.0 and e[8] == e[9] == e[10] == 0.0, kind
        if kind == "infinite_far":
            assert e[15] == 0.0 and e[11] != 0.0 and e[8] == e[9] == e[10] == 0.0
        if kind == "ortho":
            assert e[10] != 0.0 and e[11] == 0.0 and e[15] == 1.0 and e[3] == e[7] == 0.0
    left, right = (K.from_pose(k, 96, 54, "P_space") for k in ("eye_left", "eye_right"))
    assert np.isclose(np.linalg.norm(right.inv_view[:3, 3] - left.inv_view[:3, 3]), K.IPD)
    assert np.allclose(right.inv_view[:3, 3] - left.inv_view[:3, 3], K.IPD * left.inv_view[:3, 0])
    assert np.isclose(left.projection[0, 2], -right.projection[0, 2]) and left.projection[0, 2] != 0.0 and left.projection[1, 2] == right.projection[1, 2] != 0.0
    # the left eye sees 1.3 : 0.7 to its left and right, 0.9 : 1.1 below and above
    d = left.pixel_view_dirs()
    tan = np.tan(np.radians(37.5))
    edge = lambda v, axis: v[axis] / -v[2]                                      # noqa: E731
    x0, x1 = edge(d[27, 0], 0) - (edge(d[27, 1], 0) - edge(d[27, 0], 0)) / 2, edge(d[27, 95], 0) + (edge(d[27, 95], 0) - edge(d[27, 94], 0)) / 2
    assert np.isclose(x0, -1.3 * tan * 96 / 54) and np.isclose(x1, 0.7 * tan * 96 / 54)
    y_top, y_bot = edge(d[0, 48], 1) + (edge(d[0, 48], 1) - edge(d[1, 48], 1)) / 2, edge(d[53, 48], 1) - (edge(d[52, 48], 1) - edge(d[53, 48], 1)) / 2
    assert np.isclose(y_top, 1.1 * tan) and np.isclose(y_bot, -0.9 * tan)
    # the jittered picture is the symmetric one moved by (+0.3, -0.2) pixel: the view ray of pixel (x, y) is the symmetric camera's at (x - 0.3, y + 0.2)
    sym, jit = K.from_pose("rolled", 96, 54, "P_space"), K.from_pose("jitter", 96, 54, "P_space")
    step_x = sym.pixel_view_dirs()[10, 11] - sym.pixel_view_dirs()[10, 10]
    step_y = sym.pixel_view_dirs()[11, 10] - sym.pixel_view_dirs()[10, 10]
    assert np.allclose(jit.pixel_view_dirs()[10, 10], sym.pixel_view_dirs()[10, 10] - 0.3 * step_x + 0.2 * step_y, atol=1e-12)


def test_ground_sphere_from_the_projection_is_the_scene_s_on_the_control_and_right_under_ortho():
    """cameras.depth_ground_sphere (the near-far segment, for any projection) against scene.depth_ground_sphere where that one applies, and, for every
    kind, against the definition: the texel unprojects to a point on the sphere."""
    for pose in ("P_space", "P_limb"):
        plain = K.from_pose("plain", 96, 54, pose, up=(0.0, 1.0, 0.0))
        assert np.array_equal(K.depth_ground_sphere(plain), S.depth_ground_sphere(plain))
        for kind in K.KINDS:
            cam = K.demo_camera(kind, pose)
            d = K.depth_ground_sphere(cam).astype(np.float64)
            ys, xs = np.nonzero(d)
            assert len(ys) > 0 and np.all((d >= 0.0) & (d <= 1.0)), (kind, pose)
            ndc = np.stack([(xs + 0.5) / cam.width * 2 - 1, (ys + 0.5) / cam.height * 2 - 1, d[ys, xs], np.ones(len(ys))], axis=-1)
            p = ndc @ (cam.inv_view @ cam.inv_projection).T
            r = np.linalg.norm(p[:, :3] / p[:, 3:4], axis=-1)
            assert np.abs(r - R).max() < 2e-3 * R, (kind, pose, float(np.abs(r - R).max()))     # (the texel is a float32)
    pat = K.depth_pattern(K.demo_camera("ortho", "P_space"))
    assert pat.min() >= 0.05 and pat.max() <= 0.95 and pat.std() > 0.2


# ---- (a) each frame is worth drawing -------------------------------------------------------------------------------------------------------------------

def test_every_single_draw_frame_is_finite_and_shades_a_share(oracle32, lut):
    low = {}
    for kind in K.SINGLE_KINDS + ("eye_right", "rolled"):
        for pose in K.POSE_SIZES:
            cam = K.demo_camera(kind, pose)
            depth = K.depth_of(cam)
            for factor in K.depth_factors(kind):
                shares = []
                for config, sampler in K.SINGLE_CONFIGS:
                    frame = oracle_frame(oracle32, config, sampler, cam, depth, lut, factor)
                    assert np.isfinite(frame).all(), (kind, pose, config, sampler, factor)
                    shares.append(shaded_share(frame))
                print(f"{kind} {pose} {cam.width} x {cam.height} factor {factor}: shaded {min(shares):.3f} .. {max(shares):.3f}, "
                      f"ground in the depth buffer {float((depth != 0).mean()):.3f}")
                if min(shares) < 0.10 or (kind != "ortho" and max(shares) > 0.90):
                    low[kind, pose, factor] = (min(shares), max(shares))
            # the cloud configurations draw clouds, and the two cubemap samplers differ: shares of the shaded pixels
            bare, lod1, lod0 = (oracle_frame(oracle32, c, s, cam, depth, lut) for c, s in (("no_clouds_8", "declared"), ("clouds_high", "declared"), ("clouds_high", "lod0")))
            shaded = np.any(bare != 0.0, axis=-1)
            clouds, samplers = float(np.any(bare != lod1, axis=-1)[shaded].mean()), float(np.any(lod1 != lod0, axis=-1)[shaded].mean())
            print(f"{kind} {pose}: clouds_high differs from no_clouds_8 on {clouds:.3f} of the shaded pixels, its declared sampler from level 0 on {samplers:.3f}")
            assert clouds >= 0.10 and samplers >= 0.05, (kind, pose, clouds, samplers)
    assert not low, low


def test_geometric_order_frames_have_a_silhouette(oracle32, lut):
    """The 353 x 201 frames of the geometric tile order hold a silhouette: part of the frame shades, part does not."""
    w, h = K.GEO_SIZE
    assert ((w + 15) // 16) * ((h + 7) // 8) >= 512                  # (smaller launches are left in row-major order by the tile-order policies)
    for kind in K.GEO_KINDS:
        for pose in K.POSE_SIZES:
            cam = K.demo_camera(kind, pose, K.GEO_SIZE)
            frame = oracle_frame(oracle32, "no_clouds_32x8_direct", "declared", cam, K.depth_of(cam), lut)
            rows = np.any(frame != 0.0, axis=(1, 2))
            print(f"{kind} {pose}: shaded {shaded_share(frame):.3f}, pixel rows that shade {int(rows.sum())} of {h}")
            assert 0.10 <= shaded_share(frame) <= 0.90 and np.isfinite(frame).all()


def test_ortho_depth_shows_in_the_frame(oracle32, lut):
    """Under `ortho` the ray depends on the depth sample: for every configuration the oracle's frame from the D16-quantised pattern differs from the frame
    from the float pattern on at least a tenth of the shaded pixels (no depth decoder is tested on nothing: tests/test_projections_gpu.py asserts the same
    share of the kernels' frames), and from the far-plane frame likewise (the v2 variants: on every shaded pixel); X8_D24 moves about one in eight of these float32 texels, D32F none."""
    for pose in K.POSE_SIZES:
        cam = K.demo_camera("ortho", pose)
        pat = K.depth_pattern(cam)
        for config, sampler in K.SINGLE_CONFIGS:
            b = oracle_frame(oracle32, config, sampler, cam, S.depth_far(cam), lut)
            c = oracle_frame(oracle32, config, sampler, cam, pat, lut)
            shares = []
            for fmt in ("d16", "x8d24", "d32f"):
                a = oracle_frame(oracle32, config, sampler, cam, D.decode(D.quantise(pat, fmt), fmt), lut)
                shaded = np.any(a != 0.0, axis=-1)
                vs_far = float(np.any(a.view(np.uint32) != b.view(np.uint32), axis=-1)[shaded].mean())
                shares.append(float(np.any(a.view(np.uint32) != c.view(np.uint32), axis=-1)[shaded].mean()))
                assert shaded.mean() >= 0.10 and vs_far >= MIN_DEPTH_SHOWS, (config, sampler, pose, fmt, vs_far)
            print(f"ortho {pose} {config} {sampler}: shaded {shaded.mean():.3f}; the frame from the decoded texels differs from the float pattern's on "
                  f"{shares[0]:.3f} (D16), {shares[1]:.3f} (X8_D24), {shares[2]:.3f} (D32F) of it")
            assert shares[0] >= MIN_DEPTH_SHOWS and shares[1] > 0.0 and shares[2] == 0.0, (config, sampler, pose, shares)


# ---- (b) the sure-miss test ---------------------------------------------------------------------------------------------------------------------------

def _frame_constants(cam):
    """(miss_k, rcp_vw, rcp_vh, the frame's float32 inv_projection, the planet's centre in view space) of a draw of the demo planet."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS)
    try:
        for name, v in (("u_planet_radius", R), ("u_atmosphere_height", H)):
            assert lib.atmo_set_param_f32(ctx, name.encode(), (C.c_float * 1)(v), 1) == N.ATMO_OK
        frame = _to_native_frame(make_frame(cam, np.eye(4), S.DEMO_SUN_POSITION))
        out = (C.c_float * 81)()
        assert lib.atmo_debug_frame_constants(ctx, C.byref(frame), 0, out, 81, None) == N.ATMO_OK
        got = np.array(out, dtype=np.float32)
        assert got[6] == np.float32(R + H)
        return got[75], got[76], got[77], np.array(frame.inv_projection_matrix, dtype=np.float32), np.array(frame.planet_center_viewspace, dtype=np.float32)
    finally:
        lib.atmo_destroy(ctx)


def _surely_misses(cam, miss_k, rcp_vw, rcp_vh, Q, c):
    """shade_pixel's inequality per pixel, three ways: in float32 with every multiply-add fused, in float32 with none fused (the compiler may contract
    the dot products either way), and in float64 with the right-hand side grown by 1e-5 -- which covers every float32 evaluation order: at the threshold
    the rounding of cv^2 is below 4e-7 / sqrt(k / |c|^2) <= 4e-6 of the right-hand side, since the host offers the test only for k > 0.01 |c|^2."""
    F = np.float32
    px, py = np.meshgrid(np.arange(cam.width, dtype=F) + F(0.5), np.arange(cam.height, dtype=F) + F(0.5))

    def fma(a, b, c_):
        return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c_, dtype=np.float64)).astype(F)

    fnx, fny = fma(px, F(rcp_vw + rcp_vw), F(-1.0)), fma(py, F(rcp_vh + rcp_vh), F(-1.0))
    a = [fma(np.full_like(fnx, Q[i]), fnx, fma(np.full_like(fny, Q[4 + i]), fny, Q[12 + i])) for i in range(3)]
    out = []
    # fused: cv = fma(c0, ax, fma(c1, ay, c2 az)), vv likewise
    cv = fma(np.full_like(fnx, c[0]), a[0], fma(np.full_like(fnx, c[1]), a[1], (c[2] * a[2]).astype(F)))
    vv = fma(a[0], a[0], fma(a[1], a[1], (a[2] * a[2]).astype(F)))
    out.append((cv * cv).astype(F) < (F(miss_k) * vv).astype(F))
    cv = ((c[0] * a[0]).astype(F) + (c[1] * a[1]).astype(F)).astype(F) + (c[2] * a[2]).astype(F)
    vv = ((a[0] * a[0]).astype(F) + (a[1] * a[1]).astype(F)).astype(F) + (a[2] * a[2]).astype(F)
    out.append((cv * cv).astype(F) < (F(miss_k) * vv).astype(F))
    a64 = [x.astype(np.float64) for x in a]
    cv = sum(float(c[i]) * a64[i] for i in range(3))
    vv = sum(a64[i] * a64[i] for i in range(3))
    out.append(cv * cv < float(miss_k) * vv * (1.0 + 1e-5))
    return out


def test_sure_miss_implies_the_oracle_s_discard(oracle32, lut):
    live = 0
    for kind in ("plain",) + K.KINDS + ("rolled",):
        for pose in ("P_space", "P_limb", "P_ground"):
            cam = K.demo_camera(kind, pose, K.POSE_SIZES.get(pose, (96, 54))) if kind != "ortho" else K.from_pose(kind, 96, 54, pose, ortho_size=300.0)
            miss_k, rcp_vw, rcp_vh, Q, c = _frame_constants(cam)
            assert rcp_vw == np.float32(1.0) / np.float32(cam.width) and rcp_vh == np.float32(1.0) / np.float32(cam.height)
            if kind == "ortho":
                assert miss_k == 0.0, (pose, miss_k)                 # the ray depends on the depth sample: the test is off
                continue
            if pose == "P_ground":
                assert miss_k == 0.0, (kind, miss_k)                 # inside the shell
                continue
            k = float(c.astype(np.float64) @ c.astype(np.float64)) - float(np.float32(R + H)) ** 2
            assert miss_k > 0.0 and np.isclose(miss_k, k * (1.0 - 1e-3) ** 2, rtol=1e-6), (kind, pose, miss_k, k)
            frame = oracle_frame(oracle32, "no_clouds_8", "declared", cam, K.depth_of(cam), lut)
            discards = np.all(frame == 0.0, axis=-1)
            fused, plain, wide = _surely_misses(cam, miss_k, rcp_vw, rcp_vh, Q, c)
            for name, sure in (("fused", fused), ("unfused", plain), ("float64 + 1e-5", wide)):
                assert not (sure & ~discards).any(), (kind, pose, name, int((sure & ~discards).sum()))
            print(f"{kind} {pose}: miss_k {miss_k:.6g}; the oracle discards {int(discards.sum())} of {discards.size} pixels, the sure-miss test takes "
                  f"{int(fused.sum())} of them ({int((discards & ~wide).sum())} go to the exact prologue)")
            assert fused.sum() >= 0.9 * discards.sum() > 0, (kind, pose)
            live += 1
    assert live == 12


# ---- (c) the proxy's launch rectangle -----------------------------------------------------------------------------------------------------------------

def _launch_rect(cam, model, size):
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx(N.VARIANT_NO_CLOUDS)
    try:
        rect, tiles = (C.c_int * 4)(), C.c_int(-1)
        rc = lib.atmo_debug_proxy_launch_rect(ctx, C.byref(_frame(cam)), _mat(model), C.c_float(size), rect, C.byref(tiles))
        assert rc == N.ATMO_OK, lib.atmo_last_error_string(ctx)
        return tuple(rect), tiles.value
    finally:
        lib.atmo_destroy(ctx)


def _covered(cam, model, size):
    ys, xs = np.meshgrid(np.arange(cam.height, dtype=np.float64), np.arange(cam.width, dtype=np.float64), indexing="ij")
    return G.coverage(cam, model, size, xs, ys)[0]


@pytest.mark.parametrize("kind", ("plain",) + K.KINDS)
def test_launch_rect_holds_every_covered_pixel_and_little_more(kind):
    for name, cam, model in K.proxy_poses(kind):
        size = K.proxy_box_size(cam.near)
        covered = _covered(cam, model, size)
        assert covered.any() and not covered.all(), (kind, name)
        (x0, y0, x1, y1), tiles = _launch_rect(cam, model, size)
        cy, cx = np.nonzero(covered)
        box = (int(cx.min()), int(cy.min()), int(cx.max()) + 1, int(cy.max()) + 1)
        print(f"{kind} {name}: {int(covered.sum())} covered pixels in {box}, launch rectangle {(x0, y0, x1, y1)}, {tiles} tiles")
        assert x0 <= box[0] and y0 <= box[1] and box[2] <= x1 and box[3] <= y1, (kind, name, (x0, y0, x1, y1), box)
        assert x0 >= max(box[0] - 3, 0) and y0 >= max(box[1] - 3, 0) and x1 <= min(box[2] + 3, cam.width) and y1 <= min(box[3] + 3, cam.height), \
            (kind, name, (x0, y0, x1, y1), box)
        assert tiles == ((x1 - x0 + 15) // 16) * ((y1 - y0 + 7) // 8)


def test_closed_form_coverage_matches_a_walk_under_ortho():
    """proxy_geometry.coverage was written with perspective cameras in mind: under `ortho` (w == 1 along the whole segment) a plain walk along each
    segment confirms it, on a coarse grid of every pose, away from the silhouette (the walk resolves it only to a fraction of a pixel)."""
    for name, cam, model in list(K.proxy_poses("ortho")) + [("draw", K.proxy_draw_camera("ortho"), np.eye(4))]:
        size = K.proxy_box_size(cam.near)
        ys, xs = np.meshgrid(np.arange(1, cam.height, 3, dtype=np.float64), np.arange(1, cam.width, 3, dtype=np.float64), indexing="ij")
        closed, _ = G.coverage(cam, model, size, xs, ys)
        walked = G.coverage_by_march(cam, model, size, xs, ys, n=2048)
        stable = np.ones_like(closed)
        for d in (0.02, -0.02):
            stable &= G.coverage(cam, model, size, xs + d, ys)[0] == closed
            stable &= G.coverage(cam, model, size, xs, ys + d)[0] == closed
        assert closed[stable].any() and np.array_equal(closed[stable], walked[stable]), name


def test_proxy_draw_frames_have_fragments_and_next_to_no_unstable_pixel(oracle32, lut):
    """The frames tests/test_projections_gpu.py draws through the box: at least 300 passing fragments, at most 1 % of the covered pixels within rounding
    distance of a decision (proxy_geometry.frame_masks), and at least 200 passing fragments that shade.  Under `ortho` the depth pattern occludes part of the box."""
    for kind in K.KINDS:
        cam = K.proxy_draw_camera(kind)
        depth = K.depth_of(cam)
        covered, passing, unstable = G.frame_masks(cam, np.eye(4), K.proxy_box_size(cam.near), depth)
        shaded = np.any(oracle_frame(oracle32, "clouds_high", "declared", cam, depth, lut) != 0.0, axis=-1)
        print(f"proxy {kind}: {int(covered.sum())} covered, {int(passing.sum())} passing, {int(unstable.sum())} unstable "
              f"({unstable.sum() / covered.sum():.4f} of the covered); {int((shaded & passing).sum())} passing fragments shade")
        assert passing.sum() >= 300 and unstable.sum() <= 0.01 * covered.sum() and (shaded & passing).sum() >= 200
        if kind == "ortho":
            assert passing.sum() <= 0.8 * covered.sum()                  # the depth test decides


# ---- (d) the planets' plan ------------------------------------------------------------------------------------------------------------------------------

def _bbox(mask):
    ys, xs = np.nonzero(mask)
    return int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1


@pytest.mark.parametrize("kind", K.KINDS)
def test_planets_plan(kind):
    """P and M overlap on screen, Q is clear of both by at least 8 pixels (float64 coverage of their boxes) -- under the left eye's frustum and under every
    other kind: in list order P, Q, M the plan is P and Q in one launch and M in the next; P and Q alone share one; P and M alone take two."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    cam = K.planets_camera(kind)
    depth = K.planets_depth(cam)
    boxes, specs, masks = {}, {}, {}
    ctxs = {n: _host_ctx(N.VARIANT_NO_CLOUDS) for n in K.PLANETS}
    try:
        for n, (pos, r, h) in K.PLANETS.items():
            size = K.proxy_box_size(cam.near, r, h)
            masks[n], passing, unstable = G.frame_masks(cam, G.translation(*pos), size, depth)
            boxes[n] = _bbox(masks[n])
            specs[n] = dict(ctx=ctxs[n], cam=cam, model=G.translation(*pos), size=size)
            print(f"planet {n} under {kind}: covered {int(masks[n].sum())} in {boxes[n]}, passing {int(passing.sum())}, unstable {int(unstable.sum())}")
            assert passing.sum() >= 300 and unstable.sum() <= 0.01 * masks[n].sum()

        def gap(a, b):
            return max(max(a[0], b[0]) - min(a[2], b[2]), max(a[1], b[1]) - min(a[3], b[3]))

        assert gap(boxes["P"], boxes["M"]) < 0 and (masks["P"] & masks["M"]).sum() >= 100
        assert gap(boxes["P"], boxes["Q"]) >= 8 and gap(boxes["M"], boxes["Q"]) >= 8
        for order, want in (("PQM", ([0, 0, 1], 2)), ("PQ", ([0, 0], 1)), ("PM", ([0, 1], 2)), ("MQP", ([0, 0, 1], 2))):
            assert _plan(lib, _draws([specs[n] for n in order]), len(order)) == want, (kind, order)
    finally:
        for ctx in ctxs.values():
            lib.atmo_destroy(ctx)
