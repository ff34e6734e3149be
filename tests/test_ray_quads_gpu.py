"""Caller-supplied rays in quads on the device (include/atmo_ray_quads.h).  Needs an MI355X.

(a) a camera's own rays in quad order (camera_ray_quads) shaded by shade_ray_quads are the camera's atmo_render frame under the DECLARED sampler, bit for bit,
    for the three cloud families; (b) the quad index -- width, first_quad -- picks the jitter atmo_render picks, and a batch cut anywhere is the same batch;
    (c) origins that differ per quad, against the fp32 oracle's declared-sampler frames of the cameras moved to those origins; (d) the derivative is the
    partners' and nothing else's; (e) the refusals that need a device.
The contexts are made as the library makes them by default: the declared sampler, a mip chain bound (common.make_node)."""
import functools

import numpy as np
import pytest
import torch

import step_count_cases as SC
from common import TOL, demo_params, demo_textures, make_node, oracle_inputs
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.demo import CONFIGS
from godot_atmosphere_shader_amd.planet_atmosphere import make_frame
from godot_atmosphere_shader_amd.ray_quads import quad_order, quads_to_image

pytestmark = pytest.mark.gpu

KF_RAYS = 16384
W, H = 113, 67                       # odd in both directions: absent slots in the last column and the last row; 1 938 quads, a partial last wave
IN_CLOUDS = "P_clouds"               # eye at radius 103.1, the layer spans 101.6 .. 104.8
POSES = ("P_space", IN_CLOUDS)
# label -> FLAGS of the twin atmo_render_kernel under the declared sampler (the demo configuration has the label's name)
FAMILIES = {"clouds_high": 49, "clouds_high_rm": 51, "v1_clouds": 57}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _node(label, **params):
    return make_node(label, demo_textures(), demo_params(**params))


def _render_lod0(node, cam, depth):
    """atmo_render's frame under atmo_set_sampler_lod(ctx, 0); the context goes back to its default sampler."""
    N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, 0))
    try:
        out = node.render(cam, depth)
        torch.cuda.synchronize()
    finally:
        N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, -1))
    return out


def _twin_name(label):
    return f"atmo_render_kernel<{FAMILIES[label]}, 0, 1>"


def _quads_name(label):
    return f"atmo_shade_rays_kernel<{FAMILIES[label] | KF_RAYS}, 0>"


def _to_quads(rays, w, h):
    """(h * w, 8) rays in row-major order -> quad order, all-zero rows for the slots outside the image."""
    order = torch.from_numpy(quad_order(w, h)).cuda()
    return torch.where((order >= 0)[:, None], rays[order.clamp(min=0)], torch.zeros((), device="cuda")).contiguous()


@functools.lru_cache(maxsize=None)
def _camera_and_depth(pose, w=W, h=H, fovy_deg=75.0):
    cam = S.Camera.from_pose(w, h, pose, fovy_deg=fovy_deg)
    depth = S.depth_ground_sphere(cam)      # a real depth buffer: the analytic ground sphere
    depth.setflags(write=False)
    return cam, depth


def _draw_both(node, label, cam, depth, w, h):
    """(atmo_render's frame under the default sampler, the quads' output in quad order), both as numpy float32; the kernel names asserted."""
    want = node.render(cam, depth)
    torch.cuda.synchronize()
    assert node.kernel_name == _twin_name(label), node.kernel_name
    quads = node.camera_ray_quads(cam, depth)
    slots = quad_order(w, h)
    assert tuple(quads.shape) == (slots.size, 8) and slots.size == 4 * ((w + 1) // 2) * ((h + 1) // 2)
    got = node.shade_ray_quads(quads, cam, width=w)
    torch.cuda.synchronize()
    assert node.kernel_name == _quads_name(label), node.kernel_name
    return want.cpu().numpy(), got.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _frames(label, factor):
    """Drawn once per (family, u_sphere_depth_factor) and shared, read only: pose -> (the declared atmo_render frame, the level-0 atmo_render frame, the
    quads' output in quad order) at 113 x 67."""
    node = _node(label, u_sphere_depth_factor=factor)
    out = {}
    try:
        for pose in POSES:
            cam, depth_np = _camera_and_depth(pose)
            depth = _dev(depth_np)
            want, got = _draw_both(node, label, cam, depth, W, H)
            lod0 = _render_lod0(node, cam, depth).cpu().numpy()
            for a in (want, got, lod0):
                a.setflags(write=False)
            out[pose] = (want, lod0, got)
    finally:
        node.close()
    return out


def _beyond(a, b, bar):
    """Per pixel: some channel differs by more than `bar` under the project's rule (absolute up to 1, relative above)."""
    return np.any(np.abs(a - b) > bar * np.maximum(1.0, np.abs(b)), axis=-1)


# ---- (a) camera quads are the camera's frame under the declared sampler, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("label", list(FAMILIES))
def test_camera_quads_shade_to_the_camera_s_declared_frame(label):
    """113 x 67, P_space and a camera inside the cloud layer, the ground sphere's depth buffer, u_sphere_depth_factor 0 and 0.35: camera_ray_quads, then
    shade_ray_quads(width=113), then quads_to_image equals the atmo_render frame under the default (declared) sampler as uint32 words, and the absent slots
    hold zeros.  Every frame must mean something: at least 30 % of its pixels shaded; from outside the shell at least one pixel discarded and the frame
    more than 100 x TOL away from the level-0 atmo_render frame on at least 5 % of the pixels; from inside the cloud layer (where the cubemap is magnified:
    the oracle shows no pixel beyond 100 x TOL there) different from it somewhere."""
    slots = quad_order(W, H)
    for factor in (0.0, 0.35):
        for pose, (want, lod0, got) in _frames(label, factor).items():
            shaded = np.any(want != 0.0, axis=-1)
            far, any_diff = _beyond(want, lod0, 100 * TOL), np.any(want != lod0, axis=-1)
            print(f"{label} {pose} f={factor}: {shaded.mean():.3f} shaded, {int((~shaded).sum())} discarded; against level 0: {far.mean():.4f} of the pixels "
                  f"beyond 100 x TOL, {any_diff.mean():.4f} differ at all, max {np.abs(want - lod0).max():.3f}")
            assert shaded.mean() >= 0.30, (label, pose, factor, float(shaded.mean()))
            if pose == "P_space":
                assert (~shaded).any(), (label, pose, factor)
                assert far.mean() >= 0.05, (label, pose, factor, float(far.mean()))
            else:
                assert any_diff.any(), (label, pose, factor)
            a, b = _bits(quads_to_image(got, W, H)), _bits(want)
            bad = (a != b).any(axis=-1)
            assert not bad.any(), (label, pose, factor, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert (slots < 0).sum() == 4 * 57 * 34 - W * H and not _bits(got)[slots < 0].any(), (label, pose, factor)


@pytest.mark.parametrize("size", [(1, 1, 75.0), (2, 2, 75.0), (3, 3, 75.0), (300, 5, 2.0)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_camera_quads_at_the_smallest_sizes(size):
    """clouds_high at 1 x 1 (one ray and three absent ones), 2 x 2 (one whole quad), 3 x 3 (absent slots in both directions) and 300 x 5 with a camera 2 degrees
    high (x beyond 255: the jitter's wrap in x; an odd height): the same equality.  (The 2-degree strip is 60 times as wide as high: the planet spans it.)"""
    w, h, fovy = size
    slots = quad_order(w, h)
    seen = False
    for factor in (0.0, 0.35):
        node = _node("clouds_high", u_sphere_depth_factor=factor)
        try:
            for pose in POSES:
                cam, depth_np = _camera_and_depth(pose, w, h, fovy)
                want, got = _draw_both(node, "clouds_high", cam, _dev(depth_np), w, h)
                assert np.array_equal(_bits(quads_to_image(got, w, h)), _bits(want)), (size, pose, factor)
                assert not _bits(got)[slots < 0].any(), (size, pose, factor)
                seen = seen or bool(want.any())
        finally:
            node.close()
    assert seen, size   # some frame of this size shades something


# ---- (b) index plumbing -------------------------------------------------------------------------------------------------------------------------------------
def test_width_and_first_quad_place_a_quad_in_the_image():
    """clouds_high, 300 x 5 (150 quads a row, three quad rows): a batch cut at quads 1, 15, 16 and 17 (around a wavefront's 16 quads) and shaded from there
    with first_quad = the cut is the rest of the whole batch; first_quad = 128 * qpr is first_quad = 0 (the jitter's wrap in y) and first_quad = qpr is
    not; one quad; a caller's output slice is filled in place."""
    w, h = 300, 5
    qpr = (w + 1) // 2
    cam, depth_np = _camera_and_depth("P_space", w, h, 2.0)
    node = _node("clouds_high")
    try:
        depth = _dev(depth_np)
        quads = node.camera_ray_quads(cam, depth)
        n_quads = quads.shape[0] // 4
        assert n_quads == qpr * 3
        whole = node.shade_ray_quads(quads, cam, width=w)
        torch.cuda.synchronize()
        assert node.kernel_name == _quads_name("clouds_high")
        want = node.render(cam, depth)
        assert np.array_equal(_bits(quads_to_image(whole, w, h)), _bits(want))
        assert np.any(_bits(want) != 0) and np.any(_bits(want)[:, 256:] != 0)
        for cut in (1, 15, 16, 17):
            part = node.shade_ray_quads(quads[4 * cut:], cam, width=w, first_quad=cut)
            assert np.array_equal(_bits(part), _bits(whole)[4 * cut:]), cut
        wrapped = node.shade_ray_quads(quads, cam, width=w, first_quad=128 * qpr)
        assert np.array_equal(_bits(wrapped), _bits(whole))
        shifted = node.shade_ray_quads(quads, cam, width=w, first_quad=qpr)
        assert not np.array_equal(_bits(shifted), _bits(whole))
        k = qpr + 65                          # a quad of the middle rows, in the planet's disc
        assert _bits(whole)[4 * k:4 * k + 4].any(axis=-1).all()
        one = node.shade_ray_quads(quads[4 * k:4 * k + 4], cam, width=w, first_quad=k)
        assert tuple(one.shape) == (4, 4) and np.array_equal(_bits(one), _bits(whole)[4 * k:4 * k + 4])
        out = torch.full((4 * n_quads + 2, 4), 0.25, dtype=torch.float32, device="cuda")
        assert node.shade_ray_quads(quads, cam, width=w, out=out[1:-1]).data_ptr() == out[1:-1].data_ptr()
        assert np.array_equal(_bits(out[1:-1]), _bits(whole)) and (out[0] == 0.25).all() and (out[-1] == 0.25).all()
    finally:
        node.close()


# ---- (c) origins per quad, against the oracle ------------------------------------------------------------------------------------------------------------------
OW, OH = 48, 27
# as tests/test_rays_gpu.py: everything dyadic, so that c - o_k, the moved camera position and the moved sun are exact in fp32 and both sides see the same inputs
EYE = np.array([0.375, 0.125, 158.0])
SUN = (0.0, 0.0, 478.75)
ORIGINS = np.array([[1.0, 0.5, -2.0], [-2.5, 1.25, 3.0], [4.0, -3.0, 8.0]])
ROW_ORIGIN = (np.arange(OH) // 2) % 3      # row pair r (rows 2 r and 2 r + 1) is dealt origin o_(r mod 3): whole quads per origin


def _axis_camera(eye):
    cam = S.Camera.from_pose(OW, OH, dict(eye=tuple(eye), target=(eye[0], eye[1], 0.0)))
    assert np.array_equal(cam.inv_view[:3, :3], np.eye(3)) and np.array_equal(cam.inv_view[:3, 3], eye)
    return cam


@functools.lru_cache(maxsize=None)
def _origin_oracle_frames(label, declared):
    """The fp32 oracle's 48 x 27 frames of the camera moved to EYE + o_k, k = 0, 1, 2 (u_sphere_depth_factor 1: no depth read), under the declared or the
    level-0 sampler."""
    from oracle.oracle import Oracle

    oracle = Oracle("f32")
    cfg = dict(CONFIGS[label][1])
    uses_lut = not cfg.get("lite") and not cfg.get("light_steps")
    ocfg, otex = oracle_inputs(oracle, cfg, demo_textures(), SC._lut(oracle) if uses_lut else None, declared=declared)
    frames = []
    for o in ORIGINS:
        cam = _axis_camera(EYE + o)
        frame = make_frame(cam, np.eye(4), SUN)
        assert np.array_equal(frame["planet_center_viewspace"].astype(np.float64), -(EYE + o))
        img, _ = oracle.render(demo_params(u_sphere_depth_factor=1.0), otex, ocfg, frame, S.depth_far(cam), nthreads=8)
        img.setflags(write=False)
        frames.append(img)
    return frames


@pytest.mark.parametrize("label", list(FAMILIES))
def test_origins_per_quad_match_the_oracle(label):
    """Row pairs are dealt to three origins; directions from camera_rays of the unmoved camera, put in quad order.  Expected, row for row: the oracle's
    declared-sampler frame of the camera moved by that origin.  Zero sets and finite sets equal, then the project's 1e-4 rule (absolute up to 1, relative
    above)."""
    want3, lod3 = _origin_oracle_frames(label, True), _origin_oracle_frames(label, False)
    want = np.stack([want3[k][y] for y, k in enumerate(ROW_ORIGIN)])
    # on the CPU: the frames hold something, the sampler matters on the very rows an origin is dealt, and the three origins give three pictures there
    for k in range(3):
        shaded = np.any(want3[k] != 0.0, axis=-1).mean()
        rows = ROW_ORIGIN == k
        far = _beyond(want3[k][rows], lod3[k][rows], 100 * TOL).mean()
        print(f"{label} origin {k}: {shaded:.3f} shaded; declared against level 0 on its rows: {far:.4f} of the pixels beyond 100 x TOL")
        assert shaded >= 0.30, (label, k, shaded)
        assert far >= 0.05, (label, k, far)
        for j in range(3):
            if j != k:
                assert np.abs(want3[k][rows] - want3[j][rows]).max() > 100 * TOL, (label, k, j)
    node = make_node(label, demo_textures(), demo_params(u_sphere_depth_factor=1.0))
    try:
        node.set_shader_parameter("u_sun_position", SUN)
        cam = _axis_camera(EYE)
        rays = node.camera_rays(cam, _dev(S.depth_far(cam)))
        moved = rays.clone().reshape(OH, OW, 8)
        moved[:, :, 0:3] = torch.from_numpy(ORIGINS[ROW_ORIGIN].astype(np.float32)).cuda()[:, None, :]
        got = node.shade_ray_quads(_to_quads(moved.reshape(-1, 8), OW, OH), cam, width=OW)
        torch.cuda.synchronize()
        assert node.kernel_name == _quads_name(label), node.kernel_name
        got = quads_to_image(got.cpu().numpy(), OW, OH)
        # the same rays from the unmoved origin are another picture: the origins reached the kernel
        unmoved = quads_to_image(node.shade_ray_quads(_to_quads(rays, OW, OH), cam, width=OW).cpu().numpy(), OW, OH)
        assert np.abs(unmoved - got).max() > 100 * TOL
    finally:
        node.close()
    assert np.array_equal(np.all(got == 0.0, axis=-1), np.all(want == 0.0, axis=-1)), label
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), label
    err = SC.rel_err(got, want)
    print(f"\n{label}: origins per quad, max err vs the declared-sampler oracle {err:.3e} (bar {TOL:.0e})")
    assert err <= TOL, (label, err)


# ---- (d) the derivative is the partners' and nothing else's ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["clouds_high", "clouds_high_rm"])
def test_the_derivative_is_the_partners(label):
    """113 x 67, P_space.  The slot-0 ray of each quad put into all four slots, slot 0's results against the level-0 shade_rays of the same pixels (same
    pixel, same jitter): zero sets equal, within TOL; whether bit for bit is printed.  The same slot-0 rays inside their true camera quads differ from that
    by more than 100 x TOL on at least 3 % of the slot-0 pixels."""
    cam, depth_np = _camera_and_depth("P_space")
    pixel0 = quad_order(W, H)[0::4]          # slot 0 of every quad lies inside the image
    assert (pixel0 >= 0).all()
    node = _node(label)
    try:
        depth = _dev(depth_np)
        quads = node.camera_ray_quads(cam, depth)
        same = quads.reshape(-1, 4, 8)[:, 0:1, :].expand(-1, 4, -1).reshape(-1, 8).contiguous()
        got = node.shade_ray_quads(same, cam, width=W)
        torch.cuda.synchronize()
        assert node.kernel_name == _quads_name(label), node.kernel_name
        got0 = got.cpu().numpy()[0::4]
        level0 = node.shade_rays(node.camera_rays(cam, depth), cam, width=W)
        torch.cuda.synchronize()
        assert node.kernel_name == f"atmo_shade_rays_kernel<{(FAMILIES[label] & ~32) | KF_RAYS}, 0>", node.kernel_name
        want0 = level0.cpu().numpy()[pixel0]
    finally:
        node.close()
    true0 = _frames(label, 0.0)["P_space"][2][0::4]      # the same rays inside their true camera quads: (a)'s output
    err = SC.rel_err(got0, want0)
    equal = np.array_equal(_bits(got0), _bits(want0))
    off = _beyond(got0, want0, TOL)
    far = _beyond(true0, got0, 100 * TOL)
    print(f"\n{label}: four equal rays a quad against level-0 shade_rays: max err {err:.3e}, {int(off.sum())} of {off.size} slot-0 pixels beyond TOL, "
          f"bit for bit: {equal}; true camera quads against them: {far.mean():.4f} of the slot-0 pixels beyond 100 x TOL")
    assert np.array_equal(np.all(got0 == 0.0, axis=-1), np.all(want0 == 0.0, axis=-1)), label
    assert err <= TOL, (label, err)
    assert far.mean() >= 0.03, (label, float(far.mean()))


# ---- (e) the refusals that need a device ---------------------------------------------------------------------------------------------------------------------------
def test_device_only_refusals():
    """Under mode -1 with no chain bound (the cubemap given as its level 0 alone) the call is refused and the message names atmo_shade_rays; under mode 0 it is
    refused; back under mode -1 with a chain bound the context draws again, with the bytes of (a)."""
    from godot_atmosphere_shader_amd._native import AtmoError

    cam, depth_np = _camera_and_depth("P_space")
    depth = _dev(depth_np)
    tex = dict(demo_textures())
    tex["cubemap"] = [np.asarray(tex["cubemap"])]          # a list of levels: level 0 is all there is
    bare = make_node("clouds_high", tex, demo_params())
    try:
        quads = bare.camera_ray_quads(cam, depth)
        with pytest.raises(AtmoError, match=r"atmo_shade_ray_quads: no mip chain .*atmo_set_sampler_lod -1.*atmo_shade_rays") as e:
            bare.shade_ray_quads(quads, cam, width=W)
        assert e.value.code == N.ATMO_E_STATE
    finally:
        bare.close()
    node = _node("clouds_high")
    try:
        quads = node.camera_ray_quads(cam, depth)
        N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, 0))
        with pytest.raises(AtmoError, match=r"atmo_shade_ray_quads: .*atmo_set_sampler_lod 0.*atmo_shade_rays") as e:
            node.shade_ray_quads(quads, cam, width=W)
        assert e.value.code == N.ATMO_E_STATE
        N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, -1))
        again = node.shade_ray_quads(quads, cam, width=W)
        assert np.array_equal(_bits(again), _bits(_frames("clouds_high", 0.0)["P_space"][2])) and _bits(again).any()
    finally:
        node.close()
