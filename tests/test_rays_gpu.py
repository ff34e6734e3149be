"""Caller-supplied rays on the device (include/atmo_rays.h).  Needs an MI355X.

(a) a camera's own rays (camera_rays) shaded by shade_rays are the camera's atmo_render frame under the level-0 sampler, bit for bit, for all seven ray
    kernels; (b) the image index -- width, first -- picks the jitter atmo_render picks, and a batch cut anywhere is the same batch; (c) origins that
    differ per ray, against the fp32 oracle's frames of the cameras moved to those origins; (d) the sampler modes.
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

pytestmark = pytest.mark.gpu

KF_RAYS = 16384
W, H = 113, 67                       # 7 571 rays: a partial last wave, a width that is no multiple of 16
IN_CLOUDS = "P_clouds"               # eye at radius 103.1, the layer spans 101.6 .. 104.8
# label -> (demo configuration, make_node keywords, FLAGS of the twin atmo_render_kernel under the level-0 sampler, LSTEPS, the cloudless twin's label)
FAMILIES = {
    "lut": ("no_clouds_8", {}, 0, 0, None),
    "direct8": ("no_clouds_8", dict(view_steps=32, light_mode="direct", light_steps=8), 4, 8, None),
    "direct5": ("no_clouds_8", dict(view_steps=32, light_mode="direct", light_steps=5), 4, 0, None),
    "clouds_high": ("clouds_high", {}, 17, 0, "lut"),
    "clouds_high_rm": ("clouds_high_rm", {}, 19, 0, "lut"),
    "v1_no_clouds": ("v1_no_clouds", {}, 24, 0, None),
    "v1_clouds": ("v1_clouds", {}, 25, 0, "v1_no_clouds"),
}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _node(label, **params):
    config, kw, _, _, _ = FAMILIES[label]
    return make_node(config, demo_textures(), demo_params(**params), **kw)


def _render_lod0(node, cam, depth):
    """atmo_render's frame under atmo_set_sampler_lod(ctx, 0); the context goes back to its default sampler."""
    N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, 0))
    try:
        out = node.render(cam, depth)
        torch.cuda.synchronize()
        name = node.kernel_name
    finally:
        N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, -1))
    return out, name


def _rays_name(label):
    return f"atmo_shade_rays_kernel<{FAMILIES[label][2] | KF_RAYS}, {FAMILIES[label][3]}>"


@functools.lru_cache(maxsize=None)
def _camera_and_depth(pose, w=W, h=H, fovy_deg=75.0):
    cam = S.Camera.from_pose(w, h, pose, fovy_deg=fovy_deg)
    depth = S.depth_ground_sphere(cam)      # a real depth buffer: the analytic ground sphere
    depth.setflags(write=False)
    return cam, depth


_cloudless = {}


def _cloudless_frame(label, pose, factor):
    """The level-0 atmo_render frame of a cloudless family, drawn once per (family, pose, factor) and shared; read only."""
    key = (label, pose, factor)
    if key not in _cloudless:
        node = _node(label, u_sphere_depth_factor=factor)
        try:
            cam, depth = _camera_and_depth(pose)
            _cloudless[key] = _render_lod0(node, cam, _dev(depth))[0].cpu().numpy()
        finally:
            node.close()
    return _cloudless[key]


# ---- (a) camera rays are the camera's frame, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(FAMILIES))
def test_camera_rays_shade_to_the_camera_s_frame(label):
    """113 x 67, P_space and a camera inside the cloud layer, the ground sphere's depth buffer, u_sphere_depth_factor 0 and 0.35: camera_rays, then
    shade_rays(width=113), equals the atmo_render frame under the level-0 sampler as uint32 words.  Every frame must mean something: at least 30 % of its
    pixels non-zero; from outside the shell at least one pixel discarded (from inside it no ray can miss the shell: h = R^2 - |qc|^2 >= 0 for every
    direction, so the pose inside the cloud layer has no discarded pixel to show); a cloud family differs from its cloudless twin on at least 10 %."""
    _, _, flags, lsteps, cloudless = FAMILIES[label]
    for factor in (0.0, 0.35):
        node = _node(label, u_sphere_depth_factor=factor)
        try:
            for pose in ("P_space", IN_CLOUDS):
                cam, depth_np = _camera_and_depth(pose)
                depth = _dev(depth_np)
                want, twin = _render_lod0(node, cam, depth)
                assert twin == f"atmo_render_kernel<{flags}, {lsteps}, 1>", twin
                rays = node.camera_rays(cam, depth)
                assert tuple(rays.shape) == (W * H, 8)
                got = node.shade_rays(rays, cam, width=W)
                torch.cuda.synchronize()
                assert node.kernel_name == _rays_name(label), node.kernel_name
                r = rays.cpu().numpy()
                assert not r[:, :3].any() and not r[:, 7].any() and np.allclose(np.linalg.norm(r[:, 4:7], axis=1), 1.0, atol=1e-6)
                frame = want.cpu().numpy()
                shaded = np.any(frame != 0.0, axis=-1)
                print(f"{label} {pose} f={factor}: {shaded.mean():.3f} shaded, {int((~shaded).sum())} discarded")
                assert shaded.mean() >= 0.30, (label, pose, factor, float(shaded.mean()))
                if pose == "P_space":
                    assert (~shaded).any(), (label, pose, factor)
                if cloudless is not None:
                    differ = np.any(frame != _cloudless_frame(cloudless, pose, factor), axis=-1)
                    print(f"    {differ.mean():.3f} of the pixels differ from the {cloudless} frame")
                    assert differ.mean() >= 0.10, (label, pose, factor, float(differ.mean()))
                a, b = _bits(got).reshape(H, W, 4), _bits(want)
                bad = (a != b).any(axis=-1)
                assert not bad.any(), (label, pose, factor, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        finally:
            node.close()


# ---- (b) index plumbing -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["lut", "clouds_high"])
def test_width_and_first_place_a_ray_in_the_image(label):
    """A 300 x 5 viewport (x beyond 255: the jitter's wrap in x) bit for bit against atmo_render; a batch cut at rays 1, 63, 64 and 65 and shaded from
    there with first = the cut is the rest of the whole batch; first = 256 * width is first = 0 (the wrap in y) and first = width is not; one ray."""
    w, h = 300, 5
    cam, depth_np = _camera_and_depth("P_space", w, h, 2.0)   # (2 degrees high and 60 times as wide: the planet spans columns 17 .. 283)
    node = _node(label)
    try:
        depth = _dev(depth_np)
        want, _ = _render_lod0(node, cam, depth)
        rays = node.camera_rays(cam, depth)
        whole = node.shade_rays(rays, cam, width=w)
        torch.cuda.synchronize()
        assert node.kernel_name == _rays_name(label)
        assert np.array_equal(_bits(whole).reshape(h, w, 4), _bits(want))
        assert np.any(_bits(want) != 0) and np.any(_bits(want)[:, 256:] != 0)
        for cut in (1, 63, 64, 65):
            part = node.shade_rays(rays[cut:], cam, width=w, first=cut)
            assert np.array_equal(_bits(part), _bits(whole)[cut:]), cut
        wrapped = node.shade_rays(rays, cam, width=w, first=256 * w)
        assert np.array_equal(_bits(wrapped), _bits(whole))
        shifted = node.shade_rays(rays, cam, width=w, first=w)
        assert not np.array_equal(_bits(shifted), _bits(whole))
        k = 2 * w + 131                       # a shaded pixel of the middle row
        assert _bits(whole)[k].any()
        one = node.shade_rays(rays[k:k + 1], cam, width=w, first=k)
        assert tuple(one.shape) == (1, 4) and np.array_equal(_bits(one), _bits(whole)[k:k + 1])
        # an output of the caller's is filled in place, and nothing is written beside it
        out = torch.full((w * h + 2, 4), 0.25, dtype=torch.float32, device="cuda")
        assert node.shade_rays(rays, cam, width=w, out=out[1:-1]).data_ptr() == out[1:-1].data_ptr()
        assert np.array_equal(_bits(out[1:-1]), _bits(whole)) and (out[0] == 0.25).all() and (out[-1] == 0.25).all()
    finally:
        node.close()


# ---- (c) origins per ray, against the oracle ----------------------------------------------------------------------------------------------------------------
OW, OH = 48, 27
# Everything dyadic, so that c - o_k, the moved camera position and the moved sun are exact in fp32 and both sides see the same inputs: P_space's eye rounded
# to a few mantissa bits (the camera looks down -Z with an identity rotation), the sun on the z axis, three origins in view space = world directions
EYE = np.array([0.375, 0.125, 158.0])
SUN = (0.0, 0.0, 478.75)
ORIGINS = np.array([[1.0, 0.5, -2.0], [-2.5, 1.25, 3.0], [4.0, -3.0, 8.0]])
# label -> (demo configuration, make_node keywords, the oracle's step-count config)
ORIGIN_SHADERS = {"lut": ("no_clouds_8", {}, dict(view_steps=8)),
                  "direct": ("no_clouds_8", dict(view_steps=32, light_mode="direct", light_steps=8), dict(view_steps=32, light_steps=8)),   # 32 x 8
                  "clouds_high": ("clouds_high", {}, dict(CONFIGS["clouds_high"][1]))}


def _axis_camera(eye):
    cam = S.Camera.from_pose(OW, OH, dict(eye=tuple(eye), target=(eye[0], eye[1], 0.0)))
    assert np.array_equal(cam.inv_view[:3, :3], np.eye(3)) and np.array_equal(cam.inv_view[:3, 3], eye)
    return cam


@functools.lru_cache(maxsize=None)
def _origin_oracle_frames(shader):
    """The fp32 oracle's 48 x 27 frames of the camera moved to EYE + o_k, k = 0, 1, 2 (u_sphere_depth_factor 1: no depth read), level-0 sampler."""
    from oracle.oracle import Oracle

    oracle = Oracle("f32")
    cfg = dict(ORIGIN_SHADERS[shader][2])
    uses_lut = not cfg.get("lite") and not cfg.get("light_steps")
    ocfg, otex = oracle_inputs(oracle, cfg, demo_textures(), SC._lut(oracle) if uses_lut else None, declared=False)
    frames = []
    for o in ORIGINS:
        cam = _axis_camera(EYE + o)
        frame = make_frame(cam, np.eye(4), SUN)
        # what the moved camera sees is what the ray's origin moves: c - o_k and the sun moved likewise, exactly
        base = make_frame(_axis_camera(EYE), np.eye(4), SUN)
        assert np.array_equal(frame["planet_center_viewspace"], (base["planet_center_viewspace"].astype(np.float64) - o).astype(np.float32))
        assert np.array_equal(frame["sun_center_viewspace"], (base["sun_center_viewspace"].astype(np.float64) - o).astype(np.float32))
        assert np.array_equal(frame["planet_center_viewspace"].astype(np.float64), -(EYE + o))
        img, _ = oracle.render(demo_params(u_sphere_depth_factor=1.0), otex, ocfg, frame, S.depth_far(cam), nthreads=8)
        img.setflags(write=False)
        frames.append(img)
    return frames


@pytest.mark.parametrize("shader", list(ORIGIN_SHADERS))
def test_origins_per_ray_match_the_oracle(shader):
    """The frame's rows are dealt to three origins (row y: o_(y mod 3)); directions from camera_rays of the unmoved camera.  Expected, row for row: the
    oracle's frame of the camera moved by that origin.  Zero sets and finite sets equal, then the project's 1e-4 rule (absolute up to 1, relative above)."""
    want3 = _origin_oracle_frames(shader)
    rows = np.arange(OH) % 3
    want = np.stack([want3[k][y] for y, k in enumerate(rows)])
    # on the CPU: the oracle's frames hold something, and the three origins give three different pictures on the very rows they are dealt
    for k in range(3):
        assert np.any(want3[k] != 0.0, axis=-1).mean() >= 0.30, (shader, k)
        for j in range(3):
            if j != k:
                assert np.abs(want3[k][rows == k] - want3[j][rows == k]).max() > 100 * TOL, (shader, k, j)
    node = make_node(ORIGIN_SHADERS[shader][0], demo_textures(), demo_params(u_sphere_depth_factor=1.0), **ORIGIN_SHADERS[shader][1])
    try:
        node.set_shader_parameter("u_sun_position", SUN)
        cam = _axis_camera(EYE)
        rays = node.camera_rays(cam, _dev(S.depth_far(cam)))
        moved = rays.clone().reshape(OH, OW, 8)
        moved[:, :, 0:3] = torch.from_numpy(ORIGINS[rows].astype(np.float32)).cuda()[:, None, :]
        got = node.shade_rays(moved.reshape(-1, 8), cam, width=OW)
        torch.cuda.synchronize()
        assert str(KF_RAYS | {"lut": 0, "direct": 4, "clouds_high": 17}[shader]) in node.kernel_name, node.kernel_name
        got = got.cpu().numpy().reshape(OH, OW, 4)
        # the same rays from the unmoved origin are another picture: the origins reached the kernel
        unmoved = node.shade_rays(rays, cam, width=OW).cpu().numpy().reshape(OH, OW, 4)
        assert np.abs(unmoved - got).max() > 100 * TOL
    finally:
        node.close()
    assert np.array_equal(np.all(got == 0.0, axis=-1), np.all(want == 0.0, axis=-1)), shader
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), shader
    err = SC.rel_err(got, want)
    print(f"\n{shader}: origins per ray, max err vs oracle {err:.3e} (bar {TOL:.0e})")
    assert err <= TOL, (shader, err)


# ---- (d) sampler modes ------------------------------------------------------------------------------------------------------------------------------------------
def test_sampler_modes():
    """Rays sample the coverage cubemap at level 0: the default sampler mode (-1, a chain bound) and mode 0 give the same bytes; mode 1 with the chain bound is
    refused, naming the mode, and the context draws again once it is taken back."""
    from godot_atmosphere_shader_amd._native import AtmoError

    cam, depth_np = _camera_and_depth("P_space")
    node = _node("clouds_high")
    try:
        depth = _dev(depth_np)
        rays = node.camera_rays(cam, depth)
        default = node.shade_rays(rays, cam, width=W)
        N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, 0))
        level0 = node.shade_rays(rays, cam, width=W)
        assert np.array_equal(_bits(default), _bits(level0)) and _bits(default).any()
        N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, 1))
        with pytest.raises(AtmoError, match=r"atmo_shade_rays: .*atmo_set_sampler_lod 1") as e:
            node.shade_rays(rays, cam, width=W)
        assert e.value.code == N.ATMO_E_STATE
        N.check(node._ctx, node._lib.atmo_set_sampler_lod(node._ctx, -1))
        assert np.array_equal(_bits(node.shade_rays(rays, cam, width=W)), _bits(default))
    finally:
        node.close()
