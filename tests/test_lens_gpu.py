"""Lens rays on the device (include/atmo_lens.h).  Needs an MI355X.

(1) the kernels against the numpy statement (godot_atmosphere_shader_amd/lens.py): OCTAHEDRAL and CUBE_FACE byte for byte, EQUIRECT and FISHEYE within 1
    float32 ulp per direction component and byte for byte in everything else; (2) the distance buffer; (3) the tile index, and shading through it; (4) one
    semantic pin against the fp32 oracle: the -Z cube face under diag(-1, 1, 1) is a square 90-degree pinhole; (5) render_lens; (6) a graph capture.
The working sizes are 37 x 19 and 19 x 19: both odd -- absent quad slots, ragged tiles, the rho == 0 pixel, pixels outside the circle."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import step_count_cases as SC
from common import TOL, demo_params, demo_textures, make_node, oracle_inputs
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import lens as L
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.demo import CONFIGS
from godot_atmosphere_shader_amd.lens import Lens
from godot_atmosphere_shader_amd.planet_atmosphere import make_frame
from godot_atmosphere_shader_amd.ray_quads import quads_to_image

pytestmark = pytest.mark.gpu

W, H, BAND = 37, 19, (2, 12)
SENTINEL = 0.25
ORIGIN = (1.5, -2.25, 0.125)


def _rotation():
    """A generic rotation, float32: about (1, 2, 3) by 0.7 radians."""
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + math.sin(0.7) * k + (1 - math.cos(0.7)) * (k @ k)).astype(np.float32)


PERMUTATION = np.float32([[0, 0, -1], [1, 0, 0], [0, -1, 0]])      # a signed permutation: exact under BASIS


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _ordered(a):
    """float32 -> integers whose difference counts ulps (+0 and -0 are both 0)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


@pytest.fixture(scope="module")
def lut_node():
    node = make_node("no_clouds_8", demo_textures(), demo_params())
    yield node
    node.close()


def _cases(lens_of):
    """(lens, quads) over the band and the whole image, both orders, the given bases."""
    for rows in (BAND, None):
        for quads in (False, True):
            yield lens_of(rows), quads


# ---- 1. the device against the statement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["octahedral", "cube_face"])
def test_fp32_lenses_are_the_statement_s_bytes(lut_node, kind):
    for basis in (None, _rotation()):
        kw = dict(basis=basis, origin=ORIGIN, tmax=7.5)
        lenses = [lambda rows: Lens.octahedral(W, H, rows=rows, **kw)] if kind == "octahedral" else [
            functools.partial(lambda face, rows: Lens.cube_face(H, face, rows=rows, **kw), face) for face in range(6)]
        for lens_of in lenses:
            for lens, quads in _cases(lens_of):
                got = lut_node.lens_rays(lens, quads=quads)
                torch.cuda.synchronize()
                want = L.lens_rays(lens, quads=quads)
                assert tuple(got.shape) == want.shape and got.cpu().numpy().tobytes() == want.tobytes(), (lens, quads, basis is None)


@pytest.mark.parametrize("kind", ["equirect", "fisheye180", "fisheye220"])
def test_trigonometric_lenses_are_within_an_ulp(lut_node, kind):
    differ = total = 0
    for basis in (None, PERMUTATION):
        kw = dict(basis=basis, origin=ORIGIN, tmax=7.5)
        for lens, quads in _cases(lambda rows: Lens.equirect(W, H, rows=rows, **kw) if kind == "equirect" else
                                  Lens.fisheye(W, H, fov=math.radians(float(kind[7:])), rows=rows, **kw)):
            got = lut_node.lens_rays(lens, quads=quads).cpu().numpy()
            want = L.lens_rays(lens, quads=quads)
            assert got.shape == want.shape
            absent = ~np.any(want[:, 4:7] != 0, axis=1)
            assert got[:, [0, 1, 2, 3, 7]].tobytes() == want[:, [0, 1, 2, 3, 7]].tobytes(), (lens, quads)      # origin, tmax, the reserved float
            assert got[absent].tobytes() == want[absent].tobytes() and (quads or kind != "equirect" or not absent.any())
            ulps = np.abs(_ordered(got[:, 4:7]) - _ordered(want[:, 4:7]))
            assert ulps.max() <= 1, (lens, quads, int(ulps.max()), np.argwhere(ulps > 1)[:4].tolist())
            differ, total = differ + int((ulps != 0).sum()), total + 3 * int((~absent).sum())
    print(f"{kind}: {differ} of {total} direction components differ from the float64 statement's rounding, each by 1 ulp")
    if kind != "equirect":      # the rho == 0 pixel of the whole image, identity basis
        centre = lut_node.lens_rays(Lens.fisheye(W, H, fov=3.0)).cpu().numpy()[(H // 2) * W + W // 2]
        assert centre[4:7].tolist() == [0.0, 0.0, -1.0]


# ---- 2. the distance buffer ------------------------------------------------------------------------------------------------------------------------------------
def test_distance_buffer_gives_every_ray_its_own_texel(lut_node):
    dist = np.arange(H * (W + 5), dtype=np.float32).reshape(H, W + 5) * 0.5 + 1.0
    dist[3, 15] = dist[11, 20] = L.FLT_MAX
    dev = torch.from_numpy(dist).cuda()
    for lens in (Lens.fisheye(W, H, rows=BAND), Lens.octahedral(W, H), Lens.octahedral(W, H, rows=BAND)):
        for quads in (False, True):
            got = lut_node.lens_rays(lens, distance=dev, quads=quads).cpu().numpy()
            want = L.lens_rays(lens, quads=quads, distance=dist)
            assert got[:, :4].tobytes() == want[:, :4].tobytes(), (lens, quads)
            assert (want[:, 3] == np.float32(L.FLT_MAX)).sum() == 2
    # a pitch that is not the tensor's width: a view of a wider buffer
    wide = torch.zeros((H, W + 9), dtype=torch.float32, device="cuda")
    wide[:, :W + 5] = dev
    got = lut_node.lens_rays(Lens.octahedral(W, H), distance=wide[:, :W + 2]).cpu().numpy()
    assert got[:, 3].tobytes() == dist[:, :W].tobytes()


# ---- 3. the tile index ---------------------------------------------------------------------------------------------------------------------------------------------
def _fisheye_lens(rows=None):
    return Lens.fisheye(W, H, fov=math.radians(200.0), rows=rows)


@pytest.mark.parametrize("config", ["no_clouds_8", "clouds_high"])
def test_tile_index_and_shading_through_it(config):
    cam = S.Camera.from_pose(W, H, "P_space")
    node = make_node(config, demo_textures(), demo_params())
    try:
        for rows in (None, BAND):
            lens = _fisheye_lens(rows)
            y0, y1 = lens.rows
            rays, index = node.lens_rays(lens, tile_index=True)
            torch.cuda.synchronize()
            want_index = L.lens_tile_index(lens)
            assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy().view(np.uint32), want_index)
            plain_rays = node.lens_rays(lens)
            assert np.array_equal(_bits(rays), _bits(plain_rays))      # the tile map writes the rays where the row-major map does
            plain = node.shade_rays(plain_rays, cam, width=W, first=y0 * W)
            out = torch.full(((y1 - y0) * W, 4), SENTINEL, dtype=torch.float32, device="cuda")
            node.shade_rays(rays, cam, width=W, first=y0 * W, out=out, index=index)
            torch.cuda.synchronize()
            assert "indexed" in node.kernel_name
            listed = np.zeros((y1 - y0) * W, dtype=bool)
            listed[want_index[want_index != L.LIST_END]] = True
            assert 0 < listed.sum() < listed.size
            got, want = _bits(out), _bits(plain)
            assert np.array_equal(got[listed], want[listed]) and want[listed].any()
            assert (out.cpu().numpy()[~listed] == SENTINEL).all()
    finally:
        node.close()


# ---- 4. one semantic pin against the oracle ----------------------------------------------------------------------------------------------------------------------
PN = 48
EYE = np.array([0.375, 0.125, 158.0])      # dyadic, as tests/test_rays_gpu.py's: both sides see the same centre
SUN = (0.0, 0.0, 478.75)
PIN_SHADERS = {"lut": ("no_clouds_8", {}, dict(view_steps=8)),
               "direct": ("no_clouds_8", dict(view_steps=32, light_mode="direct", light_steps=8), dict(view_steps=32, light_steps=8)),
               "clouds_high": ("clouds_high", {}, dict(CONFIGS["clouds_high"][1]))}


def _pin_lens():
    return Lens.cube_face(PN, 5, basis=np.diag([-1.0, 1.0, 1.0]))


def _pin_camera():
    cam = S.Camera.from_pose(PN, PN, dict(eye=tuple(EYE), target=(EYE[0], EYE[1], 0.0)), fovy_deg=90.0)
    assert np.array_equal(cam.inv_view[:3, :3], np.eye(3)) and np.array_equal(cam.inv_view[:3, 3], EYE)
    return cam


@functools.lru_cache(maxsize=None)
def _pin_oracle_frame(shader):
    from oracle.oracle import Oracle

    oracle = Oracle("f32")
    cfg = dict(PIN_SHADERS[shader][2])
    uses_lut = not cfg.get("lite") and not cfg.get("light_steps")
    ocfg, otex = oracle_inputs(oracle, cfg, demo_textures(), SC._lut(oracle) if uses_lut else None, declared=False)
    cam = _pin_camera()
    img, _ = oracle.render(demo_params(u_sphere_depth_factor=1.0), otex, ocfg, make_frame(cam, np.eye(4), SUN), S.depth_far(cam), nthreads=8)
    img.setflags(write=False)
    return img


def _tangency_guard():
    """The smallest |h| / r^2 over the statement's directions and the four spheres the shader tests (shell, ground, cloud top and bottom), h = r^2 - |c - (c.d) d|^2
    with c the planet's centre seen from the eye: how far every pixel stays from a tangency, where an ulp of direction could flip a hit."""
    p = demo_params()
    rp, ha = float(p["u_planet_radius"]), float(p["u_atmosphere_height"])
    radii = [rp + ha, rp, rp + float(p["u_cloud_top"]) * ha, rp + float(p["u_cloud_bottom"]) * ha]
    d = L.lens_rays(_pin_lens())[:, 4:7].astype(np.float64)
    c = -EYE
    b = d @ c
    miss2 = np.sum((c[None, :] - b[:, None] * d) ** 2, axis=1)
    return min(float(np.abs(r * r - miss2).min() / (r * r)) for r in radii)


@pytest.mark.parametrize("shader", list(PIN_SHADERS))
def test_cube_face_is_a_pinhole_the_oracle_draws(shader):
    """CUBE_FACE -Z under diag(-1, 1, 1) is the 90-degree square pinhole, pixel for pixel: 48 x 48 rays shaded by shade_rays against the oracle's frame of
    that camera (far depth, u_sphere_depth_factor 1).  Zero sets and finite sets equal, then the project's 1e-4 rule; no pixel excluded."""
    guard = _tangency_guard()
    print(f"tangency guard: min |h| / r^2 = {guard:.3e}")
    assert guard >= 1e-5, guard
    lens, cam = _pin_lens(), _pin_camera()
    # the lens is the pinhole: the statement's directions against the camera's own, in float64
    i = np.arange(PN * PN)
    ndc = np.stack([(i % PN + 0.5) / PN * 2 - 1, 1 - (i // PN + 0.5) / PN * 2], axis=1)
    pin = np.concatenate([ndc, -np.ones((PN * PN, 1))], axis=1)
    pin /= np.linalg.norm(pin, axis=1, keepdims=True)
    assert np.abs(L.lens_rays(lens)[:, 4:7] - pin).max() < 2e-7
    want = _pin_oracle_frame(shader)
    assert np.any(want != 0.0, axis=-1).mean() >= 0.30, shader
    node = make_node(PIN_SHADERS[shader][0], demo_textures(), demo_params(u_sphere_depth_factor=1.0), **PIN_SHADERS[shader][1])
    try:
        node.set_shader_parameter("u_sun_position", SUN)
        got = node.shade_rays(node.lens_rays(lens), cam, width=PN)
        torch.cuda.synchronize()
        got = got.cpu().numpy().reshape(PN, PN, 4)
    finally:
        node.close()
    assert np.array_equal(np.all(got == 0.0, axis=-1), np.all(want == 0.0, axis=-1)), shader
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), shader
    err = SC.rel_err(got, want)
    print(f"{shader}: the -Z face as a pinhole, max err vs oracle {err:.3e} (bar {TOL:.0e})")
    assert err <= TOL, (shader, err)


# ---- 5. render_lens ------------------------------------------------------------------------------------------------------------------------------------------------
def _outside_circle():
    i = np.arange(W * H)
    return ((2 * (i % W) + 1 - W) ** 2 + (H - 2 * (i // W) - 1) ** 2 > min(W, H) ** 2).reshape(H, W)


def test_render_lens_picks_the_quads_for_a_declared_sampler():
    cam = S.Camera.from_pose(W, H, "P_space")
    node = make_node("clouds_high", demo_textures(), demo_params())
    try:
        for lens in (Lens.equirect(W, H), _fisheye_lens()):
            got = node.render_lens(lens, cam)
            torch.cuda.synchronize()
            assert node.kernel_name == "atmo_shade_rays_kernel<16433, 0>", node.kernel_name
            quads = node.lens_rays(lens, quads=True)
            want = quads_to_image(node.shade_ray_quads(quads, cam, width=W), W, H)
            assert tuple(got.shape) == (H, W, 4) and np.array_equal(_bits(got), _bits(want)) and _bits(got).any()
        assert not got.cpu().numpy()[_outside_circle()].any() and got.cpu().numpy()[~_outside_circle()].any()
        # asked for, the row-major path draws the level-0 picture through the tile index
        rm = node.render_lens(lens, cam, quads=False)
        assert "indexed" in node.kernel_name and not rm.cpu().numpy()[_outside_circle()].any() and not np.array_equal(_bits(rm), _bits(got))
        # two bands are the one-call image's rows: first_quad carries the jitter
        lens = Lens.equirect(W, H)
        whole = node.render_lens(lens, cam)
        parts = torch.cat([node.render_lens(lens.band(rows), cam) for rows in ((0, 8), (8, H))])
        assert np.array_equal(_bits(parts), _bits(whole))
        out = torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
        assert node.render_lens(lens, cam, out=out).data_ptr() == out.data_ptr() and np.array_equal(_bits(out), _bits(whole))
    finally:
        node.close()


def test_render_lens_goes_through_the_tile_index_without_one(lut_node):
    cam = S.Camera.from_pose(W, H, "P_space")
    for lens in (Lens.equirect(W, H), _fisheye_lens(), _fisheye_lens(BAND)):
        y0, y1 = lens.rows
        got = lut_node.render_lens(lens, cam)
        torch.cuda.synchronize()
        assert "indexed" in lut_node.kernel_name, lut_node.kernel_name
        rays, index = lut_node.lens_rays(lens, tile_index=True)
        want = torch.zeros(((y1 - y0) * W, 4), dtype=torch.float32, device="cuda")
        lut_node.shade_rays(rays, cam, width=W, first=y0 * W, out=want, index=index)
        assert tuple(got.shape) == (y1 - y0, W, 4) and np.array_equal(_bits(got).reshape(-1, 4), _bits(want)) and _bits(got).any()
    assert not got.cpu().numpy()[_outside_circle()[y0:y1]].any()
    # a caller's out is zeroed first: the absent pixels do not keep what it held
    out = torch.full((y1 - y0, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    lut_node.render_lens(lens, cam, out=out)
    assert np.array_equal(_bits(out), _bits(got))
    lens = Lens.equirect(W, H)
    whole = lut_node.render_lens(lens, cam)
    parts = torch.cat([lut_node.render_lens(lens.band(rows), cam) for rows in ((0, 7), (7, H))])      # first carries the jitter
    assert np.array_equal(_bits(parts), _bits(whole))
    with pytest.raises(N.AtmoError, match="atmo_shade_ray_quads"):
        lut_node.render_lens(lens, cam, quads=True)


def test_render_lens_with_cloud_detail_moves_with_time():
    cam = S.Camera.from_pose(W, H, "P_space")
    node = make_node("clouds_high", demo_textures(), demo_params(), cloud_detail=True)
    try:
        lens = _fisheye_lens()
        for quads, name in ((None, "atmo_detail_rays_kernel"), (False, "atmo_detail_rays_indexed_kernel")):
            a = node.render_lens(lens, cam, time=0.0, quads=quads)
            torch.cuda.synchronize()
            assert node.kernel_name.startswith(name + "<"), node.kernel_name
            b = node.render_lens(lens, cam, time=40.0, quads=quads)
            assert _bits(a).any() and not np.array_equal(_bits(a), _bits(b))
            assert not a.cpu().numpy()[_outside_circle()].any() and not b.cpu().numpy()[_outside_circle()].any()
    finally:
        node.close()


# ---- 6. capture ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_graph_capture_takes_the_call_as_it_is(lut_node):
    lens = _fisheye_lens(BAND)
    eager_rays, eager_index = lut_node.lens_rays(lens, tile_index=True)
    torch.cuda.synchronize()
    rays = torch.full_like(eager_rays, SENTINEL)
    index = torch.full_like(eager_index, 7)
    nl = lens.native()
    fn = lut_node._lib.atmo_lens_rays
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):      # one stream, no parallel branches
            N.check(lut_node._ctx, fn(lut_node._ctx, C.byref(nl), 0, None, 0, C.c_void_p(rays.data_ptr()), C.c_void_p(index.data_ptr()), C.c_void_p(side.cuda_stream)))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rays), _bits(eager_rays)) and np.array_equal(index.cpu().numpy(), eager_index.cpu().numpy())
