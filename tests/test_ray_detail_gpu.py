"""Cloud detail for ray batches, ray lists and ray quads on the device (include/atmo_ray_detail.h).  Needs an MI355X.  Every frame is 48 x 27.

(a) a camera's own rays shaded through atmo_shade_rays_detail are the camera's cloud-detail frame under the level-0 sampler, bit for bit, for every fixture
    case -- and therefore the executed reference text's (tests/golden/reference_exec_detail.npz) at the project's 1e-4 rule; (b) the same for quads under the
    declared sampler; (c) index lists: a permutation, a subset, atmo_ray_list's counted and culled list; (d) origins per ray and per quad, against the same
    node's detail draws of the cameras moved to those origins; (e) the switch, live time, and the old entry points' refusal on a device; (f) one captured
    graph, two lengths; (g) the C call by hand.

Measured on MI355X (profiles/rays/README.md, section 9, holds the maxima of (d))."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cloud_detail_cases as CD
from common import TOL, demo_params, demo_textures, make_node
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame
from godot_atmosphere_shader_amd.ray_quads import quad_order, quads_to_image
from test_reference_exec import GOLDEN

import reference_scenes as RSC  # noqa: E402  (tests/golden, on the path since test_reference_exec's import)

pytestmark = pytest.mark.gpu

KF_DETAIL, KF_RAYS, KF_INDEX = 8192, 16384, 32768
W, H = RSC.W, RSC.H
SENTINEL = 0x7FC12345    # a NaN no kernel produces
FIRST = 0


def _name(flags, quads=False, indexed=False):
    """Written from render_kernel_name's format, never asked of the library."""
    f = KF_DETAIL + KF_RAYS + flags + (32 if quads else 0) + (KF_INDEX if indexed else 0)
    return f"atmo_detail_rays_indexed_kernel<{f}, 0>" if indexed else f"atmo_detail_rays_kernel<{f}, 0>"


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(GOLDEN, "reference_exec_detail.npz")), np.load(os.path.join(GOLDEN, "reference_exec.npz"))


def _textures(shape_n=RSC.SHAPE_N):
    return dict(blue_noise=S.make_blue_noise(), shape=S.make_shape_texture(shape_n), cubemap=S.make_coverage_cubemap(RSC.CUBE_N))


def _node(case, sampler, **kw):
    params = demo_params() if case["invert"] is None else demo_params(u_cloud_shape_invert=case["invert"])
    return make_node(CD.NODE_SHADER[case["shader"]], _textures(case["shape_n"]), params, sampler=sampler, **kw)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _zero(img):
    return np.all(img == 0.0, axis=-1)


def _sentinel_out(n):
    return torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _render(node, cam, depth, time):
    out = node.render(cam, depth, time=time)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _case(shader, pose, time=CD.T1):
    return next(c for c in CD.CASES if c["shader"] == shader and c["pose"] == pose and c["time"] == time and c["shape_n"] == 32 and c["invert"] is None)


def _by_hand(node, entry, rays, out, cam, time, width=W, index=None):
    """The C entry point called by hand on the node's context: (return code, message)."""
    lib = node._lib
    nf = _to_native_frame(node.make_frame(cam, time))
    listed = ()
    if entry in ("atmo_shade_rays_detail", "atmo_shade_rays_indexed"):
        listed = (None, 0) if index is None else (C.c_void_p(index.data_ptr()), int(index.shape[0]))
    n = rays.shape[0] // 4 if "quads" in entry else rays.shape[0]
    rc = getattr(lib, entry)(node._ctx, C.byref(nf), C.c_void_p(rays.data_ptr()), C.c_void_p(out.data_ptr()), n, width, 0, *listed, None)
    torch.cuda.synchronize()
    return rc, (lib.atmo_last_error_string(node._ctx) or b"").decode()


# ---- (a) camera rays are the detail frame, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CD.CASES, ids=[c["name"] for c in CD.CASES])
def test_camera_rays_shade_to_the_detail_frame(vectors, case):
    z, base = vectors
    k = CD.key(case, "lod0")
    cam = RSC.camera_from_fixture(base, W, H, case["pose"])
    node = _node(case, "lod0", cloud_detail=True)
    try:
        depth = _dev(base[f"depth_demo_{case['pose']}"])
        want = _render(node, cam, depth, case["time"])
        assert node.kernel_name == CD.kernel_name(case, "lod0")
        rays = node.camera_rays(cam, depth)
        got = node.shade_rays(rays, cam, width=W, time=case["time"])
        torch.cuda.synchronize()
        name = node.kernel_name
    finally:
        node.close()
    assert name == _name(CD._FLAGS[case["shader"]]), name                                  # the kernel first
    got = got.cpu().numpy().reshape(H, W, 4)
    bad = (_bits(got) != _bits(want)).any(axis=-1)
    assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    discarded = np.unpackbits(z[f"discard_{k}"])[:W * H].reshape(H, W).astype(bool)
    assert np.array_equal(_zero(got), discarded), k
    err = CD.rel_err(got, z[f"rgba_{k}"])
    print(f"\n{k}: {name} max err vs the executed reference text {err:.3e} (bar {TOL:.0e})")
    assert err <= TOL, f"{k} {name}: {err:.3e}"


# ---- (b) quads ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CD.CASES, ids=[c["name"] for c in CD.CASES])
def test_camera_quads_shade_to_the_declared_detail_frame(vectors, case):
    z, base = vectors
    k = CD.key(case, "declared")
    cam = RSC.camera_from_fixture(base, W, H, case["pose"])
    node = _node(case, "declared", cloud_detail=True)
    try:
        depth = _dev(base[f"depth_demo_{case['pose']}"])
        want = _render(node, cam, depth, case["time"])
        assert node.kernel_name == CD.kernel_name(case, "declared")
        quads = node.camera_ray_quads(cam, depth)
        slots = quad_order(W, H)
        assert tuple(quads.shape) == (slots.size, 8) and (slots < 0).sum() == 2 * ((W + 1) // 2)      # the odd height: absent slots
        out = node.shade_ray_quads(quads, cam, width=W, time=case["time"])
        torch.cuda.synchronize()
        name = node.kernel_name
    finally:
        node.close()
    assert name == _name(CD._FLAGS[case["shader"]], quads=True), name
    out = out.cpu().numpy()
    assert not out[slots < 0].view(np.uint32).any()                                         # an absent ray receives zeros
    got = quads_to_image(out, W, H)
    bad = (_bits(got) != _bits(want)).any(axis=-1)
    assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    err = CD.rel_err(got, z[f"rgba_{k}"])
    print(f"\n{k}: {name} max err vs the executed reference text {err:.3e} (bar {TOL:.0e})")
    assert err <= TOL, f"{k} {name}: {err:.3e}"


# ---- (c) lists ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shader, pose", [(CD.CH, "P_space"), (CD.RM, "P_limb")])
def test_lists_give_the_plain_detail_call_s_bytes(vectors, shader, pose):
    _, base = vectors
    case = _case(shader, pose)
    cam = RSC.camera_from_fixture(base, W, H, pose)
    n = W * H
    node = _node(case, "lod0", cloud_detail=True)
    try:
        rays = node.camera_rays(cam, _dev(base[f"depth_demo_{pose}"]))
        plain = _bits(node.shade_rays(rays, cam, width=W, time=CD.T1))
        torch.cuda.synchronize()
        assert node.kernel_name == _name(CD._FLAGS[shader]) and plain.any()
        # a fixed-seed permutation
        perm = np.random.default_rng(23).permutation(n).astype(np.int32)
        out = _sentinel_out(n)
        assert node.shade_rays(rays, cam, width=W, time=CD.T1, out=out, index=_dev(perm)) is out
        torch.cuda.synchronize()
        assert node.kernel_name == _name(CD._FLAGS[shader], indexed=True), node.kernel_name
        assert np.array_equal(_bits(out), plain)
        # a subset, with an END entry and an entry beyond the batch: unlisted rows keep the sentinel
        subset = np.concatenate([perm[:301], np.array([-1, n + 5], dtype=np.int32)])
        out = _sentinel_out(n)
        node.shade_rays(rays, cam, width=W, time=CD.T1, out=out, index=_dev(subset))
        torch.cuda.synchronize()
        got, listed = _bits(out), np.zeros(n, dtype=bool)
        listed[perm[:301]] = True
        assert np.array_equal(got[listed], plain[listed]) and (got[~listed] == SENTINEL).all()
        # atmo_ray_list's counted, ordered and culled list: the plain call over the live rays, rows at and behind the count untouched
        live = 1001
        count = torch.tensor([live], dtype=torch.int32, device="cuda")
        out = _sentinel_out(n)
        index, n_listed = node.ray_list(rays, count, order=True, cull=True, camera=cam, out=out)
        node.shade_rays(rays, cam, width=W, time=CD.T1, out=out, index=index)
        torch.cuda.synchronize()
        assert node.kernel_name == _name(CD._FLAGS[shader], indexed=True)
        got = _bits(out)
        bad = (got[:live] != plain[:live]).any(axis=-1)
        assert not bad.any(), (int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
        assert (got[live:] == SENTINEL).all() and 0 < int(n_listed.item()) <= live
    finally:
        node.close()


# ---- (d) origins per ray ----------------------------------------------------------------------------------------------------------------------------------------
from test_rays_gpu import EYE, OH, ORIGINS, OW, SUN, _axis_camera  # noqa: E402  (the dyadic setup of tests/test_rays_gpu.py (c))

ORIGIN_SHADERS = {"clouds_high": 17, "clouds_high_rm": 19, "v1_clouds_high": 25}
# The time of the expected frames.  A raymarched-light frame that fails ONLY through a pixel whose alpha0 sits on the 0.3 threshold (the discontinuity
# include/atmo_cloud_detail.h states) gets the next time of cloud_detail_cases' list -- 12.25, then 3.0 -- never an excluded pixel or a wider bar.
ORIGIN_TIME = CD.T1


def _moved_frames(node, time):
    """The node's own detail draws of the camera moved to EYE + o_k, k = 0, 1, 2 (u_sphere_depth_factor 1: no depth read)."""
    frames = []
    for o in ORIGINS:
        cam = _axis_camera(EYE + o)
        frames.append(_render(node, cam, _dev(S.depth_far(cam)), time))
    return frames


def _check_origins(shader, what, got, want3, dealt, unmoved, off):
    want = np.stack([want3[k][y] for y, k in enumerate(dealt)])
    for k in range(3):
        assert np.any(want3[k] != 0.0, axis=-1).mean() >= 0.30, (shader, k)
        for j in range(3):
            if j != k:
                assert np.abs(want3[k][dealt == k] - want3[j][dealt == k]).max() > 100 * TOL, (shader, k, j)
    assert np.abs(unmoved - got).max() > 100 * TOL                                          # the origins reached the kernel
    assert (np.abs(off - got).max(-1) > 1e-3).mean() >= 0.01                                # ... and so did the detail fetch
    assert np.array_equal(_zero(got), _zero(want)), shader
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.isfinite(got).all(), shader
    err = CD.rel_err(got, want)
    print(f"\n{shader}: origins per {what}, max err vs the moved cameras' detail frames {err:.3e} (bar {TOL:.0e}), "
          f"{int((_bits(got) != _bits(want)).any(-1).sum())} of {OW * OH} pixels differ in a bit")
    assert err <= TOL, (shader, what, err)


@pytest.mark.parametrize("shader", list(ORIGIN_SHADERS))
def test_origins_per_ray_match_the_moved_cameras_detail_frames(shader):
    """Rows dealt o_(y mod 3); directions from camera_rays of the unmoved camera.  Expected, row for row: the same node's cloud-detail render of the camera
    moved by that origin, level-0 sampler.  Every pixel counts."""
    rows = np.arange(OH) % 3
    node = make_node(shader, demo_textures(), demo_params(u_sphere_depth_factor=1.0), sampler="lod0", cloud_detail=True)
    try:
        node.set_shader_parameter("u_sun_position", SUN)
        want3 = _moved_frames(node, ORIGIN_TIME)
        assert node.kernel_name == f"atmo_render_detail_kernel<{KF_DETAIL + ORIGIN_SHADERS[shader]}, 0>"
        cam = _axis_camera(EYE)
        rays = node.camera_rays(cam, _dev(S.depth_far(cam)))
        moved = rays.clone().reshape(OH, OW, 8)
        moved[:, :, 0:3] = torch.from_numpy(ORIGINS[rows].astype(np.float32)).cuda()[:, None, :]
        moved = moved.reshape(-1, 8)
        got = node.shade_rays(moved, cam, width=OW, time=ORIGIN_TIME).cpu().numpy().reshape(OH, OW, 4)
        assert node.kernel_name == _name(ORIGIN_SHADERS[shader])
        unmoved = node.shade_rays(rays, cam, width=OW, time=ORIGIN_TIME).cpu().numpy().reshape(OH, OW, 4)
        node.cloud_detail = False
        off = node.shade_rays(moved, cam, width=OW, time=ORIGIN_TIME).cpu().numpy().reshape(OH, OW, 4)
        assert node.kernel_name == f"atmo_shade_rays_kernel<{KF_RAYS + ORIGIN_SHADERS[shader]}, 0>"
    finally:
        node.close()
    _check_origins(shader, "ray", got, want3, rows, unmoved, off)


@pytest.mark.parametrize("shader", list(ORIGIN_SHADERS))
def test_origins_per_quad_match_the_moved_cameras_declared_detail_frames(shader):
    """Quad row r gets o_(r mod 3), all four slots.  Expected: rows 2 r and 2 r + 1 of the moved camera's declared-sampler detail frame."""
    rows = (np.arange(OH) // 2) % 3
    node = make_node(shader, demo_textures(), demo_params(u_sphere_depth_factor=1.0), cloud_detail=True)
    try:
        node.set_shader_parameter("u_sun_position", SUN)
        want3 = _moved_frames(node, ORIGIN_TIME)
        assert node.kernel_name == f"atmo_render_detail_kernel<{KF_DETAIL + 32 + ORIGIN_SHADERS[shader]}, 0>"
        cam = _axis_camera(EYE)
        rays = node.camera_rays(cam, _dev(S.depth_far(cam)))
        moved = rays.clone().reshape(OH, OW, 8)
        moved[:, :, 0:3] = torch.from_numpy(ORIGINS[rows].astype(np.float32)).cuda()[:, None, :]
        order = torch.from_numpy(quad_order(OW, OH)).cuda()

        def to_quads(r):
            return torch.where((order >= 0)[:, None], r.reshape(-1, 8)[order.clamp(min=0)], torch.zeros((), device="cuda")).contiguous()

        def shade(r):
            return quads_to_image(node.shade_ray_quads(to_quads(r), cam, width=OW, time=ORIGIN_TIME).cpu().numpy(), OW, OH)

        got = shade(moved)
        assert node.kernel_name == _name(ORIGIN_SHADERS[shader], quads=True)
        unmoved = shade(rays)
        node.cloud_detail = False
        off = shade(moved)
        assert node.kernel_name == f"atmo_shade_rays_kernel<{KF_RAYS + 32 + ORIGIN_SHADERS[shader]}, 0>"
    finally:
        node.close()
    _check_origins(shader, "quad", got, want3, rows, unmoved, off)


# ---- (e) the switch and time ----------------------------------------------------------------------------------------------------------------------------------------
def test_switch_and_time(vectors):
    _, base = vectors
    case = _case(CD.CH, "P_space")
    cam = RSC.camera_from_fixture(base, W, H, "P_space")
    n = W * H
    node = _node(case, "lod0", cloud_detail=True)
    try:
        rays = node.camera_rays(cam, _dev(base["depth_demo_P_space"]))
        on0 = node.shade_rays(rays, cam, width=W, time=0.0).cpu().numpy()
        on1 = node.shade_rays(rays, cam, width=W, time=CD.T1).cpu().numpy()
        assert node.kernel_name == _name(17)
        assert (np.abs(on0 - on1).max(-1) > 1e-3).mean() >= 0.01                            # AtmoFrame::time is live
        # on the device context the OLD entry points refuse, naming cloud detail, and write nothing
        index = _dev(np.arange(n, dtype=np.int32))
        quads = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
        for entry, r in (("atmo_shade_rays", rays), ("atmo_shade_rays_indexed", rays), ("atmo_shade_ray_quads", quads)):
            out = _sentinel_out(r.shape[0])
            rc, msg = _by_hand(node, entry, r, out, cam, CD.T1, index=index)
            assert rc == N.ATMO_E_STATE and msg.startswith(entry + ": ") and "cloud detail" in msg, (entry, rc, msg)
            assert (_bits(out) == SENTINEL).all(), entry
        # detail off: the new entry IS atmo_shade_rays, for both times
        node.cloud_detail = False
        for t in (0.0, CD.T1):
            old = _bits(node.shade_rays(rays, cam, width=W, time=t))
            torch.cuda.synchronize()
            old_name = node.kernel_name
            assert old_name == f"atmo_shade_rays_kernel<{KF_RAYS + 17}, 0>"
            out = _sentinel_out(n)
            rc, msg = _by_hand(node, "atmo_shade_rays_detail", rays, out, cam, t)
            assert rc == N.ATMO_OK, msg
            assert node.kernel_name == old_name and np.array_equal(_bits(out), old)
            if t == 0.0:
                off0 = old
            else:
                assert np.array_equal(old, off0)                                            # TIME is dead with the switch off
        assert (np.abs(off0.view(np.float32) - on0).max(-1) > 1e-3).mean() >= 0.01
        # on again: the first bytes again
        node.cloud_detail = True
        again = node.shade_rays(rays, cam, width=W, time=0.0).cpu().numpy()
        assert again.tobytes() == on0.tobytes() and node.kernel_name == _name(17)
    finally:
        node.close()


# ---- (f) one captured graph, two lengths ------------------------------------------------------------------------------------------------------------------------
def test_a_captured_graph_serves_two_counts(vectors):
    _, base = vectors
    case = _case(CD.CH, "P_space")
    cam = RSC.camera_from_fixture(base, W, H, "P_space")
    capacity = W * H
    node = _node(case, "lod0", cloud_detail=True)
    try:
        rays = node.camera_rays(cam, _dev(base["depth_demo_P_space"]))
        perm = torch.from_numpy(np.random.default_rng(29).permutation(capacity)).cuda()
        rays = rays[perm].contiguous()                                                        # a shuffled queue
        want = {}
        for live in (capacity, 700):                                                          # the eager pair
            count = torch.tensor([live], dtype=torch.int32, device="cuda")
            out = _sentinel_out(capacity)
            index, _ = node.ray_list(rays, count, order=True, cull=True, camera=cam, out=out)
            node.shade_rays(rays, cam, width=W, time=CD.T1, out=out, index=index)
            torch.cuda.synchronize()
            want[live] = _bits(out).copy()
            plain = _bits(node.shade_rays(rays[:live], cam, width=W, time=CD.T1))
            assert np.array_equal(want[live][:live], plain) and (want[live][live:] == SENTINEL).all() and plain.any()
        count = torch.tensor([capacity], dtype=torch.int32, device="cuda")
        out, fresh = _sentinel_out(capacity), _sentinel_out(capacity)
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):     # one stream, no parallel branches
                index, listed = node.ray_list(rays, count, order=True, cull=True, camera=cam, out=out)
                node.shade_rays(rays, cam, width=W, time=CD.T1, out=out, index=index)
        torch.cuda.synchronize()
        for live in (capacity, 700):
            count.fill_(live)                           # written on the device; the host never reads it
            out.copy_(fresh)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(out), want[live]), live
            assert 0 < int(listed.item()) <= live
    finally:
        node.close()


# ---- (g) the C call by hand ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_draws_the_c_calls_bytes(vectors):
    """PlanetAtmosphere(cloud_detail=True).shade_rays against atmo_set_cloud_detail + atmo_shade_rays_detail called by hand on another node's context."""
    _, base = vectors
    case = _case(CD.RM, "P_limb")
    cam = RSC.camera_from_fixture(base, W, H, "P_limb")
    a, b = _node(case, "lod0", cloud_detail=True), _node(case, "lod0")
    try:
        depth = _dev(base["depth_demo_P_limb"])
        rays = a.camera_rays(cam, depth)
        by_binding = _bits(a.shade_rays(rays, cam, width=W, time=CD.T1))
        low = _bits(b.shade_rays(rays, cam, width=W, time=CD.T1))              # (bakes b's LUT; the low-quality rays)
        torch.cuda.synchronize()
        assert not np.array_equal(low, by_binding)
        N.check(b._ctx, b._lib.atmo_set_cloud_detail(b._ctx, 1))
        out = _sentinel_out(W * H)
        rc, msg = _by_hand(b, "atmo_shade_rays_detail", rays, out, cam, CD.T1)
        assert rc == N.ATMO_OK, msg
        assert b.kernel_name == a.kernel_name == _name(19)
        assert np.array_equal(_bits(out), by_binding)
    finally:
        a.close()
        b.close()
