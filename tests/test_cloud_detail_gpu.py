"""The cloud-detail kernels (include/atmo_cloud_detail.h) against the reference's shader text executed with `#define CLOUDS_ALWAYS_LOW_QUALITY`
commented out (tests/golden/reference_exec_detail.npz, made by tests/golden/make_detail_vectors.py; tests/test_cloud_detail_host.py proves that the
file holds something).  Needs an MI355X.  Every frame is 48 x 27: seconds in all.

Measured on MI355X (profiles/cloud_detail/README.md holds the per-frame table): every frame within the project's 1e-4 rule."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cloud_detail_cases as CD
from common import TOL, demo_params, make_node
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import scene as S
from test_reference_exec import GOLDEN

import reference_scenes as RSC  # noqa: E402  (tests/golden, on the path since test_reference_exec's import)

pytestmark = pytest.mark.gpu
W, H = RSC.W, RSC.H
IDS = [CD.key(c, s) for c in CD.CASES for s in CD.SAMPLERS]


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(GOLDEN, "reference_exec_detail.npz")), np.load(os.path.join(GOLDEN, "reference_exec.npz"))


def _textures(shape_n=RSC.SHAPE_N):
    return dict(blue_noise=S.make_blue_noise(), shape=S.make_shape_texture(shape_n), cubemap=S.make_coverage_cubemap(RSC.CUBE_N))


def _node(case, sampler, **kw):
    params = demo_params() if case["invert"] is None else demo_params(u_cloud_shape_invert=case["invert"])
    return make_node(CD.NODE_SHADER[case["shader"]], _textures(case["shape_n"]), params, sampler=sampler, **kw)


def _draw(node, cam, depth_np, time, **kw):
    out = node.render(cam, torch.from_numpy(np.array(depth_np)).cuda(), time=time, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _zero(img):
    return np.all(img == 0.0, axis=-1)


# ---- a. every fixture frame ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, sampler", [(c, s) for c in CD.CASES for s in CD.SAMPLERS], ids=IDS)
def test_detail_frames_match_the_executed_reference(vectors, case, sampler):
    z, base = vectors
    k = CD.key(case, sampler)
    cam = RSC.camera_from_fixture(base, W, H, case["pose"])
    node = _node(case, sampler, cloud_detail=True)
    try:
        got = _draw(node, cam, base[f"depth_demo_{case['pose']}"], case["time"])
        name = node.kernel_name
    finally:
        node.close()
    assert name == CD.kernel_name(case, sampler), (name, CD.kernel_name(case, sampler))          # the kernel first
    want = z[f"rgba_{k}"]
    discarded = np.unpackbits(z[f"discard_{k}"])[:W * H].reshape(H, W).astype(bool)
    assert np.array_equal(_zero(got), discarded), k                                               # then the discard / zero sets
    assert np.array_equal(_zero(got), _zero(want)) and np.isfinite(got).all() and np.isfinite(want).all(), k
    err = CD.rel_err(got, want)
    print(f"\n{k}: {name} max err vs the executed reference text {err:.3e} (bar {TOL:.0e})")
    assert err <= TOL, f"{k} {name}: {err:.3e}"


# ---- b. the switch ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shader, sampler", [(CD.CH, "declared"), (CD.RM, "declared"), (CD.RM, "lod0"), (CD.V1CH, "lod0")])
def test_off_on_off_and_time(vectors, shader, sampler):
    """Detail off, on, off: the first frame's bits again, from the kernel it came from.  Off, t = 0 and t = 37.5 are the same bits (TIME is dead in the
    shipped text); on, they differ -- and differ from the frame with it off."""
    _, base = vectors
    case = next(c for c in CD.CASES if c["shader"] == shader and c["pose"] == "P_space" and c["time"] == CD.T1 and c["shape_n"] == 32 and c["invert"] is None)
    cam, depth = RSC.camera_from_fixture(base, W, H, "P_space"), base["depth_demo_P_space"]
    node = _node(case, sampler)
    try:
        assert node.cloud_detail is False
        off0, name_off = _draw(node, cam, depth, 0.0), node.kernel_name
        off1 = _draw(node, cam, depth, CD.T1)
        assert off0.tobytes() == off1.tobytes() and name_off.startswith("atmo_render_kernel<")
        node.cloud_detail = True
        on0, name_on = _draw(node, cam, depth, 0.0), node.kernel_name
        on1 = _draw(node, cam, depth, CD.T1)
        assert name_on == CD.kernel_name(case, sampler)
        assert (np.abs(on0 - on1).max(-1) > 1e-3).mean() >= 0.01 and (np.abs(on0 - off0).max(-1) > 1e-3).mean() >= 0.01
        node.cloud_detail = False
        again = _draw(node, cam, depth, 0.0)
        assert again.tobytes() == off0.tobytes() and node.kernel_name == name_off
        # a rect is the crop of the full frame (the quads are the viewport's), and the launch order is no part of the picture
        node.cloud_detail = True
        x0, y0, x1, y1 = rect = (7, 5, W - 9, H - 4)
        assert _draw(node, cam, depth, CD.T1, rect=rect).tobytes() == np.ascontiguousarray(on1[y0:y1, x0:x1]).tobytes()
    finally:
        node.close()


@pytest.mark.parametrize("sampler", CD.SAMPLERS)
def test_composite_is_the_blend_of_the_plain_frame(vectors, sampler):
    _, base = vectors
    case = next(c for c in CD.CASES if c["shader"] == CD.RM and c["pose"] == "P_limb" and c["time"] == CD.T1)
    cam, depth = RSC.camera_from_fixture(base, W, H, "P_limb"), base["depth_demo_P_limb"]
    node = _node(case, sampler, cloud_detail=True)
    try:
        src = _draw(node, cam, depth, CD.T1)
        dst = np.random.default_rng(5).uniform(0.0, 1.5, (H, W, 4)).astype(np.float32)
        scene = torch.from_numpy(dst.copy()).cuda()
        node.render_composite(cam, torch.from_numpy(np.array(depth)).cuda(), scene, time=CD.T1)
        torch.cuda.synchronize()
        assert node.kernel_name == CD.kernel_name(case, sampler)
        got = scene.cpu().numpy()
    finally:
        node.close()
    a = src[..., 3:4]
    ia = np.float32(1.0) - a
    want = np.concatenate([src[..., :3] * a + dst[..., :3] * ia, a + dst[..., 3:4] * ia], axis=-1).astype(np.float32)
    disc = _zero(src)
    assert 0 < disc.sum() < disc.size and np.array_equal(got[disc], dst[disc])          # a discarded fragment leaves the scene untouched
    assert got.tobytes() == want.tobytes()


def test_python_property_draws_the_c_calls_bytes(vectors):
    """PlanetAtmosphere(cloud_detail=True) against atmo_set_cloud_detail + atmo_render called by hand on another node's context."""
    _, base = vectors
    case = next(c for c in CD.CASES if c["shader"] == CD.CH and c["pose"] == "P_clouds" and c["time"] == CD.T1)
    cam, depth = RSC.camera_from_fixture(base, W, H, "P_clouds"), base["depth_demo_P_clouds"]
    lib = N.load()
    a, b = _node(case, "declared", cloud_detail=True), _node(case, "declared")
    try:
        by_property = _draw(a, cam, depth, CD.T1)
        low = _draw(b, cam, depth, CD.T1)          # (bakes b's LUT; the low-quality frame)
        assert low.tobytes() != by_property.tobytes()
        on = C.c_int(-1)
        assert lib.atmo_get_cloud_detail(a._ctx, C.byref(on)) == N.ATMO_OK and on.value == 1
        assert lib.atmo_get_cloud_detail(b._ctx, C.byref(on)) == N.ATMO_OK and on.value == 0
        N.check(b._ctx, lib.atmo_set_cloud_detail(b._ctx, 1))
        d, out = torch.from_numpy(np.array(depth)).cuda(), torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        frame = b.prepare_frame(cam, time=CD.T1)
        N.check(b._ctx, lib.atmo_render(b._ctx, C.byref(frame), d.data_ptr(), out.data_ptr(), None))
        torch.cuda.synchronize()
        assert lib.atmo_kernel_name(b._ctx).decode() == a.kernel_name == CD.kernel_name(case, "declared")
        assert out.cpu().numpy().tobytes() == by_property.tobytes()
        # ... and the draws the header refuses are refused on a device as well, with nothing drawn
        with pytest.raises(N.AtmoError) as e:
            a.render_proxy(cam, d)
        assert e.value.code == N.ATMO_E_STATE and "cloud detail" in str(e.value)
    finally:
        a.close()
        b.close()
