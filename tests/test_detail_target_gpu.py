"""Cloud detail into colour targets through a depth source on the device (include/atmo_detail_target.h).  Needs an MI355X.  Every frame is the fixtures'
48 x 27 (the batch's halves: 24 x 27): odd height, partial tiles, helper rows under the declared sampler.  Every comparison but (a)'s golden pin is
BIT-EXACT.

 (a) float identity: the new call into an RGBA32F tight target from a D32 tight depth is atmo_render's detail frame, for every fixture case under both
     samplers, from the kernel atmo_detail_target_kernel<13312 + flags, 0>; one case per shader also straight against the executed reference text;
 (b) the six families x the seven formats: the store is targets.py's encode of the float detail frame, the composite decode / blend / encode over a seeded
     destination, discarded pixels untouched;
 (c) a rect with an odd origin into pitched targets: the crop's encode inside, the sentinel outside;
 (d) D16 / X8_D24 sources with a row pitch against a D32 tight buffer of the decoded values;
 (e) off, on, off, and live time;
 (f) a batch of three views -- the halves of one image pair and a rect of a pitched pair at another time -- against its views' own single draws;
 (g) one captured graph replayed onto two depth contents;
 (h) the binding."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cloud_detail_cases as CD
from common import TOL, demo_params, make_node
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import depth_formats as D
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T
from godot_atmosphere_shader_amd.planet_atmosphere import depth_source
from test_reference_exec import GOLDEN

import reference_scenes as RSC  # noqa: E402  (tests/golden, on the path since test_reference_exec's import)

pytestmark = pytest.mark.gpu
W, H = RSC.W, RSC.H
KF_TARGET, KF_VIEWS, KF_DEPTH, KF_DETAIL = 1024, 2048, 4096, 8192
FLAGS = {CD.CH: 17, CD.RM: 19, CD.CL: 17, CD.V1CH: 25}
FORMATS = ["rgba32f", "rgba16f", "rgba8", "rgba8_srgb", "bgra8", "bgra8_srgb", "a2b10g10r10"]
FAMILIES = [(shader, sampler) for shader in (CD.CH, CD.RM, CD.V1CH) for sampler in CD.SAMPLERS]      # 49, 17, 51, 19, 57, 25
FAMILY_IDS = [f"{CD.NODE_SHADER[s]}-{m}" for s, m in FAMILIES]
RECT = (7, 5, W - 9, H - 4)     # an odd origin: helper pixels under the declared sampler
SENTINEL = 0xA5
GOLDEN_PINS = {CD.CH: "P_limb", CD.RM: "P_ground", CD.CL: "P_space", CD.V1CH: "P_space"}     # one case per shader, at t = 37.5


def _name(shader, sampler, views=False):
    """Written from render_kernel_name's format, never asked of the library."""
    flags = FLAGS[shader] + (32 if sampler == "declared" else 0) + KF_DETAIL + KF_DEPTH + KF_TARGET + (KF_VIEWS if views else 0)
    return f"atmo_detail_views_target_kernel<{flags}, 0>" if views else f"atmo_detail_target_kernel<{flags}, 0>"


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(GOLDEN, "reference_exec_detail.npz")), np.load(os.path.join(GOLDEN, "reference_exec.npz"))


def _case(shader, pose, time=CD.T1):
    return CD._case(shader, pose, time)


def _node(case, sampler, **kw):
    params = demo_params() if case["invert"] is None else demo_params(u_cloud_shape_invert=case["invert"])
    tex = dict(blue_noise=S.make_blue_noise(), shape=S.make_shape_texture(case["shape_n"]), cubemap=S.make_coverage_cubemap(RSC.CUBE_N))
    return make_node(CD.NODE_SHADER[case["shader"]], tex, params, sampler=sampler, **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _zero(img):
    return np.all(img == 0.0, axis=-1)


def _float_frame(node, cam, depth_np, time, rect=None):
    """atmo_render's frame: the reference of every byte comparison below."""
    out = node.render(cam, _dev(np.asarray(depth_np, dtype=np.float32)), time=time, rect=rect)
    torch.cuda.synchronize()
    assert node.kernel_name.startswith("atmo_render_detail_kernel<" if node.cloud_detail else "atmo_render_kernel<"), node.kernel_name
    return out.cpu().numpy()


def _buffer(rows, row_bytes, pad=0, fill=None, seed=0, fmt=None, cols=None):
    """A (rows, row_bytes + pad) uint8 device buffer: `fill` everywhere, or -- fmt, cols -- the encode of seeded random colours in [0, 1.5) (padding: SENTINEL)."""
    if fill is not None:
        host = np.full((rows, row_bytes + pad), fill, dtype=np.uint8)
    else:
        rgba = np.random.default_rng(seed).uniform(0.0, 1.5, (rows, cols, 4)).astype(np.float32)
        host = np.full((rows, row_bytes + pad), SENTINEL, dtype=np.uint8)
        host[:, :row_bytes] = np.ascontiguousarray(T.encode(rgba, fmt)).view(np.uint8).reshape(rows, row_bytes)
    return torch.from_numpy(host).cuda()


def _depth_buffer(depth_np, fmt="d32f", pad=0):
    """(device buffer, AtmoDepth fields (format, pitch)) of the depth quantised to `fmt`, rows `pad` texels further apart than a row (padding: the top code)."""
    q = D.quantise(np.asarray(depth_np, dtype=np.float32), fmt)
    if fmt == "x8d24":
        q = q | (np.random.default_rng(3).integers(0, 256, size=q.shape, dtype=np.uint32) << 24)
    tb = D.TEXEL_BYTES[D.format_id(fmt)]
    host = np.full((q.shape[0], (q.shape[1] + pad) * tb), 0xFF, dtype=np.uint8)
    host[:, :q.shape[1] * tb] = np.ascontiguousarray(q).view(np.uint8).reshape(q.shape[0], -1)
    return torch.from_numpy(host).cuda(), D.format_id(fmt), (0 if pad == 0 else host.shape[1]), D.decode(q, fmt)


def _draw(node, cam, time, depth_buf, dfmt, dpitch, target_buf, fmt, pitch, composite=False, rect=None, entry="atmo_render_detail_target", depth_off=0,
          target_off=0):
    """The C call by hand on device buffers; returns after a synchronize."""
    lib = N.load()
    node._bake_if_needed(torch.cuda.current_stream().cuda_stream)
    frame = node.prepare_frame(cam, time=time, rect=rect)
    dep = N.AtmoDepth(depth_buf.data_ptr() + depth_off, dfmt, dpitch)
    tgt = N.AtmoTarget(target_buf.data_ptr() + target_off, T.format_id(fmt), pitch)
    N.check(node._ctx, getattr(lib, entry)(node._ctx, C.byref(frame), C.byref(dep), C.byref(tgt), int(composite), _stream()))
    torch.cuda.synchronize()
    return target_buf.cpu().numpy()


def _enc(rgba, fmt):
    return np.ascontiguousarray(T.encode(rgba, fmt)).view(np.uint8).reshape(rgba.shape[0], -1)


# ---- (a) float identity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, sampler", [(c, s) for c in CD.CASES for s in CD.SAMPLERS], ids=[CD.key(c, s) for c in CD.CASES for s in CD.SAMPLERS])
def test_rgba32f_from_d32_is_the_detail_draws_frame(vectors, case, sampler):
    z, base = vectors
    cam, depth = RSC.camera_from_fixture(base, W, H, case["pose"]), base[f"depth_demo_{case['pose']}"]
    node = _node(case, sampler, cloud_detail=True)
    try:
        want = _float_frame(node, cam, depth, case["time"])
        assert node.kernel_name == CD.kernel_name(case, sampler)
        dbuf, dfmt, dpitch, _ = _depth_buffer(depth)
        got = _draw(node, cam, case["time"], dbuf, dfmt, dpitch, _buffer(H, W * 16, fill=SENTINEL), "rgba32f", 0)
        name = node.kernel_name
    finally:
        node.close()
    assert name == _name(case["shader"], sampler), (name, _name(case["shader"], sampler))
    assert got.tobytes() == want.tobytes()
    assert 0 < (~_zero(want)).sum()
    if GOLDEN_PINS[case["shader"]] == case["pose"] and case["time"] == CD.T1 and case["shape_n"] == 32 and case["invert"] is None:
        # chain-free: the new kernel's own floats against the executed reference text
        k = CD.key(case, sampler)
        frame = got.view(np.float32).reshape(H, W, 4)
        discarded = np.unpackbits(z[f"discard_{k}"])[:W * H].reshape(H, W).astype(bool)
        assert np.array_equal(_zero(frame), discarded) and np.isfinite(frame).all(), k
        err = CD.rel_err(frame, z[f"rgba_{k}"])
        print(f"\n{k}: {name} max err vs the executed reference text {err:.3e} (bar {TOL:.0e})")
        assert err <= TOL, f"{k} {name}: {err:.3e}"


def test_every_shader_has_its_golden_pin():
    pinned = [c for c in CD.CASES if GOLDEN_PINS[c["shader"]] == c["pose"] and c["time"] == CD.T1 and c["shape_n"] == 32 and c["invert"] is None]
    assert sorted(c["shader"] for c in pinned) == sorted(GOLDEN_PINS)


# ---- (b) the six families x the seven formats ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def limb(vectors):
    """Per family, made once: the node (detail on), P_limb's camera and depth, and atmo_render's float detail frame at t = 37.5."""
    _, base = vectors
    cam, depth = RSC.camera_from_fixture(base, W, H, "P_limb"), np.array(base["depth_demo_P_limb"], dtype=np.float32)
    made = {}

    def get(shader, sampler):
        if (shader, sampler) not in made:
            node = _node(_case(shader, "P_limb"), sampler, cloud_detail=True)
            made[shader, sampler] = (node, _float_frame(node, cam, depth, CD.T1))
        return made[shader, sampler] + (cam, depth)

    yield get
    for node, _ in made.values():
        node.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shader, sampler", FAMILIES, ids=FAMILY_IDS)
def test_store_and_composite_in_every_format(limb, shader, sampler, fmt):
    node, src, cam, depth = limb(shader, sampler)
    px = T.PIXEL_BYTES[T.format_id(fmt)]
    dbuf, dfmt, dpitch, _ = _depth_buffer(depth)
    got = _draw(node, cam, CD.T1, dbuf, dfmt, dpitch, _buffer(H, W * px, fill=SENTINEL), fmt, 0)
    assert node.kernel_name == _name(shader, sampler)
    assert got.tobytes() == _enc(src, fmt).tobytes()                       # discards are stored as zero: all-zero bits in every format
    disc = _zero(src)
    assert 0 < disc.sum() < disc.size
    scene = _buffer(H, W * px, seed=5, fmt=fmt, cols=W)
    dst = scene.cpu().numpy()
    got = _draw(node, cam, CD.T1, dbuf, dfmt, dpitch, scene, fmt, 0, composite=True)
    assert node.kernel_name == _name(shader, sampler)
    dst_px = dst.view(T.DTYPES[T.format_id(fmt)]).reshape(H, W, 4)
    want = np.ascontiguousarray(T.blend(src, dst_px, fmt)).view(np.uint8).reshape(H, W, px)
    got_px, dst_b = got.reshape(H, W, px), dst.reshape(H, W, px)
    assert np.array_equal(got_px[disc], dst_b[disc])                       # a discarded fragment leaves the destination's bytes alone
    assert np.array_equal(got_px[~disc], want[~disc])
    assert not np.array_equal(got_px[~disc], dst_b[~disc])


# ---- (c) pitch and rect ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgba16f", "rgba8_srgb"])
@pytest.mark.parametrize("shader, sampler", [(CD.CH, "declared"), (CD.RM, "lod0")])
def test_a_rect_into_a_pitched_target_is_the_crop(limb, shader, sampler, fmt):
    node, full, cam, depth = limb(shader, sampler)
    x0, y0, x1, y1 = RECT
    px, pad = T.PIXEL_BYTES[T.format_id(fmt)], 24
    rows, row_bytes = y1 - y0, (x1 - x0) * px
    dbuf, dfmt, dpitch, _ = _depth_buffer(depth)
    got = _draw(node, cam, CD.T1, dbuf, dfmt, dpitch, _buffer(rows, row_bytes, pad=pad, fill=SENTINEL), fmt, row_bytes + pad, rect=RECT)
    crop = np.ascontiguousarray(full[y0:y1, x0:x1])
    assert (~_zero(crop)).any()
    assert np.array_equal(got[:, :row_bytes], _enc(crop, fmt)) and (got[:, row_bytes:] == SENTINEL).all()
    # the composite addresses the whole viewport's buffer: outside the rect every byte is still the sentinel
    wide = W * px + pad
    scene = _buffer(H, W * px, pad=pad, fill=SENTINEL)
    got = _draw(node, cam, CD.T1, dbuf, dfmt, dpitch, scene, fmt, wide, composite=True, rect=RECT).reshape(H, wide)
    inside = np.zeros((H, wide), dtype=bool)
    inside[y0:y1, x0 * px:x1 * px] = True
    assert (got[~inside] == SENTINEL).all() and (got[inside] != SENTINEL).any()
    sent = np.full((rows, x1 - x0, px), SENTINEL, dtype=np.uint8).view(T.DTYPES[T.format_id(fmt)]).reshape(rows, x1 - x0, 4)
    want = np.ascontiguousarray(T.blend(crop, sent, fmt)).view(np.uint8).reshape(rows, x1 - x0, px)
    kept = ~_zero(crop)
    assert np.array_equal(got[y0:y1, x0 * px:x1 * px].reshape(rows, x1 - x0, px)[kept], want[kept])


# ---- (d) depth sources -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dfmt_name", ["d16", "x8d24"])
@pytest.mark.parametrize("shader, sampler, pose", [(CD.CH, "declared", "P_space"), (CD.RM, "lod0", "P_ground")])
def test_a_pitched_depth_source_is_its_decoded_floats(vectors, shader, sampler, pose, dfmt_name):
    _, base = vectors
    cam, depth = RSC.camera_from_fixture(base, W, H, pose), np.array(base[f"depth_demo_{pose}"], dtype=np.float32)
    node = _node(_case(shader, pose), sampler, cloud_detail=True)
    try:
        dbuf, dfmt, dpitch, decoded = _depth_buffer(depth, dfmt_name, pad=5)
        assert dpitch == (W + 5) * D.TEXEL_BYTES[dfmt] and (decoded != depth).any()      # the source is neither tight nor the floats
        for fmt in ("rgba32f", "rgba8_srgb"):
            px = T.PIXEL_BYTES[T.format_id(fmt)]
            got = _draw(node, cam, CD.T1, dbuf, dfmt, dpitch, _buffer(H, W * px, fill=SENTINEL), fmt, 0)
            assert node.kernel_name == _name(shader, sampler)
            fbuf, ffmt, fpitch, same = _depth_buffer(decoded)
            assert ffmt == N.DEPTH_D32_SFLOAT and fpitch == 0 and same.tobytes() == decoded.tobytes()
            want = _draw(node, cam, CD.T1, fbuf, ffmt, fpitch, _buffer(H, W * px, fill=SENTINEL), fmt, 0)
            assert got.tobytes() == want.tobytes(), (dfmt_name, fmt)
            if fmt == "rgba32f":
                assert want.tobytes() == _float_frame(node, cam, decoded, CD.T1).tobytes() and (~_zero(want.view(np.float32).reshape(H, W, 4))).any()
    finally:
        node.close()


# ---- (e) the switch and time -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shader, sampler", [(CD.CH, "declared"), (CD.RM, "lod0")])
def test_off_on_off_and_time(vectors, shader, sampler):
    _, base = vectors
    cam, depth = RSC.camera_from_fixture(base, W, H, "P_space"), base["depth_demo_P_space"]
    node = _node(_case(shader, "P_space"), sampler)
    dbuf, dfmt, dpitch, _ = _depth_buffer(depth, "d16", pad=3)

    def frame(time, entry="atmo_render_detail_target"):
        got = _draw(node, cam, time, dbuf, dfmt, dpitch, _buffer(H, W * 16, fill=SENTINEL), "rgba32f", 0, entry=entry)
        return got.view(np.float32).reshape(H, W, 4), node.kernel_name

    try:
        assert node.cloud_detail is False
        old, name_old = frame(0.0, "atmo_render_depth_target")
        off0, name_off = frame(0.0)
        assert off0.tobytes() == old.tobytes() and name_off == name_old and name_off.startswith("atmo_render_depth_target_kernel<")
        assert frame(CD.T1)[0].tobytes() == off0.tobytes()                              # off, TIME is dead
        node.cloud_detail = True
        on0, name_on = frame(0.0)
        on1, _ = frame(CD.T1)
        assert name_on == _name(shader, sampler)
        assert (np.abs(on0 - on1).max(-1) > 1e-3).mean() >= 0.01 and (np.abs(on0 - off0).max(-1) > 1e-3).mean() >= 0.01
        node.cloud_detail = False
        again, name_again = frame(0.0)
        assert again.tobytes() == off0.tobytes() and name_again == name_off
    finally:
        node.close()


# ---- (f) the batch -----------------------------------------------------------------------------------------------------------------------------------
HALF = W // 2
T_OTHER = 12.25


def _batch_layout(base):
    """Three views: the 24-wide halves of one 48-wide RGBA8_SRGB image and one 48-wide D16 image (t = 37.5), and RECT of a pitched pair of their own at
    another time.  [(camera, rect, time, depth array (the view's viewport), which pair, byte offsets into the pair's depth / colour buffers)]"""
    depth = np.array(base["depth_demo_P_space"], dtype=np.float32)
    left, right = S.Camera.from_pose(HALF, H, "P_space"), S.Camera.from_pose(HALF, H, "P_limb")
    whole = RSC.camera_from_fixture(base, W, H, "P_space")
    return depth, [(left, None, CD.T1, 0, 0, 0), (right, None, CD.T1, 0, HALF * 2, HALF * 4), (whole, RECT, T_OTHER, 1, 0, 0)]


def _batch_buffers(depth, composite):
    """[(depth buffer, its pitch), ...], [(colour buffer, its pitch), ...] of the two pairs, freshly filled: pair 0 the 48-wide images, pair 1 pitched;
    plain draws write the rect from the target's first pixel, composites address the viewport."""
    d0, _, _, _ = _depth_buffer(depth, "d16")
    d1, _, p1, _ = _depth_buffer(depth, "d16", pad=4)
    x0, y0, x1, y1 = RECT
    rows1, cols1 = (H, W) if composite else (y1 - y0, x1 - x0)
    c0 = _buffer(H, W * 4, seed=7, fmt="rgba8_srgb", cols=W)
    c1 = _buffer(rows1, cols1 * 4, pad=20, seed=8, fmt="rgba8_srgb", cols=cols1)
    return [(d0, W * 2), (d1, p1)], [(c0, W * 4), (c1, cols1 * 4 + 20)]


@pytest.mark.parametrize("composite", [False, True], ids=["plain", "composite"])
@pytest.mark.parametrize("shader, sampler", [(CD.CH, "declared"), (CD.RM, "lod0")])
def test_a_batch_is_its_views_own_draws(vectors, shader, sampler, composite):
    _, base = vectors
    depth, layout = _batch_layout(base)
    lib = N.load()
    node = _node(_case(shader, "P_space"), sampler, cloud_detail=True)

    def batch(entry):
        deps, cols = _batch_buffers(depth, composite)
        views = (N.AtmoViewDepthTarget * 3)()
        for i, (cam, rect, time, pair, doff, coff) in enumerate(layout):
            views[i].frame = node.prepare_frame(cam, time=time, rect=rect)
            views[i].depth = N.AtmoDepth(deps[pair][0].data_ptr() + doff, N.DEPTH_D16_UNORM, deps[pair][1])
            views[i].target = N.AtmoTarget(cols[pair][0].data_ptr() + coff, N.TARGET_RGBA8_SRGB, cols[pair][1])
        node._bake_if_needed(torch.cuda.current_stream().cuda_stream)
        N.check(node._ctx, getattr(lib, entry)(node._ctx, views, 3, int(composite), _stream()))
        torch.cuda.synchronize()
        return [c.cpu().numpy() for c, _ in cols], node.kernel_name

    def singles(entry):
        deps, cols = _batch_buffers(depth, composite)
        for cam, rect, time, pair, doff, coff in layout:
            _draw(node, cam, time, deps[pair][0], N.DEPTH_D16_UNORM, deps[pair][1], cols[pair][0], "rgba8_srgb", cols[pair][1], composite=composite, rect=rect,
                  entry=entry, depth_off=doff, target_off=coff)
        return [c.cpu().numpy() for c, _ in cols]

    try:
        untouched = [c.cpu().numpy() for c, _ in _batch_buffers(depth, composite)[1]]
        got, name = batch("atmo_render_views_detail_target")
        assert name == _name(shader, sampler, views=True), name
        want = singles("atmo_render_detail_target")
        for g, w, u in zip(got, want, untouched):
            assert g.tobytes() == w.tobytes() and g.tobytes() != u.tobytes()
        # each view's time is its own frame's: the third view drawn at the others' time is another picture
        cam, rect, _, pair, doff, coff = layout[2]
        deps, cols = _batch_buffers(depth, composite)
        other = _draw(node, cam, CD.T1, deps[pair][0], N.DEPTH_D16_UNORM, deps[pair][1], cols[pair][0], "rgba8_srgb", cols[pair][1], composite=composite, rect=rect)
        assert other.tobytes() != got[1].tobytes()
        # the switch off: the call is atmo_render_views_depth_target
        node.cloud_detail = False
        got_off, name_off = batch("atmo_render_views_detail_target")
        old_off, name_old = batch("atmo_render_views_depth_target")
        assert name_off == name_old and name_off.startswith("atmo_render_views_depth_target_kernel<")
        for g, w, on in zip(got_off, old_off, got):
            assert g.tobytes() == w.tobytes() and g.tobytes() != on.tobytes()
    finally:
        node.close()


# ---- (g) graph capture -------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_draw_replays_onto_two_depth_contents(vectors):
    _, base = vectors
    cam = RSC.camera_from_fixture(base, W, H, "P_space")
    depths = [np.array(base["depth_demo_P_space"], dtype=np.float32), np.zeros((H, W), dtype=np.float32)]     # the scene's, and the far plane everywhere
    lib = N.load()
    node = _node(_case(CD.RM, "P_space"), "declared", cloud_detail=True)
    try:
        want = []
        for d in depths:
            dbuf, dfmt, dpitch, _ = _depth_buffer(d, "d16", pad=2)
            want.append(_draw(node, cam, CD.T1, dbuf, dfmt, dpitch, _buffer(H, W * 8, pad=16, fill=SENTINEL), "rgba16f", W * 8 + 16))
        assert want[0].tobytes() != want[1].tobytes()
        dbuf, dfmt, dpitch, _ = _depth_buffer(depths[0], "d16", pad=2)
        out = _buffer(H, W * 8, pad=16, fill=SENTINEL)
        frame = node.prepare_frame(cam, time=CD.T1)
        dep, tgt = N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch), N.AtmoTarget(out.data_ptr(), N.TARGET_RGBA16F, W * 8 + 16)
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):     # one stream, no parallel branches
                N.check(node._ctx, lib.atmo_render_detail_target(node._ctx, C.byref(frame), C.byref(dep), C.byref(tgt), 0, C.c_void_p(side.cuda_stream)))
        torch.cuda.synchronize()
        assert node.kernel_name == _name(CD.RM, "declared")
        for d, w in zip(depths, want):
            dbuf.copy_(_depth_buffer(d, "d16", pad=2)[0])
            out.fill_(SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == w.tobytes()
    finally:
        node.close()


# ---- (h) the binding ---------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_writes_the_c_calls_bytes(vectors):
    _, base = vectors
    cam, depth = RSC.camera_from_fixture(base, W, H, "P_space"), np.array(base["depth_demo_P_space"], dtype=np.float32)
    node = _node(_case(CD.CH, "P_space"), "declared", cloud_detail=True)
    try:
        dbuf, dfmt, dpitch, _ = _depth_buffer(depth)
        want = _draw(node, cam, CD.T1, dbuf, dfmt, dpitch, _buffer(H, W * 8, fill=SENTINEL), "rgba16f", 0)
        out = node.render(cam, _dev(depth), time=CD.T1, target="rgba16f")
        torch.cuda.synchronize()
        assert out.dtype == torch.float16 and node.kernel_name == _name(CD.CH, "declared")
        assert out.cpu().numpy().tobytes() == want.tobytes()
        # a depth_source and a float tensor: the same entry point, RGBA32F
        q = D.quantise(depth, "d16")
        src = depth_source(torch.from_numpy(q.view(np.int16)).cuda(), "d16")
        got = node.render(cam, src, time=CD.T1)
        torch.cuda.synchronize()
        assert node.kernel_name == _name(CD.CH, "declared")
        assert got.cpu().numpy().tobytes() == _float_frame(node, cam, D.decode(q, "d16"), CD.T1).tobytes()
        # render_views with targets: each view its own render(..., target=...)
        cams = [S.Camera.from_pose(HALF, H, "P_space"), S.Camera.from_pose(HALF, H, "P_limb")]
        halves = [_dev(depth[:, :HALF]), _dev(depth[:, HALF:])]
        image = torch.full((H, W, 4), SENTINEL, dtype=torch.uint8, device="cuda")
        node.render_views(cams, halves, [image[:, :HALF], image[:, HALF:]], time=CD.T1, target="rgba8_srgb")
        torch.cuda.synchronize()
        assert node.kernel_name == _name(CD.CH, "declared", views=True)
        singles = [node.render(c, d, time=CD.T1, target="rgba8_srgb") for c, d in zip(cams, halves)]
        torch.cuda.synchronize()
        assert node.kernel_name == _name(CD.CH, "declared")
        assert image.cpu().numpy().tobytes() == torch.cat(singles, dim=1).cpu().numpy().tobytes()
        # the float-only batch keeps raising
        with pytest.raises(N.AtmoError) as e:
            node.render_views(cams, halves, time=CD.T1)
        assert e.value.code == N.ATMO_E_STATE and "cloud detail" in str(e.value)
    finally:
        node.close()
