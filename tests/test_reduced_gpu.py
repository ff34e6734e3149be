"""Reduced-resolution draws on the device (include/atmo_reduced.h).  Needs an MI355X.  Every comparison is BIT-EXACT against the numpy statement,
godot_atmosphere_shader_amd/reduced.py.  Sizes: 37 x 23 (odd, partial blocks, one workgroup), 64 x 40 (divisible), 70 x 46 (two workgroups across).

 (a) the reduction: sizes x scales x the three depth formats x four projections, one pitched source, sky patches and a NaN;
 (b) the upsample: random low frames with zero pixels, values above 1 and a depth edge, into all seven formats, plain and composite, tol 0 and 0.1; a
     pitched target whose padding survives; in a composite the pixels without alpha keep their bytes, a -0 included;
 (c) end to end: the scratch's low depth is atmo_reduced_depth's, its low frame atmo_render's of low_frame on that depth, the target the statement's
     upsample of the two -- for no_clouds, clouds_high, clouds_high_rm under the declared sampler and clouds_high with cloud detail; a captured call
     replays to the same bytes;
 (d) render_reduced writes the C call's bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import cameras as K
from common import demo_params, demo_textures, make_node
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import depth_formats as D
from godot_atmosphere_shader_amd import reduced as R
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T
from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame, depth_source

pytestmark = pytest.mark.gpu
FORMATS = ["rgba32f", "rgba16f", "rgba8", "rgba8_srgb", "bgra8", "bgra8_srgb", "a2b10g10r10"]
SENTINEL = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def lib():
    return R.bind()


_nodes = {}


def _node(config, **kw):
    """One node per configuration for the whole module (closed at its end), its LUT baked by a first draw."""
    key = (config, tuple(sorted(kw.items())))
    if key not in _nodes:
        node = make_node(config, demo_textures(), demo_params(), sampler="declared", **kw)
        cam = S.Camera.from_pose(16, 8, "P_space")
        node.render(cam, _dev(S.depth_far(cam)))
        torch.cuda.synchronize()
        _nodes[key] = node
    return _nodes[key]


@pytest.fixture(scope="module", autouse=True)
def _close_nodes():
    yield
    for node in _nodes.values():
        node.close()
    _nodes.clear()


def _camera(kind, w, h):
    if kind == "forward_z":
        return S.Camera.from_pose(w, h, "P_limb", reverse_z=False)
    return K.from_pose(kind, w, h, "P_limb", **(dict(ortho_size=300.0) if kind == "ortho" else {}))


def _scene_depth(cam, rng, nan=False):
    """Depth with structure: random depths in front of the far plane, patches of sky (the far plane's exact value), one NaN."""
    h, w = cam.height, cam.width
    far = np.float32(0.0 if cam.reverse_z else 1.0)
    d = rng.uniform(0.05, 0.95, (h, w)).astype(np.float32)
    d[rng.random((h, w)) < 0.2] = far
    d[: h // 3, w // 2:] = far
    d[h // 2:, : w // 4] = np.float32(0.5)                  # a constant patch: ties inside a block keep the first texel
    if nan:
        d[h // 2, w // 2 + 1] = np.nan
        d[4, 8] = np.nan                                    # the first texel of a block for both scales
    return d


def _depth_buffer(depth_np, fmt, pad=0):
    """(device bytes, AtmoDepth format, pitch, the decoded depth the kernels read) of `depth_np` quantised to `fmt`, rows `pad` texels further apart."""
    q = D.quantise(depth_np, fmt)
    if fmt == "x8d24":
        q = q | (np.random.default_rng(3).integers(0, 256, size=q.shape, dtype=np.uint32) << 24)     # a stencil byte, ignored
    tb = D.TEXEL_BYTES[D.format_id(fmt)]
    host = np.full((q.shape[0], (q.shape[1] + pad) * tb), 0xFF, dtype=np.uint8)
    host[:, :q.shape[1] * tb] = _bits(q).reshape(q.shape[0], -1)
    return torch.from_numpy(host).cuda(), D.format_id(fmt), (0 if pad == 0 else host.shape[1]), D.decode(q, fmt)


def _frames(node, cam, time=0.0):
    d = node.make_frame(cam, time)
    return d, _to_native_frame(d)


# ---- (a) the reduction ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "forward_z", "ortho", "eye_left"])
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("size", [(37, 23), (64, 40)])
def test_the_reduction_is_the_statement_s(lib, size, s, kind):
    node = _node("no_clouds_8")
    cam = _camera(kind, *size)
    fd, nf = _frames(node, cam)
    lw, lh = R.low_size(*size, s)
    rng = np.random.default_rng(size[0] * 10 + s)
    for fmt, pad, nan in (("d32f", 0, True), ("d16", 0, False), ("x8d24", 0, False), ("d16", 3, False), ("d32f", 5, True)):
        buf, dfmt, pitch, decoded = _depth_buffer(_scene_depth(cam, rng, nan), fmt, pad)
        want = R.reduce_depth(fd, decoded, s)
        out = torch.full((lh * lw + 8,), -7.0, dtype=torch.float32, device="cuda")       # a guard behind the low image
        src = N.AtmoDepth(buf.data_ptr(), dfmt, pitch)
        N.check(node._ctx, lib.atmo_reduced_depth(node._ctx, C.byref(nf), C.byref(src), s, C.c_void_p(out.data_ptr()), _stream()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[lh * lw:] == -7.0)
        assert got[:lh * lw].view(np.uint32).tolist() == want.reshape(-1).view(np.uint32).tolist(), (fmt, pad)
        if nan:
            assert np.isnan(want).sum() == 1     # the NaN that is a block's first texel stays, the other never replaces a choice


# ---- (b) the upsample ---------------------------------------------------------------------------------------------------------------------------------------
def _edge_scene(cam, rng, s):
    """A depth edge: a slanted near bar and a near disc (depths within the 0.1 tolerance of each other) over the far plane's exact value."""
    h, w = cam.height, cam.width
    y, x = np.mgrid[0:h, 0:w]
    near = (np.abs((x - 6) - 0.6 * (y - 2)) < 4.5) | ((x - 0.7 * w) ** 2 + (y - 0.55 * h) ** 2 < (0.2 * h) ** 2)
    far = np.float32(0.0 if cam.reverse_z else 1.0)
    depth = np.where(near, rng.uniform(0.30, 0.33, (h, w)), far).astype(np.float32)
    return depth


def _low_frame(rng, lh, lw):
    """A random low frame: colours up to 1.6, alpha in [0, 1], a quarter of the pixels (0, 0, 0, 0) and a whole corner of them, so that full pixels
    without any alpha exist."""
    rgba = rng.uniform(0.0, 1.6, (lh, lw, 4)).astype(np.float32)
    rgba[..., 3] = rng.uniform(0.0, 1.0, (lh, lw)).astype(np.float32)
    rgba[rng.random((lh, lw)) < 0.25] = 0.0
    rgba[lh // 2:, : lw // 3] = 0.0
    return rgba


def _target_buffer(rng, fmt, h, w, pad_bytes, composite):
    """(device bytes (h, row + pad), the destination as the format's (h, w, 4) array): seeded colours for a composite -- with -0 in every channel of some
    float pixels --, the sentinel otherwise; the padding is the sentinel."""
    f = T.format_id(fmt)
    px = T.PIXEL_BYTES[f]
    if composite:
        dst = T.encode(rng.uniform(0.0, 1.5, (h, w, 4)).astype(np.float32), f)
        if f in (T.RGBA32F, T.RGBA16F):
            dst[rng.random((h, w)) < 0.3] = -0.0
    else:
        dst = np.full((h, w * px), SENTINEL, dtype=np.uint8).view(T.DTYPES[f]).reshape(h, w, 4)
    host = np.full((h, w * px + pad_bytes), SENTINEL, dtype=np.uint8)
    host[:, :w * px] = _bits(dst).reshape(h, w * px)
    return torch.from_numpy(host).cuda(), dst


def _upsample(lib, node, nf, src, s, tol, low_depth, low_rgba, buf, fmt, pitch, composite):
    opt, tgt = R.AtmoReduced(s, tol), N.AtmoTarget(buf.data_ptr(), T.format_id(fmt), pitch)
    ld, lc = _dev(low_depth), _dev(low_rgba)
    N.check(node._ctx, lib.atmo_reduced_upsample(node._ctx, C.byref(nf), C.byref(src), C.byref(opt), C.c_void_p(ld.data_ptr()), C.c_void_p(lc.data_ptr()),
                                                  C.byref(tgt), int(composite), _stream()))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("composite", [False, True], ids=["plain", "composite"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_upsample_is_the_statement_s_in_every_format(lib, fmt, composite):
    node = _node("no_clouds_8")
    px = T.PIXEL_BYTES[T.format_id(fmt)]
    fallback = 0
    for (w, h), s, tol, pad, kind in (((37, 23), 2, 0.1, 0, "plain"), ((37, 23), 4, 0.0, 0, "plain"), ((70, 46), 4, 0.1, 2 * px, "eye_left"),
                                      ((64, 40), 2, 0.0, 0, "forward_z")):
        rng = np.random.default_rng(w + s + int(composite))
        cam = _camera(kind, w, h)
        fd, nf = _frames(node, cam)
        depth = _edge_scene(cam, rng, s)
        dbuf, dfmt, dpitch, decoded = _depth_buffer(depth, "d32f" if s == 2 else "d16", pad=1 if pad else 0)
        low_depth = R.reduce_depth(fd, decoded, s)
        low_rgba = _low_frame(rng, *low_depth.shape)
        pixels, det = R.upsample(fd, decoded, low_depth, low_rgba, s, tol, details=True)
        fallback += int((~det["agree"].any(axis=0)).sum())
        assert (det["agree"].any(axis=0) & ~det["agree"].all(axis=0)).sum() > 100                  # partial sums along the edge
        clear = ~(pixels[..., 3] > 0)
        assert clear.sum() > 10 and (~clear).sum() > 100
        buf, dst = _target_buffer(rng, fmt, h, w, pad, composite)
        want = R.store(pixels, fmt, dst, composite)
        got = _upsample(lib, node, nf, N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch), s, tol, low_depth, low_rgba, buf, fmt, w * px + pad if pad else 0, composite)
        assert got[:, :w * px].tobytes() == _bits(want).reshape(h, w * px).tobytes(), (w, h, s, tol)
        assert np.all(got[:, w * px:] == SENTINEL)                                                  # bytes between rows are never written
        if composite:   # the pixels without alpha keep their bytes (a -0 among them in the float formats)
            kept = got[:, :w * px].reshape(h, w, px)[clear]
            assert kept.tobytes() == _bits(dst).reshape(h, w, px)[clear].tobytes()
            if fmt in ("rgba32f", "rgba16f"):
                assert np.signbit(dst[clear]).any()
    assert fallback > 100      # pixels without a neighbour at their depth: under tol 0 most of the near surface, under 0.1 the tips of the bar


# ---- (c) end to end -----------------------------------------------------------------------------------------------------------------------------------------
CONTEXTS = [("no_clouds_8", {}), ("clouds_high", {}), ("clouds_high_rm", {}), ("clouds_high", dict(cloud_detail=True))]


def _reduced(lib, node, nf, src, s, tol, scratch, buf, fmt, pitch, composite, stream=None):
    opt, tgt = R.AtmoReduced(s, tol), N.AtmoTarget(buf.data_ptr(), T.format_id(fmt), pitch)
    N.check(node._ctx, lib.atmo_render_reduced_target(node._ctx, C.byref(nf), C.byref(src), C.byref(opt), C.c_void_p(scratch.data_ptr()), C.byref(tgt),
                                                       int(composite), stream if stream is not None else _stream()))


@pytest.mark.parametrize("size,s", [((70, 46), 4), ((64, 40), 2)], ids=["70x46s4", "64x40s2"])
@pytest.mark.parametrize("config,kw", CONTEXTS, ids=["no_clouds", "clouds_high", "clouds_high_rm", "clouds_high_detail"])
def test_the_whole_path_is_its_three_steps(lib, config, kw, size, s):
    node = _node(config, **kw)
    w, h = size
    cam = S.Camera.from_pose(w, h, "P_limb")
    time = 12.5 if kw else 0.0
    fd, nf = _frames(node, cam, time)
    depth = S.depth_ground_sphere(cam)
    dbuf, dfmt, dpitch, decoded = _depth_buffer(depth, "d32f")
    src = N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch)
    lw, lh = R.low_size(w, h, s)
    depth_floats, nbytes = R.scratch_layout(w, h, s)
    tol = 0.1
    rng = np.random.default_rng(w)
    results = {}
    for fmt, composite in (("rgba16f", True), ("rgba32f", False)):
        px = T.PIXEL_BYTES[T.format_id(fmt)]
        scratch = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
        buf, dst = _target_buffer(rng, fmt, h, w, 0, composite)
        _reduced(lib, node, nf, src, s, tol, scratch, buf, fmt, 0, composite)
        torch.cuda.synchronize()
        name = node.kernel_name
        assert name.startswith("atmo_render_detail_kernel<" if kw else "atmo_render_kernel<"), name
        sc = scratch.cpu().numpy()
        low_depth, low_rgba = sc[:lw * lh].reshape(lh, lw), sc[depth_floats:].reshape(lh, lw, 4)
        # step 1: atmo_reduced_depth's, which is the statement's
        alone = torch.empty(lw * lh, dtype=torch.float32, device="cuda")
        N.check(node._ctx, lib.atmo_reduced_depth(node._ctx, C.byref(nf), C.byref(src), s, C.c_void_p(alone.data_ptr()), _stream()))
        torch.cuda.synchronize()
        assert low_depth.tobytes() == alone.cpu().numpy().tobytes() == R.reduce_depth(fd, decoded, s).tobytes()
        # step 2: atmo_render of the statement's low frame on that depth
        low_nf = _to_native_frame(R.low_frame(fd, s))
        ref = torch.empty((lh, lw, 4), dtype=torch.float32, device="cuda")
        N.check(node._ctx, lib.atmo_render(node._ctx, C.byref(low_nf), C.c_void_p(alone.data_ptr()), C.c_void_p(ref.data_ptr()), _stream()))
        torch.cuda.synchronize()
        assert node.kernel_name == name
        assert low_rgba.tobytes() == ref.cpu().numpy().tobytes()
        assert 0.05 < (low_rgba[..., 3] > 0).mean() < 0.999, "the frame must show the atmosphere and something else"
        # step 3: the statement's upsample of the two
        want = R.store(R.upsample(fd, decoded, low_depth, low_rgba, s, tol), fmt, dst, composite)
        got = buf.cpu().numpy()
        assert got.tobytes() == _bits(want).reshape(h, w * px).tobytes(), (fmt, composite)
        results[fmt] = (got, dst)
    # one graph-captured call replays to the same bytes
    got, dst = results["rgba16f"]
    scratch = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    out = _dev(_bits(dst).reshape(h, w * 8))
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):     # one stream, no parallel branches
            _reduced(lib, node, nf, src, s, tol, scratch, out, "rgba16f", 0, True, stream=C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    out.copy_(_dev(_bits(dst).reshape(h, w * 8)))
    scratch.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == got.tobytes()


# ---- (d) the binding ----------------------------------------------------------------------------------------------------------------------------------------
def test_render_reduced_writes_the_c_call_s_bytes(lib):
    node = _node("clouds_high")
    w, h, s, tol = 70, 46, 4, 0.05
    cam = S.Camera.from_pose(w, h, "P_limb")
    fd, nf = _frames(node, cam)
    depth = S.depth_ground_sphere(cam)
    rng = np.random.default_rng(5)
    # plain, allocated by the call, from a float depth tensor
    dbuf, dfmt, dpitch, _ = _depth_buffer(depth, "d32f")
    scratch = torch.empty(R.scratch_layout(w, h, 2)[1], dtype=torch.uint8, device="cuda")     # (the larger of the two scales' below)
    buf, _ = _target_buffer(rng, "rgba16f", h, w, 0, False)
    _reduced(lib, node, nf, N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch), s, tol, scratch, buf, "rgba16f", 0, False)
    out = node.render_reduced(cam, _dev(depth), target="rgba16f", scale=s, depth_tolerance=tol)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and tuple(out.shape) == (h, w, 4)
    assert _bits(out.cpu().numpy()).tobytes() == buf.cpu().numpy().tobytes()
    own = node._reduced_scratch_tensor
    # composite into a pitched uint8 sRGB buffer from a pitched D16 source, the caller's scratch
    dbuf, dfmt, dpitch, _ = _depth_buffer(depth, "d16", pad=3)
    buf, dst = _target_buffer(rng, "rgba8_srgb", h, w, 8, True)
    twin = buf.clone()
    _reduced(lib, node, nf, N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch), 2, tol, scratch, buf, "rgba8_srgb", w * 4 + 8, True)
    d16 = dbuf.view(torch.int16).view(h, w + 3)[:, :w]
    view = twin.view(h, w + 2, 4)[:, :w]
    assert node.render_reduced(cam, depth_source(d16), "rgba8_srgb", view, scale=2, depth_tolerance=tol, composite=True, scratch=scratch) is view
    torch.cuda.synchronize()
    assert twin.cpu().numpy().tobytes() == buf.cpu().numpy().tobytes() != _bits(dst).tobytes()
    assert node._reduced_scratch_tensor is own                                          # the caller's scratch was used
    with pytest.raises(ValueError):
        node.render_reduced(cam, _dev(depth), scale=3)
    with pytest.raises(ValueError):
        node.render_reduced(cam, _dev(depth), composite=True)
    with pytest.raises(ValueError):
        node.render_reduced(cam, _dev(depth), scratch=scratch[:64])
