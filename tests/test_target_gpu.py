"""GPU tests of the packed colour targets (include/atmo_target.h): atmo_render_target / atmo_render_proxy_target into RGBA16F and RGBA8_UNORM buffers,
tight and with a row pitch, plain and composite.  Every comparison against the contract is BIT-EXACT (np.array_equal on the raw 16- / 8-bit patterns; no
tolerance): the statement is godot_atmosphere_shader_amd/targets.py (encode / decode / blend in numpy), the fp32 input is atmo_render's own frame.
One test goes to the oracle directly, with the formats' own half-ulp as its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import proxy_geometry as G
from common import CONFIGS, TOL, demo_frame, demo_params, demo_textures, has_clouds, make_node, oracle_inputs
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T

pytestmark = pytest.mark.gpu

FORMATS = ("rgba16f", "rgba8")
TORCH_DTYPE = {"rgba16f": torch.float16, "rgba8": torch.uint8, "rgba32f": torch.float32}
BITS = {"rgba16f": np.uint16, "rgba8": np.uint8, "rgba32f": np.uint32}
W, H = 251, 141           # an odd size: partial tiles on both edges, odd rows of quads
PAD = 7                   # pixels of padding per row in the pitched draws
SENTINEL = {"rgba16f": 0x5A5A, "rgba8": 0xA5}


def _bits(t, fmt):
    """The raw patterns of a (…, 4) target tensor as a numpy array."""
    a = t.detach().cpu().numpy()
    return a.view(BITS[fmt])


def _from_bits(bits, fmt):
    """A CUDA tensor holding the given raw patterns."""
    a = np.ascontiguousarray(bits, dtype=BITS[fmt]).view(T.DTYPES[T.format_id(fmt)])
    return torch.from_numpy(a).cuda()


def _random_dst(shape, fmt, seed):
    """A pseudo-random destination: all finite half patterns / all bytes are drawn from."""
    rng = np.random.default_rng(seed)
    if fmt == "rgba8":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    allh = np.arange(65536, dtype=np.uint16)
    finite = allh[(allh & 0x7C00) != 0x7C00]
    return finite[rng.integers(0, finite.size, size=shape)]


# ---- the store / blend on chosen values (atmo_debug_store_target) -------------------------------------------------------------------------

def _chosen_sources():
    f32 = np.float32
    allh = np.arange(65536, dtype=np.uint16)
    finite = allh[(allh & 0x7C00) != 0x7C00].view(np.float16).astype(f32)                   # every finite half value (both zeros)
    pos = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)             # 0 .. 65504, ascending
    nxt = np.append(pos[1:], 65536.0)                                                        # the value after 65504 on the half grid, were it finite
    mid = ((pos + nxt) / 2.0).astype(f32)                                                    # the ties: exactly representable in fp32 (65520 the last)
    assert np.array_equal(mid.astype(np.float64), (pos + nxt) / 2.0)
    ties = np.concatenate([mid, np.nextafter(mid, f32(0.0)), np.nextafter(mid, f32(np.inf))])
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 65504.0, 65519.996, 65520.0, 65536.0, 1e5, 3.0e38, -65519.996, -65520.0, -1e5, -3.0e38], dtype=f32)
    grid = np.linspace(-0.5, 1.5, 2 ** 17 + 1, dtype=np.float64).astype(f32)
    k = np.arange(255)
    half_steps = ((k + 0.5) / 255.0).astype(f32)
    half_steps = np.concatenate([half_steps, np.nextafter(half_steps, f32(0.0)), np.nextafter(half_steps, f32(1.0)), (np.arange(256) / 255.0).astype(f32)])
    return np.concatenate([finite, ties, -ties, special, grid, half_steps]).astype(f32)


@pytest.mark.parametrize("composite", [0, 1], ids=["plain", "composite"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_store_target_matches_the_statement(fmt, composite):
    """The kernels' store_target<FMT> against targets.py: sources = every finite half value, every tie between neighbouring half values and the tie's two
    fp32 neighbours, NaN, infinities, values beyond 65504, [-0.5, 1.5] on a 2^-16 grid, every (k + 0.5) / 255 and its fp32 neighbours; destinations = all
    finite half patterns / all bytes; source alphas of the composite from {0, 2^-24, 1/3, 0.5, 1}; paired by fixed pseudo-random permutations."""
    lib = N.load()
    ctx = C.c_void_p()
    assert lib.atmo_create(0, N.VARIANT_NO_CLOUDS, 0, 0, N.LIGHT_DIRECT, 8, C.byref(ctx)) == N.ATMO_OK
    try:
        values = _chosen_sources()
        n = 1 << 20
        assert values.size < n
        rng = np.random.default_rng(20260 + 2 * T.format_id(fmt) + composite)
        src = np.empty((n, 4), dtype=np.float32)
        for c in range(4):
            src[:, c] = values[rng.permutation(n) % values.size]        # every chosen value appears in every channel, against ever different partners
        if composite:
            alphas = np.array([0.0, 2.0 ** -24, 1.0 / 3.0, 0.5, 1.0], dtype=np.float32)
            src[:, 3] = alphas[rng.permutation(n) % alphas.size]
        dst_bits = _random_dst((n, 4), fmt, 7)
        pool = np.unique(dst_bits)
        assert pool.size == (256 if fmt == "rgba8" else 65536 - 2048)   # all bytes / all finite half patterns occur
        dst_host = dst_bits.view(T.DTYPES[T.format_id(fmt)])
        want = T.blend(src, dst_host, fmt) if composite else T.encode(src, fmt)
        src_dev, dst_dev = torch.from_numpy(src).cuda(), _from_bits(dst_bits, fmt)
        rc = lib.atmo_debug_store_target(ctx, T.format_id(fmt), composite, C.c_void_p(src_dev.data_ptr()), C.c_void_p(dst_dev.data_ptr()), n, None)
        assert rc == N.ATMO_OK, lib.atmo_last_error_string(ctx)
        torch.cuda.synchronize()
        got = _bits(dst_dev, fmt)
        wantb = want.view(BITS[fmt])
        bad = np.argwhere(got != wantb)
        if bad.size:
            i, c = bad[0]
            print(f"\n{len(bad)} mismatches; first: pixel {i} channel {c}: src {src[i]!r} ({src[i].view(np.uint32)}), dst {dst_bits[i]}, got {got[i, c]:#x}, want {wantb[i, c]:#x}")
        assert np.array_equal(got, wantb)
        # the comparison was not about nothing: the expected patterns hold the cases the contract names
        if fmt == "rgba16f":
            assert (wantb == 0x7C00).any() and (wantb == 0xFC00).any() and (wantb == T.HALF_QNAN).any() and (wantb == 0x7BFF).any()
            assert ((wantb & 0x7C00) == 0).sum() > 1000 and (wantb == 0x8000).any()             # subnormals and -0
        else:
            assert np.unique(wantb).size == 256
        if not composite:   # RGBA32F through the same function is a copy
            out32 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            assert lib.atmo_debug_store_target(ctx, N.TARGET_RGBA32F, 0, C.c_void_p(src_dev.data_ptr()), C.c_void_p(out32.data_ptr()), n, None) == N.ATMO_OK
            torch.cuda.synchronize()
            assert np.array_equal(out32.cpu().numpy().view(np.uint32), src.view(np.uint32))
    finally:
        lib.atmo_destroy(ctx)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------

FRAME_CASES = [("no_clouds_8", "declared"), ("no_clouds_32x8_direct", "declared")] + [(c, s) for c in ("clouds_high", "clouds_high_rm", "v1_clouds")
                                                                                      for s in ("declared", "lod0")]


def _float_frame(node, cam, depth, rect=None):
    """atmo_render's fp32 frame and its discard mask (the pixels a cleared-target draw leaves alone)."""
    frame = node.render(cam, depth, rect=rect)
    torch.cuda.synchronize()
    return frame.cpu().numpy()


def _discard_mask(config, sampler, cam, depth, tex, kw=None):
    """Which pixels are discarded: a float draw with atmo_set_target_cleared into a NaN-filled buffer leaves exactly those untouched."""
    node = make_node(config, tex, sampler=sampler, target_cleared=True, **(kw or {}))
    out = torch.full((cam.height, cam.width, 4), float("nan"), dtype=torch.float32, device="cuda")
    node.render(cam, depth, out=out)
    torch.cuda.synchronize()
    node.close()
    return torch.isnan(out).all(dim=-1).cpu().numpy()


def _pitched(rows, cols, fmt, fill_bits):
    """A (rows, cols, 4) view with a row stride of cols + PAD pixels into a sentinel-filled buffer; returns (view, whole buffer)."""
    whole = _from_bits(np.full((rows, cols + PAD, 4), fill_bits, dtype=BITS[fmt]), fmt)
    return whole[:, :cols, :], whole


def _check_frame(config, sampler, pose, w, h, repeats=1):
    tex = demo_textures()
    cam = S.Camera.from_pose(w, h, pose)
    depth_np = S.depth_ground_sphere(cam)
    depth = torch.from_numpy(depth_np).cuda()
    node = make_node(config, tex, sampler=sampler)
    ref = _float_frame(node, cam, depth)
    discarded = _discard_mask(config, sampler, cam, depth, tex)
    kept = ~discarded
    # no branch is tested on nothing
    assert kept.mean() >= 0.25 and discarded.mean() >= 0.25, (kept.mean(), discarded.mean())
    assert np.all(ref[discarded] == 0.0)
    if (config == "clouds_high" and pose == "P_space") or config == "v1_clouds":
        assert (ref > 1.0).any(), "no channel above 1: the UNORM clamp is not exercised"
    if config == "v1_clouds":
        assert ((ref != 0.0) & (np.abs(ref) < 2.0 ** -14)).any(), "no binary16 subnormal in the frame"
    print(f"\n{config} {sampler} {pose} {w}x{h}: kept {kept.mean():.3f}, discarded {discarded.mean():.3f}, channels > 1: {(ref > 1.0).sum()}, "
          f"non-zero below 2^-14: {((ref != 0.0) & (np.abs(ref) < 2.0 ** -14)).sum()}, max {ref.max():.4f}")
    for fmt in FORMATS:
        want_plain = T.encode(ref, fmt).view(BITS[fmt])
        dst_bits = _random_dst((h, w, 4), fmt, 11)
        want_blend = T.blend(ref, dst_bits.view(T.DTYPES[T.format_id(fmt)]), fmt).view(BITS[fmt]).copy()
        want_blend[discarded] = dst_bits[discarded]             # a composite never stores a discarded fragment
        for _ in range(repeats):                                # (repeats > 1: the learnt tile order and the heavy-tile split come in after a few draws)
            got = node.render(cam, depth, out=_from_bits(np.full((h, w, 4), SENTINEL[fmt], dtype=BITS[fmt]), fmt))
            torch.cuda.synchronize()
            assert np.array_equal(_bits(got, fmt), want_plain), (fmt, "plain")
            scene = node.render_composite(cam, depth, _from_bits(dst_bits, fmt))
            torch.cuda.synchronize()
            assert np.array_equal(_bits(scene, fmt), want_blend), (fmt, "composite")
        assert "target" in node.kernel_name, node.kernel_name
        alloc = node.render(cam, depth, target=fmt)             # the allocating form
        torch.cuda.synchronize()
        assert alloc.dtype == TORCH_DTYPE[fmt] and np.array_equal(_bits(alloc, fmt), want_plain)
        # pitch: a row stride of w + 7 pixels; the padding keeps its sentinel
        view, whole = _pitched(h, w, fmt, SENTINEL[fmt])
        node.render(cam, depth, out=view)
        torch.cuda.synchronize()
        wb = _bits(whole, fmt)
        assert np.array_equal(wb[:, :w], want_plain) and np.all(wb[:, w:] == SENTINEL[fmt]), (fmt, "pitched plain")
        view, whole = _pitched(h, w, fmt, SENTINEL[fmt])
        view.copy_(_from_bits(dst_bits, fmt))
        node.render_composite(cam, depth, view)
        torch.cuda.synchronize()
        wb = _bits(whole, fmt)
        assert np.array_equal(wb[:, :w], want_blend) and np.all(wb[:, w:] == SENTINEL[fmt]), (fmt, "pitched composite")
        # a sub-rect: the plain draw is the crop (tight and pitched), the composite touches the rect only
        x0, y0, x1, y1 = 37, 13, 171, 102
        crop = node.render(cam, depth, rect=(x0, y0, x1, y1), target=fmt)
        view, whole = _pitched(y1 - y0, x1 - x0, fmt, SENTINEL[fmt])
        node.render(cam, depth, out=view, rect=(x0, y0, x1, y1))
        scene = node.render_composite(cam, depth, _from_bits(dst_bits, fmt), rect=(x0, y0, x1, y1))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(crop, fmt), want_plain[y0:y1, x0:x1]), (fmt, "rect")
        wb = _bits(whole, fmt)
        assert np.array_equal(wb[:, :x1 - x0], want_plain[y0:y1, x0:x1]) and np.all(wb[:, x1 - x0:] == SENTINEL[fmt]), (fmt, "pitched rect")
        want_rect = dst_bits.copy()
        want_rect[y0:y1, x0:x1] = want_blend[y0:y1, x0:x1]
        assert np.array_equal(_bits(scene, fmt), want_rect), (fmt, "composite rect")
    stats = (node.feedback_stats(), node.split_stats())
    node.close()
    # atmo_set_target_cleared: discarded pixels keep the sentinel, kept pixels are the encoded frame
    cleared = make_node(config, tex, sampler=sampler, target_cleared=True)
    for fmt in FORMATS:
        got = cleared.render(cam, depth, out=_from_bits(np.full((h, w, 4), SENTINEL[fmt], dtype=BITS[fmt]), fmt))
        torch.cuda.synchronize()
        gb = _bits(got, fmt)
        assert np.all(gb[discarded] == SENTINEL[fmt]) and np.array_equal(gb[kept], T.encode(ref, fmt).view(BITS[fmt])[kept]), (fmt, "cleared")
    cleared.close()
    return stats


@pytest.mark.parametrize("pose", ["P_space", "P_limb"])
@pytest.mark.parametrize("config,sampler", FRAME_CASES, ids=[f"{c}-{s}" if has_clouds(c) else c for c, s in FRAME_CASES])
def test_packed_frame_is_the_encoded_float_frame(config, sampler, pose):
    _check_frame(config, sampler, pose, W, H)


@pytest.mark.parametrize("pose", ["P_space", "P_limb"])
def test_packed_frame_at_1920x1080_with_tile_order_and_heavy_split(pose):
    """clouds_high_rm under the declared sampler at 1920 x 1080, drawn often enough that the learnt tile order and the automatic heavy-tile lane split take part:
    the picture is the same bits whatever the launch."""
    feedback, split = _check_frame("clouds_high_rm", "declared", pose, 1920, 1080, repeats=8)
    print(f"\nclouds_high_rm {pose} 1920x1080: {feedback}, {split}")
    assert feedback["ordered_draws"] > 0 and feedback["sorts"] > 0
    if pose == "P_limb":   # where a draw is as long as its heaviest wavefront (the trigger of the split)
        assert split["split_draws"] > 0 and split["heavy_tiles_last"] > 0


@pytest.mark.parametrize("config,sampler", [("no_clouds_32x8_direct", "declared"), ("clouds_high", "declared"), ("clouds_high_rm", "lod0")])
def test_rgba32f_target_is_atmo_render_byte_for_byte(config, sampler):
    """RGBA32F through atmo_render_target, tight and pitched, plain and composite == atmo_render / atmo_render_composite."""
    tex = demo_textures()
    cam = S.Camera.from_pose(W, H, "P_space")
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    node = make_node(config, tex, sampler=sampler)
    ref = node.render(cam, depth)
    g = torch.Generator(device="cpu").manual_seed(5)
    scene0 = torch.rand((H, W, 4), generator=g, dtype=torch.float32).cuda()
    ref_c = node.render_composite(cam, depth, scene0.clone())
    lib, ctx = node._lib, node._ctx
    nf = node.prepare_frame(cam)
    stream = torch.cuda.current_stream().cuda_stream
    for pitch_px in (0, W, W + PAD):
        rowpx = pitch_px or W
        for composite, want, init in ((0, ref, None), (1, ref_c, scene0)):
            whole = torch.full((H, rowpx, 4), -7.0, dtype=torch.float32, device="cuda")
            if init is not None:
                whole[:, :W] = init
            t = N.AtmoTarget(whole.data_ptr(), N.TARGET_RGBA32F, pitch_px * 16)
            rc = lib.atmo_render_target(ctx, C.byref(nf), C.c_void_p(depth.data_ptr()), C.byref(t), composite, C.c_void_p(stream))
            assert rc == N.ATMO_OK, lib.atmo_last_error_string(ctx)
            torch.cuda.synchronize()
            assert torch.equal(whole[:, :W].contiguous().view(torch.int32), want.view(torch.int32)), (pitch_px, composite)
            assert bool((whole[:, W:] == -7.0).all())
            assert "target" not in node.kernel_name        # it IS the float kernel
    # the binding takes the pitch from a float32 tensor's row stride
    whole = torch.full((H, W + PAD, 4), -7.0, dtype=torch.float32, device="cuda")
    node.render(cam, depth, out=whole[:, :W])
    torch.cuda.synchronize()
    assert torch.equal(whole[:, :W].contiguous().view(torch.int32), ref.view(torch.int32)) and bool((whole[:, W:] == -7.0).all())
    node.close()


# ---- the proxy draw ---------------------------------------------------------------------------------------------------------------------------

def _proxy_poses():
    w, h = 96, 54
    yield "face_on", S.Camera(w, h, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0)), np.eye(4)
    yield "edge_on", S.Camera(w, h, (0.0, 0.0, 500.0), (0.0, 0.0, 0.0)), G.rotation_y(45.0)


@pytest.mark.parametrize("config", ["no_clouds_8", "no_clouds_32x8_direct", "clouds_high_rm", "v1_clouds"])
def test_proxy_target_is_the_encoded_proxy_frame(config):
    """atmo_render_proxy_target == encode / blend of atmo_render_proxy's float frame on the face-on and edge-on boxes; uncovered pixels untouched."""
    tex = demo_textures(cube_n=64, shape_n=32)
    for name, cam, model in _proxy_poses():
        node = make_node(config, tex)
        node.global_transform = model
        w, h = cam.width, cam.height
        depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
        marker = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
        ref_t = node.render_proxy(cam, depth, out=marker.clone())
        torch.cuda.synchronize()
        ref = ref_t.cpu().numpy()
        written = ~np.isnan(ref).all(axis=-1)                       # the passing fragments (shaded or discarded-and-zeroed)
        # (the box of edge 208 seen face-on from 600 away covers about 15 x 15 of these 96 x 54 pixels, edge-on from 500 about 25 x 17)
        assert 100 < written.sum() < w * h - 300, (name, written.sum())
        # the same with discards left alone: the pixels a composite blends
        cleared = make_node(config, tex, target_cleared=True)
        cleared.global_transform = model
        shaded_t = cleared.render_proxy(cam, depth, out=marker.clone())
        torch.cuda.synchronize()
        shaded = ~np.isnan(shaded_t.cpu().numpy()).all(axis=-1)
        cleared.close()
        assert shaded.sum() > 50 and not (shaded & ~written).any()
        for fmt in FORMATS:
            fill = _random_dst((h, w, 4), fmt, 23)
            want = fill.copy()
            want[written] = T.encode(ref, fmt).view(BITS[fmt])[written]
            got = node.render_proxy(cam, depth, out=_from_bits(fill, fmt))
            torch.cuda.synchronize()
            assert "proxy_target" in node.kernel_name, node.kernel_name
            assert np.array_equal(_bits(got, fmt), want), (name, fmt, "plain")
            want_c = fill.copy()
            want_c[shaded] = T.blend(np.nan_to_num(ref), fill.view(T.DTYPES[T.format_id(fmt)]), fmt).view(BITS[fmt])[shaded]
            scene = node.render_proxy_composite(cam, depth, _from_bits(fill, fmt))
            view, whole = _pitched(h, w, fmt, SENTINEL[fmt])
            view.copy_(_from_bits(fill, fmt))
            node.render_proxy_composite(cam, depth, view)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(scene, fmt), want_c), (name, fmt, "composite")
            wb = _bits(whole, fmt)
            assert np.array_equal(wb[:, :w], want_c) and np.all(wb[:, w:] == SENTINEL[fmt]), (name, fmt, "pitched composite")
            assert (want_c != fill).any()
        node.close()


def test_draw_atmospheres_passes_a_packed_target_through():
    from godot_atmosphere_shader_amd.planet_atmosphere import draw_atmospheres

    tex = demo_textures(cube_n=64, shape_n=32)
    cam = S.Camera(96, 54, (0.0, 0.0, 500.0), (0.0, 0.0, 0.0), far=5000.0)
    planet, moon = make_node("clouds", tex), make_node("no_clouds_8", tex)
    moon.planet_radius, moon.atmosphere_height = 27.0, 3.0
    for node, pos in ((planet, (0.0, 0.0, 0.0)), (moon, (6.0, 4.0, 455.0))):
        node.global_transform = G.translation(*pos)
        node._process(camera=cam, time=0.0)
    assert planet._mode == 1 and moon._mode == 0
    depth = torch.from_numpy(S.depth_far(cam)).cuda()
    fill = _random_dst((54, 96, 4), "rgba16f", 29)
    got = draw_atmospheres([planet, moon], cam, depth, _from_bits(fill, "rgba16f"))
    want = _from_bits(fill, "rgba16f")
    planet.render_proxy_composite(cam, depth, want)
    moon.render_composite(cam, depth, want)
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and np.array_equal(_bits(got, "rgba16f"), _bits(want, "rgba16f")) and (_bits(got, "rgba16f") != fill).any()
    planet.close()
    moon.close()


def test_packed_composite_replays_from_a_hip_graph():
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    cam = S.Camera.from_pose(W, H, "P_space")
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    fill = _random_dst((H, W, 4), "rgba16f", 31)
    ref = node.render_composite(cam, depth, _from_bits(fill, "rgba16f"))
    torch.cuda.synchronize()
    target = _from_bits(fill, "rgba16f")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            node.render_composite(cam, depth, target, stream=side)
    torch.cuda.synchronize()
    target.copy_(_from_bits(fill, "rgba16f"))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(target, "rgba16f"), _bits(ref, "rgba16f")) and (_bits(ref, "rgba16f") != fill).any()
    node.close()


# ---- against the oracle directly ----------------------------------------------------------------------------------------------------------------

def test_packed_frames_against_the_oracle(oracle32):
    """The chain does not rest on the float kernels alone: the decoded RGBA16F frame of clouds_high lies within TOL + 2^-11 |oracle| of the oracle (2^-11:
    binary16's half-ulp relative error in the normal range), the decoded RGBA8 frame within TOL + 0.5 / 255 of the oracle clamped to [0, 1]; the discard sets are
    identical."""
    tex, params = demo_textures(), demo_params()
    for pose in ("P_space", "P_limb"):
        cam = S.Camera.from_pose(W, H, pose)
        depth_np = S.depth_ground_sphere(cam)
        depth = torch.from_numpy(depth_np).cuda()
        node = make_node("clouds_high", tex, params, target_cleared=True)
        lut = node.read_optical_depth()
        ocfg, otex = oracle_inputs(oracle32, CONFIGS["clouds_high"][1], tex, lut)
        want, hits = oracle32.render(params, otex, ocfg, demo_frame(cam), depth_np, nthreads=8)
        assert hits > 0
        miss = np.all(want == 0.0, axis=-1)        # the oracle writes (0, 0, 0, 0) for a discarded fragment; a kept one has alpha > 0
        assert int((~miss).sum()) == hits
        assert 0.25 <= miss.mean() <= 0.75
        for fmt in FORMATS:
            got = node.render(cam, depth, out=_from_bits(np.full((H, W, 4), SENTINEL[fmt], dtype=BITS[fmt]), fmt))
            torch.cuda.synchronize()
            gb = _bits(got, fmt)
            untouched = np.all(gb == SENTINEL[fmt], axis=-1)
            assert np.array_equal(untouched, miss), (pose, fmt, "discard sets differ")
            dec = T.decode(gb.view(T.DTYPES[T.format_id(fmt)]), fmt)[~miss].astype(np.float64)
            o = want[~miss].astype(np.float64)
            if fmt == "rgba16f":
                err, bound = np.abs(dec - o), TOL + 2.0 ** -11 * np.abs(o)
            else:
                err, bound = np.abs(dec - np.clip(o, 0.0, 1.0)), TOL + 0.5 / 255.0
            print(f"\nclouds_high {pose} {fmt}: max |decoded - oracle| = {err.max():.3e}, worst excess over the bound {float((err - bound).max()):.3e}")
            assert np.all(err <= bound), (pose, fmt, float((err - bound).max()))
        node.close()


# ---- the native example ---------------------------------------------------------------------------------------------------------------------------

def test_native_host_draws_into_a_packed_target(tmp_path):
    """examples/atmo_render_file.cpp --target rgba16f | rgba8 (include/atmo_target.h + the HIP runtime only) writes the bytes the Python binding produces."""
    import os
    import shutil
    import subprocess

    from godot_atmosphere_shader_amd.build import LIB_PATH
    from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "atmo_render_file"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.run([hipcc, "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "atmo_render_file.cpp"),
                    "-L", libdir, "-latmo_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True)
    w, h = 96, 54
    cam = S.Camera.from_pose(w, h, "P_limb")
    depth_np = S.depth_ground_sphere(cam)
    tex = demo_textures(cube_n=16, shape_n=8)
    tex["blue_noise"] = np.zeros((256, 256), dtype=np.uint8)  # the native host leaves u_blue_noise_texture unset (zero)
    node = make_node("no_clouds_32_lut", tex, demo_params())
    node.set_shader_parameter("u_atmosphere_modulate", (1.0, 1.0, 1.0))
    node.set_shader_parameter("u_atmosphere_ambient_color", (0.0, 0.0, 0.002))
    rect = (8, 4, 90, 50)
    depth = torch.from_numpy(depth_np).cuda()
    frame = _to_native_frame(node.make_frame(cam, 0.0, rect))
    (tmp_path / "frame.bin").write_bytes(bytes(frame))
    depth_np.tofile(tmp_path / "depth.bin")
    for fmt in FORMATS:
        want = node.render(cam, depth, rect=rect, target=fmt)
        torch.cuda.synchronize()
        out = tmp_path / f"out_{fmt}.bin"
        r = subprocess.run([str(exe), str(tmp_path / "frame.bin"), str(tmp_path / "depth.bin"), str(out), "100", "8", "0.5", "32", "--target", fmt],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "atmo_render_target" in r.stdout
        got = np.fromfile(out, dtype=BITS[fmt]).reshape(want.shape)
        assert np.array_equal(got, _bits(want, fmt)) and got.any()
    node.close()
