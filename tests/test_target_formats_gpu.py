"""GPU tests of the sRGB, BGRA and 10-bit colour targets (include/atmo_target.h, formats 16 .. 19): the store and the blend on chosen values, whole
frames through atmo_render_target, a batch, a proxy draw and the native example.  Every comparison is np.array_equal on the raw bytes against
godot_atmosphere_shader_amd/targets.py (encode / decode / blend in numpy); the fp32 input is atmo_render's own frame."""
import ctypes as C

import numpy as np
import pytest
import torch

import proxy_geometry as G
from common import demo_params, demo_textures, make_node
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T

pytestmark = pytest.mark.gpu

FORMATS = ("rgba8_srgb", "bgra8", "bgra8_srgb", "a2b10g10r10")
W, H = 251, 141           # an odd size: partial tiles on both edges, odd rows of quads
PAD = 7                   # pixels of padding per row in the pitched draws
SENTINEL = 0xA5
f32 = np.float32


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _fields(buf):
    """(R, G, B, A) codes of A2B10G10R10 bytes."""
    w = np.ascontiguousarray(buf).view("<u4")[..., 0]
    return w & 1023, (w >> 10) & 1023, (w >> 20) & 1023, w >> 30


# ---- 1. the store / blend on chosen values (atmo_debug_store_target) ----------------------------------------------------------------------------

def _neighbours(x):
    x = np.asarray(x, dtype=f32)
    return np.concatenate([x, np.nextafter(x, f32(-1.0)), np.nextafter(x, f32(2.0))])


def _chosen_sources():
    halves = [((np.arange(n) + 0.5) / n).astype(f32) for n in (255, 1023, 3)]
    grid = np.linspace(-0.5, 1.5, 2 ** 17 + 1, dtype=np.float64).astype(f32)
    sub = np.array([1, 2, 0x7FFFFF, 0x80000001, 0x807FFFFF], dtype=np.uint32).view(f32)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 3e38, -3e38, 1.0, 2.0], dtype=f32)
    return np.concatenate([_neighbours(T.SRGB_THRESH[1:]), T.SRGB_DECODE] + [_neighbours(h) for h in halves] + [grid, sub, special]).astype(f32)


@pytest.fixture(scope="module")
def chosen():
    values = _chosen_sources()
    n = 1 << 20
    assert values.size < n
    rng = np.random.default_rng(1619)
    src = np.empty((n, 4), dtype=f32)
    for c in range(4):
        src[:, c] = values[rng.permutation(n) % values.size]        # every chosen value appears in every channel, against ever different partners
    alphas = np.array([0.0, 2.0 ** -24, 1.0 / 3.0, 0.5, 1.0], dtype=f32)
    src_c = src.copy()
    src_c[:, 3] = alphas[rng.permutation(n) % alphas.size]
    dst = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    for c in range(4):
        assert np.unique(dst[:, c]).size == 256                       # every byte value occurs in every channel
    r, g, b, a = _fields(dst)
    assert all(np.unique(x).size == 1024 for x in (r, g, b)) and np.unique(a).size == 4
    for x in (src, src_c, dst):
        x.setflags(write=False)
    return src, src_c, dst


@pytest.mark.parametrize("composite", [0, 1], ids=["plain", "composite"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_store_target_matches_the_statement(chosen, fmt, composite):
    """The kernels' store_target<FMT> against targets.py on 2^20 pixels: sources = every sRGB threshold with its fp32 predecessor and successor, every
    DECODE[k], every (k + 0.5) / 255, / 1023 and / 3 with both fp32 neighbours, [-0.5, 1.5] on a 2^-16 grid, NaN, -NaN, infinities, -0, subnormals, 3e38;
    destinations = random bytes with every byte (every 10-bit code, every alpha code) in every channel; composite alphas from {0, 2^-24, 1/3, 0.5, 1}.
    Since every threshold and both its neighbours are sources, a guess of the loop-free sRGB encode that is off by more than its one correction step fails here."""
    lib = N.load()
    ctx = C.c_void_p()
    assert lib.atmo_create(0, N.VARIANT_NO_CLOUDS, 0, 0, N.LIGHT_DIRECT, 8, C.byref(ctx)) == N.ATMO_OK
    try:
        src, src_c, dst = chosen
        src = src_c if composite else src
        n = src.shape[0]
        want = T.blend(src, dst, fmt) if composite else T.encode(src, fmt)
        src_dev, dst_dev = torch.tensor(src, device="cuda"), torch.tensor(dst, device="cuda")   # (copies: the fixture stays read-only)
        rc = lib.atmo_debug_store_target(ctx, T.format_id(fmt), composite, C.c_void_p(src_dev.data_ptr()), C.c_void_p(dst_dev.data_ptr()), n, None)
        assert rc == N.ATMO_OK, lib.atmo_last_error_string(ctx)
        torch.cuda.synchronize()
        got = _np(dst_dev)
        bad = np.argwhere(got != want)
        if bad.size:
            i, c = bad[0]
            print(f"\n{len(bad)} mismatching bytes; first: pixel {i} byte {c}: src {src[i]!r} ({src[i].view(np.uint32)}), dst {dst[i]}, got {got[i]}, want {want[i]}")
        assert np.array_equal(got, want)
        # the comparison was not about nothing
        if fmt == "a2b10g10r10":
            r, g, b, a = _fields(want)
            for x in (r, g, b):
                assert (x == 0).any() and (x == 1023).any() and np.unique(x).size == 1024
            assert np.unique(a).size == 4
        else:
            for c in range(4):
                assert np.unique(want[:, c]).size == 256              # all 256 codes (sRGB codes in R, G, B of the sRGB formats) occur
    finally:
        lib.atmo_destroy(ctx)


# ---- 2. frames ------------------------------------------------------------------------------------------------------------------------------------

FRAME_CASES = [("no_clouds_32x8_direct", "declared"), ("clouds_high", "declared"), ("v1_clouds", "lod0")]


def _discard_mask(config, sampler, cam, depth, tex):
    """Which pixels are discarded: a float draw with atmo_set_target_cleared into a NaN-filled buffer leaves exactly those untouched."""
    node = make_node(config, tex, sampler=sampler, target_cleared=True)
    out = torch.full((cam.height, cam.width, 4), float("nan"), dtype=torch.float32, device="cuda")
    node.render(cam, depth, out=out)
    torch.cuda.synchronize()
    node.close()
    return torch.isnan(out).all(dim=-1).cpu().numpy()


def _pitched(rows, cols):
    """A (rows, cols, 4) view with a row stride of cols + PAD pixels into a sentinel-filled buffer; returns (view, whole buffer)."""
    whole = torch.full((rows, cols + PAD, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole[:, :cols, :], whole


@pytest.mark.parametrize("config,sampler", FRAME_CASES, ids=[c for c, _ in FRAME_CASES])
def test_frame_is_the_encoded_float_frame(config, sampler):
    """251 x 141, pose P_space, all four formats: plain, composite over random destinations, pitched, a sub-rect, a cleared target and the allocating form
    against encode / blend of atmo_render's own frame; composites leave discarded pixels untouched."""
    tex = demo_textures()
    cam = S.Camera.from_pose(W, H, "P_space")
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    node = make_node(config, tex, sampler=sampler)
    ref = _np(node.render(cam, depth))
    discarded = _discard_mask(config, sampler, cam, depth, tex)
    kept = ~discarded
    # no branch is tested on nothing
    rgb = ref[kept][:, :3]
    codes = np.unique(T.srgb_encode(rgb)).size
    linear = int(((rgb != 0.0) & (rgb <= f32(0.0031308)) & (rgb > 0)).sum())
    above = int((ref > 1.0).sum())
    alpha2 = np.unique(_fields(T.encode(ref, "a2b10g10r10"))[3]).size
    print(f"\n{config} {sampler}: kept {kept.mean():.3f}, discarded {discarded.mean():.3f}, distinct sRGB codes {codes}, non-zero channels in the linear segment "
          f"{linear}, channels > 1: {above}, 2-bit alpha codes {alpha2}")
    assert kept.mean() >= 0.25 and discarded.mean() >= 0.25
    assert np.all(ref[discarded] == 0.0)
    if config in ("no_clouds_32x8_direct", "clouds_high"):
        assert codes >= 128 and linear >= 100
    if config in ("clouds_high", "v1_clouds"):
        assert above > 0
    assert alpha2 == 4
    rng = np.random.default_rng(11)
    dst = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    x0, y0, x1, y1 = 37, 13, 171, 102
    for fmt in FORMATS:
        want_plain = T.encode(ref, fmt)
        want_blend = T.blend(ref, dst, fmt)
        want_blend[discarded] = dst[discarded]                       # a composite never stores a discarded fragment
        assert (want_blend[kept] != dst[kept]).any() and np.all(want_plain[discarded] == 0)
        got = node.render(cam, depth, out=torch.full((H, W, 4), SENTINEL, dtype=torch.uint8, device="cuda"), target=fmt)
        scene = node.render_composite(cam, depth, _cuda(dst), target=fmt)
        alloc = node.render(cam, depth, target=fmt)                   # the allocating form
        torch.cuda.synchronize()
        assert "target" in node.kernel_name, node.kernel_name
        assert np.array_equal(_np(got), want_plain), (fmt, "plain")
        assert np.array_equal(_np(scene), want_blend), (fmt, "composite")
        assert alloc.dtype == torch.uint8 and tuple(alloc.shape) == (H, W, 4) and np.array_equal(_np(alloc), want_plain), (fmt, "allocated")
        # pitch: a row stride of W + 7 pixels; the padding keeps its sentinel
        view, whole = _pitched(H, W)
        node.render(cam, depth, out=view, target=fmt)
        view_c, whole_c = _pitched(H, W)
        view_c.copy_(_cuda(dst))
        node.render_composite(cam, depth, view_c, target=fmt)
        torch.cuda.synchronize()
        wb, wc = _np(whole), _np(whole_c)
        assert np.array_equal(wb[:, :W], want_plain) and np.all(wb[:, W:] == SENTINEL), (fmt, "pitched plain")
        assert np.array_equal(wc[:, :W], want_blend) and np.all(wc[:, W:] == SENTINEL), (fmt, "pitched composite")
        # a sub-rect: the plain draw is the crop (tight and pitched), the composite touches the rect only
        crop = node.render(cam, depth, rect=(x0, y0, x1, y1), target=fmt)
        view, whole = _pitched(y1 - y0, x1 - x0)
        node.render(cam, depth, out=view, rect=(x0, y0, x1, y1), target=fmt)
        scene = node.render_composite(cam, depth, _cuda(dst), rect=(x0, y0, x1, y1), target=fmt)
        torch.cuda.synchronize()
        assert np.array_equal(_np(crop), want_plain[y0:y1, x0:x1]), (fmt, "rect")
        wb = _np(whole)
        assert np.array_equal(wb[:, :x1 - x0], want_plain[y0:y1, x0:x1]) and np.all(wb[:, x1 - x0:] == SENTINEL), (fmt, "pitched rect")
        want_rect = dst.copy()
        want_rect[y0:y1, x0:x1] = want_blend[y0:y1, x0:x1]
        assert np.array_equal(_np(scene), want_rect), (fmt, "composite rect")
    # a name that contradicts the tensor's dtype is refused
    with pytest.raises(ValueError):
        node.render(cam, depth, out=torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"), target="rgba8_srgb")
    with pytest.raises(ValueError):
        node.render_composite(cam, depth, torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), target="rgba16f")
    node.close()
    # atmo_set_target_cleared: discarded pixels keep the sentinel, kept pixels are the encoded frame
    cleared = make_node(config, tex, sampler=sampler, target_cleared=True)
    for fmt in FORMATS:
        got = cleared.render(cam, depth, out=torch.full((H, W, 4), SENTINEL, dtype=torch.uint8, device="cuda"), target=fmt)
        torch.cuda.synchronize()
        gb = _np(got)
        assert np.all(gb[discarded] == SENTINEL) and np.array_equal(gb[kept], T.encode(ref, fmt)[kept]), (fmt, "cleared")
    cleared.close()


# ---- 3. a batch -----------------------------------------------------------------------------------------------------------------------------------

def test_two_views_into_the_halves_of_one_srgb_image():
    """Two 126 x 70 views of clouds_high as the side-by-side halves of one 252-pixel-wide RGBA8_SRGB image, composited in place in one launch: each half
    is byte for byte its own atmo_render_target composite; the padding of a pitched image is untouched."""
    tex = demo_textures()
    w, h = 126, 70
    cams = [S.Camera.from_pose(w, h, "P_space"), S.Camera.from_pose(w, h, "P_limb")]
    depths = [torch.from_numpy(S.depth_ground_sphere(c)).cuda() for c in cams]
    node = make_node("clouds_high", tex, sampler="declared")
    rng = np.random.default_rng(13)
    for pad in (0, PAD):
        fill = rng.integers(0, 256, size=(h, 2 * w + pad, 4), dtype=np.uint8)
        fill[:, 2 * w:] = SENTINEL
        want = fill.copy()
        for i, (cam, depth) in enumerate(zip(cams, depths)):
            single = node.render_composite(cam, depth, _cuda(fill[:, i * w:(i + 1) * w]), target="rgba8_srgb")
            torch.cuda.synchronize()
            assert node.kernel_name.startswith("atmo_render_target_kernel<"), node.kernel_name
            want[:, i * w:(i + 1) * w] = _np(single)
            changed = (want[:, i * w:(i + 1) * w] != fill[:, i * w:(i + 1) * w]).any(axis=-1).mean()
            assert changed > 0.25, (i, changed)
        image = _cuda(fill)
        outs = node.render_views(cams, depths, [image[:, :w], image[:, w:2 * w]], composite=True, target="rgba8_srgb")
        torch.cuda.synchronize()
        assert node.kernel_name.startswith("atmo_render_views_target_kernel<"), node.kernel_name
        assert outs[0].data_ptr() == image.data_ptr()
        got = _np(image)
        assert np.array_equal(got[:, :w], want[:, :w]) and np.array_equal(got[:, w:2 * w], want[:, w:2 * w]), pad
        assert np.all(got[:, 2 * w:] == SENTINEL)
    # RGBA8_SRGB is not RGBA8_UNORM: the same draw without the name blends other bytes
    plain = node.render_composite(cams[0], depths[0], _cuda(fill[:, :w]))
    torch.cuda.synchronize()
    assert not np.array_equal(_np(plain), want[:, :w])
    node.close()


# ---- 4. the proxy draw ----------------------------------------------------------------------------------------------------------------------------

def test_proxy_composite_into_a2b10g10r10():
    """atmo_render_proxy_target, composite, A2B10G10R10 at 251 x 141 on the far-mode box seen edge-on: the passing, shaded fragments are blend() of the float
    proxy draw, every other word is untouched."""
    tex = demo_textures(cube_n=64, shape_n=32)
    cam = S.Camera(W, H, (0.0, 0.0, 500.0), (0.0, 0.0, 0.0))
    model = G.rotation_y(45.0)
    depth_np = S.depth_ground_sphere(cam)
    depth = torch.from_numpy(depth_np).cuda()
    marker = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    cleared = make_node("clouds_high_rm", tex, target_cleared=True)
    cleared.global_transform = model
    size = cleared.proxy_box_size(cam)
    ref = _np(cleared.render_proxy(cam, depth, out=marker.clone()))
    torch.cuda.synchronize()
    cleared.close()
    shaded = ~np.isnan(ref).all(axis=-1)
    covered, passing, unstable = G.frame_masks(cam, model, size, depth_np)
    assert not (shaded & ~passing & ~unstable).any()                 # only fragments of the box that pass the depth test are shaded
    assert shaded.sum() > 500 and (~passing).sum() > 500, (shaded.sum(), passing.sum())      # passing and non-passing pixels both occur
    node = make_node("clouds_high_rm", tex)
    node.global_transform = model
    fill = np.random.default_rng(23).integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    want = fill.copy()
    want[shaded] = T.blend(np.nan_to_num(ref), fill, "a2b10g10r10")[shaded]
    scene = node.render_proxy_composite(cam, depth, _cuda(fill), target="a2b10g10r10")
    view, whole = _pitched(H, W)
    view.copy_(_cuda(fill))
    node.render_proxy_composite(cam, depth, view, target="rgb10a2")
    torch.cuda.synchronize()
    assert "proxy_target" in node.kernel_name, node.kernel_name
    assert np.array_equal(_np(scene), want)
    wb = _np(whole)
    assert np.array_equal(wb[:, :W], want) and np.all(wb[:, W:] == SENTINEL)
    assert (want[shaded] != fill[shaded]).any(axis=-1).mean() > 0.5
    node.close()


# ---- 5. the native example ------------------------------------------------------------------------------------------------------------------------

def test_native_host_draws_into_bgra8_srgb(tmp_path):
    """examples/atmo_render_file.cpp --target bgra8_srgb (include/atmo_target.h + the HIP runtime only) writes the bytes the Python binding produces."""
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
    want = node.render(cam, depth, rect=rect, target="bgra8_srgb")
    ref = node.render(cam, depth, rect=rect)
    torch.cuda.synchronize()
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(tmp_path / "frame.bin"), str(tmp_path / "depth.bin"), str(out), "100", "8", "0.5", "32", "--target", "bgra8_srgb"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "atmo_render_target" in r.stdout and "4 bytes each" in r.stdout
    got = np.fromfile(out, dtype=np.uint8).reshape(want.shape)
    assert np.array_equal(got, _np(want)) and np.array_equal(got, T.encode(_np(ref), "bgra8_srgb")) and got.any()
    r = subprocess.run([str(exe), str(tmp_path / "frame.bin"), str(tmp_path / "depth.bin"), str(out), "100", "8", "0.5", "32", "--target", "bgra8_linear"],
                       capture_output=True, text=True)
    assert r.returncode == 2
    node.close()
