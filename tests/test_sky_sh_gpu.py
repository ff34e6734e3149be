"""The sky as light on the device (include/atmo_sky_sh.h).  Needs an MI355X.

(1) atmo_lens_solid_angles against the numpy statement (godot_atmosphere_shader_amd/sky_sh.py): OCTAHEDRAL and CUBE_FACE byte for byte, EQUIRECT and
    FISHEYE within 1 float32 ulp, absent slots +0, both orders, a band; (2) atmo_sky_sh9 bit for bit against sh9_project at every edge of THE ORDER OF THE
    SUMS, through views of NaN-filled buffers, and within the float64 bound; (3) ACCUMULATE over six cube faces; (4) ambient_sh9 end to end on both
    shading paths, and render_lens behind its refactor; (5) a graph capture."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from common import demo_params, demo_textures, make_node
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import lens as L
from godot_atmosphere_shader_amd import sky_sh as SH
from godot_atmosphere_shader_amd.lens import Lens
from godot_atmosphere_shader_amd.ray_quads import quads_to_image
from test_sky_sh_host import random_inputs

pytestmark = pytest.mark.gpu

PAD = 3                              # rows of NaN in front of and behind every view
INSIDE = (20.0, 99.0, 5.0)           # |origin| = 101.1: inside the atmosphere (radius 100, height 8), under the clouds
FOUR_PI = 4.0 * math.pi


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _ordered(a):
    """float32 -> integers whose difference counts ulps (+0 and -0 are both 0)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


@pytest.fixture(scope="module")
def node():
    n = make_node("no_clouds_8", demo_textures(), demo_params())
    yield n
    n.close()


# ---- 1. solid angles ------------------------------------------------------------------------------------------------------------------------------------------
def _orders(lens):
    """(lens, quads) over the whole image in both orders, and over the band (2, 6) where the image has it."""
    yield lens, False
    yield lens, True
    if lens.height >= 6:
        yield lens.band((2, 6)), False
        yield lens.band((2, 6)), True


@pytest.mark.parametrize("kind", ["octahedral", "cube_face"])
def test_fp32_lenses_are_the_statement_s_bytes(node, kind):
    lenses = [Lens.octahedral(w, h) for w, h in ((7, 5), (16, 16), (33, 18))] if kind == "octahedral" else (
        [Lens.cube_face(n, n % 6) for n in (7, 16, 33)] + [Lens.cube_face(8, face) for face in range(6)])
    for whole in lenses:
        for lens, quads in _orders(whole):
            got = node.lens_solid_angles(lens, quads=quads)
            torch.cuda.synchronize()
            want = SH.solid_angles(lens, quads=quads)
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (lens.counts(quads)[0],)
            assert got.cpu().numpy().tobytes() == want.tobytes(), (lens, quads)
            if quads and (lens.width % 2 or (lens.rows[1] - lens.rows[0]) % 2):
                assert (want == 0).any()                                             # absent slots, and their +0 compared as bytes above


@pytest.mark.parametrize("kind", ["equirect", "fisheye180", "fisheye220"])
def test_trigonometric_lenses_are_within_an_ulp(node, kind):
    """The header's rule: 1 float32 ulp from the float64 statement, below sin theta = 2^-10 as above it."""
    whole = Lens.equirect(16, 8) if kind == "equirect" else Lens.fisheye(17, 13, fov=math.radians(float(kind[7:])))
    differ = total = 0
    for lens, quads in _orders(whole):
        got = node.lens_solid_angles(lens, quads=quads).cpu().numpy()
        want = SH.solid_angles(lens, quads=quads)
        absent = ~np.any(L.lens_rays(lens, quads=quads)[:, 4:7] != 0, axis=1)
        assert got.shape == want.shape and got[absent].tobytes() == want[absent].tobytes() and not want[absent].any()      # +0, bytes
        assert np.all(got[~absent] > 0.0) and (quads or kind == "equirect" or absent.any())
        ulps = np.abs(_ordered(got) - _ordered(want))
        assert ulps.max() <= 1, (lens, quads, int(ulps.max()))
        differ, total = differ + int((ulps != 0).sum()), total + int((~absent).sum())
    print(f"{kind}: {differ} of {total} weights differ from the float64 statement's rounding, each by 1 ulp")


# ---- 2. the projection -------------------------------------------------------------------------------------------------------------------------------------------
def _views(dirs, rgba, w):
    """The inputs as views into larger buffers whose remainder is NaN; zero-weight rays' rows are NaN too."""
    n = dirs.shape[0]
    rays = np.full((n + 2 * PAD, 8), np.nan, dtype=np.float32)
    rays[PAD:PAD + n, :4] = 0.0
    rays[PAD:PAD + n, 4:7] = dirs
    pix = np.full((n + 2 * PAD, 4), np.nan, dtype=np.float32)
    pix[PAD:PAD + n] = rgba
    wgt = np.full((n + 2 * PAD,), np.nan, dtype=np.float32)
    wgt[PAD:PAD + n] = w
    rays[PAD:PAD + n][w == 0] = np.nan
    pix[PAD:PAD + n][w == 0] = np.nan
    return [torch.from_numpy(a).cuda()[PAD:PAD + n] for a in (rays, pix, wgt)]


def _call(node, rays, pix, wgt, out, flags=0):
    """atmo_sky_sh9 itself, with a scratch of exactly the stated size, pre-filled with NaN."""
    lib = SH.bind(node._lib)
    n = int(rays.shape[0])
    need = C.c_size_t(0)
    N.check(node._ctx, lib.atmo_sky_sh9_scratch_bytes(n, C.byref(need)))
    assert need.value == SH.scratch_bytes(n)
    scratch = torch.full((need.value // 4 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    N.check(node._ctx, lib.atmo_sky_sh9(node._ctx, C.c_void_p(rays.data_ptr()), C.c_void_p(pix.data_ptr()), C.c_void_p(wgt.data_ptr()) if wgt is not None else None,
                                        n, flags, C.c_void_p(scratch.data_ptr()), need, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return scratch


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 256 * 4096 + 1])
def test_the_projection_is_the_statement_s_bits(node, n):
    dirs, rgba, w = random_inputs(n, 1000 + n)
    assert n < 10 or (w == 0).any()
    rays, pix, wgt = _views(dirs, rgba, w)
    out = torch.full((40,), float("nan"), dtype=torch.float32, device="cuda")
    scratch = _call(node, rays, pix, wgt, out)
    want = SH.sh9_project(dirs, rgba, w)
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got)) and got.tobytes() == want.tobytes(), (n, got, want)
    assert np.isnan(scratch.cpu().numpy()[SH.scratch_bytes(n) // 4:]).all()                 # nothing behind the stated size is written
    again = torch.full((40,), float("nan"), dtype=torch.float32, device="cuda")            # the same call twice: the same bits
    _call(node, rays, pix, wgt, again)
    assert again.cpu().numpy().tobytes() == got.tobytes()
    exact, magnitude = SH.sh9_project64(dirs, rgba, w)
    err, bound = np.abs(got.astype(np.float64) - exact), SH.sh9_error_bound(n, magnitude)
    print(f"n = {n}: largest error over its float64 bound {np.max(err[:37] / np.maximum(bound[:37], 1e-300)):.3f}")
    assert np.all(err <= bound), (n, err, bound)
    if n in (65, 4097):      # a null weight_dev: every ray weighs 1 and every row is read
        rays1, pix1, _ = _views(dirs, rgba, np.ones(n, dtype=np.float32))
        _call(node, rays1, pix1, None, out)
        want1 = SH.sh9_project(dirs, rgba, None)
        assert out.cpu().numpy().tobytes() == want1.tobytes() and want1[36] == n
        exact1, magnitude1 = SH.sh9_project64(dirs, rgba, None)
        assert np.all(np.abs(want1.astype(np.float64) - exact1) <= SH.sh9_error_bound(n, magnitude1))


def test_project_sh9_is_the_entry_point(node):
    dirs, rgba, w = random_inputs(5000, 5)
    rays, pix, wgt = _views(dirs, rgba, np.where(w == 0, np.float32(-0.0), w))          # -0 is a zero weight too
    got = node.project_sh9(rays, pix, wgt)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (40,) and got.cpu().numpy().tobytes() == SH.sh9_project(dirs, rgba, w).tobytes()
    empty = node.project_sh9(rays[:0], pix[:0], out=torch.full((40,), 3.0, device="cuda"))
    assert not empty.cpu().numpy().any()                                                # n_rays == 0: forty +0
    with pytest.raises(ValueError):
        node.project_sh9(rays, pix[:-1], wgt)
    with pytest.raises(ValueError):
        node.project_sh9(rays, pix, wgt, accumulate=True)


# ---- 3. ACCUMULATE ---------------------------------------------------------------------------------------------------------------------------------------------
def test_six_cube_faces_accumulate_as_the_statement_s_chain(node):
    rng = np.random.default_rng(6)
    out = torch.full((40,), float("nan"), dtype=torch.float32, device="cuda")
    want, exact = None, None
    for face in range(6):
        lens = Lens.cube_face(8, face)
        dirs, w = L.lens_rays(lens)[:, 4:7], SH.solid_angles(lens)
        rgba = rng.uniform(0.0, 4.0, (64, 4)).astype(np.float32)
        rays, pix, _ = _views(dirs, rgba, w)
        weights = node.lens_solid_angles(lens)
        assert weights.cpu().numpy().tobytes() == w.tobytes()
        node.project_sh9(rays, pix, weights, out=out, accumulate=face > 0)
        want = SH.sh9_project(dirs, rgba, w, prev=want)
        exact = SH.sh9_project64(dirs, rgba, w, prev=exact)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert abs(float(got[36]) - FOUR_PI) <= 2e-2 * FOUR_PI                                  # six 8 x 8 faces: the midpoint rule's 4e-3
    assert np.all(np.abs(got.astype(np.float64) - exact[0]) <= SH.sh9_error_bound(64, exact[1], calls=6))


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["no_clouds_8", "clouds_high"])
def test_ambient_sh9_is_the_projection_of_what_the_ray_calls_return(config):
    """no_clouds_8: the row-major path through the tile index.  clouds_high with its mip chain bound: the quad path under the declared sampler."""
    n = make_node(config, demo_textures(), demo_params())
    try:
        lens = Lens.octahedral(32, 32, origin=INSIDE)
        quads = config == "clouds_high"
        assert n._shades_ray_quads() == quads
        got = n.ambient_sh9(lens)
        torch.cuda.synchronize()
        assert ("indexed" in n.kernel_name) != quads, n.kernel_name
        if quads:
            rays = n.lens_rays(lens, quads=True)
            shaded = n.shade_ray_quads(rays, None, width=32)
        else:
            rays, index = n.lens_rays(lens, tile_index=True)
            shaded = torch.zeros((1024, 4), dtype=torch.float32, device="cuda")
            n.shade_rays(rays, None, width=32, out=shaded, index=index)
        torch.cuda.synchronize()
        rays_np, shaded_np = rays.cpu().numpy(), shaded.cpu().numpy()
        assert rays_np.tobytes() == L.lens_rays(lens, quads=quads).tobytes()
        assert np.all(shaded_np[:, 3] > 0.0), "every ray starts inside the atmosphere"
        want = SH.sh9_project(rays_np, shaded_np, SH.solid_angles(lens, quads=quads))
        result = got.cpu().numpy()
        assert tuple(got.shape) == (40,) and result.tobytes() == want.tobytes() and np.all(np.isfinite(result))
        assert abs(float(result[36]) - FOUR_PI) <= 1e-5 * FOUR_PI
        print(f"{config}: L00 = {result[0:4]}, irradiance up / down = {SH.sh9_irradiance(result, [INSIDE, [-c for c in INSIDE]])[:, :3].tolist()}")
        # two lenses accumulate: the same image in two bands is two calls' chain
        halves = n.ambient_sh9([lens.band((0, 16)), lens.band((16, 32)), lens.band((5, 5))])
        qpr = 16
        cut = 4 * qpr * 8 if quads else 16 * 32
        wts = SH.solid_angles(lens, quads=quads)
        chain = SH.sh9_project(rays_np[cut:], shaded_np[cut:], wts[cut:], prev=SH.sh9_project(rays_np[:cut], shaded_np[:cut], wts[:cut]))
        assert halves.cpu().numpy().tobytes() == chain.tobytes()
        # render_lens behind its refactor: the direct composition's bytes
        image = n.render_lens(lens)
        direct = quads_to_image(shaded, 32, 32) if quads else shaded.view(32, 32, 4)
        assert tuple(image.shape) == (32, 32, 4) and np.array_equal(_bits(image), _bits(direct))
        into = torch.full((32, 32, 4), 0.25, dtype=torch.float32, device="cuda")
        assert n.render_lens(lens, out=into).data_ptr() == into.data_ptr() and np.array_equal(_bits(into), _bits(direct))
        assert not n.ambient_sh9([]).cpu().numpy().any()
    finally:
        n.close()


# ---- 5. capture ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_graph_capture_takes_both_calls_as_they_are(node):
    lens = Lens.fisheye(33, 18, fov=math.radians(200.0))
    dirs, rgba, _ = random_inputs(33 * 18, 9)
    rays, pix, _ = _views(dirs, rgba, np.ones(33 * 18, dtype=np.float32))
    eager = node.project_sh9(rays, pix, node.lens_solid_angles(lens))
    torch.cuda.synchronize()
    out = torch.full((40,), float("nan"), dtype=torch.float32, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):      # one stream, no parallel branches
            weights = node.lens_solid_angles(lens)
            node.project_sh9(rays, pix, weights, out=out)
    torch.cuda.synchronize()
    for _ in range(2):
        out.fill_(float("nan"))
        weights.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), _bits(eager)) and np.isfinite(out.cpu().numpy()).all()
    device_weights = weights.cpu().numpy()
    assert (device_weights == 0).any() and np.abs(_ordered(device_weights) - _ordered(SH.solid_angles(lens))).max() <= 1
    assert out.cpu().numpy().tobytes() == SH.sh9_project(dirs, rgba, device_weights).tobytes()
