"""Reduced-resolution draws on the CPU (include/atmo_reduced.h; godot_atmosphere_shader_amd/reduced.py): the header's symbol set and the binding, the
sizes, every refusal of the three entry points on host-only contexts in the header's order (nothing touches a device), the low frame's matrix, properties
of the numpy statement on random inputs -- dyadic weights, alpha within its neighbours', no leak across a depth edge, the reduction's checkerboard -- and
the quality record: the oracle's full frame against its low frame upsampled by the statement.  (tests/test_reduced_gpu.py holds the kernels to the
statement bit for bit.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cameras as K
from common import CONFIGS, demo_frame, demo_params, demo_textures, oracle_inputs
from godot_atmosphere_shader_amd import reduced as R
from godot_atmosphere_shader_amd import scene as S
from test_rays_host import _mode_ctx, _said
from test_views_proxy_host import FAR, ROOT, _frame, _functions, _host_ctx

IMG, TEX, LOW, SCRATCH = 0x100000, 0x800000, 0x900000, 0xA00000   # addresses no refusal dereferences
W, H = FAR.width, FAR.height


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, R.bind()


def _ulps(x, n=4):
    """n ulps of the float32 values x, as float64."""
    return n * np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ---- the header and the binding ----------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_the_reduced_header(tmp_path):
    """Fails on a library without the feature: the header does not exist and the symbols are not exported."""
    N, lib = _lib()
    assert _functions("atmo_reduced.h") == set(R.REDUCED_ENTRY_POINTS) and len(R.REDUCED_ENTRY_POINTS) == 4
    assert tuple(R.signatures()) == R.REDUCED_ENTRY_POINTS
    for sym in R.REDUCED_ENTRY_POINTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int and sym not in N.EXPORTED_SYMBOLS
        assert not any(sym in symbols for symbols, _, _, _ in N.HEADERS.values())      # declared by reduced.py, not by a block of _native.HEADERS
    assert lib is N.load() and lib.atmo_abi_version() == N.ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "atmo_reduced.h")).read()
    assert '#include "atmo_depth.h"' in text and "Not here" in text
    for name in ("atmo.h", "atmo_target.h", "atmo_depth.h", "atmo_detail_target.h"):   # the older headers do not know the new one
        assert "atmo_reduced" not in open(os.path.join(ROOT, "include", name)).read(), name
    # the structure is 8 bytes on both sides
    assert C.sizeof(R.AtmoReduced) == 8 and R.AtmoReduced.scale.offset == 0 and R.AtmoReduced.depth_tolerance.offset == 4
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "atmo_reduced.h"\n'
                   'int main(void) { printf("%zu %zu %zu", sizeof(AtmoReduced), offsetof(AtmoReduced, scale), offsetof(AtmoReduced, depth_tolerance)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["8", "0", "4"]


def test_a_library_without_the_symbols_is_refused_by_name():
    class Fn:
        restype = argtypes = None

    class Old:
        atmo_reduced_size = Fn()   # some, not all

    with pytest.raises(RuntimeError, match=r"atmo_reduced_depth \(include/atmo_reduced\.h\)"):
        R.bind(Old())
    assert Old.atmo_reduced_size.argtypes is not None


def test_the_sizes():
    N, lib = _lib()

    def size(w, h, s):
        lw, lh, nbytes = C.c_int(-1), C.c_int(-1), C.c_size_t(0)
        rc = lib.atmo_reduced_size(w, h, s, C.byref(lw), C.byref(lh), C.byref(nbytes))
        return rc, lw.value, lh.value, nbytes.value

    for (w, h, s), (lw, lh) in {(64, 40, 2): (32, 20), (64, 40, 4): (16, 10), (1920, 1080, 4): (480, 270),       # divisible
                                (37, 23, 2): (19, 12), (37, 23, 4): (10, 6), (70, 46, 4): (18, 12), (5, 3, 4): (2, 1),   # odd
                                (1, 1, 2): (1, 1), (1, 1, 4): (1, 1), (1, 9, 4): (1, 3), (65536, 1, 2): (32768, 1)}.items():   # 1-pixel sides
        depth_floats = (lw * lh + 3) // 4 * 4
        assert size(w, h, s) == (N.ATMO_OK, lw, lh, 4 * depth_floats + 16 * lw * lh), (w, h, s)
        assert R.low_size(w, h, s) == (lw, lh) and R.scratch_layout(w, h, s) == (depth_floats, 4 * depth_floats + 16 * lw * lh)
    assert size(1, 1, 4)[3] == 32                                                # one float padded to 16 bytes, one float4
    assert lib.atmo_reduced_size(64, 40, 2, None, None, None) == N.ATMO_OK       # every output is optional
    for w, h, s in ((64, 40, 3), (64, 40, 1), (64, 40, 8), (64, 40, 0), (64, 40, -2), (0, 40, 2), (64, 0, 2), (65537, 40, 2), (64, 65537, 4), (-1, -1, 2)):
        assert size(w, h, s) == (N.ATMO_E_ARG, -1, -1, 0), (w, h, s)
    with pytest.raises(ValueError):
        R.low_size(64, 40, 3)


# ---- the refusals, in the header's order ------------------------------------------------------------------------------------------------------------
def _call(lib, ctx, entry, frame=True, rect=None, depth=True, texels=TEX, dfmt=0, dpitch=0, opt=True, scale=2, tol=0.1, low_depth=LOW, low_rgba=SCRATCH,
          scratch=SCRATCH, target=True, pixels=IMG, fmt=1, pitch=0, composite=0):
    N, _ = _lib()
    f, d, t, o = _frame(FAR, rect), N.AtmoDepth(texels, dfmt, dpitch), N.AtmoTarget(pixels, fmt, pitch), R.AtmoReduced(scale, tol)
    f_, d_, t_, o_ = C.byref(f) if frame else None, C.byref(d) if depth else None, C.byref(t) if target else None, C.byref(o) if opt else None
    if entry == "atmo_reduced_depth":
        rc = lib.atmo_reduced_depth(ctx, f_, d_, scale, low_depth, None)
    elif entry == "atmo_reduced_upsample":
        rc = lib.atmo_reduced_upsample(ctx, f_, d_, o_, low_depth, low_rgba, t_, composite, None)
    else:
        rc = lib.atmo_render_reduced_target(ctx, f_, d_, o_, scratch, t_, composite, None)
    return _said(lib, ctx, rc)


# (what the message must hold, the one thing wrong), in the order of the checks
FRAME = [("null frame", dict(frame=False))]
TARGET = [("null target", dict(target=False)), ("unknown target format", dict(fmt=3)), ("null target pixels", dict(pixels=0)),
          ("aligned to the pixel size", dict(pixels=IMG + 4)), ("rect outside the viewport", dict(rect=(0, 0, W + 1, H))),
          ("row_pitch_bytes", dict(pitch=W * 8 - 8)), ("row_pitch_bytes", dict(pitch=W * 8 + 4))]
OPT = [("null opt", dict(opt=False)), ("scale must be 2 or 4", dict(scale=3)), ("scale must be 2 or 4", dict(scale=0)), ("depth_tolerance", dict(tol=-0.5)),
       ("depth_tolerance", dict(tol=float("nan"))), ("depth_tolerance", dict(tol=float("inf")))]
RECT = [("whole viewport", dict(rect=(0, 0, W - 1, H))), ("whole viewport", dict(rect=(2, 0, W, H))), ("whole viewport", dict(rect=(5, 5, 5, 30)))]
DEPTH = [("null depth", dict(depth=False)), ("unknown depth format", dict(dfmt=3)), ("null depth texels", dict(texels=0)),
         ("aligned to the texel size", dict(texels=TEX + 2)), ("depth row_pitch_bytes", dict(dpitch=W * 4 - 4)), ("depth row_pitch_bytes", dict(dfmt=1, dpitch=W * 2 + 1))]
CHECKS = {
    "atmo_reduced_depth": FRAME + [("rect outside the viewport", dict(rect=(0, 0, W + 1, H)))] + OPT[1:3] + RECT +
                          [("null low_depth_dev", dict(low_depth=0)), ("4-byte aligned", dict(low_depth=LOW + 2))] + DEPTH,
    "atmo_reduced_upsample": FRAME + TARGET + OPT + RECT + [("null low_depth_dev or low_rgba_dev", dict(low_depth=0)),
                                                            ("null low_depth_dev or low_rgba_dev", dict(low_rgba=0)), ("4-byte aligned", dict(low_depth=LOW + 1)),
                                                            ("16-byte aligned", dict(low_rgba=SCRATCH + 8))] + DEPTH,
    "atmo_render_reduced_target": FRAME + TARGET + OPT + RECT + [("null scratch_dev", dict(scratch=0)), ("16-byte aligned", dict(scratch=SCRATCH + 8))] + DEPTH,
}


@pytest.mark.parametrize("entry", list(CHECKS))
def test_every_refusal_in_the_header_s_order(entry):
    """Each wrong argument alone is ATMO_E_ARG under the entry point's name; two wrong arguments are refused for the one the header lists first; a
    well-formed call on a host-only context gets as far as ATMO_E_NO_DEVICE."""
    N, lib = _lib()
    ctx = _mode_ctx(N, lib, N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)   # direct light without clouds needs no texture
    try:
        checks = CHECKS[entry]
        for needle, wrong in checks:
            rc, msg = _call(lib, ctx, entry, **wrong)
            assert rc == N.ATMO_E_ARG and msg.startswith(entry + ": ") and needle in msg, (wrong, rc, msg)
        for (needle, first), (_, second) in zip(checks, checks[1:]):
            if set(first) & set(second):
                continue    # two values of one argument
            rc, msg = _call(lib, ctx, entry, **first, **second)
            assert rc == N.ATMO_E_ARG and needle in msg, (first, second, rc, msg)
        for composite in (0, 1):
            for scale in (2, 4):
                rc, msg = _call(lib, ctx, entry, scale=scale, composite=composite, tol=0.0)
                assert rc == N.ATMO_E_NO_DEVICE and msg.startswith(entry + ": ") and "host-only" in msg, (rc, msg)
        null = {"atmo_reduced_depth": (None, None, None, 2, None, None), "atmo_reduced_upsample": (None, None, None, None, None, None, None, 0, None),
                "atmo_render_reduced_target": (None, None, None, None, None, None, 0, None)}[entry]
        assert getattr(lib, entry)(*null) == N.ATMO_E_ARG            # a null ctx: no message to hold
    finally:
        lib.atmo_destroy(ctx)


def test_what_atmo_render_would_refuse_the_low_frame_for_comes_behind_the_arguments():
    N, lib = _lib()
    entry = "atmo_render_reduced_target"
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)                                     # LUT light, clouds: nothing bound
    try:
        rc, msg = _call(lib, ctx, entry)
        assert rc == N.ATMO_E_STATE and msg.startswith(entry + ": ") and "u_optical_depth_texture not set" in msg, (rc, msg)
        assert _call(lib, ctx, entry, depth=False)[0] == N.ATMO_E_ARG           # ... behind the depth source
        assert lib.atmo_set_cloud_detail(ctx, 1) == N.ATMO_OK and lib.atmo_set_precision(ctx, 0) == N.ATMO_OK
        rc, msg = _call(lib, ctx, entry)                                       # cloud detail in a mode without its kernel: atmo_render's refusal
        assert rc == N.ATMO_E_STATE and msg.startswith(entry + ": ") and "cloud-detail kernel" in msg, (rc, msg)
        # the two passes draw nothing: they do not look at the context's mode or textures
        assert _call(lib, ctx, "atmo_reduced_depth")[0] == N.ATMO_E_NO_DEVICE and _call(lib, ctx, "atmo_reduced_upsample")[0] == N.ATMO_E_NO_DEVICE
    finally:
        lib.atmo_destroy(ctx)


# ---- the low frame ----------------------------------------------------------------------------------------------------------------------------------------
def _cam(kind, w, h, pose="P_space"):
    return K.from_pose(kind, w, h, pose, **(dict(ortho_size=300.0) if kind == "ortho" else {}))


@pytest.mark.parametrize("kind", ["plain", "eye_left", "ortho"])
def test_the_low_matrix_is_the_caller_s_bits_where_the_scale_divides(kind):
    frame = demo_frame(_cam(kind, 64, 40))
    frame["inv_projection_matrix"] = np.array(frame["inv_projection_matrix"], dtype=np.float32)
    frame["inv_projection_matrix"][13] = np.float32(-0.0)                  # a sign a product with kx - 1 = 0 would lose
    for s in (2, 4):
        low = R.low_frame(frame, s)
        assert (low["viewport_w"], low["viewport_h"], low["rect"]) == (64 // s, 40 // s, (0, 0, 64 // s, 40 // s))
        assert low["inv_projection_matrix"].dtype == np.float32
        assert low["inv_projection_matrix"].tobytes() == frame["inv_projection_matrix"].tobytes()
        assert all(np.array_equal(low[k], frame[k]) for k in ("inv_view_matrix", "planet_center_viewspace", "sun_center_viewspace")) and low["time"] == frame["time"]
    assert R.low_frame(demo_frame(_cam(kind, 70, 40)), 4)["inv_projection_matrix"].tobytes() != np.asarray(frame["inv_projection_matrix"], dtype=np.float32).tobytes()


@pytest.mark.parametrize("kind", ["plain", "eye_left", "jitter", "ortho"])
def test_every_block_centre_of_the_low_frame_maps_to_its_place_in_the_full_frame(kind):
    """70 x 46 at s = 4: 18 x 12 low pixels, the last column and row partial.  The view-space point of low pixel (i, j) at a depth, through the low matrix,
    is the full frame's point at the NDC of the block's centre, 2 (s i + s / 2) / W - 1."""
    w, h, s = 70, 46, 4
    frame = demo_frame(_cam(kind, w, h))
    low = R.low_frame(frame, s)
    assert (low["viewport_w"], low["viewport_h"]) == (18, 12)
    m = np.asarray(frame["inv_projection_matrix"], dtype=np.float64).reshape(4, 4).T         # column-major -> rows
    ml = np.asarray(low["inv_projection_matrix"], dtype=np.float64).reshape(4, 4).T
    scale = np.abs(m).max(axis=1)
    for j in range(12):
        for i in range(18):
            n_low = np.array([2.0 * (i + 0.5) / 18 - 1.0, 2.0 * (j + 0.5) / 12 - 1.0])
            n_full = np.array([2.0 * (s * i + s / 2) / w - 1.0, 2.0 * (s * j + s / 2) / h - 1.0])
            for d in (0.0, 0.37, 1.0):
                got, want = ml @ np.array([*n_low, d, 1.0]), m @ np.array([*n_full, d, 1.0])
                assert np.all(np.abs(got - want) <= 4e-7 * scale), (i, j, d, got, want)       # one fp32 rounding per element of the low matrix
    # and the C side forms the same matrix: tests/test_reduced_gpu.py draws the low frame with it and compares bits


# ---- properties of the statement ------------------------------------------------------------------------------------------------------------------------
def _random_low(rng, lh, lw, zero_share=0.25):
    rgba = rng.uniform(0.0, 1.6, (lh, lw, 4)).astype(np.float32)
    rgba[..., 3] = rng.uniform(0.0, 1.0, (lh, lw)).astype(np.float32)
    rgba[rng.random((lh, lw)) < zero_share] = 0.0
    return rgba


@pytest.mark.parametrize("s", [2, 4])
def test_the_weights_are_exact_dyadics_that_sum_to_one(s):
    rng = np.random.default_rng(s)
    w, h = 37, 23
    frame = demo_frame(_cam("plain", w, h))
    depth = rng.uniform(0.2, 0.9, (h, w)).astype(np.float32)
    low_depth = R.reduce_depth(frame, depth, s)
    _, det = R.upsample(frame, depth, low_depth, _random_low(rng, *low_depth.shape), s, 0.1, details=True)
    wts = det["weights"]
    assert wts.dtype == np.float32 and np.all(wts > 0.0)
    assert np.array_equal(wts * (2 * s) ** 2, np.rint(wts * (2 * s) ** 2))                     # multiples of 1 / (2 s)^2
    assert np.all(((wts[0] + wts[1]) + wts[2]) + wts[3] == np.float32(1.0))
    ia, ib, f = R.taps(w, s)
    assert np.all(np.rint(f * 2 * s) % 2 == 1) and ia[0] == ib[0] == 0 and ib[-1] == ia[-1] + (0 if (w - 1) % s >= s // 2 else 1) == (w + s - 1) // s - 1
    assert np.all((ib - ia >= 0) & (ib - ia <= 1))


@pytest.mark.parametrize("s", [2, 4])
def test_alpha_lies_within_its_neighbours_where_all_are_valid(s):
    rng = np.random.default_rng(10 + s)
    w, h = 37, 23
    frame = demo_frame(_cam("plain", w, h))
    depth = np.full((h, w), 0.25, dtype=np.float32)                                            # one depth everywhere: every neighbour agrees
    low_rgba = _random_low(rng, *R.low_size(w, h, s)[::-1])
    out, det = R.upsample(frame, depth, R.reduce_depth(frame, depth, s), low_rgba, s, 0.0, details=True)
    assert det["valid"].all() and det["agree"].all()
    lo, hi = det["alpha"].min(axis=0), det["alpha"].max(axis=0)
    assert np.all(out[..., 3] >= lo - _ulps(lo)) and np.all(out[..., 3] <= hi + _ulps(hi))
    assert np.all(out[..., :3][out[..., 3] > 0] >= 0.0) and np.all(out[..., :3][~(out[..., 3] > 0)] == 0.0)
    assert np.all(out[..., :3].max(axis=-1) <= 1.6 + _ulps(1.6, 16))                            # C / A is an average of the neighbours' colours, a few roundings away


@pytest.mark.parametrize("s", [2, 4])
def test_nothing_leaks_across_a_depth_edge(s):
    """A near occluder (a slanted bar and a disc) over reverse-Z sky, tol = 0.1.  The low pixels that carry the sky's depth are opaque-ish (alpha 0.6 .. 1),
    those that carry the occluder's nearly clear (0 .. 0.1): a leak in either direction would show."""
    rng = np.random.default_rng(20 + s)
    w, h = 61, 43
    frame = demo_frame(_cam("plain", w, h))
    y, x = np.mgrid[0:h, 0:w]
    occluder = (np.abs((x - 8) - 0.7 * (y - 3)) < 6.5) | ((x - 44) ** 2 + (y - 24) ** 2 < 9.5 ** 2)
    depth = np.where(occluder, rng.uniform(0.30, 0.31, (h, w)), 0.0).astype(np.float32)        # within the tolerance of each other; the sky is exactly 0
    low_depth = R.reduce_depth(frame, depth, s)
    low_rgba = _random_low(rng, *low_depth.shape, zero_share=0.0)
    low_rgba[..., 3] = np.where(low_depth == 0.0, rng.uniform(0.6, 1.0, low_depth.shape), rng.uniform(0.0, 0.1, low_depth.shape)).astype(np.float32)
    out, det = R.upsample(frame, depth, low_depth, low_rgba, s, 0.1, details=True)
    agree, alpha = det["agree"], det["alpha"]
    some = agree.any(axis=0)
    mixed = some & ~agree.all(axis=0)                      # pixels along the edge: neighbours on both sides of it
    assert (mixed & occluder).sum() > 20 and (mixed & ~occluder).sum() > 20, "the scene must put both kinds of pixel on the edge"
    assert np.array_equal(det["valid"][:, some], agree[:, some])
    bound = np.where(agree, alpha, -np.inf).max(axis=0)    # the largest alpha among the valid neighbours
    for side in (occluder, ~occluder):
        sel = some & side
        assert np.all(out[..., 3][sel] <= bound[sel] + _ulps(bound[sel]))
    assert np.all(out[..., 3][some & occluder] <= 0.1 + _ulps(0.1)) and np.all(out[..., 3][some & ~occluder] >= 0.6 - _ulps(0.6))
    # without a valid neighbour: the closest in depth alone, its alpha passed through
    none = ~some
    assert np.all(det["valid"][:, none].sum(axis=0) == 1)
    assert none.any() and np.array_equal(out[..., 3][none], (alpha * det["valid"]).sum(axis=0)[none])


@pytest.mark.parametrize("kind", ["plain", "ortho"])
@pytest.mark.parametrize("s", [2, 4])
def test_the_reduction_picks_a_texel_of_its_own_block_on_a_checkerboard(s, kind):
    rng = np.random.default_rng(30 + s)
    w, h = 37, 23
    frame = demo_frame(_cam(kind, w, h))
    depth = rng.uniform(0.05, 0.95, (h, w)).astype(np.float32)
    depth[5, 9] = depth[12, 20] = np.nan                   # (5, 9) is not a block's first texel for either scale; (12, 20) is for both
    low, ys, xs = R.reduce_depth(frame, depth, s, return_index=True)
    lw, lh = R.low_size(w, h, s)
    j, i = np.mgrid[0:lh, 0:lw]
    assert low.shape == (lh, lw) and np.array_equal(ys // s, j) and np.array_equal(xs // s, i) and ys.max() < h and xs.max() < w
    assert low.tobytes() == depth[ys, xs].tobytes()
    assert np.isnan(low[12 // s, 20 // s]) and not np.isnan(low[5 // s, 9 // s]) and np.isnan(low).sum() == 1
    # |q| of every texel: even cells hold their block's smallest, odd cells the largest (blocks with a NaN apart)
    aq = np.abs(R.eye_q(frame, *np.meshgrid(np.arange(w), np.arange(h)), depth))
    picked = aq[ys, xs]
    for jj in range(lh):
        for ii in range(lw):
            block = aq[jj * s:(jj + 1) * s, ii * s:(ii + 1) * s]
            if np.isnan(block).any():
                continue
            assert picked[jj, ii] == (block.max() if (ii + jj) & 1 else block.min()), (ii, jj)
    if kind == "plain":   # reverse-Z perspective: |q| grows with the depth value, so the farthest texel is the smallest depth
        full = low[:h // s, :w // s]
        blocks = depth[:h // s * s, :w // s * s].reshape(h // s, s, w // s, s)
        with np.errstate(invalid="ignore"):
            want = np.where((i + j)[:h // s, :w // s] & 1, blocks.max(axis=(1, 3)), blocks.min(axis=(1, 3)))
        ok = ~np.isnan(want)
        assert np.array_equal(full[ok], want[ok])


def test_the_sky_is_zero_and_every_projection_orders_depth():
    """q is 0 for a reverse-Z sky texel under an infinite far plane; |q| is larger for the nearer of two depths under every camera kind of tests/cameras.py."""
    for kind in ("plain", "eye_left", "jitter", "infinite_far", "ortho"):
        cam = _cam(kind, 37, 23)
        frame = demo_frame(cam)
        x, y = np.meshgrid(np.arange(37), np.arange(23))
        near, far = R.eye_q(frame, x, y, np.float32(0.8)), R.eye_q(frame, x, y, np.float32(0.2))
        assert near.dtype == np.float32 and np.all(np.abs(near) > np.abs(far)), kind
        if kind == "infinite_far":
            assert np.all(R.eye_q(frame, x, y, np.float32(0.0)) == 0.0)


# ---- quality: a record, not a bar -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lut(oracle32):
    return oracle32.bake_optical_depth(S.DEMO_PLANET_RADIUS, S.DEMO_ATMOSPHERE_HEIGHT, S.DEMO_SHADER_PARAMS["u_density"])


@pytest.mark.parametrize("config", ["no_clouds_8", "clouds_high"])
def test_the_reduced_frame_is_closer_to_the_full_frame_than_a_nearest_neighbour_enlargement(oracle32, lut, config):
    """The oracle's full frame at 64 x 40 against the oracle's low frame (low_frame, on reduce_depth's depth) upsampled by the statement at s = 2, in
    premultiplied colour.  The figures are printed (profiles/reduced/README.md records them); the assertion is only that the filter beats pixel
    repetition in the mean."""
    w, h, s = 64, 40, 2
    cam = S.Camera.from_pose(w, h, "P_limb")
    depth = S.depth_ground_sphere(cam)
    frame = demo_frame(cam)
    cfg, tex = oracle_inputs(oracle32, CONFIGS[config][1], demo_textures(), lut, declared=True)
    full = oracle32.render(demo_params(), tex, cfg, frame, depth, nthreads=8)[0]
    low_depth = R.reduce_depth(frame, depth, s)
    low = oracle32.render(demo_params(), tex, cfg, R.low_frame(frame, s), low_depth, nthreads=8)[0]
    assert 0.1 < np.any(full != 0.0, axis=-1).mean() < 0.99 and low.shape == (h // s, w // s, 4)
    up = R.upsample(frame, depth, low_depth, low, s, 0.1)
    nearest = np.repeat(np.repeat(low, s, axis=0), s, axis=1)

    def premultiplied(img):
        img = img.astype(np.float64)
        return np.concatenate([img[..., :3] * img[..., 3:4], img[..., 3:4]], axis=-1)

    err_up, err_nn = np.abs(premultiplied(up) - premultiplied(full)), np.abs(premultiplied(nearest) - premultiplied(full))
    print(f"\nreduced quality {config} {w}x{h} s={s}: upsample mean {err_up.mean():.3e} max {err_up.max():.3e}; "
          f"nearest-neighbour mean {err_nn.mean():.3e} max {err_nn.max():.3e}")
    assert err_up.mean() < err_nn.mean()
