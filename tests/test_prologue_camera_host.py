"""CPU tests of the camera prologue of the cloudless direct-light kernels (include/atmo_debug_prologue.h; shade_pixel in csrc/atmo_kernels.hip, the
predicates in csrc/atmo_api.hip: prologue_camera_fill).  The kernels take short forms of the prologue where the host's mask says that they give the general
forms' bits.  Here both forms are restated in numpy float32 -- unfused, in the source's operation order -- and compared BITWISE wherever the library's
predicate accepts; the predicate itself is held to a restatement, and no test passes on nothing: the demo poses, the cameras of the bitwise goldens and the
off-axis cameras are accepted, the orthographic one is rejected.  (tests/test_prologue_camera_gpu.py draws the same with the switch on and off.)"""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

import cameras as K
import random_scenes as RS
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame, make_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "direct_diet"))
import direct_diet_cases as DC  # noqa: E402

F = np.float32
CAMERA, POW2, NO_SPHERE_DEPTH = 1, 2, 4
LOG2E = F(1.44269504088896340736)


def _bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


def _host_ctx(view_steps=32, light_steps=8, **params):
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = C.c_void_p()
    assert lib.atmo_debug_create_host_only(N.VARIANT_NO_CLOUDS, view_steps, 0, N.LIGHT_DIRECT, light_steps, C.byref(ctx)) == N.ATMO_OK
    for name, v in params.items():
        v = np.atleast_1d(np.asarray(v, dtype=F))
        assert lib.atmo_set_param_f32(ctx, name.encode(), (C.c_float * len(v))(*v.tolist()), len(v)) == N.ATMO_OK, name
    return ctx


def _mode_skips(ctx, frame):
    from godot_atmosphere_shader_amd import _native as N

    m, sx, sy = C.c_uint(99), C.c_int(99), C.c_int(99)
    assert N.load().atmo_debug_prologue_mode(ctx, C.byref(frame), C.byref(m), C.byref(sx), C.byref(sy)) == N.ATMO_OK
    return m.value, sx.value, sy.value


def _mode(ctx, frame):
    return _mode_skips(ctx, frame)[0]


def _frame(cam, model=None):
    return _to_native_frame(make_frame(cam, np.eye(4) if model is None else model, S.DEMO_SUN_POSITION))


def _matrices(frame):
    return np.array(frame.inv_projection_matrix, dtype=F), np.array(frame.inv_view_matrix, dtype=F)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------------------

def predicate(P, V, center, radius, height, view_steps, factor):
    """prologue_camera_fill's mask, restated: bit patterns and exact comparisons only."""
    P, V = np.asarray(P, dtype=F), np.asarray(V, dtype=F)
    zero = lambda x: (int(_bits(x)) & 0x7FFFFFFF) == 0            # noqa: E731
    bounded = lambda x: bool(np.abs(F(x)) <= F(2.0 ** 40))        # noqa: E731  (false for NaN and inf)
    cam = all(zero(P[i]) for i in (1, 2, 3, 4, 6, 7, 8, 9, 10))
    cam = cam and zero(V[3]) and zero(V[7]) and zero(V[11]) and int(_bits(V[15])) == 0x3F800000
    cam = cam and P[11] != 0 and all(bool(np.abs(P[i]) >= F(2.0 ** -40)) for i in (0, 5, 14))
    cam = cam and all(bounded(x) for x in P) and all(bounded(x) for x in V) and all(bounded(x) for x in center)
    cam = cam and bounded(F(radius) + F(height)) and bounded(radius)
    mode = CAMERA if cam else 0
    if view_steps >= 1 and view_steps & (view_steps - 1) == 0:
        mode |= POW2
    if cam and zero(F(factor)):
        mode |= NO_SPHERE_DEPTH
    return mode


def skips(P, w, h):
    """... and its centre column / row: where nx (ny) is 0, under a -0 constant term and a negative scale, the short row's zero has another sign."""
    minus_zero = lambda x: int(_bits(x)) == 0x80000000            # noqa: E731
    return (w // 2 if minus_zero(P[12]) and P[0] < 0 and w % 2 else -1, h // 2 if minus_zero(P[13]) and P[5] < 0 and h % 2 else -1)


def general_rows(P, V, nx, ny, nz):
    """shade_pixel's two 4 x 4 products: every product and sum rounded on its own, summed left to right."""
    with np.errstate(all="ignore"):
        v = [((P[0 + r] * nx + P[4 + r] * ny) + P[8 + r] * nz) + P[12 + r] * F(1.0) for r in range(4)]
        ww = ((V[3] * v[0] + V[7] * v[1]) + V[11] * v[2]) + V[15] * v[3]
    return v[0], v[1], v[2], v[3], ww


def short_rows(P, nx, ny, nz):
    """... and the camera form.  `ok`: the lanes that may take it (a finite, nonzero vw -- the kernel sends a WAVE with any other lane to the general form)."""
    with np.errstate(all="ignore"):
        vw = P[11] * nz + P[15]
        vx, vy = P[0] * nx + P[12], P[5] * ny + P[13]
    vz = np.full_like(nx, P[14])
    ok = np.isfinite(vw) & (vw != 0)
    return vx, vy, vz, vw, vw, ok


def pixel_inputs(w, h, rng):
    """(px, py, nx, ny, nz) vectors: every pixel centre of a w x h viewport (nx = 2 uvx - 1 with pixel_coord's exact quotient, tools/uv_division.c: +0 on
    the centre column of an odd width, never -0) against nz in {0, -0, 1, a denormal, -denormal, NaN, inf, -inf, random}."""
    xs = (((np.arange(w, dtype=F) + F(0.5)) / F(w)) * F(2.0) - F(1.0)).astype(F)
    ys = (((np.arange(h, dtype=F) + F(0.5)) / F(h)) * F(2.0) - F(1.0)).astype(F)
    assert not (_bits(xs) == 0x80000000).any() and not (_bits(ys) == 0x80000000).any()
    assert (w % 2 == 0 or int(_bits(xs[w // 2])) == 0) and (h % 2 == 0 or int(_bits(ys[h // 2])) == 0)
    zs = np.concatenate([np.array([0.0, -0.0, 1.0, 1e-41, -1e-41, np.nan, np.inf, -np.inf], dtype=F), rng.uniform(0.0, 1.0, 12).astype(F)])
    ix, iy, iz = np.meshgrid(np.arange(w), np.arange(h), np.arange(len(zs)), indexing="ij")
    ix, iy, iz = ix.ravel(), iy.ravel(), iz.ravel()
    return ix, iy, xs[ix], ys[iy], zs[iz]


def assert_rows_equal(P, V, w, h, skip, rng, label):
    """Bitwise, on every lane the kernel lets take the short rows: a finite, nonzero vw, and not on the skipped column / row."""
    px, py, nx, ny, nz = pixel_inputs(w, h, rng)
    g = general_rows(P, V, nx, ny, nz)
    s = short_rows(P, nx, ny, nz)
    ok = s[5] & (px != skip[0]) & (py != skip[1])
    assert ok.any() and (~ok).any(), label
    # every lane with a non-finite depth sample, and every lane with vw = +-0, is one the kernel's test catches
    assert not ok[~np.isfinite(nz)].any(), label
    for name, a, b in zip(("vx", "vy", "vz", "vw", "ww"), g, s):
        differ = _bits(a)[ok] != _bits(b)[ok]
        assert not differ.any(), (label, name, int(differ.sum()))
    return int(ok.sum())


# ---- the cameras ------------------------------------------------------------------------------------------------------------------------------------------

def demo_cameras():
    for pose in S.POSES:
        for w, h in ((67, 35), (64, 36), (1920, 1080)):
            yield f"{pose} {w}x{h}", S.Camera.from_pose(w, h, pose)
        yield f"{pose} forward-z", S.Camera.from_pose(67, 35, pose, reverse_z=False)


def projection_cameras():
    for kind in K.KINDS:
        for pose in ("P_space", "P_limb"):
            yield f"{kind} {pose}", K.demo_camera(kind, pose)


def test_header_symbols_and_binding():
    from godot_atmosphere_shader_amd import _native as N

    with open(os.path.join(ROOT, "include", "atmo_debug_prologue.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(atmo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(N.PROLOGUE_SYMBOLS) == {"atmo_debug_prologue_mode", "atmo_debug_prologue_constants"}
    lib = N.load()
    for sym in N.PROLOGUE_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS
    assert (N.PROLOGUE_CAMERA, N.PROLOGUE_POW2_STEPS, N.PROLOGUE_NO_SPHERE_DEPTH) == (CAMERA, POW2, NO_SPHERE_DEPTH)
    for name, bit in (("ATMO_PROLOGUE_CAMERA", 1), ("ATMO_PROLOGUE_POW2_STEPS", 2), ("ATMO_PROLOGUE_NO_SPHERE_DEPTH", 4)):
        assert re.search(rf"#define {name} {bit}u\b", header)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5


def test_the_predicate_accepts_the_cameras_that_are_drawn():
    """Every demo pose as bench.py and the direct-diet cases build it (scene.Camera.from_pose; both z conventions), every camera of the bitwise goldens
    (tests/golden/direct_diet): all three bits, so the goldens run the short forms and tie them to the parent build's bits.  The off-axis, jittered and
    infinite-far cameras: accepted.  The orthographic one: rejected -- and so is the forward-z camera as numpy inverts it, whose element 10 is -4.9e-17, not
    a zero: "about zero" is no premise.  Everywhere the library's mask is the restated predicate's."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx()
    try:
        seen = {}
        cams = list(demo_cameras()) + [(f"golden {p}", S.Camera.from_pose(DC.W, DC.H, DC.POSES[p])) for p in DC.POSES] + list(projection_cameras())
        for label, cam in cams:
            frame = _frame(cam)
            P, V = _matrices(frame)
            got = _mode(ctx, frame)
            want = predicate(P, V, np.array(frame.planet_center_viewspace, dtype=F), S.DEMO_PLANET_RADIUS, S.DEMO_ATMOSPHERE_HEIGHT, 32, 0.0)
            assert got == want, (label, got, want)
            seen[label] = got
            if "forward-z" in label:
                assert 0 < abs(float(P[10])) < 1e-15
        for label, got in seen.items():
            if label.startswith("ortho") or "forward-z" in label:
                assert got == POW2, (label, got)
            else:
                assert got == CAMERA | POW2 | NO_SPHERE_DEPTH, (label, got)
        assert sum(label.startswith("ortho") for label in seen) == 2 and sum(label.startswith("eye_") for label in seen) == 4
    finally:
        lib.atmo_destroy(ctx)


def test_steps_and_depth_factor_bits():
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    frame = _frame(S.Camera.from_pose(67, 35, "P_space"))
    for steps, factor, want in ((32, 0.0, 7), (16, 0.0, 7), (8, -0.0, 7), (24, 0.0, 5), (12, 0.35, 1), (32, 1.0, 3), (32, 1e-45, 3), (1, 0.0, 7)):
        ctx = _host_ctx(view_steps=steps, u_sphere_depth_factor=factor)
        try:
            assert _mode(ctx, frame) == want, (steps, factor)
        finally:
            lib.atmo_destroy(ctx)


def test_the_environment_switch_forces_the_mask_to_zero(monkeypatch):
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    frame = _frame(S.Camera.from_pose(67, 35, "P_space"))
    monkeypatch.setenv("ATMO_PROLOGUE_CAMERA", "0")
    ctx = _host_ctx()
    monkeypatch.delenv("ATMO_PROLOGUE_CAMERA")
    on = _host_ctx()
    try:
        # read when the context is made, as atmo_create does (tests/test_prologue_camera_gpu.py holds the switch on a device)
        assert _mode(on, frame) == 7
        assert _mode(ctx, frame) == 0
    finally:
        lib.atmo_destroy(ctx)
        lib.atmo_destroy(on)


def test_short_rows_equal_the_general_rows_bit_for_bit_where_the_predicate_accepts():
    """The demo poses, both z conventions, the off-axis / jittered / infinite-far cameras, at odd viewports (nx = +0 on the centre column of 67, ny = +0 on
    the centre row of 35) and an even one; then the same matrices with the sign bit set on random subsets of their zeros and with the signs of the two
    scales flipped.  The library's mask and its skipped column / row are the restatement's, and on every lane that is left the rows are equal."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx()
    rng = np.random.default_rng(20250611)
    accepted = rejected = lanes = skipped = 0
    try:
        cams = [(label, cam) for label, cam in list(demo_cameras()) + list(projection_cameras()) if "1920" not in label]
        for label, cam in cams:
            for trial in range(9):
                w, h = ((67, 35), (64, 36), (67, 36))[trial % 3]
                cam.width, cam.height = w, h     # the matrices stay: any viewport may be drawn with them
                frame = _frame(cam)
                P, V = _matrices(frame)
                if trial:   # the sign bit on a random subset of the zeros (trial 1: on all of them), a random sign on the x and y scales
                    if "forward-z" in label:
                        P[10] = F(0.0)   # the exact inverse's zero, where numpy's has -4.9e-17: the forward-z matrices are accepted with it
                    for m in (P, V):
                        z = np.flatnonzero(m == 0)
                        pick = z if trial == 1 else z[rng.random(len(z)) < 0.5]
                        m[pick] = F(-0.0)
                    for i in (0, 5):
                        P[i] = -P[i] if rng.random() < 0.5 else P[i]
                    frame.inv_projection_matrix[:] = P.tolist()
                    frame.inv_view_matrix[:] = V.tolist()
                    P2, V2 = _matrices(frame)
                    assert np.array_equal(_bits(P), _bits(P2)) and np.array_equal(_bits(V), _bits(V2))
                mode, sx, sy = _mode_skips(ctx, frame)
                assert mode == predicate(P, V, np.array(frame.planet_center_viewspace, dtype=F), S.DEMO_PLANET_RADIUS, S.DEMO_ATMOSPHERE_HEIGHT, 32, 0.0)
                if mode & CAMERA:
                    assert (sx, sy) == skips(P, w, h), (label, trial)
                    accepted += 1
                    skipped += (sx >= 0) + (sy >= 0)
                    lanes += assert_rows_equal(P, V, w, h, (sx, sy), rng, (label, trial))
                else:
                    assert (label.startswith("ortho") or ("forward-z" in label and trial == 0)) and (sx, sy) == (-1, -1)
                    rejected += 1
        print(f"{accepted} matrices accepted ({lanes} lanes compared, {skipped} skipped columns / rows), {rejected} rejected")
        assert accepted == 9 * (len(cams) - 2) - 5 and rejected == 18 + 5 and skipped >= 20
    finally:
        lib.atmo_destroy(ctx)


def test_the_skipped_row_is_where_the_short_form_has_other_bits():
    """The demo camera as numpy's inverse leaves it: P[13] = -0 and P[5] < 0.  On the centre row of a 35-row viewport ny = +0, a = P[5] ny = -0, and the
    short row's -0 + -0 = -0 stands against the general row's +0 on the lanes where P[1] nx or P[9] nz is +0: the library names row 17, and only there do
    the rows differ."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = _host_ctx()
    try:
        cam = S.Camera.from_pose(67, 35, "P_space")
        frame = _frame(cam)
        P, V = _matrices(frame)
        assert int(_bits(P[13])) == 0x80000000 and P[5] < 0 and int(_bits(P[12])) == 0
        assert _mode_skips(ctx, frame) == (7, -1, 17)
        px, py, nx, ny, nz = pixel_inputs(67, 35, np.random.default_rng(3))
        g, s = general_rows(P, V, nx, ny, nz), short_rows(P, nx, ny, nz)
        differ = (_bits(g[1]) != _bits(s[1])) & s[5]
        assert differ.any() and (py[differ] == 17).all()
        # bench.py's viewports are even: nothing to skip
        for w, h in ((1920, 1080), (3840, 2160), (64, 36)):
            assert _mode_skips(ctx, _frame(S.Camera.from_pose(w, h, "P_space"))) == (7, -1, -1)
    finally:
        lib.atmo_destroy(ctx)


def test_random_scenes_share():
    """tests/random_scenes.SEEDS (47 scenes, all scene.Camera): every camera is accepted; the steps bit follows the variant's view steps (16, 64, 8, 8, 12,
    8 by seed % 6: all but the fifth), the depth-factor bit the scene's factor (0, 0.35 or 1)."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    counts = {CAMERA: 0, POW2: 0, NO_SPHERE_DEPTH: 0}
    zero_factor = 0
    for seed in RS.SEEDS:
        params, cam_kw, sun = RS.random_scene_parts(np.random.default_rng(1000 + seed), seed)
        steps = RS.variant_of(seed)[1]["view_steps"]
        ctx = _host_ctx(view_steps=steps, u_planet_radius=params["u_planet_radius"], u_atmosphere_height=params["u_atmosphere_height"],
                        u_sphere_depth_factor=params["u_sphere_depth_factor"])
        try:
            cam = S.Camera(**cam_kw)
            frame = _to_native_frame(make_frame(cam, np.eye(4), sun))
            got = _mode(ctx, frame)
            P, V = _matrices(frame)
            assert got == predicate(P, V, np.array(frame.planet_center_viewspace, dtype=F), params["u_planet_radius"], params["u_atmosphere_height"], steps,
                                    params["u_sphere_depth_factor"]), seed
            for bit in counts:
                counts[bit] += bool(got & bit)
            zero_factor += params["u_sphere_depth_factor"] == 0.0
        finally:
            lib.atmo_destroy(ctx)
    print(counts, zero_factor)
    assert len(RS.SEEDS) == 47
    assert counts[CAMERA] == 47
    assert counts[POW2] == sum(seed % 6 != 4 for seed in RS.SEEDS) == 38
    assert counts[NO_SPHERE_DEPTH] == zero_factor == 25     # the scenes whose u_sphere_depth_factor was drawn as 0 (of 0, 0.35, 1)


def test_division_by_a_power_of_two_is_the_product_with_its_reciprocal():
    """x / n == x * (1 / n) in their bits for n = 8, 16, 32, 64: random x over the whole exponent range, both signs, and the edges -- zeros, the smallest
    subnormals and normals (the quotient is subnormal and rounds to even on the subnormal grid either way), the largest finite, inf, NaN."""
    rng = np.random.default_rng(7)
    x = (rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32)).view(F)
    edge_bits = np.array([0, 1, 2, 3, 5, 7, 31, 32, 33, 63, 64, 65, 0x7FFFFF, 0x800000, 0x800001, 0xFFFFFF, 0x1000000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000],
                         dtype=np.uint32)
    x = np.concatenate([x, edge_bits.view(F), (edge_bits | np.uint32(0x80000000)).view(F)])
    for n in (8, 16, 32, 64):
        inv = F(1.0) / F(n)
        assert float(inv) * n == 1.0
        with np.errstate(all="ignore"):
            q, p = x / F(n), x * inv
        same = (_bits(q) == _bits(p)) | (np.isnan(q) & np.isnan(p))
        assert same.all(), (n, x[~same][:4])
        assert (np.abs(q[np.isfinite(q)]) < F(2.0 ** -126)).sum() > 1000    # subnormal quotients are among them


def test_dropping_the_ground_sphere_term_leaves_linear_depth():
    """linear_depth (1 - f) + gd f for f = +-0 and a finite gd of either sign is linear_depth in its bits, for +0, positive, inf and NaN linear_depth (the root
    of a sum of squares is never -0)."""
    ld = np.array([0.0, 1e-45, 1e-30, 0.37, 1.0, 153.25, 3e38, np.inf, np.nan], dtype=F)
    gd = np.array([10000000.0, 57.5, 1e-45, 0.0, -0.0, -3.25, -1e38, 3e38], dtype=F)
    for f in (F(0.0), F(-0.0)):
        with np.errstate(all="ignore"):
            got = ld[:, None] * (F(1.0) - f) + gd[None, :] * f
        assert np.array_equal(_bits(got), _bits(np.broadcast_to(ld[:, None], got.shape)))
    # ... and the squares' sum: no -0, whatever the signs of the zeros that go in
    z = np.array([0.0, -0.0], dtype=F)
    for a, b, c in itertools.product(z, z, z):
        assert int(_bits(np.sqrt(a * a + b * b + c * c))) == 0


def test_handed_over_constants_are_the_kernels_own_products():
    """atmosphere_radius^2, planet_radius^2, density^2, density^2 / 8, -coeff * LOG2E, (float)view_steps and the exact 1 / view_steps: one float32 operation
    each on the values of atmo_debug_frame_constants -- what the kernels evaluated per wave."""
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    frame = _frame(S.Camera.from_pose(67, 35, "P_limb"))
    cases = [dict(), dict(u_planet_radius=637.1, u_atmosphere_height=33.3, u_density=0.731, u_scattering_strength=1.7),
             dict(u_planet_radius=2.0 ** -45, u_atmosphere_height=2.0 ** -49, u_density=3.3e7)]
    for steps, over in itertools.product((32, 24, 5), cases):
        ctx = _host_ctx(view_steps=steps, **over)
        try:
            out = (C.c_float * 16)()
            n = C.c_int(0)
            assert lib.atmo_debug_prologue_constants(ctx, C.byref(frame), out, 16, C.byref(n)) == N.ATMO_OK and n.value == 16
            assert lib.atmo_debug_prologue_constants(ctx, C.byref(frame), out, 15, None) == N.ATMO_E_ARG
            v = np.array(out, dtype=F)
            fc = (C.c_float * 81)()
            assert lib.atmo_debug_frame_constants(ctx, C.byref(frame), 0, fc, 81, None) == N.ATMO_OK
            fc = np.array(fc, dtype=F)
            ratm, coeff = fc[6], fc[7:10]
            assert np.array_equal(_bits(v[9]), _bits(ratm)) and np.array_equal(_bits(v[12:15]), _bits(coeff))
            rpl, dens = v[10], v[11]
            got = (C.c_float * 1)()
            assert lib.atmo_get_param_f32(ctx, b"u_planet_radius", got, 1) == N.ATMO_OK and F(got[0]) == rpl
            assert lib.atmo_get_param_f32(ctx, b"u_density", got, 1) == N.ATMO_OK and F(got[0]) == dens
            want = [F(1.0) / F(steps) if steps & (steps - 1) == 0 else F(0.0), F(steps), ratm * ratm, rpl * rpl, dens * dens, (dens * dens) * F(0.125),
                    -coeff[0] * LOG2E, -coeff[1] * LOG2E, -coeff[2] * LOG2E]
            assert np.array_equal(_bits(v[:9]), _bits(np.array(want, dtype=F))), (steps, over, v[:9], want)
        finally:
            lib.atmo_destroy(ctx)
