"""The sky as light on the CPU (include/atmo_sky_sh.h; godot_atmosphere_shader_amd/sky_sh.py): the header's symbol set and the binding, every refusal of the
entry points on a host-only context in the header's order (nothing touches a device), the scratch size, and the numpy statement itself -- the solid
angles of every lens summed over the sphere, quad order and bands, known answers of the projection, the float32 order of the sums against float64 -- and
the three kernel families in the compiled assembly.  (tests/test_sky_sh_gpu.py holds the kernels to the statement.)"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import test_kernel_twins_host as T
from godot_atmosphere_shader_amd import lens as L
from godot_atmosphere_shader_amd import sky_sh as SH
from godot_atmosphere_shader_amd.lens import Lens
from godot_atmosphere_shader_amd.ray_quads import quad_order
from test_rays_host import _mode_ctx, _said
from test_views_proxy_host import ROOT, _functions

RAYS, RGBA, WEIGHT, SCRATCH, OUT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000   # addresses no refusal dereferences
FOUR_PI = 4.0 * math.pi


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, SH.bind()


def _ctx(N, lib):
    return _mode_ctx(N, lib, N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)   # direct light without clouds needs no texture


# ---- the header and the binding ----------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_the_sky_sh_header():
    """Fails on a library without the feature: the header does not exist and the symbols are not exported."""
    N, lib = _lib()
    assert _functions("atmo_sky_sh.h") == set(SH.SKY_SH_ENTRY_POINTS) and len(SH.SKY_SH_ENTRY_POINTS) == 3
    assert tuple(SH.signatures()) == SH.SKY_SH_ENTRY_POINTS
    tuples = {name: value for name, value in vars(N).items() if name.endswith("_SYMBOLS") and isinstance(value, tuple)}
    assert len(tuples) > 10
    for sym in SH.SKY_SH_ENTRY_POINTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int
        assert not any(sym in symbols for symbols in tuples.values()), sym
        assert not any(sym in symbols for symbols, _, _, _ in N.HEADERS.values())      # declared by sky_sh.py, not by a block of _native.HEADERS
    assert lib is N.load() and lib.atmo_abi_version() == N.ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "atmo_sky_sh.h")).read()
    assert '#include "atmo_lens.h"' in text and "THE ORDER OF THE 37 SUMS" in text and "Not here" in text
    for name in ("atmo.h", "atmo_rays.h", "atmo_lens.h", "atmo_reduced.h"):   # the older headers do not know the new one
        assert "atmo_sky_sh" not in open(os.path.join(ROOT, "include", name)).read(), name
    # the order's constants are the header's, in one place
    assert (SH.LANES, SH.RAYS_PER_LANE, SH.SEGMENT, SH.FLOATS, SH.SUMS, SH.ACCUMULATE) == (256, 16, 4096, 40, 37, 1)


def test_a_library_without_the_symbols_is_refused_by_name():
    class Fn:
        restype = argtypes = None

    class Old:
        atmo_lens_solid_angles = Fn()   # some, not all

    with pytest.raises(RuntimeError, match=r"atmo_sky_sh9_scratch_bytes \(include/atmo_sky_sh\.h\)"):
        SH.bind(Old())
    assert Old.atmo_lens_solid_angles.argtypes is not None


def test_the_scratch_size():
    N, lib = _lib()
    for n, want in ((0, 0), (1, 160), (4096, 160), (4097, 320), (1 << 28, 160 << 16)):
        got = C.c_size_t(12345)
        assert lib.atmo_sky_sh9_scratch_bytes(n, C.byref(got)) == N.ATMO_OK and got.value == want == SH.scratch_bytes(n), n
    got = C.c_size_t(12345)
    assert lib.atmo_sky_sh9_scratch_bytes((1 << 28) + 1, C.byref(got)) == N.ATMO_E_ARG and got.value == 12345
    assert lib.atmo_sky_sh9_scratch_bytes(1, None) == N.ATMO_E_ARG
    with pytest.raises(ValueError):
        SH.scratch_bytes((1 << 28) + 1)


# ---- the refusals, in the header's order ------------------------------------------------------------------------------------------------------------
def _solid(lib, ctx, lens=True, kind=L.OCTAHEDRAL, width=8, height=8, rows=(0, 8), face=0, fov=1.0, flags=0, weight=WEIGHT):
    N, _ = _lib()
    nl = N.AtmoLens()
    nl.kind, nl.width, nl.height, nl.y0, nl.y1, nl.face, nl.fov = kind, width, height, rows[0], rows[1], face, fov
    return _said(lib, ctx, lib.atmo_lens_solid_angles(ctx, C.byref(nl) if lens else None, flags, weight, None))


def _project(lib, ctx, rays=RAYS, rgba=RGBA, weight=WEIGHT, n=5000, flags=0, scratch=SCRATCH, scratch_bytes=320, out=OUT):
    return _said(lib, ctx, lib.atmo_sky_sh9(ctx, rays, rgba, weight, n, flags, scratch, scratch_bytes, out, None))


# (what the message must hold, the one thing wrong), in the order of the checks
SOLID_CHECKS = [("null lens", dict(lens=False)), ("unknown lens kind", dict(kind=4)), ("unknown flag bits", dict(flags=2)),
                ("width and height", dict(width=0)), ("2^28", dict(width=1 << 15, height=(1 << 13) + 1, rows=(0, 2))), ("band", dict(rows=(0, 9))),
                ("fov", dict(kind=L.FISHEYE, fov=7.0)), ("square", dict(kind=L.CUBE_FACE, width=9)), ("face", dict(kind=L.CUBE_FACE, face=6)),
                ("even y0", dict(flags=1, rows=(1, 8))), ("null weight_dev", dict(weight=0)), ("4-byte aligned", dict(weight=WEIGHT + 2))]
PROJECT_CHECKS = [("null out_dev", dict(out=0)), ("out_dev must be 16-byte aligned", dict(out=OUT + 8)), ("unknown flag bits", dict(flags=2)),
                  ("null rays_dev", dict(rays=0)), ("null rgba_dev", dict(rgba=0)), ("rays_dev must be 16-byte aligned", dict(rays=RAYS + 8)),
                  ("rgba_dev must be 16-byte aligned", dict(rgba=RGBA + 4)), ("weight_dev must be 4-byte aligned", dict(weight=WEIGHT + 1)),
                  ("2^28", dict(n=(1 << 28) + 1, scratch_bytes=1 << 40)), ("null scratch_dev", dict(scratch=0)),
                  ("scratch_dev must be 16-byte aligned", dict(scratch=SCRATCH + 4)), ("scratch_bytes is below", dict(scratch_bytes=319))]


@pytest.mark.parametrize("entry", ["atmo_lens_solid_angles", "atmo_sky_sh9"])
def test_every_refusal_in_the_header_s_order(entry):
    """Each wrong argument alone is ATMO_E_ARG under the entry point's name; of two wrong arguments the one the header lists first is named; a well-formed
    call on a host-only context gets as far as ATMO_E_NO_DEVICE."""
    N, lib = _lib()
    ctx = _ctx(N, lib)
    call, checks = (_solid, SOLID_CHECKS) if entry == "atmo_lens_solid_angles" else (_project, PROJECT_CHECKS)
    try:
        for needle, wrong in checks:
            rc, msg = call(lib, ctx, **wrong)
            assert rc == N.ATMO_E_ARG and msg.startswith(entry + ": ") and needle in msg, (wrong, rc, msg)
        for (needle, first), (_, second) in zip(checks, checks[1:]):
            if set(first) & set(second):
                continue    # two values of one argument
            rc, msg = call(lib, ctx, **first, **second)
            assert rc == N.ATMO_E_ARG and needle in msg, (first, second, rc, msg)
        rc, msg = call(lib, ctx)
        assert rc == N.ATMO_E_NO_DEVICE and msg.startswith(entry + ": ") and "host-only" in msg, (rc, msg)
        if entry == "atmo_lens_solid_angles":
            assert _solid(lib, ctx, flags=1)[0] == N.ATMO_E_NO_DEVICE and _solid(lib, ctx, kind=L.FISHEYE, fov=6.2831855)[0] == N.ATMO_E_NO_DEVICE
            assert _solid(lib, ctx, rows=(3, 3), kind=9, weight=0)[0] == N.ATMO_OK        # an empty band: nothing else is looked at
            assert lib.atmo_lens_solid_angles(None, None, 0, None, None) == N.ATMO_E_ARG  # a null ctx: no message to hold
        else:
            assert _project(lib, ctx, weight=0)[0] == N.ATMO_E_NO_DEVICE                  # a null weight_dev: every ray weighs 1
            assert _project(lib, ctx, flags=1)[0] == N.ATMO_E_NO_DEVICE
            # n_rays == 0: behind out_dev and the flags, in front of everything else
            assert _project(lib, ctx, n=0, flags=1, rays=0, rgba=0, scratch=0, scratch_bytes=0)[0] == N.ATMO_OK
            assert _project(lib, ctx, n=0, out=0)[0] == N.ATMO_E_ARG and _project(lib, ctx, n=0, flags=4)[0] == N.ATMO_E_ARG
            assert _project(lib, ctx, n=0, rays=0)[0] == N.ATMO_E_NO_DEVICE               # the memset of 40 floats is all a host-only context lacks
            assert lib.atmo_sky_sh9(None, RAYS, RGBA, None, 1, 0, SCRATCH, 160, OUT, None) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)


# ---- solid angles: the statement ----------------------------------------------------------------------------------------------------------------------
COVERAGE = {"octahedral": ([Lens.octahedral(32, 32)], FOUR_PI, 1e-5),
            "cube": ([Lens.cube_face(16, f) for f in range(6)], FOUR_PI, 2e-3),
            "equirect": ([Lens.equirect(64, 32)], FOUR_PI, 1e-3),
            "fisheye180": ([Lens.fisheye(64, 64, fov=math.pi)], 2.0 * math.pi, 5e-3),
            "fisheye360": ([Lens.fisheye(64, 64, fov=2.0 * math.pi)], FOUR_PI, 1e-4)}


@pytest.mark.parametrize("name", list(COVERAGE))
def test_the_solid_angles_cover_the_sphere(name):
    """The tolerances are the midpoint rule's own error at these sizes, measured in float64 with margin (1.2e-7, 9.6e-4, 4.0e-4, 2.7e-3, 2.2e-6)."""
    lenses, want, tol = COVERAGE[name]
    total = 0.0
    for lens in lenses:
        w = SH.solid_angles(lens)
        assert w.dtype == np.float32 and w.shape == (lens.counts()[0],) and np.all(w >= 0.0) and not np.signbit(w).any()
        total += float(w.astype(np.float64).sum())
    err = abs(total - want) / want
    print(f"{name}: sum of the solid angles {total:.9f}, {err:.2e} relative from {want:.9f} (tolerance {tol:.0e})")
    assert err <= tol, (name, total, err)


def test_the_float32_lenses_restate_the_lens_s_own_root():
    """sky_sh.py forms n and len once more: the directions they give are lens.py's bytes."""
    i = np.arange(33 * 18)
    x, y = i % 33, i // 33
    with np.errstate(all="ignore"):
        lens = Lens.octahedral(33, 18)
        d, _ = L.lens_directions(lens, x, y)
        n3 = ((np.float32(4.0) / np.float32(33)) / np.float32(18)) / SH.solid_angles(lens)       # RN(RN(n n) n), up to the quotient's rounding
        assert np.allclose(n3, 1.0 / np.abs(d).sum(axis=1).astype(np.float64) ** 3, rtol=1e-6)  # |p| of the L1 octahedron along d is 1 / |d|_1
        lens = Lens.cube_face(18, 3)
        d, _ = L.lens_directions(lens, i[:324] % 18, i[:324] // 18)
        len3 = (np.float32(1.0) / np.float32(9.0) / np.float32(9.0)) / SH.solid_angles(lens)
        assert np.allclose(len3, 1.0 / np.abs(d).max(axis=1).astype(np.float64) ** 3, rtol=1e-6)  # len = 1 / the direction's largest component


@pytest.mark.parametrize("lens", [Lens.octahedral(7, 5), Lens.cube_face(9, 2), Lens.equirect(33, 18), Lens.fisheye(17, 13, fov=math.radians(220.0))], ids=repr)
def test_quad_order_and_bands(lens):
    whole = SH.solid_angles(lens)
    order = quad_order(lens.width, lens.height)
    want = np.where(order >= 0, whole[np.clip(order, 0, None)], np.float32(0.0))
    got = SH.solid_angles(lens, quads=True)
    assert got.tobytes() == want.tobytes() and not np.signbit(got[order < 0]).any()
    if lens.kind == L.FISHEYE:
        absent = ~np.any(L.lens_rays(lens)[:, 4:7] != 0, axis=1)
        assert absent.any() and np.all(whole[absent] == 0.0) and np.all(whole[~absent] > 0.0)
    y0, y1 = 2, lens.height - 1 if lens.height % 2 == 0 else 4
    band = lens.band((y0, y1))
    assert SH.solid_angles(band).tobytes() == whole[y0 * lens.width:y1 * lens.width].tobytes()
    if y1 % 2 == 0:
        qpr = (lens.width + 1) // 2
        assert SH.solid_angles(band, quads=True).tobytes() == got[4 * qpr * (y0 // 2):4 * qpr * (y1 // 2)].tobytes()


def test_no_weight_is_negative_where_theta_passes_pi():
    lens = Lens.fisheye(64, 64, fov=L.MAX_FOV)      # 6.2831855f exceeds 2 pi: sin theta turns negative along the circle
    w = SH.solid_angles(lens)
    assert np.all(w >= 0.0) and not np.signbit(w).any()


# ---- the projection: known answers ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def octa():
    lens = Lens.octahedral(32, 32)
    dirs, w = L.lens_rays(lens)[:, 4:7], SH.solid_angles(lens)
    dirs.setflags(write=False)
    w.setflags(write=False)
    return dirs, w


def _normals():
    n = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=np.float64)
    assert n.shape == (26, 3)
    return n


def test_a_white_sky_is_band_zero_and_pi_of_irradiance(octa):
    dirs, w = octa
    sh = SH.sh9_project(dirs, np.ones((dirs.shape[0], 4), dtype=np.float32), w)
    assert sh.dtype == np.float32 and sh.shape == (40,) and not sh[37:].any()
    assert np.all(np.abs(sh[0:4] - math.sqrt(FOUR_PI)) <= 1e-5 * math.sqrt(FOUR_PI)), sh[0:4]
    assert np.all(np.abs(sh[4:16]) < 1e-5), sh[4:16]
    assert abs(float(sh[36]) - FOUR_PI) <= 1e-5 * FOUR_PI
    e = SH.sh9_irradiance(sh, _normals())
    print(f"white sky: band 2 leaks {np.abs(sh[16:36]).max():.3e}; irradiance within {np.abs(e / math.pi - 1.0).max():.3e} of pi")
    assert e.shape == (26, 4) and np.all(np.abs(e - math.pi) <= 2e-3 * math.pi)
    # sh9_eval is the same sum without the cosine lobe's factors: along +Z only Y0, Y2 and Y6 are not zero
    up = SH.sh9_eval(sh, [(0.0, 0.0, 2.0)])
    want = 0.28209479 * sh[0:4] + 0.48860251 * sh[8:12] + 0.31539157 * 2.0 * sh[24:28]
    assert up.shape == (1, 4) and np.allclose(up[0], want, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_linear_sky_is_its_band_one_coefficient(octa, axis):
    dirs, w = octa
    rgba = np.ones((dirs.shape[0], 4), dtype=np.float32)
    rgba[:, :3] = dirs[:, axis:axis + 1]                     # radiance d . s, alpha 1
    sh = SH.sh9_project(dirs, rgba, w)
    k = {0: 3, 1: 1, 2: 2}[axis]                             # Y3 is x, Y1 is y, Y2 is z
    want = FOUR_PI / 3.0 * 0.48860251
    assert np.all(np.abs(sh[4 * k:4 * k + 3] - want) <= 5e-3 * want), (axis, sh[4 * k:4 * k + 3], want)
    others = [j for j in (1, 2, 3) if j != k]
    assert all(np.all(np.abs(sh[4 * j:4 * j + 3]) < 1e-5) for j in others) and np.all(np.abs(sh[0:3]) < 1e-5)


def test_the_basis_is_orthonormal_under_the_lens_s_own_weights(octa):
    dirs, w = octa
    y = SH.sh9_basis(dirs).astype(np.float64)
    assert SH.sh9_basis(dirs).dtype == np.float32 and y.shape == (1024, 9)
    gram = (y * w[:, None].astype(np.float64)).T @ y
    assert np.abs(gram - np.eye(9)).max() < 5e-3, np.abs(gram - np.eye(9)).max()


# ---- the float32 order of the sums against float64 -------------------------------------------------------------------------------------------------------
def random_inputs(n, seed):
    """Directions on the sphere, weights in [0, 1) with a tenth of them zero, rgba in [0, 4): float32."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, 3))
    dirs = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    rgba = rng.uniform(0.0, 4.0, (n, 4)).astype(np.float32)
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    w[rng.random(n) < 0.1] = 0.0
    return dirs, rgba, w


@pytest.mark.parametrize("n", [1, 257, 4097, 3 * 4096 + 5, 300 * 4096 + 1])
def test_the_float32_sums_lie_within_the_bound_of_the_float64_sums(n):
    dirs, rgba, w = random_inputs(n, n)
    got = SH.sh9_project(dirs, rgba, w)
    want, magnitude = SH.sh9_project64(dirs, rgba, w)
    bound = SH.sh9_error_bound(n, magnitude)
    assert got.dtype == np.float32 and np.all(np.isfinite(got)) and want.shape == magnitude.shape == bound.shape == (40,)
    assert bound[36] == (16 + 8 + -(-SH.segments(n) // 256) + 8 + 1 + 6) * 2.0 ** -24 * magnitude[36] * 1.01
    err = np.abs(got.astype(np.float64) - want)
    print(f"n = {n}: largest error over its bound {np.max(err[:37] / np.maximum(bound[:37], 1e-300)):.3f}")
    assert np.all(err <= bound), (n, err, bound)
    # a zero weight keeps its ray out of every sum, whatever the ray holds
    dirs2, rgba2 = dirs.copy(), rgba.copy()
    dirs2[w == 0], rgba2[w == 0] = np.nan, np.nan
    assert SH.sh9_project(dirs2, rgba2, w).tobytes() == got.tobytes()
    # ACCUMULATE is one more float32 addition per sum
    again = SH.sh9_project(dirs, rgba, w, prev=got)
    assert again[:37].tobytes() == (got[:37] + got[:37]).tobytes() and not again[37:].any()
    assert SH.sh9_project(dirs[:0], rgba[:0], w[:0], prev=got).tobytes() == got.tobytes() and not SH.sh9_project(dirs[:0], rgba[:0]).any()


def test_the_order_of_the_sums_is_the_header_s():
    """Spelled out in plain loops on a case small enough for them: two segments, the second ragged."""
    n = 4096 + 300
    dirs, rgba, w = random_inputs(n, 7)
    t = SH._terms(dirs, rgba, w, np.float32)
    assert t.dtype == np.float32 and t.shape == (n, 37)
    k, ch, i = 6, 1, int(np.flatnonzero(w)[0])
    y6 = np.float32(0.31539157) * (np.float32(3.0) * (dirs[i, 2] * dirs[i, 2]) - np.float32(1.0))
    assert t[i, 4 * k + ch] == (w[i] * y6) * (rgba[i, ch] * rgba[i, 3]) and t[i, 36] == w[i] and t[i, 4 * k + 3] == (w[i] * y6) * rgba[i, 3]
    partials = []
    for seg in range(2):
        v = np.zeros((256, 37), dtype=np.float32)
        for lane in range(256):
            for j in range(16):
                r = 4096 * seg + 256 * j + lane
                if r < n:
                    v[lane] = v[lane] + t[r]
        s = 128
        while s >= 1:
            for lane in range(s):
                v[lane] = v[lane] + v[lane + s]
            s //= 2
        partials.append(v[0].copy())
    v = np.zeros((256, 37), dtype=np.float32)
    v[0], v[1] = partials
    s = 128
    while s >= 1:
        for lane in range(s):
            v[lane] = v[lane] + v[lane + s]
        s //= 2
    assert SH.sh9_project(dirs, rgba, w)[:37].tobytes() == v[0].tobytes()


# ---- the kernels in the compiled assembly ----------------------------------------------------------------------------------------------------------------
def test_the_three_kernel_families_have_no_stack_frame():
    """Present under their mangled names (tools/twin_resources.py reads the compiler's own numbers), no private-memory stack, names of their own."""
    numbers = T.twin_resources.kernels(T._asm())
    solid = {n: k for n, k in numbers.items() if n.startswith("_ZN4atmo28atmo_lens_solid_angle_kernelILi")}
    assert len(solid) == 8 and {n[len("_ZN4atmo28atmo_lens_solid_angle_kernel"):].split("EE")[0] + "EE" for n in solid} == {
        f"ILi{kind}ELi{quads}EE" for kind in range(4) for quads in range(2)}
    (segment,) = [k for n, k in numbers.items() if n.startswith("_ZN4atmo27atmo_sky_sh9_segment_kernelE")]
    (total,) = [k for n, k in numbers.items() if n.startswith("_ZN4atmo25atmo_sky_sh9_total_kernelE")]
    for name, k in list(solid.items()) + [("segment", segment), ("total", total)]:
        print(name, k)
        assert k["scratch"] == 0 and k["spill_reads"] == 0, name
    assert segment["vgprs"] >= 37 and segment["vgprs"] <= 128        # 37 running sums in registers, and two workgroups of four waves a SIMD can hold
    text = open(os.path.join(ROOT, "include", "atmo_sky_sh.h")).read()
    assert f"{segment['vgprs']} VGPRs, 37888 bytes of LDS" in text and f"one workgroup, {total['vgprs']} VGPRs" in text   # the header states what the compiler gives

    def base(mangled):     # _ZN4atmo<length><name>...
        m = T.re.match(r"_ZN4atmo(\d+)", mangled)
        return mangled[m.end():m.end() + int(m.group(1))] if m else mangled

    names = {base(n) for n in numbers}
    new_names = {"atmo_lens_solid_angle_kernel", "atmo_sky_sh9_segment_kernel", "atmo_sky_sh9_total_kernel"}
    assert new_names <= names
    for a in new_names:
        for b in names - {a}:
            assert a not in b and b not in a, (a, b)
