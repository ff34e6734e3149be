"""CPU tests of the lens header (include/atmo_lens.h): the header's symbol set and the binding, every refusal of atmo_lens_rays on a host-only context in the
header's order (nothing touches a device), atmo_lens_ray_counts, and the numpy statement of the four lenses (godot_atmosphere_shader_amd/lens.py): the cube
face against the oracle's texel-to-direction table bit for bit, the octahedral map against the ray key at every pixel of 512 x 512, the float64 inverse of
every lens, the equirect's known answers, the quad order and the tile index against brute force.  (tests/test_lens_gpu.py holds the kernels to the numpy
statement.)"""
import ctypes as C
import math

import numpy as np
import pytest

from test_rays_host import _said
from test_views_proxy_host import ROOT, _functions, _host_ctx

RAYS, INDEX, DIST = 0x10000, 0x40000, 0x70000   # addresses no refusal dereferences
WHO = "atmo_lens_rays: "
NAMES = {"atmo_lens_ray_counts", "atmo_lens_rays"}
W, H, BAND = 37, 19, (2, 12)


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, N.load()


def _lenses(rows=None):
    from godot_atmosphere_shader_amd.lens import Lens

    return [Lens.equirect(W, H, rows=rows), Lens.fisheye(W, H, fov=math.radians(180.0), rows=rows), Lens.fisheye(W, H, fov=math.radians(220.0), rows=rows),
            Lens.octahedral(W, H, rows=rows), Lens.cube_face(H, 5, rows=rows)]


# ---- 1. header, symbols, tuples ----------------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_the_lens_header():
    N, lib = _lib()
    from godot_atmosphere_shader_amd import lens as L

    assert _functions("atmo_lens.h") == set(N.LENS_SYMBOLS) == NAMES and len(N.LENS_SYMBOLS) == len(NAMES)
    for sym in N.LENS_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS
    tuples = {k: v for k, v in vars(N).items() if k.endswith("_SYMBOLS") and k != "LENS_SYMBOLS"}
    assert {"CORE_SYMBOLS", "DEBUG_SYMBOLS", "RAYS_SYMBOLS", "RAY_QUADS_SYMBOLS", "RAY_ORDER_SYMBOLS", "RAY_LIST_SYMBOLS", "RAY_DETAIL_SYMBOLS",
            "EXPORTED_SYMBOLS"} <= set(tuples)
    for name, other in tuples.items():     # disjoint from every other tuple
        assert not set(N.LENS_SYMBOLS) & set(other), name
    assert N.EXPORTED_SYMBOLS == (N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_PROXY_SYMBOLS +
                                  N.VIEWS_TARGET_SYMBOLS)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5
    # the struct is the header's, field for field: 6 integers, fov, tmax, origin[3], basis[9] -- 20 words
    assert C.sizeof(N.AtmoLens) == 4 * (6 + 2 + 3 + 9) and N.AtmoLens.fov.offset == 24 and N.AtmoLens.origin.offset == 32 and N.AtmoLens.basis.offset == 44
    header = open(ROOT + "/include/atmo_lens.h").read()
    assert "ATMO_LENS_EQUIRECT = 0, ATMO_LENS_FISHEYE = 1, ATMO_LENS_OCTAHEDRAL = 2, ATMO_LENS_CUBE_FACE = 3" in header
    assert "#define ATMO_LENS_QUADS 1u" in header and N.LENS_QUADS == L.LENS_QUADS == 1
    assert (N.LENS_EQUIRECT, N.LENS_FISHEYE, N.LENS_OCTAHEDRAL, N.LENS_CUBE_FACE) == (L.EQUIRECT, L.FISHEYE, L.OCTAHEDRAL, L.CUBE_FACE) == (0, 1, 2, 3)
    for older in ("atmo.h", "atmo_debug.h"):      # the older headers keep their function sets: they do not know the new one
        assert "lens" not in open(ROOT + "/include/" + older).read()


# ---- 2. argument checks ----------------------------------------------------------------------------------------------------------------------------------------
def _lens(N, **kw):
    s = N.AtmoLens()
    s.kind, s.width, s.height, s.y0, s.y1, s.face, s.fov, s.tmax = N.LENS_EQUIRECT, W, H, 0, H, 0, 3.0, 1e30
    s.basis[0] = s.basis[4] = s.basis[8] = 1.0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_lens_rays_refuses_in_the_header_s_order():
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    nan = float("nan")
    try:
        def call(lens=None, flags=0, dist=None, pitch=0, rays=RAYS, index=None, **kw):
            s = _lens(N, **kw) if lens is None else lens
            return _said(lib, ctx, lib.atmo_lens_rays(ctx, C.byref(s) if s is not False else None, flags, dist, pitch, rays, index, None))

        refusals = [
            dict(lens=False),
            dict(kind=4), dict(kind=-1), dict(flags=2), dict(flags=0x80000001),
            dict(width=0), dict(height=0, y1=5), dict(width=-3), dict(width=2 ** 14 + 1, height=2 ** 14, y1=4), dict(width=2 ** 28, height=2, y1=2),
            dict(y0=-1), dict(y1=H + 1), dict(y0=5, y1=4), dict(y0=-2, y1=-1),
            dict(kind=N.LENS_FISHEYE, fov=0.0), dict(kind=N.LENS_FISHEYE, fov=-1.0), dict(kind=N.LENS_FISHEYE, fov=nan), dict(kind=N.LENS_FISHEYE, fov=6.2831860),
            dict(kind=N.LENS_FISHEYE, fov=float("inf")),
            dict(kind=N.LENS_CUBE_FACE), dict(kind=N.LENS_CUBE_FACE, width=H, face=6), dict(kind=N.LENS_CUBE_FACE, width=H, face=-1),
            dict(flags=1, y0=1), dict(flags=1, y1=11), dict(flags=1, y0=3, y1=H),
            dict(rays=None), dict(rays=RAYS + 8), dict(rays=RAYS + 4), dict(index=INDEX + 2), dict(index=INDEX + 1),
            dict(flags=1, index=INDEX),
            dict(dist=DIST, pitch=W - 1), dict(dist=DIST, pitch=0), dict(pitch=W), dict(pitch=1),
        ]
        for kw in refusals:
            rc, msg = call(**kw)
            assert rc == N.ATMO_E_ARG and msg.startswith(WHO), (kw, rc, msg)
        # what is fine gets as far as the device, which a host-only context lacks
        fine = [
            dict(), dict(index=INDEX), dict(dist=DIST, pitch=W), dict(dist=DIST, pitch=W + 11, index=INDEX + 4), dict(y0=2, y1=12, index=INDEX), dict(y0=3, y1=4),
            dict(flags=1), dict(flags=1, y0=2, y1=12), dict(flags=1, y0=18, y1=H), dict(width=2 ** 14, height=2 ** 14, y1=2 ** 14), dict(width=1, height=1, y1=1),
            dict(kind=N.LENS_FISHEYE, fov=6.2831855), dict(kind=N.LENS_FISHEYE, fov=1e-6), dict(kind=N.LENS_OCTAHEDRAL, face=77, fov=nan),
            dict(kind=N.LENS_CUBE_FACE, width=H, face=0), dict(kind=N.LENS_CUBE_FACE, width=H, face=5, flags=1), dict(fov=nan, face=-4),
        ]
        for kw in fine:
            rc, msg = call(**kw)
            assert rc == N.ATMO_E_NO_DEVICE and msg.startswith(WHO), (kw, rc, msg)
        # an empty band is ATMO_OK: nothing is enqueued and nothing else is looked at
        assert call(y0=7, y1=7, kind=9, width=0, rays=None, flags=6, pitch=3)[0] == N.ATMO_OK
        assert call(y0=0, y1=0, rays=RAYS + 4)[0] == N.ATMO_OK
        assert lib.atmo_lens_rays(None, C.byref(_lens(N)), 0, None, 0, RAYS, None, None) == N.ATMO_E_ARG
        # the order: the lens, the kind and the flags, the image, the band, fov and face, the quads' rows, the pointers, quads with an index, the distance
        assert "null lens" in call(lens=False, rays=None)[1]
        assert "kind" in call(kind=7, flags=2, width=0)[1]
        assert "flag" in call(flags=2, width=0)[1]
        assert "at least 1" in call(width=0, y1=H + 1)[1]
        assert "2^28" in call(width=2 ** 15, height=2 ** 14, y1=2 ** 14 + 1)[1]
        assert "band" in call(kind=N.LENS_FISHEYE, fov=0.0, y1=H + 1)[1]
        assert "fov" in call(kind=N.LENS_FISHEYE, fov=nan, flags=1, y0=1)[1]
        assert "width == height" in call(kind=N.LENS_CUBE_FACE, face=9)[1]
        assert "face" in call(kind=N.LENS_CUBE_FACE, width=H, face=9, flags=1, y0=1)[1]
        assert "ATMO_LENS_QUADS" in call(flags=1, y0=1, rays=None)[1]
        assert "null rays_dev" in call(rays=None, index=INDEX + 2, flags=1)[1]
        assert "rays_dev must be 16-byte aligned" in call(rays=RAYS + 8, index=INDEX + 2)[1]
        assert "index_dev must be 4-byte aligned" in call(index=INDEX + 2, flags=1)[1]
        assert "row-major only" in call(flags=1, index=INDEX, dist=DIST, pitch=1)[1]
        assert "below width" in call(dist=DIST, pitch=W - 1)[1]
        assert "without a distance buffer" in call(pitch=W)[1]
    finally:
        lib.atmo_destroy(ctx)


def test_lens_ray_counts():
    N, lib = _lib()
    from godot_atmosphere_shader_amd.lens import Lens

    n, m = C.c_uint32(99), C.c_uint32(99)

    def counts(flags=0, **kw):
        s = _lens(N, **kw)
        return lib.atmo_lens_ray_counts(C.byref(s), flags, C.byref(n), C.byref(m)), n.value, m.value

    # 37 x 19, rows (2, 12): 10 rows of 37; 19 quads a row in 5 quad rows; 3 tiles a row in 3 tile rows
    assert counts(y0=2, y1=12) == (N.ATMO_OK, 370, 576) and counts(1, y0=2, y1=12) == (N.ATMO_OK, 380, 576)
    assert counts() == (N.ATMO_OK, 37 * 19, 64 * 3 * 5) and counts(1) == (N.ATMO_OK, 4 * 19 * 10, 64 * 3 * 5)
    assert counts(y0=5, y1=5, kind=9) == (N.ATMO_OK, 0, 0)
    assert counts(width=16, height=4, y1=4) == (N.ATMO_OK, 64, 64) and counts(width=17, height=5, y1=5) == (N.ATMO_OK, 85, 256)
    assert counts(width=2 ** 28, height=1, y1=1) == (N.ATMO_OK, 2 ** 28, 2 ** 30) and counts(1, width=2 ** 28, height=1, y1=1) == (N.ATMO_OK, 2 ** 29, 2 ** 30)
    assert counts(width=1, height=2 ** 28, y1=2 ** 28) == (N.ATMO_OK, 2 ** 28, 2 ** 32 - 1)      # saturated: atmo_lens_rays refuses an index that long
    for kw in (dict(kind=4), dict(width=0), dict(y1=H + 1), dict(kind=N.LENS_FISHEYE, fov=7.0), dict(kind=N.LENS_CUBE_FACE), dict(flags=1, y0=1), dict(flags=4)):
        before = (n.value, m.value)
        assert counts(**kw)[0] == N.ATMO_E_ARG and (n.value, m.value) == before, kw
    assert lib.atmo_lens_ray_counts(None, 0, C.byref(n), C.byref(m)) == N.ATMO_E_ARG
    s = _lens(N)
    assert lib.atmo_lens_ray_counts(C.byref(s), 0, None, None) == N.ATMO_OK
    # lens.py counts the same, and its native() is the struct
    for lens in _lenses() + _lenses(BAND):
        for quads in (False, True):
            nl = lens.native()
            assert lib.atmo_lens_ray_counts(C.byref(nl), int(quads), C.byref(n), C.byref(m)) == N.ATMO_OK
            assert lens.counts(quads) == (n.value, m.value), (lens, quads)
    nl = Lens.cube_face(8, 3, basis=np.arange(9.0).reshape(3, 3), origin=(1, 2, 3), tmax=5.0).native()
    assert (nl.kind, nl.width, nl.height, nl.y0, nl.y1, nl.face) == (3, 8, 8, 0, 8, 3) and list(nl.origin) == [1, 2, 3] and nl.tmax == 5.0
    assert list(nl.basis) == [0, 3, 6, 1, 4, 7, 2, 5, 8]      # column-major
    for bad in (dict(rows=(3, 2)), dict(rows=(0, H + 1)), dict(fov=0.0), dict(fov=7.0)):
        with pytest.raises(ValueError):
            Lens.fisheye(W, H, **{"fov": 3.0, **bad})


# ---- 3. the cube face is the coverage cubemap's table ------------------------------------------------------------------------------------------------------------
def test_cube_face_is_the_oracle_s_texel_direction_bit_for_bit(oracle32):
    from godot_atmosphere_shader_amd.lens import Lens, lens_directions, lens_rays

    for n in (8, 5):
        for face in range(6):
            rays = lens_rays(Lens.cube_face(n, face, tmax=3.5, origin=(1.0, -2.0, 0.25)))
            want = np.array([oracle32.noise_cubemap_direction(n, face, x, y) for y in range(n) for x in range(n)], dtype=np.float32)
            x, y = np.arange(n * n) % n, np.arange(n * n) // n
            assert lens_directions(Lens.cube_face(n, face), x, y)[0].tobytes() == want.tobytes(), (n, face)      # the lens-space direction: the table's bits
            # ... and behind the identity BASIS the ray's: the same bits but for the sign of a zero component (odd N: the middle column's or row's -0), which
            # the header's three rounded products and two sums do not keep -- RN(RN(1 * -0) + RN(0 * dy)) is +0 where dy > 0
            got = rays[:, 4:7]
            assert rays.shape == (n * n, 8) and np.array_equal(got, want) and np.array_equal(got.view(np.uint32)[want != 0], want.view(np.uint32)[want != 0])
            assert (want == 0).any() == (n % 2 == 1)
            assert np.array_equal(rays[:, :4], np.tile(np.float32([1.0, -2.0, 0.25, 3.5]), (n * n, 1))) and not rays[:, 7].any()


# ---- 4. the octahedral map against the ray key ----------------------------------------------------------------------------------------------------------------------
def _deinterleave(key):
    out = np.zeros_like(key)
    for b in range(9):
        out |= ((key >> np.uint32(2 * b)) & np.uint32(1)) << np.uint32(b)
    return out


def test_octahedral_pixels_are_the_ray_key_s_cells():
    """Every pixel of a 512 x 512 map: its ray's key de-interleaves to (x, y).  A centre sits half a cell from every cell edge; the rounding is ulps."""
    from godot_atmosphere_shader_amd import ray_order as R
    from godot_atmosphere_shader_amd.lens import Lens, lens_rays

    rays = lens_rays(Lens.octahedral(512, 512))
    keys = R.ray_keys(rays)
    i = np.arange(512 * 512, dtype=np.uint32)
    assert np.array_equal(_deinterleave(keys), i % 512) and np.array_equal(_deinterleave(keys >> np.uint32(1)), i // 512)
    norm = np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1)
    assert np.abs(norm - 1.0).max() < 3e-7


# ---- 5. the inverse round trip ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_lens_inverts_to_its_pixel_centres():
    from godot_atmosphere_shader_amd.lens import FISHEYE, lens_pixel, lens_rays

    rot = _rotation()
    for lens in _lenses():
        for basis in (None, rot):
            if basis is not None:
                lens = type(lens)(lens.kind, lens.width, lens.height, face=lens.face, fov=lens.fov, basis=basis)
            rays = lens_rays(lens)
            w, h = lens.width, lens.height
            i = np.arange(w * h)
            x, y = i % w, i // w
            present = np.any(rays[:, 4:7] != 0.0, axis=1)
            if lens.kind == FISHEYE:
                absent = (2 * x + 1 - w) ** 2 + (h - 2 * y - 1) ** 2 > min(w, h) ** 2
                assert np.array_equal(~present, absent) and 0 < absent.sum() < w * h
                assert not rays[absent].any() and not np.signbit(rays[absent]).any()
                if basis is None:
                    assert rays[(h // 2) * w + w // 2, 4:7].tolist() == [0.0, 0.0, -1.0]      # rho == 0
            else:
                assert present.all()
            back = lens_pixel(lens, rays[present, 4:7])
            err = np.abs(back - np.stack([x + 0.5, y + 0.5], axis=1)[present]).max()
            assert err < 1e-3, (lens, err)


def _rotation():
    """A generic rotation, float32: about (1, 2, 3) by 0.7 radians."""
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + math.sin(0.7) * k + (1 - math.cos(0.7)) * (k @ k)).astype(np.float32)


# ---- 6. equirect known answers ------------------------------------------------------------------------------------------------------------------------------------------
def test_equirect_known_answers():
    from godot_atmosphere_shader_amd.lens import Lens, lens_rays

    d = lens_rays(Lens.equirect(4, 2))[:, 4:7]
    h, r = 0.5, math.sqrt(0.5)
    want = np.array([[-h, r, h], [-h, r, -h], [h, r, -h], [h, r, h], [-h, -r, h], [-h, -r, -h], [h, -r, -h], [h, -r, h]], dtype=np.float64)
    ulps = np.abs(d.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert ulps.max() <= 1.0, ulps
    assert np.abs(d[2].astype(np.float64) - [h, r, -h]).max() <= np.spacing(np.float32(r))      # pixel (2, 0)


# ---- 7. orders ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_quad_order_and_tile_index_against_brute_force():
    from godot_atmosphere_shader_amd.lens import LIST_END, lens_rays, lens_tile_index
    from godot_atmosphere_shader_amd.ray_quads import quad_order

    for rows in (BAND, None):
        for lens in _lenses(rows):
            w = lens.width
            y0, y1 = lens.rows
            whole = lens_rays(lens.band((0, lens.height)))
            plain = lens_rays(lens)
            assert plain.tobytes() == whole[y0 * w:y1 * w].tobytes()                  # a band is the image's rows
            # the quad order: ray_quads.quad_order of the band's rows, absent slots all-zero
            order = quad_order(w, y1 - y0)
            quads = lens_rays(lens, quads=True)
            want = np.where((order >= 0)[:, None], plain[np.maximum(order, 0)], np.float32(0.0))
            assert quads.shape == (order.shape[0], 8) and quads.tobytes() == want.tobytes(), lens
            # the tile index, entry by entry
            index = lens_tile_index(lens)
            tpr = (w + 15) // 16
            brute = []
            for t in range(tpr * ((y1 - y0 + 3) // 4)):
                for l in range(64):
                    x, y = 16 * (t % tpr) + (l & 15), y0 + 4 * (t // tpr) + (l >> 4)
                    ray = (y - y0) * w + x
                    brute.append(ray if x < w and y < y1 and plain[ray, 4:7].any() else LIST_END)
            assert index.dtype == np.uint32 and index.tolist() == brute, lens
            listed = index[index != LIST_END]
            assert np.array_equal(np.sort(listed), np.nonzero(np.any(plain[:, 4:7] != 0, axis=1))[0])      # every present ray once


def test_distance_is_every_ray_s_own_texel():
    from godot_atmosphere_shader_amd.lens import FLT_MAX, Lens, lens_pixel, lens_rays

    dist = np.arange(H * (W + 3), dtype=np.float32).reshape(H, W + 3) + 1.0
    dist[3, 15] = FLT_MAX
    lens = Lens.fisheye(W, H, rows=BAND)
    for quads in (False, True):
        rays = lens_rays(lens, quads=quads, distance=dist)
        present = np.any(rays[:, 4:7] != 0, axis=1)
        back = np.rint(lens_pixel(lens, rays[present, 4:7]) - 0.5).astype(int)
        assert np.array_equal(rays[present, 3], dist[back[:, 1], back[:, 0]]) and not rays[~present].any()
    assert lens_rays(lens, distance=dist)[(3 - 2) * W + 15, 3] == np.float32(FLT_MAX)
