"""CPU tests of the cloud shape volume generator (include/atmo_noise_volume.h): the contract as tests/noise_volume_host.py states it in float32
numpy -- its range, its exact identities, a second scalar statement, wrap continuity --, every refusal of atmo_generate_noise_volume on a host-only
context, the NoiseVolume resource without a device, and the header's symbol set.  (tests/test_noise_volume_gpu.py holds the kernels to the statement
byte for byte.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noise_volume_host as H
from godot_atmosphere_shader_amd.noise_cubemap import SeededValueNoise
from noise_host import get_noise_3dv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAMLESS = [k for k, c in H.CASES.items() if c["seamless"] and c["n"] > 1]


# ---- the statement -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(H.CASES))
def test_t_is_a_non_negative_float_and_the_bytes_span_the_range(name):
    """t in [+0, 1], no sign bit, no NaN: what makes unsigned min / max atomics on the float's bits legitimate.  Normalised volumes hold both 0 and 255
    (n > 1); n = 1 takes the mx == mn branch and keeps its byte; invert is 255 - b."""
    c = H.CASES[name]
    t = H.case_t(name)
    assert t.dtype == np.float32 and t.shape == (c["n"],) * 3
    assert not (t.view(np.uint32) >> 31).any() and not np.isnan(t).any() and t.min() >= 0.0 and t.max() <= 1.0
    b = H.case_volume(name, normalize=True)
    if c["n"] > 1:
        assert b.min() == 0 and b.max() == 255
        assert np.array_equal(np.sort(t.ravel()).view(np.uint32), np.sort(t.ravel().view(np.uint32)))   # unsigned bit order == float order
    else:
        assert b.tolist() == [[[147]]] and np.array_equal(b, H.case_volume(name, normalize=False))
    for norm in (True, False):
        assert np.array_equal(H.case_volume(name, norm, invert=True), 255 - H.case_volume(name, norm))


def test_base_period_rounds_half_to_even():
    assert [H.base_period(n, f) for n, f in ((1, 0.1), (5, 0.3), (16, 0.25), (24, 0.125), (64, 0.1))] == [1, 2, 4, 3, 6]
    assert float(np.float32(5) * np.float32(0.3)) == 1.5                      # the n = 5 case: the fp32 product is the tie itself, rintf gives 2
    assert H.base_period(4, 0.625) == 2 and H.base_period(4, 0.875) == 4      # 2.5 -> 2, 3.5 -> 4: the ties themselves go to even


def test_not_seamless_is_get_noise_3dv_at_the_integer_coordinates():
    c = H.CASES["n33"]
    nz = H.case_noise(c)
    n = c["n"]
    rng = np.random.default_rng(33)
    xyz = rng.integers(0, n, size=(500, 3))
    p = (xyz.astype(np.float32) + np.asarray(c["offset"], dtype=np.float32)).astype(np.float32)
    want = np.float32(0.5) + np.float32(0.5) * get_noise_3dv(nz, p)
    got = H.case_t("n33")[xyz[:, 2], xyz[:, 1], xyz[:, 0]]
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    # and without an offset the volume is the noise at (x, y, z) itself
    t0 = H.volume_t(8, nz, (0.0, 0.0, 0.0), False)
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    v = get_noise_3dv(nz, np.stack([x, y, z], axis=-1).astype(np.float32))
    assert np.array_equal(t0, np.float32(0.5) + np.float32(0.5) * v)


def test_the_two_exact_identities_of_the_power_of_two_case():
    """n = 16, frequency 0.25 (P_0 = 4): an offset of whole periods reproduces the bytes; an offset of whole texels rotates them."""
    c = H.CASES["n16"]
    nz = H.case_noise(c)
    assert H.base_period(16, c["frequency"]) == 4
    base = H.case_volume("n16")
    assert np.array_equal(H.generate_volume_host(16, nz, (16.0, -32.0, 48.0), True), base)
    rolled = H.generate_volume_host(16, nz, (3.0, 0.0, -5.0), True)
    assert np.array_equal(rolled, np.roll(np.roll(base, -3, axis=2), 5, axis=0)) and not np.array_equal(rolled, base)


@pytest.mark.parametrize("name", list(H.CASES))
def test_the_scalar_statement_agrees_bit_for_bit(name):
    """One texel at a time, every operation rounded through np.float32, written separately: t's bits and all four byte forms on <= 200 sample texels."""
    c = H.CASES[name]
    n, nz, t = c["n"], H.case_noise(c), H.case_t(name)
    rng = np.random.default_rng(n)
    samples = {(0, 0, 0), (n - 1, n - 1, n - 1), (n - 1, 0, n // 2)} | {tuple(int(v) for v in rng.integers(0, n, 3)) for _ in range(197)}
    mn, mx = t.min(), t.max()
    for (x, y, z) in samples:
        s = H.texel_t_scalar(n, nz, c["offset"], c["seamless"], x, y, z)
        assert s.dtype == np.float32 and s.view(np.uint32) == t[z, y, x].view(np.uint32), (x, y, z)
        for norm in (True, False):
            for inv in (True, False):
                assert H.texel_byte_scalar(s, mn, mx, norm, inv) == H.case_volume(name, norm, inv)[z, y, x], (x, y, z, norm, inv)


def _steps(u):
    """(largest step across the wrap, largest step between interior neighbours) of the bytes, over the three axes."""
    u = u.astype(np.int32)
    wrap = max(int(np.abs(u.take(-1, axis=a) - u.take(0, axis=a)).max()) for a in range(3))
    inner = max(int(np.abs(np.diff(u, axis=a)).max()) for a in range(3))
    return wrap, inner


def test_seamless_volumes_wrap_continuously_and_the_plain_one_does_not():
    """Un-normalised bytes: texel n - 1 and texel 0 differ no more than interior neighbours do.  The figures are the statement's own."""
    got = {k: _steps(H.case_volume(k, normalize=False)) for k in SEAMLESS + ["n33"]}
    for k in SEAMLESS:
        assert got[k][0] <= got[k][1], (k, got[k])
    assert got["n33"][0] > got["n33"][1]          # the non-seamless case: the check discriminates
    assert got == {"n5": (86, 96), "n16": (66, 97), "n24": (48, 54), "n64": (30, 45), "n33": (159, 52)}


# ---- the header, the binding, the refusals ---------------------------------------------------------------------------------------------------------

def _functions(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(atmo_[a-z0-9_]+)\s*\(", header))


def test_binding_exposes_the_noise_volume_header():
    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.build import build_native

    build_native()
    lib = N.load()
    assert _functions("atmo_noise_volume.h") == set(N.NOISE_VOLUME_SYMBOLS) == {"atmo_generate_noise_volume"}
    for sym in N.NOISE_VOLUME_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS
    # a tuple of its own beside EXPORTED_SYMBOLS, which stays the union of the seven older headers' tuples; the feature is detected by symbol
    assert N.EXPORTED_SYMBOLS == (N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_PROXY_SYMBOLS +
                                  N.VIEWS_TARGET_SYMBOLS)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5
    # the struct is the header's: 2 + 1 + 1 + 1 + 3 + 3 words
    assert C.sizeof(N.AtmoNoiseVolume) == 44 and N.AtmoNoiseVolume.offset.offset == 20 and N.AtmoNoiseVolume.seamless.offset == 32
    for name in os.listdir(os.path.join(ROOT, "include")):       # the older headers do not know the new one
        if name != "atmo_noise_volume.h":
            assert "noise_volume" not in open(os.path.join(ROOT, "include", name)).read(), name


@pytest.fixture()
def host_ctx():
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = C.c_void_p()
    assert lib.atmo_debug_create_host_only(N.VARIANT_CLOUDS_HIGH, 8, 8, N.LIGHT_LUT, 0, C.byref(ctx)) == N.ATMO_OK
    yield lib, ctx
    assert lib.atmo_destroy(ctx) == N.ATMO_OK


def _desc(**kw):
    from godot_atmosphere_shader_amd import _native as N

    d = dict(size=16, seed=7, frequency=0.25, octaves=3, gain=0.6, offset=(0.0, 0.0, 0.0), seamless=1, invert=0, normalize=1)
    d.update(kw)
    return N.AtmoNoiseVolume(d["size"], d["seed"], d["frequency"], d["octaves"], d["gain"], (C.c_float * 3)(*d["offset"]), d["seamless"], d["invert"],
                             d["normalize"])


INF, NAN = float("inf"), float("nan")
REFUSALS = [
    (dict(size=0), "size"), (dict(size=513), "size"), (dict(size=-4), "size"),
    (dict(octaves=0), "octaves"), (dict(octaves=17), "octaves"),
    (dict(frequency=0.0), "frequency"), (dict(frequency=-0.25), "frequency"), (dict(frequency=INF), "frequency"), (dict(frequency=NAN), "frequency"),
    (dict(gain=0.0), "gain"), (dict(gain=-0.5), "gain"), (dict(gain=INF), "gain"), (dict(gain=NAN), "gain"),
    (dict(offset=(NAN, 0.0, 0.0)), "offset[0]"), (dict(offset=(0.0, -INF, 0.0)), "offset[1]"), (dict(offset=(0.0, 0.0, INF)), "offset[2]"),
    # seamless: P_0 << (octaves - 1) above 2^24 -- 512 * 64 = 2^15 cells, << 10 = 2^25
    (dict(size=512, frequency=64.0, octaves=11), "frequency"),
    (dict(size=512, frequency=1.0e30, octaves=1), "frequency"),
    # (n + max |offset|) * freq_last reaches 2^30: seamless (freq_last = 4 * 4 / 16 = 1) and not (0.25 * 4 = 1)
    (dict(offset=(0.0, -float(2 ** 30), 0.0)), "offset"), (dict(offset=(float(2 ** 30), 0.0, 0.0), seamless=0), "offset"),
    (dict(size=512, frequency=3.0e6, octaves=1, seamless=0), "offset"),
]


def test_every_refusal_its_code_and_the_field_it_names(host_ctx):
    """All before the device is touched: a host-only context gives the same answers.  Then the accepted neighbours of the bounds get past the
    argument checks (a host-only context has no device: ATMO_E_NO_DEVICE, not ATMO_E_ARG)."""
    from godot_atmosphere_shader_amd import _native as N

    lib, ctx = host_ctx
    assert lib.atmo_generate_noise_volume(None, C.byref(_desc()), 0, None, None) == N.ATMO_E_ARG
    assert lib.atmo_generate_noise_volume(ctx, None, 1, None, None) == N.ATMO_E_ARG
    assert b"atmo_generate_noise_volume" in lib.atmo_last_error_string(ctx) and b"v is null" in lib.atmo_last_error_string(ctx)
    for kw, field in REFUSALS:
        for bind in (0, 1):
            assert lib.atmo_generate_noise_volume(ctx, C.byref(_desc(**kw)), bind, None, None) == N.ATMO_E_ARG, kw
            msg = lib.atmo_last_error_string(ctx).decode()
            assert msg.startswith("atmo_generate_noise_volume: " + field), (kw, msg)
    accepted = [dict(), dict(size=1), dict(size=512, frequency=64.0, octaves=10), dict(octaves=16, seamless=0, frequency=0.001),
                dict(offset=(0.0, float(2 ** 29), 0.0)), dict(size=5, frequency=0.3, octaves=2, offset=(-7.25, 3.5, 100.0))]
    for kw in accepted:
        assert lib.atmo_generate_noise_volume(ctx, C.byref(_desc(**kw)), 1, None, None) == N.ATMO_E_NO_DEVICE, kw
        assert b"host-only" in lib.atmo_last_error_string(ctx)
    w = C.c_int(-1)
    assert lib.atmo_get_texture_size(ctx, b"u_cloud_shape_texture", C.byref(w), None, None, None) == N.ATMO_OK and w.value == 0   # nothing bound


# ---- the resource ------------------------------------------------------------------------------------------------------------------------------

def test_resource_properties_and_deferred_update():
    """NoiseTexture3D's surface: defaults as Godot's, an update requested on every property / noise change and coalesced, the cubic rule."""
    from godot_atmosphere_shader_amd import NoiseVolume

    calls = []

    class Stub(NoiseVolume):
        def _generate(self, desc):
            calls.append((desc.size, desc.seed, tuple(desc.offset), desc.seamless, desc.invert, desc.normalize))
            return np.zeros((desc.size,) * 3, dtype=np.uint8)

    nv = Stub()
    assert (nv.width, nv.height, nv.depth, nv.size) == (64, 64, 64, 64)
    assert (nv.seamless, nv.invert, nv.normalize, nv.offset) == (False, False, True, (0.0, 0.0, 0.0))
    assert isinstance(nv.noise, SeededValueNoise)
    changed = []
    nv.connect_changed(lambda: changed.append(1))
    assert calls == []                      # deferred: nothing generated yet
    nv.size = 16
    assert (nv.width, nv.height, nv.depth) == (16, 16, 16)
    nv.seamless = True
    nv.offset = (1, 2.5, -3)
    nv.noise.seed = 42                      # Noise.changed -> _request_update
    nv.process_deferred()
    assert calls == [(16, 42, (1.0, 2.5, -3.0), 1, 0, 1)] and changed == [1]      # several requests, one update
    nv.process_deferred()
    nv.seamless = True                      # no change, no request
    nv.process_deferred()
    assert len(calls) == 1
    nv.noise = SeededValueNoise(seed=3, frequency=0.1)
    assert nv.get_data().shape == (16, 16, 16) and len(calls) == 2 and calls[1][1] == 3      # access runs the pending update
    nv.invert, nv.normalize = True, False
    assert nv.get_data() is not None and calls[2][3:] == (1, 1, 0)
    # the shape texture is cubic: one side changed alone is held until it is used, and then refused with the reason
    nv.width = 32
    with pytest.raises(ValueError, match="cubic"):
        nv.get_data()
    with pytest.raises(ValueError, match="32 x 16 x 16"):
        nv.size
    nv.height = nv.depth = 32
    assert nv.get_data().shape == (32, 32, 32) and len(calls) == 4
    with pytest.raises(ValueError):
        nv.offset = (1.0, 2.0)
    assert Stub(size=8, width=99).size == 8 and Stub(width=4, height=4, depth=4).size == 4
    with pytest.raises(ValueError, match="cubic"):
        Stub(width=8).get_data()


def test_node_takes_a_noise_volume_only_for_the_shape_texture():
    """planet_atmosphere._upload_texture: a value with bind_to goes down the device path of u_cloud_shape_texture; arrays and None as before."""
    from godot_atmosphere_shader_amd.planet_atmosphere import PlanetAtmosphere

    bound = []

    class Resource:
        def bind_to(self, node, stream=None):
            bound.append((node, stream))

    class Node:   # the method under test, without a device
        _upload_texture = PlanetAtmosphere._upload_texture

    node = Node()
    node._upload_texture("u_cloud_shape_texture", Resource())
    assert bound == [(node, None)]
    with pytest.raises(ValueError, match="u_cloud_coverage_cubemap does not take a NoiseVolume"):
        node._upload_texture("u_cloud_coverage_cubemap", Resource())
