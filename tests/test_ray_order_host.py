"""CPU tests of the coherent-ray-queue header (include/atmo_ray_order.h): the header's symbol set and the binding, THE KEY in numpy
(godot_atmosphere_shader_amd/ray_order.py) on hand-written directions whose cells are spelled out here and on a million seeded ones, the scratch size, every
refusal of the four device entry points on host-only contexts in the header's order (nothing touches a device), and the seven indexed kernels in the
compiled assembly (one compile, shared with tests/test_kernel_twins_host.py).  (tests/test_ray_order_gpu.py holds the kernels to the numpy statement and
the indexed shading to atmo_shade_rays, bit for bit.)"""
import ctypes as C

import numpy as np

import test_kernel_twins_host as T
from test_rays_host import RAYS, RGBA, _mode_cases, _mode_ctx, _said
from test_views_proxy_host import FAR, _frame, _functions, _host_ctx

INDEX, KEYS, SCRATCH = 0x40000, 0x50000, 0x60000   # addresses no refusal dereferences
WHO = "atmo_shade_rays_indexed: "
BAD_KEY = 2 ** 18 - 1
NAMES = {"atmo_ray_order_scratch_bytes", "atmo_ray_order", "atmo_shade_rays_indexed", "atmo_debug_ray_keys", "atmo_debug_sort_ray_keys"}

# (direction, (qu, qv), key): the cell is worked out by hand from the header's items -- u = dx / s, v = dy / s, the fold where dz's sign bit is set,
# q = floor(t * 256 + 256) clamped to 0 .. 511 -- and the key is the cell's bits interleaved, qu's on the even positions.
HAND = [
    # the six axes: u or v = +-1 exactly (512 clamps to 511); -z folds the centre (0, 0) out to the corner (1, 1)
    ((1, 0, 0), (511, 256), 218453), ((-1, 0, 0), (0, 256), 131072), ((0, 1, 0), (256, 511), 240298), ((0, -1, 0), (256, 0), 65536),
    ((0, 0, 1), (256, 256), 196608), ((0, 0, -1), (511, 511), 262143),
    # the eight octant centres: |u| = |v| = RN(1/3) -> 341 / 170 above, folded to RN(1 - RN(1/3)) = 0.6666666 -> 426 / 85 below
    ((1, 1, 1), (341, 341), 209715), ((-1, 1, 1), (170, 341), 157286), ((1, -1, 1), (341, 170), 104857), ((-1, -1, 1), (170, 170), 52428),
    ((1, 1, -1), (426, 426), 249036), ((-1, 1, -1), (85, 426), 170393), ((1, -1, -1), (426, 85), 91750), ((-1, -1, -1), (85, 85), 13107),
    # a direction on each fold line |u| + |v| = 1, dz = +0 and dz = -0: the fold maps the line onto itself
    ((0.5, 0.5, 0.0), (384, 384), 245760), ((-0.5, 0.5, 0.0), (128, 384), 180224), ((-0.5, -0.5, -0.0), (128, 128), 49152),
    ((0.5, -0.5, -0.0), (384, 128), 114688), ((-0.25, 0.75, -0.0), (192, 448), 192512), ((-0.25, 0.75, 0.0), (192, 448), 192512),
    # dz = -0.0 against +0.0: the sign bit folds, u' = 1 - RN(1/3) = 0.6666666 and u = RN(2/3) land in the same cell
    ((0.5, 0.25, 0.0), (426, 341), 222822), ((0.5, 0.25, -0.0), (426, 341), 222822), ((1, 0, -0.0), (511, 256), 218453),
    # denormal directions: the quotients are the IEEE ones (u = 1; v = -0.5 exactly)
    ((1e-40, 0, 0), (511, 256), 218453), ((0, -1e-42, 1e-42), (256, 128), 98304),
    # a non-unit direction and its unit form: u = 3/19, v = 4/19 -> 40.4 + 256, 53.9 + 256
    ((3, 4, 12), (296, 309), 200290), ((3 / 13, 4 / 13, 12 / 13), (296, 309), 200290),
    # zero, NaN, infinite and overflowing directions
    ((0, 0, 0), None, BAD_KEY), ((-0.0, -0.0, -0.0), None, BAD_KEY), ((float("nan"), 1, 0), None, BAD_KEY), ((0, 1, float("nan")), None, BAD_KEY),
    ((float("inf"), 0, 0), None, BAD_KEY), ((0, 0, -float("inf")), None, BAD_KEY), ((3e38, 3e38, 0), None, BAD_KEY),
]


def hand_directions():
    return np.array([d for d, _, _ in HAND], dtype=np.float32)


def seeded_directions(n, seed=20261020):
    """Uniform on the sphere, float32, normalised in double (the key does not care)."""
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, N.load()


def _interleave(qu, qv):
    return sum(((qu >> b) & 1) << (2 * b) | ((qv >> b) & 1) << (2 * b + 1) for b in range(9))


def test_binding_exposes_the_ray_order_header():
    N, lib = _lib()
    from godot_atmosphere_shader_amd import ray_order as R

    assert _functions("atmo_ray_order.h") == set(N.RAY_ORDER_SYMBOLS) == NAMES and len(N.RAY_ORDER_SYMBOLS) == len(NAMES)
    for sym in N.RAY_ORDER_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS
    tuples = {k: v for k, v in vars(N).items() if k.endswith("_SYMBOLS") and k != "RAY_ORDER_SYMBOLS"}
    assert {"CORE_SYMBOLS", "DEBUG_SYMBOLS", "RAYS_SYMBOLS", "RAY_QUADS_SYMBOLS", "EXPORTED_SYMBOLS"} <= set(tuples)
    for name, other in tuples.items():     # disjoint from every other tuple
        assert not set(N.RAY_ORDER_SYMBOLS) & set(other), name
    assert N.EXPORTED_SYMBOLS == (N.CORE_SYMBOLS + N.DEBUG_SYMBOLS + N.SCENE_SYMBOLS + N.TARGET_SYMBOLS + N.VIEWS_SYMBOLS + N.VIEWS_PROXY_SYMBOLS +
                                  N.VIEWS_TARGET_SYMBOLS)
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5
    header = open(T.ROOT + "/include/atmo_ray_order.h").read()
    assert "#define ATMO_RAY_KEY_BITS 18 " in header and R.KEY_BITS == N.RAY_KEY_BITS == 18


def test_keys_of_hand_written_directions():
    from godot_atmosphere_shader_amd import ray_order as R

    for _, cell, key in HAND:     # the table itself: a key is its cell's bits interleaved
        assert cell is None or _interleave(*cell) == key, (cell, key)
    got = R.ray_keys(hand_directions())
    assert got.dtype == np.uint32
    for (d, cell, key), g in zip(HAND, got.tolist()):
        assert g == key, (d, cell, key, g)
    # AtmoRay rows give what their directions give; origin, tmax and the reserved float take no part
    rows = np.full((len(HAND), 8), 7.5, dtype=np.float32)
    rows[:, 4:7] = hand_directions()
    assert np.array_equal(R.ray_keys(rows), got)
    assert np.array_equal(R.ray_order(rows), np.argsort(got, kind="stable"))
    assert R.ray_keys(np.zeros((0, 8), dtype=np.float32)).shape == (0,)


def test_rays_of_one_key_are_less_than_a_degree_apart():
    """1e6 seeded uniform directions: every key below 2^18, and two directions of equal key less than 1.0 degree apart (the cell's diagonal 2 sqrt(2) / 512
    times the map's stretch of at most 3 bounds it by 0.95; every pair inside every cell is looked at)."""
    from godot_atmosphere_shader_amd import ray_order as R

    d = seeded_directions(1_000_000)
    keys = R.ray_keys(d)
    assert int(keys.max()) < 2 ** 18
    order = np.argsort(keys, kind="stable")
    k, p = keys[order], d[order].astype(np.float64)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    worst, pairs, step = 0.0, 0, 1
    while True:
        same = np.nonzero(k[step:] == k[:-step])[0]
        if same.size == 0:
            break
        worst = max(worst, float(np.linalg.norm(p[same] - p[same + step], axis=1).max()))   # the chord: monotone in the angle
        pairs += same.size
        step += 1
    angle = np.degrees(2.0 * np.arcsin(worst / 2.0))
    print(f"{pairs} pairs of equal key in {np.unique(k).size} cells, the widest {angle:.4f} degrees apart")
    assert pairs > 1_000_000 and angle < 1.0, (pairs, angle)


def test_scratch_bytes():
    N, lib = _lib()
    b = C.c_size_t(12345)
    assert lib.atmo_ray_order_scratch_bytes(0, C.byref(b)) == N.ATMO_OK and b.value < 2 ** 20
    last = b.value
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 7571, 2 ** 20, 2 ** 20 + 1, 2_073_600, 2 ** 28 - 1, 2 ** 28):
        assert lib.atmo_ray_order_scratch_bytes(n, C.byref(b)) == N.ATMO_OK
        assert b.value >= last and b.value >= 8 * n and b.value % 16 == 0, (n, b.value, last)      # monotone; at least one buffer of pairs
        last = b.value
    assert lib.atmo_ray_order_scratch_bytes(2 ** 28 + 1, C.byref(b)) == N.ATMO_E_ARG and b.value == last
    assert lib.atmo_ray_order_scratch_bytes(2 ** 32 - 1, C.byref(b)) == N.ATMO_E_ARG
    assert lib.atmo_ray_order_scratch_bytes(5, None) == N.ATMO_E_ARG


def _need(lib, n):
    b = C.c_size_t()
    assert lib.atmo_ray_order_scratch_bytes(n, C.byref(b)) == 0
    return b.value


def test_the_order_s_entry_points_refuse_in_the_header_s_order():
    """atmo_ray_order, atmo_debug_ray_keys, atmo_debug_sort_ray_keys on a host-only context: the count, null pointers, alignment, the scratch size, each
    message under the entry point's name, and ATMO_E_NO_DEVICE behind all of them."""
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    n = 5000
    need = _need(lib, n)
    try:
        def caller(fn, **defaults):     # the entry point with its arguments by name, in the header's order, `stream` last
            return lambda **kw: _said(lib, ctx, fn(ctx, *{**defaults, **kw}.values(), None))

        order = caller(lib.atmo_ray_order, rays=RAYS, n=n, index=INDEX, scratch=SCRATCH, bytes=need)
        keys = caller(lib.atmo_debug_ray_keys, rays=RAYS, n=n, keys=KEYS)
        sort = caller(lib.atmo_debug_sort_ray_keys, keys=KEYS, n=n, index=INDEX, scratch=SCRATCH, bytes=need)
        table = [
            (order, "atmo_ray_order: ", [dict(n=2 ** 28 + 1), dict(rays=None), dict(index=None), dict(scratch=None), dict(rays=RAYS + 8), dict(rays=RAYS + 4),
                                         dict(index=INDEX + 2), dict(scratch=SCRATCH + 8), dict(bytes=need - 1), dict(bytes=0)]),
            (keys, "atmo_debug_ray_keys: ", [dict(n=2 ** 28 + 1), dict(rays=None), dict(keys=None), dict(rays=RAYS + 8), dict(keys=KEYS + 1)]),
            (sort, "atmo_debug_sort_ray_keys: ", [dict(n=2 ** 28 + 1), dict(keys=None), dict(index=None), dict(scratch=None), dict(keys=KEYS + 2),
                                                  dict(index=INDEX + 1), dict(scratch=SCRATCH + 4), dict(bytes=need - 1)]),
        ]
        for call, who, cases in table:
            for kw in cases:
                rc, msg = call(**kw)
                assert rc == N.ATMO_E_ARG and msg.startswith(who), (who, kw, rc, msg)
            rc, msg = call()
            assert rc == N.ATMO_E_NO_DEVICE and msg.startswith(who), (who, rc, msg)
            rc, msg = call(bytes=need + 4096) if call is not keys else call(keys=KEYS + 4)     # more scratch than needed, a 4-byte aligned key array: fine
            assert rc == N.ATMO_E_NO_DEVICE, (who, rc, msg)
        # the order of the checks: the count in front of null pointers, those in front of alignment, alignment in front of the scratch size
        assert "2^28" in order(n=2 ** 28 + 1, rays=None)[1] and "2^28" in sort(n=2 ** 28 + 1, keys=None)[1] and "2^28" in keys(n=2 ** 28 + 1, keys=None)[1]
        assert "null index_dev" in order(index=None, rays=RAYS + 8, bytes=0)[1]
        assert "null scratch_dev" in sort(scratch=None, keys=KEYS + 2, bytes=0)[1]
        assert "rays_dev must be 16-byte aligned" in order(rays=RAYS + 8, bytes=0)[1]
        assert "index_dev must be 4-byte aligned" in order(index=INDEX + 2, scratch=SCRATCH + 8, bytes=0)[1]
        assert "scratch_dev must be 16-byte aligned" in order(scratch=SCRATCH + 8, bytes=0)[1]
        assert "atmo_ray_order_scratch_bytes" in order(bytes=need - 1)[1]
        # nothing to do is ATMO_OK with nothing else looked at; no context is ATMO_E_ARG
        assert lib.atmo_ray_order(ctx, None, 0, None, None, 0, None) == N.ATMO_OK
        assert lib.atmo_debug_ray_keys(ctx, None, 0, None, None) == N.ATMO_OK
        assert lib.atmo_debug_sort_ray_keys(ctx, None, 0, None, None, 0, None) == N.ATMO_OK
        assert lib.atmo_ray_order(None, RAYS, n, INDEX, SCRATCH, need, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_ray_keys(None, RAYS, n, KEYS, None) == N.ATMO_E_ARG
        assert lib.atmo_debug_sort_ray_keys(None, KEYS, n, INDEX, SCRATCH, need, None) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)


def _shade(lib, ctx, frame=True, rays=RAYS, rgba=RGBA, n=64, width=8, first=0, index=INDEX, n_index=64):
    f = _frame(FAR)
    return _said(lib, ctx, lib.atmo_shade_rays_indexed(ctx, C.byref(f) if frame else None, rays, rgba, n, width, first, index, n_index, None))


def test_indexed_shading_refuses_as_atmo_shade_rays_does():
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    try:
        assert lib.atmo_set_precision(ctx, 0) == N.ATMO_OK   # the first mode refusal stands behind every argument check
        # nothing to shade: ATMO_OK with nothing else looked at
        assert lib.atmo_shade_rays_indexed(ctx, None, None, None, 0, 0, 0, None, 5, None) == N.ATMO_OK
        assert lib.atmo_shade_rays_indexed(ctx, None, None, None, 5, 0, 0, None, 0, None) == N.ATMO_OK
        assert _shade(lib, ctx, n=0, width=0, rays=RAYS + 4)[0] == N.ATMO_OK and _shade(lib, ctx, n_index=0, width=0, index=INDEX + 1)[0] == N.ATMO_OK
        assert lib.atmo_shade_rays_indexed(None, None, None, None, 0, 0, 0, None, 0, None) == N.ATMO_E_ARG
        for kw in (dict(frame=False), dict(rays=None), dict(rgba=None), dict(rays=RAYS + 4), dict(rays=RAYS + 8), dict(rgba=RGBA + 4), dict(index=None),
                   dict(index=INDEX + 1), dict(index=INDEX + 2), dict(width=0), dict(first=2 ** 32 - 63), dict(first=2 ** 32 - 1, n=2), dict(first=2, n=2 ** 32 - 1)):
            rc, msg = _shade(lib, ctx, **kw)
            assert rc == N.ATMO_E_ARG and msg.startswith(WHO), (kw, rc, msg)
        # the largest batch and list get as far as the mode; a list longer than the batch is fine (duplicates)
        for kw in (dict(first=2 ** 32 - 64), dict(first=0, n=2 ** 32 - 1), dict(n_index=2 ** 32 - 1), dict(n=1, n_index=4096), dict(index=INDEX + 4)):
            rc, msg = _shade(lib, ctx, **kw)
            assert rc == N.ATMO_E_STATE and msg.startswith(WHO) and "atmo_set_precision 0" in msg, (kw, rc, msg)
        # atmo_shade_rays' order, the list's two checks behind the other pointers' and in front of width
        assert "null frame" in _shade(lib, ctx, rays=None, index=None, width=0)[1]
        assert "16-byte aligned" in _shade(lib, ctx, rays=RAYS + 4, index=None, width=0)[1]
        assert "null index_dev" in _shade(lib, ctx, index=None, width=0, first=2 ** 32 - 1)[1]
        assert "index_dev must be 4-byte aligned" in _shade(lib, ctx, index=INDEX + 2, width=0)[1]
        assert "width" in _shade(lib, ctx, width=0, first=2 ** 32 - 1)[1]
        assert "2^32" in _shade(lib, ctx, first=2 ** 32 - 1)[1]
    finally:
        lib.atmo_destroy(ctx)


def test_indexed_shading_has_atmo_shade_rays_mode_table():
    """tests/test_rays_host.py's table of modes, each context with one thing wrong: the same refusal, under this entry point's name -- and word for word
    atmo_shade_rays' message behind the name."""
    N, lib = _lib()
    for needle, variant, kw in _mode_cases(N):
        ctx = _mode_ctx(N, lib, variant, **kw)
        try:
            rc, msg = _shade(lib, ctx)
            assert rc == N.ATMO_E_STATE and msg.startswith(WHO) and needle in msg, (needle, kw, rc, msg)
            f = _frame(FAR)
            plain = _said(lib, ctx, lib.atmo_shade_rays(ctx, C.byref(f), RAYS, RGBA, 64, 8, 0, None))
            assert plain == (rc, "atmo_shade_rays: " + msg[len(WHO):]), (plain, msg)
        finally:
            lib.atmo_destroy(ctx)
    # behind the modes the textures' check, and behind every check the device
    ctx = _mode_ctx(N, lib, N.VARIANT_CLOUDS_HIGH, sampler=1)
    try:
        rc, msg = _shade(lib, ctx)
        assert rc == N.ATMO_E_STATE and msg.startswith(WHO) and "u_optical_depth_texture not set" in msg, (rc, msg)
    finally:
        lib.atmo_destroy(ctx)
    ctx = _mode_ctx(N, lib, N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)   # needs no texture: a well-formed call gets as far as the device
    try:
        rc, msg = _shade(lib, ctx)
        assert rc == N.ATMO_E_NO_DEVICE and msg.startswith(WHO), (rc, msg)
        assert _shade(lib, ctx, index=None)[0] == N.ATMO_E_ARG
        assert lib.atmo_set_lane_split(ctx, 2) == N.ATMO_OK
        assert _shade(lib, ctx)[0] == N.ATMO_E_STATE
    finally:
        lib.atmo_destroy(ctx)


# ---- the binding, without a device -----------------------------------------------------------------------------------------------------------------------------
def test_shade_rays_with_an_index_reaches_the_indexed_entry_point():
    import pytest
    import torch

    import test_binding_calls_host as B
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    names = ("ctx", "frame", "rays", "rgba", "n", "width", "first", "index", "n_index", "stream")
    node, cam = B._node(), B._cam()
    rays, out, index = B._fake((70, 8)), B._fake((70, 4)), B._fake((33,), torch.int32)
    assert node.shade_rays(rays, cam, width=10, first=30, out=out, stream=B._Stream(), time=B.TIME, index=index) is out
    (name, args), = [c for c in node._lib.calls if c[0] != "atmo_destroy"]
    assert name == "atmo_shade_rays_indexed"
    assert dict(zip(names, args)) == dict(ctx=B.CTX, frame=bytes(PA._to_native_frame(node.make_frame(cam, B.TIME))), rays=rays.data_ptr(), rgba=out.data_ptr(),
                                          n=70, width=10, first=30, index=index.data_ptr(), n_index=33, stream=B.STREAM)
    # with an index and no `out`, `out` is created with zeros: rows the list does not name read as a discarded ray's
    node = B._node()
    seen = []

    class Watch(B._AllocateAsCuda):
        def __torch_function__(self, func, types, args=(), kwargs=None):
            if func in (torch.empty, torch.zeros):
                seen.append(func)
            return super().__torch_function__(func, types, args, kwargs)

    with Watch():
        made = node.shade_rays(rays, stream=B.STREAM, index=index)
    assert seen == [torch.zeros] and tuple(made.shape) == (70, 4) and made.dtype == torch.float32
    for bad in (torch.zeros((5,), dtype=torch.int32), B._fake((5,), torch.int64), B._fake((10,), torch.int32)[::2], [0, 1], np.arange(4, dtype=np.int32)):
        with pytest.raises(TypeError, match="index must be a contiguous CUDA int32 tensor"):
            node.shade_rays(rays, cam, out=out, stream=B.STREAM, index=bad)
    with pytest.raises(ValueError, match=r"index must have shape \(m,\)"):
        node.shade_rays(rays, cam, out=out, stream=B.STREAM, index=B._fake((5, 1), torch.int32))

    node = B._node(lib=B.library_without("atmo_shade_rays_indexed", "atmo_ray_order", "atmo_ray_order_scratch_bytes"))
    with pytest.raises(RuntimeError, match=r"atmo_shade_rays_indexed \(include/atmo_ray_order.h\)"):
        node.shade_rays(rays, cam, out=out, stream=B.STREAM, index=index)
    with pytest.raises(RuntimeError, match=r"atmo_ray_order \(include/atmo_ray_order.h\)"), B._AllocateAsCuda():
        node.ray_order(rays, stream=B.STREAM)
    assert node.shade_rays(rays, cam, out=out, stream=B.STREAM) is out        # the plain call of such a library still serves


# ---- the seven kernels in the compiled assembly ----------------------------------------------------------------------------------------------------------------
# atmo_shade_rays_indexed_kernel<FLAGS | 16384 | 32768, LSTEPS> beside atmo_shade_rays_kernel<FLAGS | 16384, LSTEPS>: one per family of rays_family_supported
KERNELS = {(0, 0): "lut", (4, 8): "direct x8", (4, 0): "direct", (17, 0): "clouds_high", (19, 0): "clouds_high_rm", (24, 0): "v1_no_clouds", (25, 0): "v1_clouds"}


def _mangled(kernel, flags, lsteps):
    return f"_ZN4atmo{len(kernel)}{kernel}ILi{flags}ELi{lsteps}EE"


def test_the_indexed_kernels_cost_what_their_twins_cost():
    """Present under their mangled names, no stack frame, a VGPR count on the occupancy step of the atmo_shade_rays_kernel twin or a better one, and as many
    vector loads inside loops (the index entry is loaded once, in front of everything)."""
    text = T._asm()
    numbers = T.twin_resources.kernels(text)
    by_prefix = lambda p: [k for name, k in numbers.items() if name.startswith(p)]   # noqa: E731  (the mangled name, then the argument types)
    waves = T.twin_resources.vgpr_waves
    assert len([n for n in numbers if "atmo_shade_rays_indexed_kernel" in n]) == len(KERNELS)
    for (flags, lsteps), label in KERNELS.items():
        (new,), (twin,) = (by_prefix(_mangled("atmo_shade_rays_indexed_kernel", flags | 16384 | 32768, lsteps)),
                           by_prefix(_mangled("atmo_shade_rays_kernel", flags | 16384, lsteps)))
        print(f"{label}: atmo_shade_rays_indexed_kernel<{flags | 49152}, {lsteps}> {new}; atmo_shade_rays_kernel<{flags | 16384}, {lsteps}> {twin}")
        assert new["scratch"] == 0, label
        assert waves(new["vgprs"]) >= waves(twin["vgprs"]), (label, new["vgprs"], twin["vgprs"])
        assert new["loop_vector"] == twin["loop_vector"], label
    # the order's own kernels: no stack frame either
    mine = {n: k for n, k in numbers.items() if "atmo_ray_key_kernel" in n or "atmo_ray_sort_" in n}
    assert len(mine) == 7, sorted(mine)      # the key kernel, two histograms, the scan, three scatters
    for name, k in mine.items():
        assert k["scratch"] == 0, name
    # a name of its own: no older kernel's name is a substring of a new one's, nor the reverse
    def base(mangled):     # _ZN4atmo<length><name>...
        m = T.re.match(r"_ZN4atmo(\d+)", mangled)
        return mangled[m.end():m.end() + int(m.group(1))]

    names = {base(n) for n in numbers}
    new_names = {"atmo_shade_rays_indexed_kernel", "atmo_ray_key_kernel", "atmo_ray_sort_hist_kernel", "atmo_ray_sort_scan_kernel",
                 "atmo_ray_sort_scatter_kernel"}
    assert new_names <= names, names
    for a in new_names:
        for b in names - {a}:
            assert a not in b and b not in a, (a, b)
