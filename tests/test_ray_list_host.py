"""CPU tests of the ray-list header (include/atmo_ray_list.h): the header's symbol set and the binding, every refusal of atmo_ray_list on a host-only
context in the header's order (nothing touches a device), THE CULL's constants, the scratch size, and the numpy statement
(godot_atmosphere_shader_amd/ray_list.py) on hand cases -- with the cull's REACH on the project's camera queues: it removes at least 0.98 of the rays whose
fp32 h is negative and none whose h is not.  (tests/test_ray_list_gpu.py holds the kernels to the numpy statement and the list + indexed shading to
atmo_shade_rays, bit for bit.)"""
import ctypes as C

import numpy as np
import pytest

from godot_atmosphere_shader_amd import scene as S
from test_rays_host import RAYS, RGBA, _said
from test_views_proxy_host import FAR, _frame, _functions, _host_ctx

F = np.float32
INDEX, SCRATCH, COUNT, LISTED = 0x40000, 0x60000, 0x70000, 0x80000   # addresses no refusal dereferences
WHO = "atmo_ray_list: "
ORDER, CULL, END = 1, 2, 0xFFFFFFFF
NAMES = {"atmo_ray_list_scratch_bytes", "atmo_ray_list", "atmo_debug_ray_cull_constants"}
R_SHELL = 108.0      # the demo scene: planet radius 100 + atmosphere height 8


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, N.load()


def hand_consts(c=(0.0, 0.0, -300.0), radius=R_SHELL):
    """The five floats of atmo_debug_ray_cull_constants for a centre and a shell radius, formed as the header forms them."""
    r2 = F(radius) * F(radius)
    return np.array([c[0], c[1], c[2], r2, r2 * F(1.02)], dtype=F)


def hand_rays(c=(0.0, 0.0, -300.0), radius=R_SHELL):
    """(rows, culled, labels): AtmoRay rows around a shell of `radius` at `c` whose distance from the origin is a few radii, and what THE CULL says of each."""
    c = np.asarray(c, dtype=np.float64)
    dist = float(np.linalg.norm(c))
    to_c = c / dist
    side = np.cross(to_c, (0.0, 1.0, 0.0) if abs(to_c[1]) < 0.9 else (1.0, 0.0, 0.0))
    side /= np.linalg.norm(side)
    limb = np.arcsin(radius / dist)

    def aimed(angle):     # from the origin, `angle` radians off the centre
        return np.cos(angle) * to_c + np.sin(angle) * side

    off_limb = aimed(limb + np.radians(10.0))
    cases = [
        ("10 degrees off the limb", (0, 0, 0), off_limb, True),
        ("the same origin, aimed at the planet", (0, 0, 0), to_c, False),
        ("just inside the limb", (0, 0, 0), aimed(limb - np.radians(0.5)), False),
        ("straight away from the planet: the LINE hits, and h is the line's", (0, 0, 0), -to_c, False),
        ("away from the planet, 10 degrees off the limb", (0, 0, 0), -off_limb, True),
        ("a NaN direction component", (0, 0, 0), (off_limb[0], np.nan, off_limb[2]), False),
        ("a NaN origin component", (np.nan, 0, 0), off_limb, False),
        ("a zero direction", (0, 0, 0), (0, 0, 0), False),
        ("dd = 0.2", (0, 0, 0), off_limb * np.sqrt(0.2), False),
        ("dd = 1.8", (0, 0, 0), off_limb * np.sqrt(1.8), False),
        ("dd = 0.3: inside the band", (0, 0, 0), off_limb * np.sqrt(0.3), True),
        ("dd = 1.7: inside the band", (0, 0, 0), off_limb * np.sqrt(1.7), True),
        ("an origin inside the shell", c + 0.5 * radius * side, to_c, False),
        ("an origin at 1.005 R, along the tangent: a miss, but within 1 % of the shell", c + 1.005 * radius * side, to_c, False),
        ("an origin at 1.05 R, along the tangent", c + 1.05 * radius * side, to_c, True),
        ("an origin at 1.05 R, looking in", c + 1.05 * radius * side, -side, False),
    ]
    rows = np.zeros((len(cases), 8), dtype=F)
    for k, (_, o, d, _) in enumerate(cases):
        rows[k, 0:3], rows[k, 3], rows[k, 4:7] = o, 3.0e38, d
    return rows, np.array([x[3] for x in cases]), [x[0] for x in cases]


def h_fp32(rows, consts):
    """ray_sphere's h as the ray kernels form it, float32 operation for operation: c' = c - origin, oc = 0 - c', b = dot(oc, d), qc = oc - b d,
    h = R2 - dot(qc, qc) (sphere_setup and hit_radius of csrc/atmo_kernels.hip)."""
    r, k = np.asarray(rows, dtype=F), np.asarray(consts, dtype=F)
    with np.errstate(all="ignore"):
        oc = [F(0.0) - (k[j] - r[:, j]) for j in range(3)]
        d = [r[:, 4 + j] for j in range(3)]
        b = (oc[0] * d[0] + oc[1] * d[1]) + oc[2] * d[2]
        qc = [oc[j] - b * d[j] for j in range(3)]
        h = k[3] - ((qc[0] * qc[0] + qc[1] * qc[1]) + qc[2] * qc[2])
    assert h.dtype == np.float32
    return h


def camera_queue(pose, w=113, h=67):
    """(rows, consts): the float32 camera rays of a pose -- origin 0, Camera.pixel_view_dirs normalised -- and the cull's constants of that camera's frame
    in numpy: the view-space centre make_frame hands the library, R2 of the demo scene."""
    from godot_atmosphere_shader_amd.planet_atmosphere import make_frame

    cam = S.Camera.from_pose(w, h, pose)
    d = cam.pixel_view_dirs().reshape(-1, 3)
    rows = np.zeros((w * h, 8), dtype=F)
    rows[:, 3] = 3.0e38
    rows[:, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    c = np.asarray(make_frame(cam, np.eye(4), (0.0, 0.0, 500.0))["planet_center_viewspace"], dtype=F)
    return rows, hand_consts(c)


def test_binding_exposes_the_ray_list_header():
    N, lib = _lib()
    from godot_atmosphere_shader_amd import ray_list as RL

    assert _functions("atmo_ray_list.h") == set(N.RAY_LIST_SYMBOLS) == NAMES and len(N.RAY_LIST_SYMBOLS) == len(NAMES)
    for sym in N.RAY_LIST_SYMBOLS:
        assert getattr(lib, sym) is not None and sym not in N.EXPORTED_SYMBOLS      # (AttributeError on a library without the symbols: a failure)
    tuples = {k: v for k, v in vars(N).items() if k.endswith("_SYMBOLS") and k != "RAY_LIST_SYMBOLS"}
    assert {"CORE_SYMBOLS", "RAYS_SYMBOLS", "RAY_QUADS_SYMBOLS", "RAY_ORDER_SYMBOLS", "EXPORTED_SYMBOLS"} <= set(tuples)
    for name, other in tuples.items():     # disjoint from every other tuple
        assert not set(N.RAY_LIST_SYMBOLS) & set(other), name
    assert lib.atmo_abi_version() == N.ABI_VERSION == 5
    header = open(_root() + "/include/atmo_ray_list.h").read()
    for line in ("#define ATMO_RAY_LIST_ORDER 1 ", "#define ATMO_RAY_LIST_CULL  2 ", "#define ATMO_RAY_LIST_END   0xFFFFFFFFu "):
        assert line in header, line
    assert (RL.ORDER, RL.CULL, RL.END) == (N.RAY_LIST_ORDER, N.RAY_LIST_CULL, N.RAY_LIST_END) == (ORDER, CULL, END)
    assert '#include "atmo_ray_order.h"' in header


def _root():
    import os

    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need(lib, capacity):
    b = C.c_size_t()
    assert lib.atmo_ray_list_scratch_bytes(capacity, C.byref(b)) == 0
    return b.value


def test_scratch_bytes_are_monotone():
    N, lib = _lib()
    b, o = C.c_size_t(12345), C.c_size_t()
    assert lib.atmo_ray_list_scratch_bytes(0, C.byref(b)) == N.ATMO_OK and b.value < 2 ** 20
    last = b.value
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 7571, 2 ** 20, 2 ** 20 + 1, 2_073_600, 2 ** 28 - 1, 2 ** 28):
        assert lib.atmo_ray_list_scratch_bytes(n, C.byref(b)) == N.ATMO_OK and lib.atmo_ray_order_scratch_bytes(n, C.byref(o)) == N.ATMO_OK
        assert b.value >= last and b.value > o.value and b.value % 16 == 0, (n, b.value, o.value, last)    # monotone; the order's and the live word
        last = b.value
    assert lib.atmo_ray_list_scratch_bytes(2 ** 28 + 1, C.byref(b)) == N.ATMO_E_ARG and b.value == last
    assert lib.atmo_ray_list_scratch_bytes(2 ** 32 - 1, C.byref(b)) == N.ATMO_E_ARG
    assert lib.atmo_ray_list_scratch_bytes(5, None) == N.ATMO_E_ARG


def test_scratch_bytes_are_the_layout_s():
    """Two buffers of n pairs (16 n bytes), 64 histogram words per chunk of 1024 elements and 64 totals (256 bytes each); the list's live word in 16 bytes
    of its own behind them."""
    N, lib = _lib()
    b, o = C.c_size_t(), C.c_size_t()
    for n, want in ((0, 256), (1, 528), (1024, 16_896), (1025, 17_168), (2 ** 28, 4_362_076_416)):
        assert want == 16 * n + 256 * (-(-n // 1024) + 1)
        assert lib.atmo_ray_order_scratch_bytes(n, C.byref(o)) == N.ATMO_OK and lib.atmo_ray_list_scratch_bytes(n, C.byref(b)) == N.ATMO_OK
        assert (o.value, b.value) == (want, want + 16), (n, o.value, b.value)


def test_atmo_ray_list_refuses_in_the_header_s_order():
    """The capacity, the flags, null pointers, CULL's two, 16-byte alignment, 4-byte alignment, the scratch size -- each under the entry point's name -- and
    ATMO_E_NO_DEVICE behind all of them."""
    N, lib = _lib()
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    cap = 5000
    need = _need(lib, cap)
    f = _frame(FAR)
    try:
        def call(**kw):     # the arguments by name, in the header's order, `stream` last
            a = dict(frame=C.byref(f), rays=RAYS, count=COUNT, capacity=cap, flags=ORDER | CULL, rgba=RGBA, index=INDEX, listed=LISTED, scratch=SCRATCH,
                     bytes=need)
            a.update(kw)
            return _said(lib, ctx, lib.atmo_ray_list(ctx, *a.values(), None))

        refused = [dict(capacity=2 ** 28 + 1), dict(flags=4), dict(flags=7), dict(flags=-1), dict(flags=1 << 16), dict(rays=None), dict(index=None),
                   dict(scratch=None), dict(frame=None), dict(rgba=None), dict(frame=None, flags=CULL), dict(rgba=None, flags=CULL), dict(rays=RAYS + 8),
                   dict(rays=RAYS + 4), dict(rgba=RGBA + 8), dict(rgba=RGBA + 4, flags=0), dict(scratch=SCRATCH + 8), dict(index=INDEX + 2), dict(index=INDEX + 1),
                   dict(count=COUNT + 2), dict(listed=LISTED + 1), dict(bytes=need - 1), dict(bytes=0)]
        for kw in refused:
            rc, msg = call(**kw)
            assert rc == N.ATMO_E_ARG and msg.startswith(WHO), (kw, rc, msg)
        # what is fine gets as far as the device: no count word, no listed word, no flags and then neither frame nor rgba, more scratch, 4-byte alignment
        fine = [dict(), dict(count=None), dict(listed=None), dict(flags=0, frame=None, rgba=None), dict(flags=ORDER, frame=None, rgba=None), dict(flags=CULL),
                dict(bytes=need + 4096), dict(index=INDEX + 4, count=COUNT + 4, listed=LISTED + 4), dict(capacity=1, bytes=_need(lib, 1)),
                dict(capacity=2 ** 28, bytes=_need(lib, 2 ** 28))]
        for kw in fine:
            rc, msg = call(**kw)
            assert rc == N.ATMO_E_NO_DEVICE and msg.startswith(WHO), (kw, rc, msg)
        # the order of the checks
        assert "2^28" in call(capacity=2 ** 28 + 1, flags=4, rays=None)[1]
        assert "unknown flag bits" in call(flags=4, rays=None)[1]
        assert "null rays_dev" in call(rays=None, index=None, scratch=None, frame=None)[1]
        assert "null index_dev" in call(index=None, scratch=None, frame=None)[1]
        assert "null scratch_dev" in call(scratch=None, frame=None, rgba=None)[1]
        assert "needs a frame" in call(frame=None, rgba=None, rays=RAYS + 8)[1]
        assert "needs rgba_dev" in call(rgba=None, rays=RAYS + 8)[1]
        assert "rays_dev must be 16-byte aligned" in call(rays=RAYS + 8, rgba=RGBA + 8, scratch=SCRATCH + 8, index=INDEX + 2)[1]
        assert "rgba_dev must be 16-byte aligned" in call(rgba=RGBA + 8, scratch=SCRATCH + 8, index=INDEX + 2)[1]
        assert "scratch_dev must be 16-byte aligned" in call(scratch=SCRATCH + 8, index=INDEX + 2, bytes=0)[1]
        assert "index_dev must be 4-byte aligned" in call(index=INDEX + 2, count=COUNT + 1, listed=LISTED + 1, bytes=0)[1]
        assert "count_dev must be 4-byte aligned" in call(count=COUNT + 1, listed=LISTED + 1, bytes=0)[1]
        assert "listed_dev must be 4-byte aligned" in call(listed=LISTED + 1, bytes=0)[1]
        assert "atmo_ray_list_scratch_bytes" in call(bytes=need - 1)[1]
        # nothing to list is ATMO_OK with nothing else looked at; no context is ATMO_E_ARG
        assert lib.atmo_ray_list(ctx, None, None, None, 0, 99, None, None, None, None, 0, None) == N.ATMO_OK
        assert call(capacity=0, flags=4, rays=RAYS + 1, bytes=0)[0] == N.ATMO_OK
        assert lib.atmo_ray_list(None, C.byref(f), RAYS, COUNT, cap, 3, RGBA, INDEX, LISTED, SCRATCH, need, None) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)


def test_cull_constants_of_the_demo_scene():
    """c as the frame gives it, R2 = 11664 for radius 100 + height 8, and the fifth value RN(R2 * 1.02f); with atmo_set_host_double_precision the same
    centre (the negation touches the inverse view matrix' origin, which the cull does not read)."""
    from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame, make_frame

    N, lib = _lib()
    cam = S.Camera.from_pose(113, 67, "P_limb")
    frame = make_frame(cam, np.eye(4), (0.0, 0.0, 500.0))
    nf = _to_native_frame(frame)
    ctx = _host_ctx(N.VARIANT_CLOUDS_HIGH)
    try:
        for name, value in (("u_planet_radius", 100.0), ("u_atmosphere_height", 8.0)):      # the demo scene's planet
            assert lib.atmo_set_param_f32(ctx, name.encode(), (C.c_float * 1)(value), 1) == N.ATMO_OK, name
        for double in (0, 1):
            assert lib.atmo_set_host_double_precision(ctx, double) == N.ATMO_OK
            out, n = (C.c_float * 8)(*([7.0] * 8)), C.c_int(0)
            assert lib.atmo_debug_ray_cull_constants(ctx, C.byref(nf), out, 8, C.byref(n)) == N.ATMO_OK and n.value == 5
            v = np.array(out, dtype=F)
            assert np.array_equal(v[:3], np.asarray(frame["planet_center_viewspace"], dtype=F)) and np.linalg.norm(v[:3]) > 100.0
            assert v[3] == F(11664.0) and v[4] == F(11664.0) * F(1.02)
            assert np.array_equal(v[5:], [7.0, 7.0, 7.0])
            assert np.array_equal(v[:5], hand_consts(frame["planet_center_viewspace"]))
        assert lib.atmo_debug_ray_cull_constants(ctx, C.byref(nf), out, 5, C.byref(n)) == N.ATMO_OK
        for args in ((None, out, 5, C.byref(n)), (C.byref(nf), None, 5, C.byref(n)), (C.byref(nf), out, 5, None), (C.byref(nf), out, 4, C.byref(n))):
            assert lib.atmo_debug_ray_cull_constants(ctx, *args) == N.ATMO_E_ARG, args
        assert lib.atmo_debug_ray_cull_constants(None, C.byref(nf), out, 5, C.byref(n)) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)


def test_the_numpy_list_on_hand_cases():
    from godot_atmosphere_shader_amd import ray_list as RL
    from godot_atmosphere_shader_amd import ray_order as R
    from test_ray_order_host import seeded_directions

    rows, culled, _ = hand_rays()
    rows = np.concatenate([rows, np.zeros((200, 8), dtype=F)])
    rows[len(culled):, 4:7] = seeded_directions(200, seed=3)         # origin 0, 300 from the centre: some hit, most miss
    consts = hand_consts()
    cap = rows.shape[0]
    mask = RL.cull_mask(rows, consts)
    assert 20 < mask.sum() < cap - 10
    for n in (0, 1, 7, 64, cap - 1, cap):
        # ORDER: ray_order of the live rows, then the END tail
        index, listed, zeros = RL.ray_list(rows, n, ORDER)
        assert index.dtype == np.uint32 and index.shape == (cap,) and listed == n and not zeros.any()
        assert np.array_equal(index[:n], R.ray_order(rows[:n])) and (index[n:] == END).all()
        # no flags: the identity
        index, listed, zeros = RL.ray_list(rows, n, 0)
        assert listed == n and np.array_equal(index[:n], np.arange(n)) and (index[n:] == END).all() and not zeros.any()
        # CULL: the kept rows ascending; the culled rows of the live part get zeros
        index, listed, zeros = RL.ray_list(rows, n, CULL, consts)
        kept = np.nonzero(~mask[:n])[0]
        assert listed == kept.size and np.array_equal(index[:listed], kept) and (index[listed:] == END).all()
        assert np.array_equal(zeros[:n], mask[:n]) and not zeros[n:].any()
        # ORDER | CULL: the kept rows in the stable order of their keys
        index, listed, zeros2 = RL.ray_list(rows, n, ORDER | CULL, consts)
        assert listed == kept.size and np.array_equal(index[:listed], kept[np.argsort(R.ray_keys(rows[kept]), kind="stable")])
        assert (index[listed:] == END).all() and np.array_equal(zeros2, zeros)
    # a count beyond the capacity clamps; no count word is the capacity
    for flags in (0, ORDER, CULL, ORDER | CULL):
        want = RL.ray_list(rows, cap, flags, consts)
        for n in (cap + 5, 2 ** 32 - 1, None):
            got = RL.ray_list(rows, n, flags, consts)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2]), (flags, n)
    # rows behind the count take no part, whatever they hold
    dirty = rows.copy()
    dirty[64:] = np.nan
    for flags in (0, ORDER, CULL, ORDER | CULL):
        a, b = RL.ray_list(rows, 64, flags, consts), RL.ray_list(dirty, 64, flags, consts)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    with pytest.raises(ValueError):
        RL.ray_list(rows, 5, 4)
    with pytest.raises(ValueError):
        RL.ray_list(rows, 5, CULL)
    assert RL.ray_list(np.zeros((0, 8), dtype=F), 0, ORDER | CULL, consts)[0].shape == (0,)


def test_cull_mask_on_hand_rays():
    from godot_atmosphere_shader_amd import ray_list as RL

    for c in ((0.0, 0.0, -300.0), (-0.357289, -0.105603, -157.92054), (120.0, -200.0, 90.0)):
        rows, want, labels = hand_rays(c)
        consts = hand_consts(c)
        got = RL.cull_mask(rows, consts)
        assert got.dtype == bool
        for g, w, label in zip(got.tolist(), want.tolist(), labels):
            assert g == w, (c, label, g, w)
        # sound on the hand rays too: what is culled has a negative fp32 h
        assert (h_fp32(rows, consts)[got] < 0).all()
    with pytest.raises(ValueError):
        RL.cull_mask(np.zeros((3, 3), dtype=F), hand_consts())
    with pytest.raises(ValueError):
        RL.cull_mask(np.zeros((3, 8), dtype=F), np.zeros(4, dtype=F))


def test_the_cull_s_reach_on_the_camera_queues():
    """113 x 67 camera rays of P_space, P_limb and P_night: the cull removes at least 0.98 of the rays whose fp32 h is negative and none whose h is not
    (0.9925, 0.9996 and 0.9946 when the header was written); P_clouds and P_ground have no missing ray, and nothing is culled there."""
    from godot_atmosphere_shader_amd import ray_list as RL

    for pose, share in (("P_space", 0.37), ("P_limb", 0.64), ("P_night", 0.49)):
        rows, consts = camera_queue(pose)
        h = h_fp32(rows, consts)
        miss, mask = h < 0, RL.cull_mask(rows, consts)
        reach = (mask & miss).sum() / miss.sum()
        print(f"{pose}: {miss.mean():.4f} of the rays miss, the cull removes {reach:.4f} of them, {int((mask & ~miss).sum())} false culls")
        assert abs(miss.mean() - share) < 0.01, (pose, float(miss.mean()))
        assert not (mask & ~miss).any(), pose
        assert reach >= 0.98, (pose, reach)
    for pose in ("P_clouds", "P_ground"):
        rows, consts = camera_queue(pose)
        assert not (h_fp32(rows, consts) < 0).any() and not RL.cull_mask(rows, consts).any(), pose


def test_ray_list_binding_without_a_device(monkeypatch):
    """PlanetAtmosphere.ray_list reaches atmo_ray_list with the header's arguments; with cull and no out, out is torch.zeros; a library without the symbols
    raises, naming the header.  (The caller's stream becomes torch's current one while the scratch is allocated: stood in for here, where there is no device.)"""
    import contextlib

    import torch

    monkeypatch.setattr(torch.cuda, "ExternalStream", lambda handle, device=None: handle)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())

    import test_binding_calls_host as B
    from godot_atmosphere_shader_amd import planet_atmosphere as PA

    names = ("ctx", "frame", "rays", "count", "capacity", "flags", "rgba", "index", "listed", "scratch", "bytes", "stream")
    node, cam = B._node(), B._cam()
    rays, out, count = B._fake((70, 8)), B._fake((70, 4)), B._fake((1,), torch.int32)
    seen = []

    class Watch(B._AllocateAsCuda):
        def __torch_function__(self, func, types, args=(), kwargs=None):
            if func in (torch.empty, torch.zeros):
                seen.append(func)
            return super().__torch_function__(func, types, args, kwargs)

    with Watch():
        index, listed = node.ray_list(rays, count, order=True, cull=True, camera=cam, out=out, stream=B.STREAM)
    assert tuple(index.shape) == (70,) and index.dtype == torch.int32 and tuple(listed.shape) == (1,) and listed.dtype == torch.int32
    assert torch.zeros not in seen
    calls = dict((c[0], c[1]) for c in node._lib.calls if c[0] != "atmo_destroy")
    assert set(calls) == {"atmo_ray_list_scratch_bytes", "atmo_ray_list"}
    a = dict(zip(names, calls["atmo_ray_list"]))
    assert a["ctx"] == B.CTX and a["frame"] == bytes(PA._to_native_frame(node.make_frame(cam, 0.0))) and a["rays"] == rays.data_ptr()
    assert a["count"] == count.data_ptr() and a["capacity"] == 70 and a["flags"] == 3 and a["rgba"] == out.data_ptr() and a["index"] == index.data_ptr()
    assert a["listed"] == listed.data_ptr() and a["stream"] == B.STREAM
    # no count word, queue order, no cull: neither frame nor rgba
    node = B._node()
    with B._AllocateAsCuda():
        node.ray_list(rays, order=False, stream=B.STREAM)
    a = dict(zip(names, [c for c in node._lib.calls if c[0] == "atmo_ray_list"][0][1]))
    assert a["frame"] is None and a["count"] is None and a["flags"] == 0 and a["rgba"] is None
    # cull and no out: zeros
    node = B._node()
    del seen[:]
    with Watch():
        node.ray_list(rays, cull=True, stream=B.STREAM)
    assert seen.count(torch.zeros) == 1
    for bad in (torch.zeros((1,), dtype=torch.int32), B._fake((1,), torch.int64), 5, np.zeros(1, dtype=np.int32)):
        with pytest.raises(TypeError, match="count must be a contiguous CUDA int32 tensor"):
            node.ray_list(rays, bad, stream=B.STREAM)
    with pytest.raises(ValueError, match="count must have one element"):
        node.ray_list(rays, B._fake((2,), torch.int32), stream=B.STREAM)
    with pytest.raises(ValueError, match="out must have one row per ray"):
        node.ray_list(rays, cull=True, out=B._fake((69, 4)), stream=B.STREAM)

    node = B._node(lib=B.library_without("atmo_ray_list", "atmo_ray_list_scratch_bytes"))
    with pytest.raises(RuntimeError, match=r"atmo_ray_list \(include/atmo_ray_list.h\)"), B._AllocateAsCuda():
        node.ray_list(rays, stream=B.STREAM)
