"""Temporal draws on the CPU (include/atmo_temporal.h; godot_atmosphere_shader_amd/temporal.py): the header's declarations against the binding's
signatures, the phase sequence, the phase frame's pixel centres, the history layout, the still-camera condition of the snap, and the numpy statement's own
behaviour on synthetic low frames.  (tests/test_temporal_gpu.py holds the kernels to the statement bit for bit.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cameras as K
from godot_atmosphere_shader_amd import reduced as R
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import temporal as TP
from godot_atmosphere_shader_amd.planet_atmosphere import make_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(37, 23), (64, 40)]
KINDS = ["plain", "forward_z", "ortho", "eye_left"]


def _camera(kind, w, h, pose="P_limb"):
    if kind == "forward_z":
        return S.Camera.from_pose(w, h, pose, reverse_z=False)
    return K.from_pose(kind, w, h, pose, **(dict(ortho_size=300.0) if kind == "ortho" else {}))


def _frame(cam):
    return make_frame(cam, np.eye(4), (0.0, 0.0, 1000.0))


def _scene_depth(cam, rng):
    """Random depths in front of the far plane with patches of sky (the far plane's exact value)."""
    h, w = cam.height, cam.width
    far = np.float32(0.0 if cam.reverse_z else 1.0)
    d = rng.uniform(0.05, 0.95, (h, w)).astype(np.float32)
    d[rng.random((h, w)) < 0.2] = far
    d[: h // 3, w // 2:] = far
    return d


def _low(rng, lh, lw):
    rgba = rng.uniform(0.0, 1.6, (lh, lw, 4)).astype(np.float32)
    rgba[..., 3] = rng.uniform(0.05, 1.0, (lh, lw)).astype(np.float32)
    return rgba


def _header():
    return open(os.path.join(ROOT, "include", "atmo_temporal.h")).read()


# ---- the header and the binding ----------------------------------------------------------------------------------------------------------------------
def test_the_signatures_are_the_header_s_declarations(tmp_path):
    from godot_atmosphere_shader_amd import _native as N

    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decls = {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"\bint\s+(atmo_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)}
    table = TP.signatures()
    assert tuple(table) == TP.TEMPORAL_ENTRY_POINTS == tuple(decls) and len(decls) == 5
    kinds = {"int": C.c_int, "int *": C.POINTER(C.c_int), "size_t *": C.POINTER(C.c_size_t), "const AtmoFrame *": C.POINTER(N.AtmoFrame),
             "const AtmoDepth *": C.POINTER(N.AtmoDepth), "const AtmoTarget *": C.POINTER(N.AtmoTarget), "const AtmoTemporal *": C.POINTER(TP.AtmoTemporal),
             "AtmoContext *": C.c_void_p, "void *": C.c_void_p, "const void *": C.c_void_p, "float *": C.c_void_p, "const float *": C.c_void_p}
    for name, args in decls.items():
        types = [kinds[re.sub(r"\s*\w+$", "", a).strip()] for a in args]          # the declaration without the parameter's name
        assert table[name] == (C.c_int, types), name
    lib = TP.bind()
    assert lib is N.load() and lib.atmo_abi_version() == N.ABI_VERSION == 5
    for sym in TP.TEMPORAL_ENTRY_POINTS:
        assert getattr(lib, sym).argtypes is not None and sym not in N.EXPORTED_SYMBOLS
    text = _header()
    assert '#include "atmo_reduced.h"' in text and "Not here" in text
    for name in ("atmo.h", "atmo_depth.h", "atmo_reduced.h"):       # the older headers do not know the new one
        assert "atmo_temporal" not in open(os.path.join(ROOT, "include", name)).read(), name
    # the structure on both sides
    assert C.sizeof(TP.AtmoTemporal) == 152
    offsets = [getattr(TP.AtmoTemporal, f).offset for f, _ in TP.AtmoTemporal._fields_]
    assert offsets == [0, 4, 8, 12, 16, 20, 24, 88]
    src = tmp_path / "size.c"
    fields = ", ".join(f"offsetof(AtmoTemporal, {f})" for f, _ in TP.AtmoTemporal._fields_)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "atmo_temporal.h"\n'
                   f'int main(void) {{ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(AtmoTemporal), {fields}); return 0; }}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == [152] + offsets


def test_a_library_without_the_symbols_is_refused_by_name():
    class Fn:
        restype = argtypes = None

    class Old:
        atmo_temporal_size = Fn()   # some, not all

    with pytest.raises(RuntimeError, match=r"atmo_temporal_phase \(include/atmo_temporal\.h\)"):
        TP.bind(Old())


# ---- phases ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_the_phase_sequence_is_a_permutation_in_bayer_order(s):
    seq = TP.phase_sequence(s)
    assert sorted(seq) == list(range(s * s))
    m2 = np.array([[0, 2], [3, 1]])
    bayer = m2 if s == 2 else np.array([[4 * m2[y % 2, x % 2] + m2[y // 2, x // 2] for x in range(4)] for y in range(4)])
    for rank, p in enumerate(seq):
        ox, oy = TP.phase_offset(s, p)
        assert bayer[oy, ox] == rank
    for a, b in zip(seq[0::2], seq[1::2]):      # far apart in the block: every pair of frames 2 k, 2 k + 1 shares neither a row nor a column
        (ax, ay), (bx, by) = TP.phase_offset(s, a), TP.phase_offset(s, b)
        assert abs(ax - bx) == abs(ay - by) == s // 2
    lib = TP.bind()
    for f in range(-2 * s * s, 3 * s * s):
        assert lib.atmo_temporal_phase(s, f) == seq[f % (s * s)] == TP.phase_of_frame(s, f)
    assert " ".join(map(str, seq)) in _header()
    assert lib.atmo_temporal_phase(3, 0) == -1
    with pytest.raises(ValueError):
        TP.phase_offset(s, s * s)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("size", SIZES)
def test_a_low_pixel_s_centre_is_its_full_pixel_s(size, s, kind):
    """In float64, the clip-space ray of low pixel i through phase_frame is that of full pixel i s + ox through the frame: NDC within 1e-6."""
    w, h = size
    frame = _frame(_camera(kind, w, h))
    m = np.asarray(frame["inv_projection_matrix"], dtype=np.float64).reshape(4, 4).T
    lw, lh = R.low_size(w, h, s)
    for p in range(s * s):
        ox, oy = TP.phase_offset(s, p)
        low = TP.phase_frame(frame, s, p)
        assert (low["viewport_w"], low["viewport_h"], low["rect"]) == (lw, lh, (0, 0, lw, lh))
        ml = np.asarray(low["inv_projection_matrix"], dtype=np.float64).reshape(4, 4).T
        a = np.linalg.solve(m, ml)       # low NDC -> full NDC, homogeneous: diag(kx, ky, 1, 1) with the translation
        i, j = np.arange(lw), np.arange(lh)
        nx = a[0, 0] * (2 * (i + 0.5) / lw - 1) + a[0, 3]
        ny = a[1, 1] * (2 * (j + 0.5) / lh - 1) + a[1, 3]
        assert np.abs(nx - (2 * (i * s + ox + 0.5) / w - 1)).max() < 1e-6 and np.abs(ny - (2 * (j * s + oy + 0.5) / h - 1)).max() < 1e-6
        off = a - np.diag(np.diag(a))
        off[:2, 3] = 0
        assert np.abs(off).max() < 1e-6 and abs(a[2, 2] - 1) < 1e-6 and abs(a[3, 3] - 1) < 1e-6


def test_the_history_layout_is_the_header_s():
    lib = TP.bind()
    assert "Each part is padded to a multiple of 16 bytes" in _header()
    for (w, h) in SIZES + [(1, 1), (5, 3), (1920, 1080), (70, 46)]:
        n = w * h
        pad = lambda v: (v + 15) // 16 * 16
        assert TP.history_layout(w, h) == (16 * n, 16 * n + pad(4 * n), 16 * n + pad(4 * n) + pad(n))
        for s in (2, 4):
            lw, lh, sc, hb = C.c_int(), C.c_int(), C.c_size_t(), C.c_size_t()
            assert lib.atmo_temporal_size(w, h, s, C.byref(lw), C.byref(lh), C.byref(sc), C.byref(hb)) == 0
            assert (lw.value, lh.value, sc.value, hb.value) == (*R.low_size(w, h, s), R.scratch_layout(w, h, s)[1], TP.history_layout(w, h)[2])
    assert lib.atmo_temporal_size(64, 40, 3, None, None, None, None) == 2 and lib.atmo_temporal_size(64, 40, 2, None, None, None, None) == 0
    rng = np.random.default_rng(0)
    parts = (rng.random((3, 5, 4)).astype(np.float32), rng.random((3, 5)).astype(np.float32), rng.integers(0, 256, (3, 5)).astype(np.uint8))
    back = TP.unpack_history(TP.pack_history(*parts), 5, 3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts, back))


# ---- the snap ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES)
def test_the_snap_is_reached_under_a_still_camera(size, kind):
    """With prev_clip_from_view built from the same camera, every pixel's (fpx, fpy) lies within 1 / 64 of its own centre -- random scene depths and sky
    texels alike -- and its expected q is the one the previous frame stored for it, far inside any tolerance."""
    w, h = size
    cam = _camera(kind, w, h)
    frame = _frame(cam)
    depth = _scene_depth(cam, np.random.default_rng(w))
    front, fpx, fpy, qe = TP.reproject(frame, depth, TP.prev_clip_from_view(frame, cam), frame["inv_projection_matrix"])
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert front.all()
    ex, ey = np.abs(fpx - x).max(), np.abs(fpy - y).max()
    print(f"{kind} {w}x{h}: max |fpx - x| = {ex:.3g}, max |fpy - y| = {ey:.3g}")
    assert ex <= TP.SNAP_RADIUS and ey <= TP.SNAP_RADIUS
    _, q0 = TP.view_point(frame, depth)
    assert np.all(np.abs(qe - q0) <= 1e-3 * np.maximum(np.abs(qe), np.abs(q0)))


# ---- the statement's own behaviour ---------------------------------------------------------------------------------------------------------------------
def _still(kind="plain", size=(37, 23), seed=1):
    cam = _camera(kind, *size)
    frame = _frame(cam)
    depth = _scene_depth(cam, np.random.default_rng(seed))
    return cam, frame, depth, TP.prev_clip_from_view(frame, cam), frame["inv_projection_matrix"]


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("size", SIZES)
def test_still_frames_in_sequence_order_fill_the_history_with_the_low_frames(size, s):
    w, h = size
    cam, frame, depth, pcv, pip = _still(size=size)
    rng = np.random.default_rng(s)
    lw, lh = R.low_size(w, h, s)
    want = np.zeros((h, w, 4), np.float32)
    want_age = np.zeros((h, w), np.int64)
    hist = None
    n = s * s
    for f, p in enumerate(TP.phase_sequence(s)):
        ox, oy = TP.phase_offset(s, p)
        low = _low(rng, lh, lw)
        low[0, 0] = (np.nan, -0.0, 0.0, 0.5)                        # bits, not values
        ys, xs = np.arange(oy, h, s), np.arange(ox, w, s)
        want[np.ix_(ys, xs)] = low[: len(ys), : len(xs)]
        want_age[np.ix_(ys, xs)] = n - 1 - f
        out = TP.resolve(frame, depth, TP.phase_depth(depth, s, p), low, s, p, 0.1, 0.1, n, hist, pcv, pip, reset=f == 0, details=True)
        hist = out[:3]
        path = out[3]["path"]
        assert (path == TP.FRESH).sum() == len(ys) * len(xs)
        if f > 0:
            assert set(np.unique(path)) <= {TP.FRESH, TP.SNAP, TP.FALLBACK} and (path == TP.BILINEAR).sum() == 0
    assert hist[0].tobytes() == want.tobytes()
    assert hist[2].tolist() == want_age.tolist() and set(np.unique(hist[2])) == set(range(n))
    assert hist[1].tobytes() == TP.view_point(frame, depth)[1].tobytes()


def test_reset_never_reads_the_previous_history():
    cam, frame, depth, pcv, pip = _still()
    s, p = 2, 3
    low = _low(np.random.default_rng(2), *R.low_size(37, 23, s)[::-1])
    ld = TP.phase_depth(depth, s, p)

    class Poison:
        def __array__(self, *a, **k):
            raise AssertionError("the previous history was read")

    a = TP.resolve(frame, depth, ld, low, s, p, 0.1, reset=True, prev=(Poison(), Poison(), Poison()), details=True)
    b = TP.resolve(frame, depth, ld, low, s, p, 0.1, reset=True, prev=None)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b))
    path = a[3]["path"]
    assert set(np.unique(path)) == {TP.FRESH, TP.FALLBACK} and np.all((a[2] == 255) == (path == TP.FALLBACK)) and np.all(a[2][path == TP.FRESH] == 0)
    with pytest.raises(ValueError):
        TP.resolve(frame, depth, ld, low, s, p, 0.1, reset=False, prev=None)


def _moved(kind="plain", size=(64, 40), dx=0.0, yaw_deg=0.0, pose="P_limb"):
    """(frame, previous camera): the current camera is the previous one moved by `dx` along its right vector and turned by `yaw_deg` about the world's y."""
    prev = _camera(kind, *size, pose)
    cur = _camera(kind, *size, pose)
    a = np.radians(yaw_deg)
    rot = np.eye(4)
    rot[0, 0], rot[0, 2], rot[2, 0], rot[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    cur.inv_view = rot @ prev.inv_view
    cur.inv_view[:3, 3] += dx * cur.inv_view[:3, 0]
    cur.view = np.linalg.inv(cur.inv_view)
    return cur, _frame(cur), prev


def test_a_pixel_reprojected_off_screen_takes_the_fallback():
    cur, frame, prev = _moved(yaw_deg=12.0)
    s, p = 2, 0
    depth = S.depth_far(cur)
    h, w = depth.shape
    rng = np.random.default_rng(3)
    hist = (_low(rng, h, w), TP.view_point(_frame(prev), depth)[1], np.zeros((h, w), np.uint8))
    out = TP.resolve(frame, depth, TP.phase_depth(depth, s, p), _low(rng, *R.low_size(w, h, s)[::-1]), s, p, 0.1, 0.1, 8, hist,
                     TP.prev_clip_from_view(frame, prev), _frame(prev)["inv_projection_matrix"], details=True)
    path, fpx, fpy = out[3]["path"], out[3]["fpx"], out[3]["fpy"]
    # no tap of the footprint lies in the image
    gone = (np.floor(fpx) + 1 < 0) | (np.floor(fpx) >= w) | (np.floor(fpy) + 1 < 0) | (np.floor(fpy) >= h)
    not_fresh = path != TP.FRESH
    assert (gone & not_fresh).sum() > 100 and np.all(path[gone & not_fresh] == TP.FALLBACK) and np.all(out[2][gone & not_fresh] == 255)
    assert (path == TP.BILINEAR).sum() > 100      # the rest of the sky is reused: a rotation reprojects directions


def test_disagreeing_q_and_age_255_are_never_reused_and_age_saturates():
    cam, frame, depth, pcv, pip = _still(size=(64, 40))
    s, p = 2, 0
    h, w = depth.shape
    rng = np.random.default_rng(4)
    q0 = TP.view_point(frame, depth)[1]
    prev_rgba = _low(rng, h, w)
    prev_q = q0.copy()
    moved = np.zeros((h, w), bool)
    moved[5:15, 10:30] = True                                  # a foreground object stood here last frame and has moved away
    prev_q[moved] = np.float32(1.0 / 0.3)
    age = rng.integers(0, 6, (h, w)).astype(np.uint8)
    never = np.zeros((h, w), bool)
    never[20:30, 40:60] = True
    age[never] = 255
    old = np.zeros((h, w), bool)
    old[32:38, 2:20] = True
    age[old] = 254
    low = _low(rng, *R.low_size(w, h, s)[::-1])
    out = TP.resolve(frame, depth, TP.phase_depth(depth, s, p), low, s, p, 0.1, 0.1, 255, (prev_rgba, prev_q, age), pcv, pip, details=True)
    path = out[3]["path"]
    nf = path != TP.FRESH
    assert np.all(path[moved & nf] == TP.FALLBACK) and np.all(out[2][moved & nf] == 255)
    assert np.all(path[never & nf] == TP.FALLBACK) and np.all(out[2][never & nf] == 255)
    assert np.all(path[old & nf] == TP.SNAP) and np.all(out[2][old & nf] == 254)                     # 254 + 1 saturates
    rest = nf & ~moved & ~never & ~old
    assert np.all(path[rest] == TP.SNAP) and np.all(out[2][rest] == age[rest] + 1)
    assert out[0][rest].tobytes() == prev_rgba[rest].tobytes()
    # max_age: a texel as old as max_age is not reused
    out = TP.resolve(frame, depth, TP.phase_depth(depth, s, p), low, s, p, 0.1, 0.1, 3, (prev_rgba, prev_q, age), pcv, pip, details=True)
    assert np.all((out[3]["path"][rest] == TP.SNAP) == (age[rest] < 3)) and (age[rest] >= 3).any()


def test_the_fallback_reads_only_low_texels_whose_pixel_exists():
    """37 x 23 at s = 4, phase 15 (ox = oy = 3): low column 9 would be pixel 39.  Poisoned, it changes nothing."""
    cam, frame, depth, pcv, pip = _still()
    s, p = 4, 15
    lw, lh = R.low_size(37, 23, s)
    low = _low(np.random.default_rng(5), lh, lw)
    ld = TP.phase_depth(depth, s, p)
    a = TP.resolve(frame, depth, ld, low, s, p, 0.1, reset=True)
    low2, ld2 = low.copy(), ld.copy()
    low2[:, 9], ld2[:, 9] = np.nan, np.nan
    assert (9 * 4 + 3 >= 37) and (5 * 4 + 3 >= 23)
    low2[5], ld2[5] = np.nan, np.nan
    b = TP.resolve(frame, depth, ld2, low2, s, p, 0.1, reset=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and not np.isnan(a[0]).any()


# ---- the cases tests/test_temporal_gpu.py holds the resolve kernel to: chosen here, on the statement alone ----------------------------------------------
RESOLVE_CASES = {
    # name: (motion, camera kind, size, scale, phase, depth format of the GPU test)
    "orbit_plain_s2": ("orbit", "plain", (64, 40), 2, 3, "d32f"),
    "orbit_eye_left_s4": ("orbit", "eye_left", (37, 23), 4, 6, "d16"),
    "translate_forward_z_s2": ("translate", "forward_z", (37, 23), 2, 1, "d32f"),
    "translate_ortho_s4": ("translate", "ortho", (64, 40), 4, 9, "x8d24"),
    "still_plain_s4": ("still", "plain", (37, 23), 4, 5, "d32f"),
    "still_eye_left_s2": ("still", "eye_left", (64, 40), 2, 2, "d16"),
}


def _ground(cam):
    return S.depth_ground_sphere(cam) if not cam.reverse_z else K.depth_of(cam)


def resolve_case(name, quantise=None):
    """The inputs of one resolve: a dict with the frame, the depth (`quantise`: what makes the depth buffer's decoded values of it), a random low frame,
    a previous history -- the previous camera's q of ITS depth, ages 0 .. 5 with a tenth of the texels and one patch at 255, a tenth of the texels
    discarded (0, 0, 0, 0) -- and the two matrices."""
    motion, kind, size, s, p, _ = RESOLVE_CASES[name]
    if motion == "orbit":
        cur, frame, prev = _moved(kind, size, yaw_deg=1.0)
    elif motion == "translate":
        # (the sky does not move under a translation and snaps: the perspective case looks at the planet from space, where the ground fills the picture)
        cur, frame, prev = _moved(kind, size, dx=20.0 if kind == "ortho" else 0.6, pose="P_limb" if kind == "ortho" else "P_space")
    else:
        cur, frame, prev = _moved(kind, size)
    w, h = size
    rng = np.random.default_rng(sum(map(ord, name)))
    depth, prev_depth = _ground(cur), _ground(prev)
    if quantise is not None:
        depth, prev_depth = quantise(depth), quantise(prev_depth)
    prev_frame = _frame(prev)
    prev_rgba = _low(rng, h, w)
    prev_rgba[rng.random((h, w)) < 0.1] = 0.0
    age = rng.integers(0, 6, (h, w)).astype(np.uint8)
    age[rng.random((h, w)) < (0.05 if motion == "still" else 0.1)] = 255
    if motion != "still":
        age[h // 2: h // 2 + h // 4, w // 8: w // 2] = 255
    lw, lh = R.low_size(w, h, s)
    low = _low(rng, lh, lw)
    low[rng.random((lh, lw)) < 0.2] = 0.0
    return dict(frame=frame, depth=depth, s=s, p=p, low_rgba=low, low_depth=TP.phase_depth(depth, s, p), prev=(prev_rgba, TP.view_point(prev_frame, prev_depth)[1], age),
                prev_clip=TP.prev_clip_from_view(frame, prev), prev_inv_projection=prev_frame["inv_projection_matrix"], motion=motion,
                depth_tolerance=0.1, history_tolerance=0.1, max_age=6 if motion == "still" else 5)


def resolve_shares(path):
    """(snap, bilinear, fallback) as shares of the pixels that are not fresh."""
    nf = (path != TP.FRESH).sum()
    return tuple(float((path == k).sum()) / nf for k in (TP.SNAP, TP.BILINEAR, TP.FALLBACK))


def check_coverage(motion, path):
    snap, bilinear, fallback = resolve_shares(path)
    if motion == "still":
        assert snap >= 0.8, (snap, bilinear, fallback)
    else:
        assert bilinear >= 0.2 and fallback >= 0.05, (snap, bilinear, fallback)


@pytest.mark.parametrize("name", list(RESOLVE_CASES))
def test_the_resolve_cases_cover_every_path(name):
    c = resolve_case(name)
    out = TP.resolve(c["frame"], c["depth"], c["low_depth"], c["low_rgba"], c["s"], c["p"], c["depth_tolerance"], c["history_tolerance"], c["max_age"],
                     c["prev"], c["prev_clip"], c["prev_inv_projection"], details=True)
    print(name, "snap / bilinear / fallback of the non-fresh pixels: %.3f / %.3f / %.3f" % resolve_shares(out[3]["path"]))
    check_coverage(c["motion"], out[3]["path"])
    assert np.isfinite(out[0]).all() and set(np.unique(out[2])) <= set(range(0, 7)) | {255}
