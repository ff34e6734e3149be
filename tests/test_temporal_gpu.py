"""Temporal draws on the device (include/atmo_temporal.h).  Needs an MI355X.  Every comparison is BIT-EXACT against the numpy statement,
godot_atmosphere_shader_amd/temporal.py, or against the entry points the whole path is made of.

 (a) the phase depth: every phase, the three depth formats, a padded pitch, both sizes and scales;
 (b) the resolve: the six cases of tests/test_temporal.py (an orbit, a translation, a still camera; their shares of the paths asserted first) into all
     seven formats, plain and composite -- the target's bytes, the history's rgba and q, the history's ages;
 (c) the whole path is its three steps, with and without a previous history, for four contexts;
 (d) a still camera: scale^2 calls leave the history the scatter of scale^2 plain draws of the phase frames;
 (e) every refusal, and that it leaves target and history alone;
 (f) render_temporal writes the C calls' bytes over three frames of a moving camera."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import demo_params, demo_textures, make_node
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import depth_formats as D
from godot_atmosphere_shader_amd import reduced as R
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T
from godot_atmosphere_shader_amd import temporal as TP
from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame
from test_reduced_gpu import CONTEXTS, FORMATS, SENTINEL, _bits, _depth_buffer, _dev, _stream, _target_buffer
from test_temporal import RESOLVE_CASES, _camera, _moved, _scene_depth, check_coverage, resolve_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return TP.bind()


_nodes = {}


def _node(config, **kw):
    """One node per configuration for the whole module (closed at its end), its LUT baked by a first draw."""
    key = (config, tuple(sorted(kw.items())))
    if key not in _nodes:
        node = make_node(config, demo_textures(), demo_params(), sampler="declared", **kw)
        cam = S.Camera.from_pose(16, 8, "P_space")
        node.render(cam, _dev(S.depth_far(cam)))
        torch.cuda.synchronize()
        _nodes[key] = node
    return _nodes[key]


@pytest.fixture(scope="module", autouse=True)
def _close_nodes():
    yield
    for node in _nodes.values():
        node.close()
    _nodes.clear()


def _frames(node, cam, time=0.0):
    d = node.make_frame(cam, time)
    return d, _to_native_frame(d)


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _history(parts=None, w=0, h=0):
    """A history buffer on the device: `parts` packed, or the sentinel everywhere."""
    if parts is not None:
        return _dev(TP.pack_history(*parts, fill=SENTINEL))
    return torch.full((TP.history_layout(w, h)[2],), SENTINEL, dtype=torch.uint8, device="cuda")


def _assert_history(buf, want, w, h):
    """The device buffer's three parts are `want`'s, bit for bit, and its padding was not written."""
    got = buf.cpu().numpy()
    rgba, q, age = TP.unpack_history(got, w, h)
    assert rgba.tobytes() == want[0].tobytes(), "history rgba"
    assert q.tobytes() == want[1].tobytes(), "history q"
    assert age.tolist() == want[2].tolist(), "history ages"
    assert got.tobytes() == TP.pack_history(*want, fill=SENTINEL).tobytes(), "history padding"


# ---- (a) the phase depth ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("size", [(37, 23), (64, 40)])
def test_the_phase_depth_is_the_statement_s(lib, size, s):
    node = _node("no_clouds_8")
    cam = _camera("plain", *size)
    _, nf = _frames(node, cam)
    lw, lh = R.low_size(*size, s)
    rng = np.random.default_rng(size[0] + s)
    for fmt, pad in (("d32f", 0), ("d16", 0), ("x8d24", 0), ("d16", 3), ("d32f", 5)):
        buf, dfmt, pitch, decoded = _depth_buffer(_scene_depth(cam, rng), fmt, pad)
        src = N.AtmoDepth(buf.data_ptr(), dfmt, pitch)
        for p in range(s * s):
            out = torch.full((lh * lw + 8,), -7.0, dtype=torch.float32, device="cuda")       # a guard behind the low image
            N.check(node._ctx, lib.atmo_temporal_depth(node._ctx, C.byref(nf), C.byref(src), s, p, _ptr(out), _stream()))
            got = out.cpu().numpy()
            assert np.all(got[lh * lw:] == -7.0)
            assert got[:lh * lw].tobytes() == TP.phase_depth(decoded, s, p).tobytes(), (fmt, pad, p)


# ---- (b) the resolve ----------------------------------------------------------------------------------------------------------------------------------------
_cases = {}


def _case(name):
    """The case's inputs on the decoded depth of its buffer's format, and the statement's result: computed once, shared by the fourteen format tests."""
    if name not in _cases:
        fmt = RESOLVE_CASES[name][5]
        c = resolve_case(name, quantise=lambda d: D.decode(D.quantise(d, fmt), fmt))
        out = TP.resolve(c["frame"], c["depth"], c["low_depth"], c["low_rgba"], c["s"], c["p"], c["depth_tolerance"], c["history_tolerance"], c["max_age"],
                         c["prev"], c["prev_clip"], c["prev_inv_projection"], details=True)
        for a in out[:3]:
            a.setflags(write=False)
        _cases[name] = (c, out)
    return _cases[name]


def _resolve(lib, node, nf, src, opt, low_depth, low_rgba, prev, cur, buf, fmt, pitch, composite):
    tgt = N.AtmoTarget(buf.data_ptr(), T.format_id(fmt), pitch)
    ld, lc = _dev(low_depth), _dev(low_rgba)
    rc = lib.atmo_temporal_resolve(node._ctx, C.byref(nf), C.byref(src), C.byref(opt), _ptr(ld), _ptr(lc), _ptr(prev), _ptr(cur), C.byref(tgt), int(composite),
                                   _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("composite", [False, True], ids=["plain", "composite"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_resolve_is_the_statement_s_in_every_format(lib, fmt, composite):
    node = _node("no_clouds_8")
    px = T.PIXEL_BYTES[T.format_id(fmt)]
    for k, name in enumerate(RESOLVE_CASES):
        c, (pixels, q0, age, det) = _case(name)
        check_coverage(c["motion"], det["path"])                       # the condition of the comparison: every path is taken
        w, h = RESOLVE_CASES[name][2]
        pad = 2 * px if k % 2 else 0
        nf = _to_native_frame(c["frame"])
        dbuf, dfmt, dpitch, decoded = _depth_buffer(c["depth"], RESOLVE_CASES[name][5], pad=1 if pad else 0)
        assert decoded.tobytes() == c["depth"].tobytes()               # (quantising twice changes nothing)
        rng = np.random.default_rng(k + 10 * int(composite))
        buf, dst = _target_buffer(rng, fmt, h, w, pad, composite)
        want = R.store(pixels, fmt, dst, composite)
        opt = TP.options(c["s"], c["p"], c["depth_tolerance"], c["history_tolerance"], c["max_age"], False, c["prev_clip"], c["prev_inv_projection"])
        prev, cur = _history(c["prev"]), _history(w=w, h=h)
        N.check(node._ctx, _resolve(lib, node, nf, N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch), opt, c["low_depth"], c["low_rgba"], prev, cur, buf, fmt,
                                    w * px + pad if pad else 0, composite))
        got = buf.cpu().numpy()
        assert got[:, :w * px].tobytes() == _bits(want).reshape(h, w * px).tobytes(), (name, "target")
        assert np.all(got[:, w * px:] == SENTINEL)                     # bytes between rows are never written
        _assert_history(cur, (pixels, q0, age), w, h)
        assert prev.cpu().numpy().tobytes() == TP.pack_history(*c["prev"], fill=SENTINEL).tobytes()      # the previous history is only read
        if composite:
            clear = ~(pixels[..., 3] > 0)
            assert clear.sum() > 10                                    # pixels without alpha keep their bytes in the target, and are in the history
            assert got[:, :w * px].reshape(h, w, px)[clear].tobytes() == _bits(dst).reshape(h, w, px)[clear].tobytes()


def test_a_reset_resolve_reads_no_previous_history(lib):
    node = _node("no_clouds_8")
    name = "orbit_plain_s2"
    c, _ = _case(name)
    w, h = RESOLVE_CASES[name][2]
    pixels, q0, age = TP.resolve(c["frame"], c["depth"], c["low_depth"], c["low_rgba"], c["s"], c["p"], c["depth_tolerance"], reset=True)
    dbuf, dfmt, dpitch, _ = _depth_buffer(c["depth"], "d32f")
    buf, dst = _target_buffer(np.random.default_rng(0), "rgba32f", h, w, 0, False)
    opt = TP.options(c["s"], c["p"], c["depth_tolerance"], reset=True)
    cur = _history(w=w, h=h)
    N.check(node._ctx, _resolve(lib, node, _to_native_frame(c["frame"]), N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch), opt, c["low_depth"], c["low_rgba"], None,
                                cur, buf, "rgba32f", 0, False))
    assert buf.cpu().numpy().tobytes() == pixels.tobytes()
    _assert_history(cur, (pixels, q0, age), w, h)
    assert set(np.unique(age)) == {0, 255}


# ---- (c) the whole path --------------------------------------------------------------------------------------------------------------------------------------
def _temporal(lib, node, nf, src, opt, scratch, prev, cur, buf, fmt, pitch, composite):
    tgt = N.AtmoTarget(buf.data_ptr(), T.format_id(fmt), pitch)
    return lib.atmo_render_temporal_target(node._ctx, C.byref(nf), C.byref(src), C.byref(opt), _ptr(scratch), _ptr(prev), _ptr(cur), C.byref(tgt),
                                           int(composite), _stream())


@pytest.mark.parametrize("size,s", [((70, 46), 4), ((64, 40), 2)], ids=["70x46s4", "64x40s2"])
@pytest.mark.parametrize("config,kw", CONTEXTS, ids=["no_clouds", "clouds_high", "clouds_high_rm", "clouds_high_detail"])
def test_the_whole_path_is_its_three_steps(lib, config, kw, size, s):
    node = _node(config, **kw)
    w, h = size
    time = 12.5 if kw else 0.0
    lw, lh = R.low_size(w, h, s)
    depth_floats, nbytes = R.scratch_layout(w, h, s)
    rng = np.random.default_rng(w)
    cams = [_moved("plain", size, yaw_deg=k)[0] for k in (0.0, 1.0)]
    hist = [_history(w=w, h=h), _history(w=w, h=h)]
    twin = [_history(w=w, h=h), _history(w=w, h=h)]
    for f, (cam, fmt, composite) in enumerate(zip(cams, ("rgba32f", "rgba16f"), (False, True))):
        p = TP.phase_of_frame(s, f + 1)
        fd, nf = _frames(node, cam, time)
        px = T.PIXEL_BYTES[T.format_id(fmt)]
        dbuf, dfmt, dpitch, decoded = _depth_buffer(S.depth_ground_sphere(cam), "d32f")
        src = N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch)
        prev_cam = cams[f - 1] if f else None
        opt = TP.options(s, p, 0.1, 0.1, None, f == 0, TP.prev_clip_from_view(fd, prev_cam) if f else None,
                         S.col_major(prev_cam.inv_projection) if f else None)
        scratch = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
        buf, dst = _target_buffer(rng, fmt, h, w, 0, composite)
        N.check(node._ctx, _temporal(lib, node, nf, src, opt, scratch, hist[1 - f] if f else None, hist[f], buf, fmt, 0, composite))
        torch.cuda.synchronize()
        name = node.kernel_name
        assert name.startswith("atmo_render_detail_kernel<" if kw else "atmo_render_kernel<"), name
        sc = scratch.cpu().numpy()
        low_depth, low_rgba = sc[:lw * lh].reshape(lh, lw), sc[depth_floats:].reshape(lh, lw, 4)
        # step 1: atmo_temporal_depth's, which is the statement's
        alone = torch.empty(lw * lh, dtype=torch.float32, device="cuda")
        N.check(node._ctx, lib.atmo_temporal_depth(node._ctx, C.byref(nf), C.byref(src), s, p, _ptr(alone), _stream()))
        torch.cuda.synchronize()
        assert low_depth.tobytes() == alone.cpu().numpy().tobytes() == TP.phase_depth(decoded, s, p).tobytes()
        # step 2: atmo_render of the statement's phase frame on that depth
        low_nf = _to_native_frame(TP.phase_frame(fd, s, p))
        ref = torch.empty((lh, lw, 4), dtype=torch.float32, device="cuda")
        N.check(node._ctx, lib.atmo_render(node._ctx, C.byref(low_nf), _ptr(alone), _ptr(ref), _stream()))
        torch.cuda.synchronize()
        assert node.kernel_name == name
        assert low_rgba.tobytes() == ref.cpu().numpy().tobytes()
        assert 0.05 < (low_rgba[..., 3] > 0).mean() < 0.999, "the frame must show the atmosphere and something else"
        # step 3: atmo_temporal_resolve of the two
        buf2 = _dev(_bits(dst).reshape(h, w * px))
        N.check(node._ctx, _resolve(lib, node, nf, src, opt, low_depth, low_rgba, twin[1 - f] if f else None, twin[f], buf2, fmt, 0, composite))
        assert buf.cpu().numpy().tobytes() == buf2.cpu().numpy().tobytes() != _bits(dst).tobytes()
        assert hist[f].cpu().numpy().tobytes() == twin[f].cpu().numpy().tobytes()
        # ... which is the statement's
        prev_parts = TP.unpack_history(twin[1 - f].cpu().numpy(), w, h) if f else None
        pixels, q0, age, det = TP.resolve(fd, decoded, low_depth, low_rgba, s, p, 0.1, 0.1, None, prev_parts, opt.prev_clip_from_view[:], opt.prev_inv_projection[:],
                                          reset=f == 0, details=True)
        assert buf.cpu().numpy().tobytes() == _bits(R.store(pixels, fmt, dst, composite)).reshape(h, w * px).tobytes()
        _assert_history(hist[f], (pixels, q0, age), w, h)
        if f:
            assert (det["path"] == TP.BILINEAR).mean() > 0.1      # the second frame does reuse the first


# ---- (d) a still camera ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_a_still_camera_fills_the_history_with_full_resolution_samples(lib, s):
    """After s^2 calls in sequence order, reset on the first, the history's rgba is the scatter of s^2 plain atmo_render draws of the phase frames, bit for
    bit, and the RGBA32F target the same bytes: every pixel holds a ray marched at its own centre."""
    node = _node("clouds_high")
    w, h = 37, 23
    cam = _camera("plain", w, h)
    fd, nf = _frames(node, cam)
    lw, lh = R.low_size(w, h, s)
    dbuf, dfmt, dpitch, decoded = _depth_buffer(S.depth_ground_sphere(cam), "d32f")
    src = N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch)
    scratch = torch.zeros(R.scratch_layout(w, h, s)[1], dtype=torch.uint8, device="cuda")
    hist = [_history(w=w, h=h), _history(w=w, h=h)]
    buf = torch.full((h, w * 16), SENTINEL, dtype=torch.uint8, device="cuda")
    want = np.zeros((h, w, 4), np.float32)
    want_age = np.zeros((h, w), np.int64)
    n = s * s
    for f in range(n):
        p = lib.atmo_temporal_phase(s, f)
        assert p == TP.phase_sequence(s)[f]
        ox, oy = TP.phase_offset(s, p)
        opt = TP.options(s, p, 0.1, 0.1, n, f == 0, TP.prev_clip_from_view(fd, cam), fd["inv_projection_matrix"])
        N.check(node._ctx, _temporal(lib, node, nf, src, opt, scratch, hist[(f + 1) & 1] if f else None, hist[f & 1], buf, "rgba32f", 0, False))
        # the plain draw of the phase frame
        ld = _dev(TP.phase_depth(decoded, s, p))
        ref = torch.empty((lh, lw, 4), dtype=torch.float32, device="cuda")
        low_nf = _to_native_frame(TP.phase_frame(fd, s, p))
        N.check(node._ctx, lib.atmo_render(node._ctx, C.byref(low_nf), _ptr(ld), _ptr(ref), _stream()))
        torch.cuda.synchronize()
        ys, xs = np.arange(oy, h, s), np.arange(ox, w, s)
        want[np.ix_(ys, xs)] = ref.cpu().numpy()[: len(ys), : len(xs)]
        want_age[np.ix_(ys, xs)] = n - 1 - f
    rgba, q, age = TP.unpack_history(hist[(n - 1) & 1].cpu().numpy(), w, h)
    assert rgba.tobytes() == want.tobytes()
    assert buf.cpu().numpy().tobytes() == want.tobytes()
    assert age.tolist() == want_age.tolist()
    assert q.tobytes() == TP.view_point(fd, decoded)[1].tobytes()
    assert 0.05 < (want[..., 3] > 0).mean() and len(np.unique(want[..., 3])) > 50


# ---- (e) the refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_entry_point_and_touches_nothing(lib):
    node = _node("no_clouds_8")
    w, h, s = 37, 23, 2
    cam = _camera("plain", w, h)
    fd, _ = _frames(node, cam)
    lw, lh = R.low_size(w, h, s)
    dbuf, dfmt, dpitch, _ = _depth_buffer(S.depth_ground_sphere(cam), "d32f")
    scratch = torch.zeros(R.scratch_layout(w, h, s)[1] + 16, dtype=torch.uint8, device="cuda")
    low = torch.zeros(lw * lh * 4 + 4, dtype=torch.float32, device="cuda")
    prev, cur = _history(w=w, h=h), _history(w=w, h=h)
    both = torch.full((2 * prev.numel() - 64,), SENTINEL, dtype=torch.uint8, device="cuda")      # two histories that overlap by 64 bytes
    buf = torch.full((h, w * 8), SENTINEL, dtype=torch.uint8, device="cuda")
    A, NODEV = N.ATMO_E_ARG, None

    def call(entry, frame=True, rect=None, depth=True, texels=None, dfmt_=dfmt, opt=True, scale=s, phase=1, tol=0.1, htol=0.1, max_age=8, reset=0,
             low_depth=0, low_rgba=0, scratch_off=0, prev_ptr="prev", cur_ptr="cur", target=True, pixels=None, fmt=1, pitch=0):
        f = _to_native_frame(dict(fd, rect=rect) if rect else fd)
        d = N.AtmoDepth(dbuf.data_ptr() if texels is None else texels, dfmt_, dpitch)
        t = N.AtmoTarget(buf.data_ptr() if pixels is None else pixels, fmt, pitch)
        o = TP.options(scale, phase, tol, htol, max_age, reset, TP.prev_clip_from_view(fd, cam), fd["inv_projection_matrix"])
        o.max_age = max_age
        ptrs = {"prev": prev.data_ptr(), "cur": cur.data_ptr(), None: None, "odd": cur.data_ptr() + 8, "overlap": both.data_ptr() + prev.numel() - 64,
                "both": both.data_ptr()}
        f_, d_, t_, o_ = C.byref(f) if frame else None, C.byref(d) if depth else None, C.byref(t) if target else None, C.byref(o) if opt else None
        if entry == "atmo_temporal_depth":
            rc = lib.atmo_temporal_depth(node._ctx, f_, d_, scale, phase, C.c_void_p(low.data_ptr() + low_depth if low_depth is not None else None), _stream())
        elif entry == "atmo_temporal_resolve":
            rc = lib.atmo_temporal_resolve(node._ctx, f_, d_, o_, C.c_void_p(low.data_ptr() + low_depth if low_depth is not None else None),
                                           C.c_void_p(low.data_ptr() + 16 + low_rgba if low_rgba is not None else None), C.c_void_p(ptrs[prev_ptr]),
                                           C.c_void_p(ptrs[cur_ptr]), t_, 0, _stream())
        else:
            rc = lib.atmo_render_temporal_target(node._ctx, f_, d_, o_, C.c_void_p(scratch.data_ptr() + scratch_off if scratch_off is not None else None),
                                                 C.c_void_p(ptrs[prev_ptr]), C.c_void_p(ptrs[cur_ptr]), t_, 0, _stream())
        return rc, (lib.atmo_last_error_string(node._ctx) or b"").decode()

    common = [("null frame", dict(frame=False)), ("null target", dict(target=False)), ("unknown target format", dict(fmt=3)), ("null target pixels", dict(pixels=0)),
              ("row_pitch_bytes", dict(pitch=w * 8 - 8)), ("null opt", dict(opt=False)), ("scale must be 2 or 4", dict(scale=3)),
              ("depth_tolerance", dict(tol=-1.0)), ("depth_tolerance", dict(tol=float("nan"))), ("whole viewport", dict(rect=(0, 0, w - 1, h))),
              ("phase must be 0 .. scale^2 - 1", dict(phase=4)), ("phase must be 0 .. scale^2 - 1", dict(phase=-1)), ("history_tolerance", dict(htol=-0.5)),
              ("history_tolerance", dict(htol=float("inf"))), ("max_age must be 1 .. 255", dict(max_age=0)), ("max_age must be 1 .. 255", dict(max_age=256))]
    history = [("null history_cur_dev", dict(cur_ptr=None)), ("16-byte aligned", dict(cur_ptr="odd")), ("overlap", dict(prev_ptr="both", cur_ptr="overlap")),
               ("overlap", dict(prev_ptr="cur")), ("null history_prev_dev without reset", dict(prev_ptr=None))]
    depth = [("null depth", dict(depth=False)), ("unknown depth format", dict(dfmt_=3)), ("null depth texels", dict(texels=0))]
    checks = {
        "atmo_temporal_depth": [("null frame", dict(frame=False)), ("scale must be 2 or 4", dict(scale=3)), ("phase must be 0 .. scale^2 - 1", dict(phase=4)),
                                ("whole viewport", dict(rect=(0, 0, w - 1, h))), ("null low_depth_dev", dict(low_depth=None)),
                                ("4-byte aligned", dict(low_depth=2))] + depth,
        "atmo_temporal_resolve": common + [("null low_depth_dev or low_rgba_dev", dict(low_depth=None)), ("null low_depth_dev or low_rgba_dev", dict(low_rgba=None)),
                                           ("16-byte aligned", dict(low_rgba=8))] + history + depth,
        "atmo_render_temporal_target": common + [("null scratch_dev", dict(scratch_off=None)), ("16-byte aligned", dict(scratch_off=8))] + history + depth,
    }
    for entry, cases in checks.items():
        for k, (what, kw) in enumerate(cases):
            rc, said = call(entry, **kw)
            assert rc == A and entry + ":" in said and what in said, (entry, kw, rc, said)
            for _, later in cases[k + 1:k + 2]:      # two wrong arguments: the one the header lists first
                rc, said = call(entry, **dict(later, **kw))
                assert rc == A and what in said, (entry, kw, later, said)
    torch.cuda.synchronize()
    for t in (buf, prev, cur, both):
        assert bool((t == SENTINEL).all())
    assert not bool(low.any()) and not bool(scratch.any())
    # a null previous history is fine under reset, and a well-formed call draws
    rc, said = call("atmo_render_temporal_target", prev_ptr=None, reset=1)
    torch.cuda.synchronize()
    assert rc == N.ATMO_OK and not bool((buf == SENTINEL).all()) and bool((prev == SENTINEL).all())
    assert TP.unpack_history(cur.cpu().numpy(), w, h)[2].max() == 255


# ---- (f) the binding ----------------------------------------------------------------------------------------------------------------------------------------
def test_render_temporal_writes_the_c_calls_bytes_over_three_frames(lib):
    node = _node("clouds_high")
    w, h, s, tol, htol = 64, 40, 2, 0.05, 0.2
    cams = [_moved("plain", (w, h), yaw_deg=float(k))[0] for k in range(3)]
    scratch = torch.zeros(R.scratch_layout(w, h, s)[1], dtype=torch.uint8, device="cuda")
    mine = [_history(w=w, h=h), _history(w=w, h=h)]
    history = None
    rng = np.random.default_rng(6)
    reused = 0
    for f, cam in enumerate(cams):
        fd, nf = _frames(node, cam)
        depth = S.depth_ground_sphere(cam)
        dbuf, dfmt, dpitch, _ = _depth_buffer(depth, "d32f")
        opt = TP.options(s, TP.phase_of_frame(s, f), tol, htol, None, f == 0, TP.prev_clip_from_view(fd, cams[f - 1]) if f else None,
                         S.col_major(cams[f - 1].inv_projection) if f else None)
        buf, _ = _target_buffer(rng, "rgba16f", h, w, 0, False)
        N.check(node._ctx, _temporal(lib, node, nf, N.AtmoDepth(dbuf.data_ptr(), dfmt, dpitch), opt, scratch, mine[(f + 1) & 1] if f else None, mine[f & 1], buf,
                                     "rgba16f", 0, False))
        out, history = node.render_temporal(cam, _dev(depth), scale=s, history=history, depth_tolerance=tol, history_tolerance=htol)
        torch.cuda.synchronize()
        assert out.dtype == torch.float16 and tuple(out.shape) == (h, w, 4) and history.frame_index == f + 1
        assert _bits(out.cpu().numpy()).tobytes() == buf.cpu().numpy().tobytes()
        got, want = history.parts(), TP.unpack_history(mine[f & 1].cpu().numpy(), w, h)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        reused += int(((want[2] > 0) & (want[2] < 255)).sum())
    assert reused > w * h // 2                                            # frames two and three do reuse their predecessors
    # a history made for another viewport or scale starts over
    cam = _camera("plain", 37, 23)
    _, other = node.render_temporal(cam, _dev(S.depth_ground_sphere(cam)), scale=s, history=history)
    assert other is not history and other.frame_index == 1 and set(np.unique(other.parts()[2])) == {0, 255}
    _, other4 = node.render_temporal(cams[0], _dev(S.depth_ground_sphere(cams[0])), scale=4, history=history)
    assert other4 is not history
    with pytest.raises(ValueError):
        node.render_temporal(cams[0], _dev(S.depth_ground_sphere(cams[0])), scale=3)
    with pytest.raises(ValueError):
        node.render_temporal(cams[0], _dev(S.depth_ground_sphere(cams[0])), composite=True)
