"""What the Python binding (godot_atmosphere_shader_amd/planet_atmosphere.py) hands to libatmo_hip.so, recorded without a device: for every public draw
method, which C entry point is reached and with which arguments, and which exception every bad argument raises.

The node is made with object.__new__ and carries a recorder in place of the library; tensors are CPU tensors of a torch.Tensor subclass that says
is_cuda (addresses, strides and dtypes are the real ones); the stream is always given, as an int or as an object with `cuda_stream`.  The expectations are
this file's own tables, written from the methods' docstrings and from include/atmo*.h: ABI (the argument lists), SINGLE and BATCH (which entry point
serves which draw), `_colour` (which AtmoTarget a tensor means) and the message constants at the end.  Run it after any change to the binding."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.overrides import TorchFunctionMode

from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import planet_atmosphere as PA
from godot_atmosphere_shader_amd import scene as S

W, H = 24, 10              # view 0
W2, H2 = 16, 12            # view 1: another viewport size
RECT, RECT2 = (3, 2, 19, 9), (1, 0, 16, 7)
CTX, STREAM, TIME = 0xC0DE, 0x5EED, 0.25
R_PLANET, H_ATMO = 100.0, 8.0
TRANSFORM = np.array([[0.0, 0.0, 1.0, 5.0], [0.0, 1.0, 0.0, -7.0], [-1.0, 0.0, 0.0, 11.0], [0.0, 0.0, 0.0, 1.0]])   # a quarter turn and an offset

# the argument lists of the entry points, from include/atmo.h, atmo_scene.h, atmo_target.h, atmo_views.h, atmo_views_target.h, atmo_views_proxy.h
ABI = {
    "atmo_bake_optical_depth": ("ctx", "stream"),
    "atmo_render": ("ctx", "frame", "depth", "colour", "stream"),
    "atmo_render_composite": ("ctx", "frame", "depth", "colour", "stream"),
    "atmo_render_target": ("ctx", "frame", "depth", "target", "composite", "stream"),
    "atmo_render_proxy": ("ctx", "frame", "model", "box_size", "depth", "colour", "stream"),
    "atmo_render_proxy_composite": ("ctx", "frame", "model", "box_size", "depth", "colour", "stream"),
    "atmo_render_proxy_target": ("ctx", "frame", "model", "box_size", "depth", "target", "composite", "stream"),
    "atmo_render_views": ("ctx", "views", "n", "composite", "stream"),
    "atmo_render_views_target": ("ctx", "views_target", "n", "composite", "stream"),
    "atmo_render_views_proxy": ("ctx", "views", "n", "model", "box_size", "composite", "stream"),
    "atmo_render_views_proxy_target": ("ctx", "views_target", "n", "model", "box_size", "composite", "stream"),
}
# (through the box proxy?, an AtmoTarget?, composite?) -> the entry point of one draw; the *_target entry points take composite as an argument
SINGLE = {
    (False, False, False): "atmo_render", (False, False, True): "atmo_render_composite",
    (False, True, False): "atmo_render_target", (False, True, True): "atmo_render_target",
    (True, False, False): "atmo_render_proxy", (True, False, True): "atmo_render_proxy_composite",
    (True, True, False): "atmo_render_proxy_target", (True, True, True): "atmo_render_proxy_target",
}
# (through the box proxy?, AtmoTargets?) -> the entry point of a view batch
BATCH = {(False, False): "atmo_render_views", (False, True): "atmo_render_views_target",
         (True, False): "atmo_render_views_proxy", (True, True): "atmo_render_views_proxy_target"}
# public single draws: name -> (proxy, composite); "draw@near" / "draw@far" are `draw` in the two modes `_process` sets
SINGLE_METHODS = {"render": (False, False), "render_composite": (False, True), "render_proxy": (True, False), "render_proxy_composite": (True, True),
                  "draw@near": (False, True), "draw@far": (True, True)}
BATCH_METHODS = {"render_views": (False, False), "render_views+composite": (False, True), "render_views_proxy": (True, False),
                 "render_views_proxy+composite": (True, True), "draw_views@near": (False, True), "draw_views@far": (True, True)}


class FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: everything else about it is real."""

    @property
    def is_cuda(self):
        return True


class _AllocateAsCuda(TorchFunctionMode):
    """The tensors a draw allocates itself (torch.empty / torch.zeros on the depth's device, here the CPU) become FakeCuda as well."""

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        return out.as_subclass(FakeCuda) if func in (torch.empty, torch.zeros) else out


class _Stream:
    cuda_stream = STREAM


class Recorder:
    """Stands for libatmo_hip.so: every atmo_* call is stored by value at call time and answers ATMO_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("atmo_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, tuple(_by_value(a) for a in args)))
            return N.ATMO_OK
        return entry

    def draws(self):
        """The recorded calls, decoded by ABI into {argument name: value} (a context being destroyed is not a draw)."""
        return [(name, _decode(name, args)) for name, args in self.calls if name != "atmo_destroy"]


def library_without(*names):
    """A Recorder that stands for a library without the symbols `names`: an older build, which the optional headers' entry points are detected against."""
    class Old(Recorder):
        def __getattr__(self, name):
            if name in names:
                raise AttributeError(name)
            return super().__getattr__(name)

    return Old()


def _by_value(a):
    if isinstance(a, (C.c_void_p, C.c_float)):
        return a.value or 0
    if isinstance(a, (C.Array, C.Structure)):
        return bytes(a)
    if hasattr(a, "_obj"):      # byref(structure)
        return bytes(a._obj)
    return a


def _frame_fields(raw):
    f = N.AtmoFrame.from_buffer_copy(raw)
    return dict(rect=(f.x0, f.y0, f.x1, f.y1), viewport=(f.viewport_w, f.viewport_h), bytes=bytes(raw))


def _target_fields(raw):
    t = N.AtmoTarget.from_buffer_copy(raw)
    return (t.pixels or 0, t.format, t.row_pitch_bytes)


def _decode(name, args):
    kinds = ABI[name]
    assert len(kinds) == len(args), (name, len(args))
    out = {}
    for kind, a in zip(kinds, args):
        if kind == "frame":
            a = _frame_fields(a)
        elif kind == "target":
            a = _target_fields(a)
        elif kind == "model":
            a = tuple(np.frombuffer(a, dtype=np.float32).tolist())
        elif kind in ("views", "views_target"):
            struct = N.AtmoView if kind == "views" else N.AtmoViewTarget
            views = (struct * (len(a) // C.sizeof(struct))).from_buffer_copy(a)
            a = [dict(frame=_frame_fields(bytes(v.frame)), depth=v.depth_dev or 0,
                      **(dict(colour=v.rgba_dev or 0) if kind == "views" else dict(target=_target_fields(bytes(v.target))))) for v in views]
        out[kind] = a
    return out


def _node(mode=PA.MODE_FAR, ctx=CTX, lib=None, transform=TRANSFORM):
    node = object.__new__(PA.PlanetAtmosphere)
    node._lib = lib if lib is not None else Recorder()
    node._ctx = C.c_void_p(ctx)
    node._params = {"u_sun_position": (50.0, 20.0, 400.0)}
    node._planet_radius, node._atmosphere_height = R_PLANET, H_ATMO
    node.global_transform = transform
    node._mode = mode
    node._bake_pending = node._uses_baked_optical_depth = False
    return node


def _cam(w=W, h=H, near=0.25):
    return S.Camera(w, h, (31.0, 17.0, 420.0), (0.0, 0.0, 0.0), near=near)


def _fake(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)


def _depth(cam):
    return _fake((cam.height, cam.width))


COLOURS = ["f32", "f32_pitched", "f16", "u8", "u8:bgra8_srgb", "u8_pitched:bgra8"]
_FORMATS = {"f32": N.TARGET_RGBA32F, "f16": N.TARGET_RGBA16F, "u8": N.TARGET_RGBA8_UNORM, "bgra8_srgb": N.TARGET_BGRA8_SRGB, "bgra8": N.TARGET_BGRA8_UNORM,
            "rgba8_srgb": N.TARGET_RGBA8_SRGB}
_DTYPES = {"f32": torch.float32, "f16": torch.float16, "u8": torch.uint8}
PAD, LEFT = 5, 2           # a pitched tensor: columns LEFT .. LEFT + cols of an image PAD columns wider


def _colour(kind, rows, cols):
    """(tensor, target name or None, what the library must be given: the tensor's address for the float entry points -- a contiguous float32 tensor --,
    else the AtmoTarget's (pixels, format, row pitch in bytes) -- atmo_target.h: the dtype says the format unless `target` names one)."""
    layout, _, name = kind.partition(":")
    dt, pitched = layout.split("_")[0], layout.endswith("_pitched")
    image = _fake((rows, cols + PAD if pitched else cols, 4), _DTYPES[dt])
    size = 4 * image.element_size()
    t = image[:, LEFT:LEFT + cols] if pitched else image
    pixels = image.data_ptr() + (LEFT * size if pitched else 0)
    if kind == "f32":
        return t, None, pixels
    return t, name or None, (pixels, _FORMATS[name or dt], image.shape[1] * size)


def _frame(node, cam, rect):
    """The frame a draw of `rect` of `cam` passes (make_frame / _to_native_frame are not under test here), and its rect and viewport stated apart."""
    raw = bytes(PA._to_native_frame(node.make_frame(cam, TIME, rect)))
    return dict(rect=tuple(rect) if rect is not None else (0, 0, cam.width, cam.height), viewport=(cam.width, cam.height), bytes=raw)


def _model(transform=TRANSFORM):
    return tuple(float(np.float32(transform[r][c])) for c in range(4) for r in range(4))   # column-major


def _box(near):
    return C.c_float(1.75 * (R_PLANET + H_ATMO + near) * 1.1).value   # planet_atmosphere.gd:300-321, as the C float the library receives


def _streams():
    return [pytest.param(STREAM, id="int"), pytest.param(_Stream(), id="obj")]


def _single(node, method, cam, depth, colour, **kw):
    name, _, mode = method.partition("@")
    if mode:
        node._mode = PA.MODE_NEAR if mode == "near" else PA.MODE_FAR
    return getattr(node, name)(cam, depth, colour, time=TIME, **kw)


def _expect_single(node, method, cam, depth, rect, given, box=None):
    proxy, composite = SINGLE_METHODS[method]
    packed = isinstance(given, tuple)
    want = dict(ctx=node._ctx.value, frame=_frame(node, cam, rect), depth=depth.data_ptr(), stream=STREAM)
    want["target" if packed else "colour"] = given
    if packed:
        want["composite"] = int(composite)
    if proxy:
        want.update(model=_model(), box_size=_box(cam.near) if box is None else box)
    return (SINGLE[(proxy, packed, composite)], want)


@pytest.mark.parametrize("stream", _streams())
@pytest.mark.parametrize("rect", [None, RECT], ids=["whole", "rect"])
@pytest.mark.parametrize("kind", COLOURS)
@pytest.mark.parametrize("method", list(SINGLE_METHODS))
def test_single_draw_reaches_its_entry_point(method, kind, rect, stream):
    node, cam = _node(), _cam()
    depth = _depth(cam)
    x0, y0, x1, y1 = rect or (0, 0, W, H)
    rows, cols = (H, W) if SINGLE_METHODS[method][1] else (y1 - y0, x1 - x0)   # a composite blends into the whole viewport's buffer
    t, target, given = _colour(kind, rows, cols)
    kw = {} if target is None else {"target": target}
    assert _single(node, method, cam, depth, t, rect=rect, stream=stream, **kw) is t
    assert node._lib.draws() == [_expect_single(node, method, cam, depth, rect, given)]


@pytest.mark.parametrize("rect", [None, RECT], ids=["whole", "rect"])
@pytest.mark.parametrize("target,dtype,fmt", [(None, torch.float32, None), ("rgba16f", torch.float16, N.TARGET_RGBA16F),
                                              ("rgba8_srgb", torch.uint8, N.TARGET_RGBA8_SRGB)])
@pytest.mark.parametrize("method", ["render", "render_proxy"])
def test_single_draw_allocates_its_output(method, target, dtype, fmt, rect):
    node, cam = _node(), _cam()
    depth = _depth(cam)
    x0, y0, x1, y1 = rect or (0, 0, W, H)
    with _AllocateAsCuda():
        out = getattr(node, method)(cam, depth, rect=rect, stream=STREAM, time=TIME, target=target)
    assert out.dtype == dtype and tuple(out.shape) == (y1 - y0, x1 - x0, 4)
    if method == "render_proxy":
        assert not out.any()   # the box's misses are left as they were: zero-filled (render's own output is torch.empty: nothing to assert)
    given = out.data_ptr() if fmt is None else (out.data_ptr(), fmt, (x1 - x0) * 4 * out.element_size())
    assert node._lib.draws() == [_expect_single(node, method, cam, depth, rect, given)]


@pytest.mark.parametrize("method", ["render_proxy", "render_proxy_composite"])
def test_proxy_draw_takes_a_box_size(method):
    node, cam = _node(), _cam()
    depth = _depth(cam)
    t, _, given = _colour("f16", H, W)
    getattr(node, method)(cam, depth, t, stream=STREAM, time=TIME, box_size=37.5)
    assert node._lib.draws() == [_expect_single(node, method, cam, depth, None, given, box=37.5)]


def test_render_raw_and_render_prepared_are_atmo_render():
    node, cam = _node(), _cam()
    frame = node.make_frame(cam, TIME, RECT)
    node.render_raw(frame, 0x1000, 0x2000, STREAM)
    native = node.prepare_frame(cam, TIME, RECT)
    assert isinstance(native, N.AtmoFrame)
    node.render_prepared(native, 0x3000, 0x4000, STREAM)
    node.render_prepared(native, 0x3000, 0x4000)
    want = dict(ctx=CTX, frame=_frame(node, cam, RECT), stream=STREAM)
    assert node._lib.draws() == [("atmo_render", dict(want, depth=0x1000, colour=0x2000)), ("atmo_render", dict(want, depth=0x3000, colour=0x4000)),
                                 ("atmo_render", dict(want, depth=0x3000, colour=0x4000, stream=0))]


@pytest.mark.parametrize("kind", ["f32", "u8:bgra8_srgb"])
def test_draw_atmospheres_draws_every_node_in_its_mode_farthest_first(kind):
    lib, cam = Recorder(), _cam()
    at = lambda z: np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, z], [0, 0, 0, 1.0]])   # noqa: E731
    near = _node(PA.MODE_NEAR, 0xA, lib, at(300.0))     # 120 from the camera
    far = _node(PA.MODE_FAR, 0xB, lib, at(-900.0))      # 1320 from it
    depth = _depth(cam)
    t, target, given = _colour(kind, H, W)
    kw = {} if target is None else {"target": target}
    assert PA.draw_atmospheres([near, far], cam, depth, t, stream=_Stream(), time=TIME, **kw) is t
    packed = isinstance(given, tuple)
    got = lib.draws()
    assert [(name, a["ctx"]) for name, a in got] == [(SINGLE[(True, packed, True)], 0xB), (SINGLE[(False, packed, True)], 0xA)]
    for (_, a), node in zip(got, (far, near)):
        assert a["frame"] == _frame(node, cam, None) and a["depth"] == depth.data_ptr() and a["stream"] == STREAM
        assert a["target" if packed else "colour"] == given and (not packed or a["composite"] == 1)
    assert got[0][1]["model"] == _model(at(-900.0)) and got[0][1]["box_size"] == _box(cam.near)


# ---- view batches ------------------------------------------------------------------------------------------------------------------------------------
def _batch(node, method, cams, depths, outs, **kw):
    name, _, mode = method.partition("@")
    name, _, comp = name.partition("+")
    if mode:
        node._mode = PA.MODE_NEAR if mode == "near" else PA.MODE_FAR
    if comp:
        kw["composite"] = True
    return getattr(node, name)(cams, depths, outs, time=TIME, **kw)


def _expect_batch(node, method, cams, depths, rects, givens, box=None):
    """`givens`: per view what `_colour` states.  One float32 tensor with a pitch makes the whole batch a target batch, in which a contiguous float32
    tensor is an RGBA32F target of pitch 0 (atmo_target.h: 0 = tight)."""
    proxy, composite = BATCH_METHODS[method]
    packed = any(isinstance(g, tuple) for g in givens)
    views = []
    for i, (cam, depth, g) in enumerate(zip(cams, depths, givens)):
        v = dict(frame=_frame(node, cam, rects[i] if rects is not None else None), depth=depth.data_ptr())
        if packed:
            v["target"] = g if isinstance(g, tuple) else (g, N.TARGET_RGBA32F, 0)
        else:
            v["colour"] = g
        views.append(v)
    want = {"ctx": CTX, "views_target" if packed else "views": views, "n": len(cams), "composite": int(composite), "stream": STREAM}
    if proxy:
        want.update(model=_model(), box_size=_box(cams[0].near) if box is None else box)
    return (BATCH[(proxy, packed)], want)


def _views(n):
    cams = [_cam(), _cam(W2, H2, near=0.5)][:n]
    return cams, [_depth(c) for c in cams], [RECT, RECT2][:n]


def _view_colours(kinds, cams, rects, composite):
    out = []
    for kind, cam, rect in zip(kinds, cams, rects if rects is not None else [None] * len(cams)):
        x0, y0, x1, y1 = rect or (0, 0, cam.width, cam.height)
        out.append(_colour(kind, *((cam.height, cam.width) if composite else (y1 - y0, x1 - x0))))
    return out


@pytest.mark.parametrize("stream", _streams())
@pytest.mark.parametrize("with_rects", [False, True], ids=["whole", "rects"])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("kind", COLOURS)
@pytest.mark.parametrize("method", list(BATCH_METHODS))
def test_view_batch_reaches_its_entry_point(method, kind, n, with_rects, stream):
    node = _node()
    cams, depths, rects = _views(n)
    rects = rects if with_rects else None
    cols = _view_colours([kind] * n, cams, rects, BATCH_METHODS[method][1])
    kw = {} if cols[0][1] is None else {"target": cols[0][1]}
    got = _batch(node, method, cams, depths, [c[0] for c in cols], rects=rects, stream=stream, **kw)
    assert len(got) == n and all(g is c[0] for g, c in zip(got, cols))
    assert node._lib.draws() == [_expect_batch(node, method, cams, depths, rects, [c[2] for c in cols])]


@pytest.mark.parametrize("order", [("f32", "f32_pitched"), ("f32_pitched", "f32")], ids=["tight_first", "pitched_first"])
@pytest.mark.parametrize("method", list(BATCH_METHODS))
def test_mixed_float_batch_is_a_target_batch_of_rgba32f(method, order):
    node = _node()
    cams, depths, rects = _views(2)
    cols = _view_colours(order, cams, rects, BATCH_METHODS[method][1])
    _batch(node, method, cams, depths, [c[0] for c in cols], rects=rects, stream=STREAM)
    (name, args), = node._lib.draws()
    assert name == BATCH[(BATCH_METHODS[method][0], True)] and [v["target"][1] for v in args["views_target"]] == [N.TARGET_RGBA32F] * 2
    assert (name, args) == _expect_batch(node, method, cams, depths, rects, [c[2] for c in cols])


@pytest.mark.parametrize("method", list(BATCH_METHODS))
def test_a_batch_of_no_views_calls_nothing(method):
    node = _node()
    assert _batch(node, method, [], [], [], stream=STREAM) == []
    assert node._lib.draws() == []


@pytest.mark.parametrize("with_rects", [False, True], ids=["whole", "rects"])
@pytest.mark.parametrize("target,dtype,fmt", [(None, torch.float32, None), ("rgba16f", torch.float16, N.TARGET_RGBA16F),
                                              ("bgra8", torch.uint8, N.TARGET_BGRA8_UNORM)])
@pytest.mark.parametrize("method", ["render_views", "render_views_proxy"])
def test_view_batch_allocates_its_outputs(method, target, dtype, fmt, with_rects):
    node = _node()
    cams, depths, rects = _views(2)
    rects = rects if with_rects else None
    with _AllocateAsCuda():
        outs = getattr(node, method)(cams, depths, rects=rects, stream=STREAM, time=TIME, target=target)
    givens = []
    for out, cam, rect in zip(outs, cams, rects or [None, None]):
        x0, y0, x1, y1 = rect or (0, 0, cam.width, cam.height)
        assert out.dtype == dtype and tuple(out.shape) == (y1 - y0, x1 - x0, 4)
        if method == "render_views_proxy":
            assert not out.any()
        givens.append(out.data_ptr() if fmt is None else (out.data_ptr(), fmt, (x1 - x0) * 4 * out.element_size()))
    assert node._lib.draws() == [_expect_batch(node, method, cams, depths, rects, givens)]


def test_proxy_batch_takes_a_box_size():
    node = _node()
    cams, depths, rects = _views(2)
    cols = _view_colours(["u8", "u8"], cams, None, False)
    node.render_views_proxy(cams, depths, [c[0] for c in cols], stream=STREAM, time=TIME, box_size=41.0)
    assert node._lib.draws() == [_expect_batch(node, "render_views_proxy", cams, depths, None, [c[2] for c in cols], box=41.0)]


@pytest.mark.parametrize("composite", [False, True])
@pytest.mark.parametrize("proxy", [False, True])
@pytest.mark.parametrize("targets", [False, True])
@pytest.mark.parametrize("n", [0, 2])
def test_prepared_view_batches(n, targets, proxy, composite):
    """prepare_views[_target] fills the argument block from raw addresses; the four render_views*_prepared enqueue it with what they are given."""
    node = _node()
    cams, _, rects = _views(n)
    depth_ptrs, outs = [0x1000, 0x2000][:n], [0x3000, 0x4000][:n]
    if targets:
        given = [(0x3000, N.TARGET_RGBA16F, 512), (0x4000, N.TARGET_RGBA16F, 0)][:n]
        views = node.prepare_views_target(cams, depth_ptrs, [N.AtmoTarget(*g) for g in given], rects, TIME)
        assert isinstance(views, C.Array) and views._type_ is N.AtmoViewTarget and len(views) == max(n, 1)
    else:
        given = outs
        views = node.prepare_views(cams, depth_ptrs, outs, rects, TIME)
        assert isinstance(views, C.Array) and views._type_ is N.AtmoView and len(views) == max(n, 1)
    model = node.proxy_model()
    fn = getattr(node, "render_views" + ("_proxy" if proxy else "") + ("_target" if targets else "") + "_prepared")
    fn(views, n, *((model, 33.0) if proxy else ()), composite, STREAM)
    fn(views, n, *((model, 33.0) if proxy else ()))                       # the defaults: plain, the null stream
    want = [dict(frame=_frame(node, c, r), depth=d, **({"target": g} if targets else {"colour": g})) for c, r, d, g in zip(cams, rects, depth_ptrs, given)]
    blank = N.AtmoViewTarget() if targets else N.AtmoView()
    if n == 0:   # the block of an empty batch holds one zeroed entry (ctypes has no empty arrays to pass)
        want = [dict(frame=_frame_fields(bytes(blank.frame)), depth=0, **({"target": (0, 0, 0)} if targets else {"colour": 0}))]
    args = {"ctx": CTX, "views_target" if targets else "views": want, "n": n, "composite": int(composite), "stream": STREAM}
    if proxy:
        args.update(model=_model(), box_size=33.0)
    assert node._lib.draws() == [(BATCH[(proxy, targets)], args), (BATCH[(proxy, targets)], dict(args, composite=0, stream=0))]


# ---- the optical-depth bake goes in front of the draw, on the draw's stream ----------------------------------------------------------------------------
def _any_draw(node, method):
    """One valid call of every public draw method (the raw and prepared ones included)."""
    cam = _cam()
    depth = _depth(cam)
    if method in SINGLE_METHODS:
        return _single(node, method, cam, depth, _colour("f16" if SINGLE_METHODS[method][1] else "f32", H, W)[0], stream=_Stream())
    if method in BATCH_METHODS:
        cams, depths, _ = _views(2)
        cols = _view_colours(["f32", "f32_pitched"] if "proxy" in method else ["f32", "f32"], cams, None, BATCH_METHODS[method][1])
        return _batch(node, method, cams, depths, [c[0] for c in cols], stream=STREAM)
    if method == "draw_atmospheres":
        return PA.draw_atmospheres([node], cam, depth, _colour("u8", H, W)[0], stream=STREAM)
    if method == "render_raw":
        return node.render_raw(node.make_frame(cam), 0x1000, 0x2000, STREAM)
    if method == "render_prepared":
        return node.render_prepared(node.prepare_frame(cam), 0x1000, 0x2000, STREAM)
    cams, _, _ = _views(2)
    if "target" in method:
        views = node.prepare_views_target(cams, [0x1000, 0x2000], [N.AtmoTarget(0x3000, N.TARGET_RGBA8_UNORM, 0), N.AtmoTarget(0x4000, N.TARGET_RGBA8_UNORM, 0)])
    else:
        views = node.prepare_views(cams, [0x1000, 0x2000], [0x3000, 0x4000])
    return getattr(node, method)(views, 2, *((node.proxy_model(), 30.0) if "proxy" in method else ()), False, STREAM)


EVERY_DRAW = list(SINGLE_METHODS) + list(BATCH_METHODS) + ["draw_atmospheres", "render_raw", "render_prepared", "render_views_prepared",
                                                            "render_views_target_prepared", "render_views_proxy_prepared",
                                                            "render_views_proxy_target_prepared"]


@pytest.mark.parametrize("method", EVERY_DRAW)
def test_a_pending_bake_goes_in_front_of_the_draw_once(method):
    node = _node()
    node._bake_pending = node._uses_baked_optical_depth = True
    _any_draw(node, method)
    first = node._lib.draws()
    assert len(first) == 2 and first[0] == ("atmo_bake_optical_depth", dict(ctx=CTX, stream=STREAM)) and first[1][0] != "atmo_bake_optical_depth"
    assert first[1][1]["stream"] == STREAM and node._bake_pending is False and node._params["u_optical_depth_texture"] == "<baked on device>"
    node._lib.calls.clear()
    _any_draw(node, method)
    assert [name for name, _ in node._lib.draws()] == [first[1][0]]          # nothing pending: the draw alone


@pytest.mark.parametrize("method", EVERY_DRAW)
def test_no_bake_for_a_shader_without_the_lut(method):
    node = _node()
    node._bake_pending = True      # (a direct-light or v1 context: requested, never used)
    _any_draw(node, method)
    assert len(node._lib.draws()) == 1 and node._lib.draws()[0][0] != "atmo_bake_optical_depth" and node._bake_pending is False


# ---- refusals: exception class and text, one bad argument at a time; nothing reaches the library ------------------------------------------------------
DEPTH_KIND = "depth must be a contiguous CUDA float32 tensor"
DEPTH_SHAPE = "depth must have shape (viewport_h, viewport_w)"
DEPTH_BOTH = "depth must be a contiguous CUDA float32 tensor of shape (viewport_h, viewport_w)"
# `render` and the view batches tell the tensor's kind (TypeError) from its shape (ValueError); the other single draws raise one TypeError for both
DEPTH_ERRORS = {"render": ((TypeError, DEPTH_KIND), (ValueError, DEPTH_SHAPE))}
DEPTH_ERRORS.update({m: ((TypeError, DEPTH_BOTH), (TypeError, DEPTH_BOTH)) for m in SINGLE_METHODS if m != "render"})
DEPTH_ERRORS.update({m: ((TypeError, "view 1: " + DEPTH_KIND), (ValueError, "view 1: " + DEPTH_SHAPE)) for m in BATCH_METHODS})


def _bad_depths(cam):
    h, w = cam.height, cam.width
    yield "cpu", torch.zeros((h, w)), 0
    yield "float64", _fake((h, w), torch.float64), 0
    yield "strided", _fake((h, 2 * w))[:, ::2], 0
    yield "numpy", np.zeros((h, w), dtype=np.float32), 0
    yield "none", None, 0
    yield "transposed_shape", _fake((w, h)), 1
    yield "flat", _fake((h * w,)), 1


def _raises(node, exc, message, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert type(e.value) is exc and str(e.value) == message
    assert node._lib.draws() == []


@pytest.mark.parametrize("bad", ["cpu", "float64", "strided", "numpy", "none", "transposed_shape", "flat"])
@pytest.mark.parametrize("method", list(SINGLE_METHODS) + list(BATCH_METHODS))
def test_a_bad_depth_is_refused(method, bad):
    node = _node()
    if method in SINGLE_METHODS:
        cam = _cam()
        depth, which = next((d, k) for name, d, k in _bad_depths(cam) if name == bad)
        exc, message = DEPTH_ERRORS[method][which]
        _raises(node, exc, message, _single, node, method, cam, depth, _colour("f32", H, W)[0], stream=STREAM)
    else:
        cams, depths, _ = _views(2)
        depths[1], which = next((d, k) for name, d, k in _bad_depths(cams[1]) if name == bad)
        exc, message = DEPTH_ERRORS[method][which]
        cols = _view_colours(["f32", "f32"], cams, None, BATCH_METHODS[method][1])
        _raises(node, exc, message, _batch, node, method, cams, depths, [c[0] for c in cols], stream=STREAM)


def _what(method, view=None):
    composite = (SINGLE_METHODS if view is None else BATCH_METHODS)[method][1]
    return ("" if view is None else f"view {view}: ") + ("scene_rgba" if composite else "out")


def _bad_colours(what, rows, cols):
    shape = f"{what} must be a CUDA float32, float16 or uint8 tensor of shape ({rows}, {cols}, 4)"
    stride = f"{what}: the pixels of a row must be contiguous and the row stride at least a row (a row pitch is the only stride supported)"
    yield "one_row_short", _fake((rows - 1, cols, 4)), None, shape
    yield "three_channels", _fake((rows, cols, 3)), None, shape
    yield "float64", _fake((rows, cols, 4), torch.float64), None, shape
    yield "int32", _fake((rows, cols, 4), torch.int32), None, shape
    yield "cpu", torch.zeros((rows, cols, 4)), None, shape
    yield "numpy", np.zeros((rows, cols, 4), dtype=np.float32), None, shape
    yield "every_other_pixel", _fake((rows, 2 * cols, 4))[:, ::2], None, stride
    yield "every_other_channel", _fake((rows, cols, 8), torch.float16)[:, :, ::2], None, stride
    yield "transposed", _fake((cols, rows, 4), torch.uint8).transpose(0, 1), None, stride
    yield "float32_named_rgba8", _fake((rows, cols, 4)), "rgba8", f"{what}: target='rgba8' is a uint8 format, the tensor is torch.float32"
    yield "uint8_named_rgba16f", _fake((rows, cols, 4), torch.uint8), "rgba16f", f"{what}: target='rgba16f' is a float16 format, the tensor is torch.uint8"
    yield "float16_named_bgra8_srgb", _fake((rows, cols, 4), torch.float16), "bgra8_srgb", \
        f"{what}: target='bgra8_srgb' is a uint8 format, the tensor is torch.float16"
    yield "unknown_name", _fake((rows, cols, 4), torch.uint8), "rgb565", UNKNOWN_FORMAT


UNKNOWN_FORMAT = ("unknown target format 'rgb565': one of ['a2b10g10r10', 'bgra8', 'bgra8_srgb', 'bgra8_unorm', 'rgb10a2', 'rgba16f', 'rgba32f', 'rgba8', "
                  "'rgba8_srgb', 'rgba8_unorm']")
BAD_COLOURS = [name for name, *_ in _bad_colours("", 2, 2)]


@pytest.mark.parametrize("bad", BAD_COLOURS)
@pytest.mark.parametrize("method", list(SINGLE_METHODS) + list(BATCH_METHODS))
def test_a_bad_colour_tensor_is_refused(method, bad):
    node = _node()
    if method in SINGLE_METHODS:
        cam = _cam()
        rows, cols = (H, W) if SINGLE_METHODS[method][1] else (RECT[3] - RECT[1], RECT[2] - RECT[0])
        t, target, message = next(c[1:] for c in _bad_colours(_what(method), rows, cols) if c[0] == bad)
        _raises(node, ValueError, message, _single, node, method, cam, _depth(cam), t, rect=RECT, stream=STREAM, **({"target": target} if target else {}))
    else:
        cams, depths, rects = _views(2)
        composite = BATCH_METHODS[method][1]
        rows, cols = (H2, W2) if composite else (RECT2[3] - RECT2[1], RECT2[2] - RECT2[0])
        t, target, message = next(c[1:] for c in _bad_colours(_what(method, 1), rows, cols) if c[0] == bad)
        dtype = t.dtype if target is not None else torch.float32      # view 0 is right, also under the name that view 1 contradicts ...
        good = _fake((H, W, 4) if composite else (RECT[3] - RECT[1], RECT[2] - RECT[0], 4), dtype if bad != "unknown_name" else torch.uint8)
        if bad == "unknown_name":                                      # ... but an unknown name is already refused at view 0
            message = UNKNOWN_FORMAT
        elif target is not None:
            message = message.replace("view 1", "view 0")              # and a name that contradicts the dtype contradicts view 0's as well
        _raises(node, ValueError, message, _batch, node, method, cams, depths, [good, t], rects=rects, stream=STREAM, **({"target": target} if target else {}))


@pytest.mark.parametrize("method", ["render", "render_proxy", "render_views", "render_views_proxy"])
def test_an_unknown_target_name_is_refused_when_allocating(method):
    node, cam = _node(), _cam()
    args = (cam, _depth(cam)) if method in SINGLE_METHODS else ([cam], [_depth(cam)])
    _raises(node, ValueError, UNKNOWN_FORMAT, getattr(node, method), *args, stream=STREAM, target="rgb565")


@pytest.mark.parametrize("method", list(BATCH_METHODS))
def test_a_malformed_batch_is_refused(method):
    node = _node()
    composite = BATCH_METHODS[method][1]
    one_per_view = "cameras, depths, outs and rects must have one entry per view"
    cams, depths, rects = _views(2)
    outs = [c[0] for c in _view_colours(["f32", "f32"], cams, None, composite)]
    many = N.MAX_VIEWS + 1
    _raises(node, ValueError, f"at most {N.MAX_VIEWS} views per batch", _batch, node, method, [cams[0]] * many, [depths[0]] * many, [outs[0]] * many, stream=STREAM)
    _raises(node, ValueError, one_per_view, _batch, node, method, cams, depths[:1], outs, stream=STREAM)
    _raises(node, ValueError, one_per_view, _batch, node, method, cams, depths, outs[:1], stream=STREAM)
    _raises(node, ValueError, one_per_view, _batch, node, method, cams, depths, outs, rects=rects[:1], stream=STREAM)
    _raises(node, ValueError, one_per_view, _batch, node, method, cams[:1], depths, outs, stream=STREAM)
    if composite:
        _raises(node, ValueError, "composite=True blends into the views' scene buffers: pass them as outs", _batch, node, method, cams, depths, None, stream=STREAM)


def test_prepare_views_refuse_lists_that_disagree():
    node = _node()
    cams, _, rects = _views(2)
    tgts = [N.AtmoTarget(0x3000, N.TARGET_RGBA16F, 0)] * 2
    for fn, third, name in ((node.prepare_views, [0x3000, 0x4000], "outs"), (node.prepare_views_target, tgts, "targets")):
        message = f"cameras, depths, {name} and rects must have one entry per view"
        _raises(node, ValueError, message, fn, cams, [0x1000], third)
        _raises(node, ValueError, message, fn, cams, [0x1000, 0x2000], third[:1])
        _raises(node, ValueError, message, fn, cams, [0x1000, 0x2000], third, rects[:1])
        _raises(node, ValueError, message, fn, cams[:1], [0x1000, 0x2000], third)
