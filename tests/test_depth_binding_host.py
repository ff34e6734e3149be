"""What the Python binding hands to libatmo_hip.so when a draw's `depth` is a `depth_source(...)` (include/atmo_depth.h), recorded without a device with the
recorder and the fake tensors of tests/test_binding_calls_host.py: every draw method reaches the depth-source entry point of its row with the right
AtmoDepth (pointer, format, pitch in bytes) and every colour tensor as an AtmoTarget; plain tensors still reach the older entry points; bad wrappers raise
before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_binding_calls_host as B
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import depth_formats as D
from godot_atmosphere_shader_amd import planet_atmosphere as PA

W, H, STREAM, TIME = B.W, B.H, B.STREAM, B.TIME
DPAD, DLEFT = 5, 3          # a pitched depth: columns DLEFT .. DLEFT + cols of an image DPAD columns wider

# the argument lists of the four entry points, from include/atmo_depth.h
ABI = {
    "atmo_render_depth_target": ("ctx", "frame", "depth", "target", "composite", "stream"),
    "atmo_render_proxy_depth_target": ("ctx", "frame", "model", "box_size", "depth", "target", "composite", "stream"),
    "atmo_render_views_depth_target": ("ctx", "views", "n", "composite", "stream"),
    "atmo_render_views_proxy_depth_target": ("ctx", "views", "n", "model", "box_size", "composite", "stream"),
}
SINGLE = {False: "atmo_render_depth_target", True: "atmo_render_proxy_depth_target"}
BATCH = {False: "atmo_render_views_depth_target", True: "atmo_render_views_proxy_depth_target"}
DEPTHS = ["d32f", "d32f_pitched", "d16", "d16_pitched", "x8d24", "x8d24_pitched"]
_TORCH = {"d32f": torch.float32, "d16": torch.int16, "x8d24": torch.int32}


def _depth_fields(raw):
    d = N.AtmoDepth.from_buffer_copy(raw)
    return (d.texels or 0, d.format, d.row_pitch_bytes)


def _decode(name, args):
    kinds = ABI[name]
    assert len(kinds) == len(args), (name, len(args))
    out = {}
    for kind, a in zip(kinds, args):
        if kind == "frame":
            a = B._frame_fields(a)
        elif kind == "target":
            a = B._target_fields(a)
        elif kind == "depth":
            a = _depth_fields(a)
        elif kind == "model":
            a = tuple(np.frombuffer(a, dtype=np.float32).tolist())
        elif kind == "views":
            views = (N.AtmoViewDepthTarget * (len(a) // C.sizeof(N.AtmoViewDepthTarget))).from_buffer_copy(a)
            a = [dict(frame=B._frame_fields(bytes(v.frame)), depth=_depth_fields(bytes(v.depth)), target=B._target_fields(bytes(v.target))) for v in views]
        out[kind] = a
    return out


def _draws(node):
    return [(name, _decode(name, args)) for name, args in node._lib.calls if name != "atmo_destroy"]


def _source(kind, rows, cols):
    """(the wrapper, what the library must be given: the AtmoDepth's (texels, format, row pitch in bytes))."""
    name, pitched = kind.split("_")[0], kind.endswith("_pitched")
    image = B._fake((rows, cols + DPAD if pitched else cols), _TORCH[name])
    t = image[:, DLEFT:DLEFT + cols] if pitched else image
    size = image.element_size()
    return PA.depth_source(t), (image.data_ptr() + (DLEFT * size if pitched else 0), D.FORMATS[name], image.shape[1] * size)


def _as_target(given):
    """Every colour tensor is an AtmoTarget for these entry points: a contiguous float32 tensor is RGBA32F without a pitch."""
    return given if isinstance(given, tuple) else (given, N.TARGET_RGBA32F, 0)


@pytest.mark.parametrize("stream", B._streams())
@pytest.mark.parametrize("rect", [None, B.RECT], ids=["whole", "rect"])
@pytest.mark.parametrize("colour", ["f32", "f32_pitched", "f16", "u8_pitched:bgra8"])
@pytest.mark.parametrize("kind", DEPTHS)
@pytest.mark.parametrize("method", list(B.SINGLE_METHODS))
def test_single_draw_with_a_depth_source_reaches_its_entry_point(method, kind, colour, rect, stream):
    node, cam = B._node(), B._cam()
    src, given_depth = _source(kind, H, W)
    proxy, composite = B.SINGLE_METHODS[method]
    x0, y0, x1, y1 = rect or (0, 0, W, H)
    rows, cols = (H, W) if composite else (y1 - y0, x1 - x0)
    t, target, given = B._colour(colour, rows, cols)
    kw = {} if target is None else {"target": target}
    assert B._single(node, method, cam, src, t, rect=rect, stream=stream, **kw) is t
    want = dict(ctx=node._ctx.value, frame=B._frame(node, cam, rect), depth=given_depth, target=_as_target(given), composite=int(composite), stream=STREAM)
    if proxy:
        want.update(model=B._model(), box_size=B._box(cam.near))
    assert _draws(node) == [(SINGLE[proxy], want)]


@pytest.mark.parametrize("method", ["render", "render_proxy"])
def test_single_draw_with_a_depth_source_allocates_its_output(method):
    node, cam = B._node(), B._cam()
    src, given_depth = _source("d16_pitched", H, W)
    with B._AllocateAsCuda():
        out = getattr(node, method)(cam, src, stream=STREAM, time=TIME, target="rgba16f")
    assert out.dtype == torch.float16 and tuple(out.shape) == (H, W, 4)
    (name, args), = _draws(node)
    assert name == SINGLE[method == "render_proxy"] and args["depth"] == given_depth and args["target"] == (out.data_ptr(), N.TARGET_RGBA16F, W * 8)


@pytest.mark.parametrize("stream", B._streams())
@pytest.mark.parametrize("with_rects", [False, True], ids=["whole", "rects"])
@pytest.mark.parametrize("colour", ["f32", "f16", "u8_pitched:bgra8"])
@pytest.mark.parametrize("method", list(B.BATCH_METHODS))
def test_view_batch_with_depth_sources_reaches_its_entry_point(method, colour, with_rects, stream):
    """Two views of different sizes whose depth formats and pitches differ."""
    node = B._node()
    cams, _, rects = B._views(2)
    rects = rects if with_rects else None
    proxy, composite = B.BATCH_METHODS[method]
    srcs = [_source(k, c.height, c.width) for k, c in zip(("x8d24_pitched", "d16"), cams)]
    cols = B._view_colours([colour] * 2, cams, rects, composite)
    kw = {} if cols[0][1] is None else {"target": cols[0][1]}
    got = B._batch(node, method, cams, [s[0] for s in srcs], [c[0] for c in cols], rects=rects, stream=stream, **kw)
    assert len(got) == 2 and all(g is c[0] for g, c in zip(got, cols))
    views = [dict(frame=B._frame(node, cam, rects[i] if rects is not None else None), depth=srcs[i][1], target=_as_target(cols[i][2]))
             for i, cam in enumerate(cams)]
    want = dict(ctx=B.CTX, views=views, n=2, composite=int(composite), stream=STREAM)
    if proxy:
        want.update(model=B._model(), box_size=B._box(cams[0].near))
    assert _draws(node) == [(BATCH[proxy], want)]


def test_draw_atmospheres_passes_a_depth_source_through():
    lib, cam = B.Recorder(), B._cam()
    at = lambda z: np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, z], [0, 0, 0, 1.0]])   # noqa: E731
    near, far = B._node(PA.MODE_NEAR, 0xA, lib, at(300.0)), B._node(PA.MODE_FAR, 0xB, lib, at(-900.0))
    src, given_depth = _source("x8d24", H, W)
    t, _, given = B._colour("f16", H, W)
    assert PA.draw_atmospheres([near, far], cam, src, t, stream=B._Stream(), time=TIME) is t
    got = [(name, _decode(name, args)) for name, args in lib.calls]
    assert [(name, a["ctx"]) for name, a in got] == [(SINGLE[True], 0xB), (SINGLE[False], 0xA)]
    assert all(a["depth"] == given_depth and a["target"] == given and a["composite"] == 1 and a["stream"] == STREAM for _, a in got)


def test_plain_tensors_still_reach_the_older_entry_points():
    node, cam = B._node(), B._cam()
    depth = B._depth(cam)
    for kind in ("f32", "f16"):
        t, _, _ = B._colour(kind, H, W)
        node.render(cam, depth, t, stream=STREAM, time=TIME)
        node.render_proxy_composite(cam, depth, t, stream=STREAM, time=TIME)
    cams, depths, _ = B._views(2)
    cols = B._view_colours(["f16"] * 2, cams, None, False)
    node.render_views(cams, depths, [c[0] for c in cols], stream=STREAM, time=TIME)
    assert [name for name, _ in node._lib.calls] == ["atmo_render", "atmo_render_proxy_composite", "atmo_render_target", "atmo_render_proxy_target",
                                                    "atmo_render_views_target"]
    assert node._lib.draws()[0][1]["depth"] == depth.data_ptr()


def test_depth_source_states_the_format_and_the_pitch():
    for kind in DEPTHS:
        src, (ptr, fmt, pitch) = _source(kind, H, W)
        assert isinstance(src, PA.DepthSource) and (src.tensor.data_ptr(), src.format, src.pitch_bytes) == (ptr, fmt, pitch)
        assert PA.depth_source(src.tensor, D.NAMES[fmt]).format == fmt      # a name that agrees with the dtype
    if hasattr(torch, "uint16"):
        assert PA.depth_source(B._fake((H, W), torch.uint16)).format == D.D16
    assert PA.depth_source(B._fake((1, W), torch.int16)).pitch_bytes == 2 * W


@pytest.mark.parametrize("case", ["transposed", "element_stride_2", "float64", "uint8", "cpu", "not_a_tensor", "3d", "format_mismatch", "unknown_format",
                                  "row_stride_below_a_row"])
def test_a_bad_depth_source_is_refused_at_once(case):
    make = {
        "transposed": lambda: PA.depth_source(B._fake((W, H)).t()),
        "element_stride_2": lambda: PA.depth_source(B._fake((H, 2 * W), torch.int16)[:, ::2]),
        "float64": lambda: PA.depth_source(B._fake((H, W), torch.float64)),
        "uint8": lambda: PA.depth_source(B._fake((H, W), torch.uint8)),
        "cpu": lambda: PA.depth_source(torch.zeros((H, W))),
        "not_a_tensor": lambda: PA.depth_source(np.zeros((H, W), dtype=np.float32)),
        "3d": lambda: PA.depth_source(B._fake((H, W, 1))),
        "format_mismatch": lambda: PA.depth_source(B._fake((H, W), torch.int16), "x8d24"),
        "unknown_format": lambda: PA.depth_source(B._fake((H, W), torch.int16), "d24s8"),
        "row_stride_below_a_row": lambda: PA.depth_source(B._fake((1, W), torch.int32).expand(H, W)),
    }[case]
    with pytest.raises(TypeError if case in ("float64", "uint8", "cpu", "not_a_tensor") else ValueError):
        make()


def test_a_depth_source_of_the_wrong_shape_raises_before_anything_reaches_the_library():
    node, cam = B._node(), B._cam()
    t, _, _ = B._colour("f16", H, W)
    wrong = PA.depth_source(B._fake((H, W + 1), torch.int16))
    for method in B.SINGLE_METHODS:
        with pytest.raises(ValueError, match="shape"):
            B._single(node, method, cam, wrong, t, stream=STREAM)
    cams, depths, _ = B._views(2)
    cols = B._view_colours(["f16"] * 2, cams, None, True)
    good = PA.depth_source(B._fake((cams[0].height, cams[0].width), torch.int32))
    for method in B.BATCH_METHODS:
        with pytest.raises(ValueError, match="view 1: depth must have shape"):
            B._batch(node, method, cams, [good, wrong], [c[0] for c in cols], stream=STREAM)
        with pytest.raises(TypeError, match="all tensors or all"):
            B._batch(node, method, cams, [good, depths[1]], [c[0] for c in cols], stream=STREAM)
    assert node._lib.calls == []


def test_the_planets_batch_takes_float_depth_only():
    node, cam = B._node(), B._cam()
    src, _ = _source("d16", H, W)
    t, _, _ = B._colour("f16", H, W)
    with pytest.raises(TypeError, match="depth_source"):
        PA.render_planets([(node, cam, src, t, None, None, None)], stream=STREAM)
    with pytest.raises(TypeError, match="depth_source"):
        PA.draw_atmospheres_batched([node], cam, src, t, stream=STREAM)
    assert node._lib.calls == []
