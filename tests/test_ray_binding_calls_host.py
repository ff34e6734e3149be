"""What the ray methods of the Python binding (shade_rays, shade_ray_quads, ray_order, ray_list, camera_rays, camera_ray_quads, lens_rays, render_lens)
hand to libatmo_hip.so, recorded without a device, in the manner of tests/test_binding_calls_host.py: for every method the exact sequence of entry points
-- the bake first where there is one -- with every decoded argument, what it allocates (torch.empty or torch.zeros, and whether on the call's stream),
which exception every bad argument raises with its full text, and which of two faults wins.

The stream is always given, as an int or as an object with `cuda_stream`; torch.cuda.ExternalStream and torch.cuda.stream are stood in for and counted.
The expectations are this file's own tables: ABI (the argument names, from include/atmo_rays.h, atmo_ray_quads.h, atmo_ray_order.h, atmo_ray_list.h,
atmo_ray_detail.h and atmo_lens.h) and the message constants.  Run it after any change to the binding."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import planet_atmosphere as PA
from godot_atmosphere_shader_amd.lens import Lens
from godot_atmosphere_shader_amd.ray_quads import quad_order, quads_to_image
from test_binding_calls_host import CTX, STREAM, TIME, Recorder, _AllocateAsCuda, _cam, _fake, _node

_SHADE = ("ctx", "frame", "rays", "rgba", "n", "width", "first")
_QUADS = ("ctx", "frame", "rays", "rgba", "n_quads", "width", "first_quad", "stream")
ABI = {
    "atmo_bake_optical_depth": ("ctx", "stream"),
    "atmo_shade_rays": _SHADE + ("stream",),
    "atmo_debug_frame_rays": ("ctx", "frame", "depth", "rays", "stream"),
    "atmo_shade_ray_quads": _QUADS,
    "atmo_ray_order_scratch_bytes": ("n", "bytes"),
    "atmo_ray_order": ("ctx", "rays", "n", "index", "scratch", "scratch_bytes", "stream"),
    "atmo_shade_rays_indexed": _SHADE + ("index", "n_index", "stream"),
    "atmo_ray_list_scratch_bytes": ("capacity", "bytes"),
    "atmo_ray_list": ("ctx", "frame", "rays", "count", "capacity", "flags", "rgba", "index", "listed", "scratch", "scratch_bytes", "stream"),
    "atmo_shade_rays_detail": _SHADE + ("index", "n_index", "stream"),
    "atmo_shade_ray_quads_detail": _QUADS,
    "atmo_lens_ray_counts": ("lens", "flags", "n_rays", "n_index"),
    "atmo_lens_rays": ("ctx", "lens", "flags", "distance", "pitch", "rays", "index", "stream"),
}
RAY_ENTRIES = tuple(n for n in ABI if n != "atmo_bake_optical_depth")
BAKE = ("atmo_bake_optical_depth", dict(ctx=CTX, stream=STREAM))
SCRATCH_BYTES, SCRATCH_WORDS = 100, 28      # what the size queries answer here, and the int32 words that holds in whole 16-byte units
NO_BYTES, NO_COUNT = bytes(C.c_size_t(0)), bytes(C.c_uint32(0))      # the words a query is handed
F32, I32 = torch.float32, torch.int32
CUDA0 = torch.device("cuda", 0)


class _Stream:
    cuda_stream = STREAM


class _World:
    """camera=None: ray space is world space."""
    width = height = 1
    view = inv_view = inv_projection = np.eye(4)


class Lib(Recorder):
    """A Recorder that answers the size queries: SCRATCH_BYTES for the two *_scratch_bytes, `counts` for atmo_lens_ray_counts (written behind the record,
    so the record holds the zeros the binding handed over).  `without`: the entry points this library lacks."""

    def __init__(self, counts=(0, 0), without=()):
        super().__init__()
        self.counts, self.without = counts, without

    def __getattr__(self, name):
        if name in object.__getattribute__(self, "without"):
            raise AttributeError(name)
        entry = super().__getattr__(name)
        if name.endswith("_scratch_bytes"):
            def sized(n, need):
                rc = entry(n, need)
                need._obj.value = SCRATCH_BYTES
                return rc
            return sized
        if name == "atmo_lens_ray_counts":
            def counted(lens, flags, n_rays, n_index):
                rc = entry(lens, flags, n_rays, n_index)
                n_rays._obj.value, n_index._obj.value = self.counts
                return rc
            return counted
        return entry


class Rig:
    """The stand-ins of a call: torch.cuda.ExternalStream (`made`: handle and device of each) and torch.cuda.stream (`entered`), and every torch.empty /
    torch.zeros of the call: `seen` = (which, shape, dtype, inside the stream context?), `tensors` = what each returned."""

    def __init__(self, monkeypatch):
        self.made, self.entered, self.depth, self.seen, self.tensors = [], 0, 0, [], []
        monkeypatch.setattr(torch.cuda, "ExternalStream", self._external)
        monkeypatch.setattr(torch.cuda, "stream", self._stream)

    def _external(self, handle, device=None):
        self.made.append((handle, device))
        return ("external", handle)

    @contextlib.contextmanager
    def _stream(self, s):
        assert s == ("external", STREAM)
        self.entered += 1
        self.depth += 1
        try:
            yield
        finally:
            self.depth -= 1

    def run(self, fn, *args, **kw):
        with _Watch(self):
            return fn(*args, **kw)


class _Watch(_AllocateAsCuda):
    """Notes every allocation in the rig, and sends one that asks for device=cuda (a lens without a distance buffer) to the CPU."""

    def __init__(self, rig):
        super().__init__()
        self.rig = rig

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        if func not in (torch.empty, torch.zeros):
            return super().__torch_function__(func, types, args, kwargs)
        if torch.device(kwargs.get("device", "cpu")).type == "cuda":
            kwargs["device"] = "cpu"
        out = super().__torch_function__(func, types, args, kwargs)
        self.rig.seen.append((func.__name__, tuple(args[0]), kwargs.get("dtype"), self.rig.depth > 0))
        self.rig.tensors.append(out)
        return out


@pytest.fixture
def rig(monkeypatch):
    return Rig(monkeypatch)


def _ray_node(detail=False, bake=False, lib=None):
    node = _node(lib=lib if lib is not None else Lib())
    node._device = 0
    if detail:
        node._cloud_detail, node._shader = True, PA.SHADERS["planet_atmosphere_clouds_high"]
    node._bake_pending = node._uses_baked_optical_depth = bake
    return node


def _calls(node):
    out = []
    for name, args in node._lib.calls:
        assert len(ABI[name]) == len(args), (name, len(args))
        out.append((name, dict(zip(ABI[name], args))))
    return out


def _frame(node, cam, time, rect=None):
    return bytes(PA._to_native_frame(PA.make_frame(cam if cam is not None else _World, node.global_transform, node._params["u_sun_position"], time, rect)))


def _bits(t):
    return t.contiguous().view(torch.int32)


STREAMS = [pytest.param(STREAM, id="int"), pytest.param(_Stream(), id="obj")]
BOTH = [False, True]


# ---- shade_rays and shade_ray_quads ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("make_out", BOTH, ids=["out", "no_out"])
@pytest.mark.parametrize("placed", BOTH, ids=["width_defaulted", "width_given"])
@pytest.mark.parametrize("with_camera", BOTH, ids=["world", "camera"])
@pytest.mark.parametrize("detail", BOTH, ids=["plain_node", "detail_node"])
@pytest.mark.parametrize("indexed", BOTH, ids=["whole", "index"])
def test_shade_rays(rig, indexed, detail, with_camera, placed, make_out, stream):
    node, cam = _ray_node(detail, bake=True), _cam() if with_camera else None
    rays, index, out = _fake((70, 8)), _fake((33,), I32) if indexed else None, None if make_out else _fake((70, 4))
    got = rig.run(node.shade_rays, rays, cam, out=out, stream=stream, time=TIME, index=index, **(dict(width=10, first=30) if placed else {}))
    assert tuple(got.shape) == (70, 4) and got.dtype == F32 and (make_out or got is out)
    assert rig.seen == ([("zeros" if indexed else "empty", (70, 4), F32, False)] if make_out else []) and rig.made == [] and rig.entered == 0
    name = "atmo_shade_rays_detail" if detail else "atmo_shade_rays_indexed" if indexed else "atmo_shade_rays"
    want = dict(ctx=CTX, frame=_frame(node, cam, TIME), rays=rays.data_ptr(), rgba=got.data_ptr(), n=70, width=10 if placed else 70, first=30 if placed else 0,
                stream=STREAM)
    if indexed:
        want.update(index=index.data_ptr(), n_index=33)
    elif detail:
        want.update(index=None, n_index=0)      # atmo_shade_rays_detail: a null list is the whole batch
    assert _calls(node) == [BAKE, (name, want)] and node._bake_pending is False


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("make_out", BOTH, ids=["out", "no_out"])
@pytest.mark.parametrize("with_camera", BOTH, ids=["world", "camera"])
@pytest.mark.parametrize("detail", BOTH, ids=["plain_node", "detail_node"])
def test_shade_ray_quads(rig, detail, with_camera, make_out, stream):
    node, cam = _ray_node(detail, bake=True), _cam() if with_camera else None
    quads, out = _fake((72, 8)), None if make_out else _fake((72, 4))
    got = rig.run(node.shade_ray_quads, quads, cam, width=11, first_quad=30, out=out, stream=stream, time=TIME)
    assert tuple(got.shape) == (72, 4) and got.dtype == F32 and (make_out or got is out)
    assert rig.seen == ([("empty", (72, 4), F32, False)] if make_out else []) and rig.made == [] and rig.entered == 0
    want = dict(ctx=CTX, frame=_frame(node, cam, TIME), rays=quads.data_ptr(), rgba=got.data_ptr(), n_quads=18, width=11, first_quad=30, stream=STREAM)
    assert _calls(node) == [BAKE, ("atmo_shade_ray_quads_detail" if detail else "atmo_shade_ray_quads", want)]
    node._lib.calls.clear()      # first_quad defaults to 0; nothing pending: no bake
    rig.run(node.shade_ray_quads, quads, cam, width=11, out=got, stream=stream, time=TIME)
    assert _calls(node) == [("atmo_shade_ray_quads_detail" if detail else "atmo_shade_ray_quads", dict(want, first_quad=0))]


# ---- ray_order and ray_list ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_ray_order(rig, stream):
    node, rays = _ray_node(bake=True), _fake((70, 8))
    order = rig.run(node.ray_order, rays, stream=stream)
    assert rig.seen == [("empty", (70,), I32, False), ("empty", (SCRATCH_WORDS,), I32, True)] and order is rig.tensors[0]
    assert rig.made == [(STREAM, rays.device)] and rig.entered == 1
    assert _calls(node) == [("atmo_ray_order_scratch_bytes", dict(n=70, bytes=NO_BYTES)),
                            ("atmo_ray_order", dict(ctx=CTX, rays=rays.data_ptr(), n=70, index=order.data_ptr(), scratch=rig.tensors[1].data_ptr(),
                                                    scratch_bytes=SCRATCH_BYTES, stream=STREAM))]
    assert node._bake_pending is True      # the order reads no table: the bake waits for a draw


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("make_out", BOTH, ids=["out", "no_out"])
@pytest.mark.parametrize("counted", BOTH, ids=["no_count", "count"])
@pytest.mark.parametrize("with_camera", BOTH, ids=["world", "camera"])
@pytest.mark.parametrize("cull", BOTH, ids=["all", "cull"])
@pytest.mark.parametrize("order", BOTH, ids=["queue_order", "ray_order"])
def test_ray_list(rig, order, cull, with_camera, counted, make_out, stream):
    node, cam = _ray_node(bake=True), _cam() if with_camera else None
    rays, count, out = _fake((70, 8)), _fake((1,), I32) if counted else None, None if make_out else _fake((70, 4))
    index, listed = rig.run(node.ray_list, rays, count, order=order, cull=cull, camera=cam, out=out, stream=stream)
    allocated = [("empty", (SCRATCH_WORDS,), I32, True), ("empty", (70,), I32, True), ("empty", (1,), I32, True)]
    if cull and make_out:
        allocated.append(("zeros", (70, 4), F32, True))
        out = rig.tensors[3]
    assert rig.seen == allocated and index is rig.tensors[1] and listed is rig.tensors[2]
    assert rig.made == [(STREAM, rays.device)] and rig.entered == 1
    want = dict(ctx=CTX, frame=_frame(node, cam, 0.0) if cull else None, rays=rays.data_ptr(), count=count.data_ptr() if counted else None, capacity=70,
                flags=(N.RAY_LIST_ORDER if order else 0) | (N.RAY_LIST_CULL if cull else 0), rgba=out.data_ptr() if cull else None, index=index.data_ptr(),
                listed=listed.data_ptr(), scratch=rig.tensors[0].data_ptr(), scratch_bytes=SCRATCH_BYTES, stream=STREAM)
    assert (N.RAY_LIST_ORDER, N.RAY_LIST_CULL) == (1, 2)
    assert _calls(node) == [("atmo_ray_list_scratch_bytes", dict(capacity=70, bytes=NO_BYTES)), ("atmo_ray_list", want)]
    assert node._bake_pending is True


def test_ray_list_without_the_cull_does_not_look_at_out(rig):
    node = _ray_node()
    rig.run(node.ray_list, _fake((70, 8)), cull=False, out="not a tensor", stream=STREAM)
    assert _calls(node)[1][1]["rgba"] is None


# ---- camera_rays and camera_ray_quads ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("rect", [None, (3, 2, 19, 9)], ids=["whole", "rect"])
def test_camera_rays(rig, rect, stream):
    node, cam = _ray_node(bake=True), _cam()
    depth = _fake((cam.height, cam.width))
    rays = rig.run(node.camera_rays, cam, depth, rect=rect, stream=stream)
    x0, y0, x1, y1 = rect or (0, 0, cam.width, cam.height)
    assert rig.seen == [("empty", ((y1 - y0) * (x1 - x0), 8), F32, False)] and rays is rig.tensors[0] and rig.made == [] and rig.entered == 0
    assert _calls(node) == [("atmo_debug_frame_rays", dict(ctx=CTX, frame=_frame(node, cam, 0.0, rect), depth=depth.data_ptr(), rays=rays.data_ptr(),
                                                           stream=STREAM))]
    assert node._bake_pending is True


@pytest.mark.parametrize("stream", STREAMS)
def test_camera_ray_quads(rig, stream):
    node, cam = _ray_node(bake=True), _cam(5, 3)      # odd both ways: slots outside the image
    depth = _fake((3, 5))
    quads = rig.run(node.camera_ray_quads, cam, depth, stream=stream)
    assert rig.seen == [("empty", (15, 8), F32, False), ("zeros", (), F32, True)]      # the dump as camera_rays makes it; the gather on the call's stream
    assert rig.made == [(STREAM, depth.device)] and rig.entered == 1
    rays = rig.tensors[0]
    assert _calls(node) == [("atmo_debug_frame_rays", dict(ctx=CTX, frame=_frame(node, cam, 0.0), depth=depth.data_ptr(), rays=rays.data_ptr(), stream=STREAM))]
    order = torch.as_tensor(quad_order(5, 3))
    want = torch.where((order >= 0).unsqueeze(1), _bits(rays)[order.clamp(min=0)], torch.zeros((), dtype=I32))
    assert tuple(quads.shape) == (24, 8) and quads.dtype == F32 and quads.is_contiguous() and torch.equal(_bits(quads), want) and (order < 0).sum() == 9


# ---- lens_rays and render_lens -----------------------------------------------------------------------------------------------------------------------------------------
LW, LH, BAND = 19, 7, (2, 7)      # an even y0, y1 == height: a band both orders take


def _lens():
    return Lens.equirect(LW, LH, rows=BAND, origin=(1.5, -2.25, 0.125), tmax=7.5)


def _distance():
    return _fake((LH, LW + 5))[:, :LW + 2]      # a row stride larger than its width, which is larger than the lens's


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("with_distance", BOTH, ids=["tmax", "distance"])
@pytest.mark.parametrize("mode", ["row_major", "tile_index", "quads"])
def test_lens_rays(rig, mode, with_distance, stream):
    lens, quads, tiled = _lens(), mode == "quads", mode == "tile_index"
    n_rays, n_index = lens.counts(quads)
    assert (n_rays, n_index) == ((120, 256) if quads else (95, 256))
    node, distance = _ray_node(bake=True, lib=Lib(counts=(n_rays, n_index))), _distance() if with_distance else None
    got = rig.run(node.lens_rays, lens, distance=distance, quads=quads, tile_index=tiled, stream=stream)
    rays, index = got if tiled else (got, None)
    assert rig.seen == [("empty", (n_rays, 8), F32, True)] + ([("empty", (n_index,), I32, True)] if tiled else [])
    assert rays is rig.tensors[0] and (not tiled or index is rig.tensors[1])
    assert rig.made == [(STREAM, distance.device if with_distance else CUDA0)] and rig.entered == 1
    raw, flags = bytes(lens.native()), N.LENS_QUADS if quads else 0
    assert _calls(node) == [
        ("atmo_lens_ray_counts", dict(lens=raw, flags=flags, n_rays=NO_COUNT, n_index=NO_COUNT)),
        ("atmo_lens_rays", dict(ctx=CTX, lens=raw, flags=flags, distance=distance.data_ptr() if with_distance else None, pitch=LW + 5 if with_distance else 0,
                                rays=rays.data_ptr(), index=index.data_ptr() if tiled else None, stream=STREAM))]
    assert N.LENS_QUADS == 1 and node._bake_pending is True


def test_lens_rays_of_a_one_row_image_take_the_distance_s_width_as_the_pitch(rig):
    lens, distance = Lens.equirect(5, 1), _fake((1, 9))
    node = _ray_node(lib=Lib(counts=lens.counts()))
    rig.run(node.lens_rays, lens, distance=distance, stream=STREAM)
    assert _calls(node)[1][1]["pitch"] == 9


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("make_out", BOTH, ids=["out", "no_out"])
@pytest.mark.parametrize("with_distance", BOTH, ids=["tmax", "distance"])
@pytest.mark.parametrize("quads", [True, False, None], ids=["quads", "row_major", "picked"])
def test_render_lens(rig, quads, with_distance, make_out, stream):
    lens, cam, rows = _lens(), _cam(), BAND[1] - BAND[0]
    n_rays, n_index = lens.counts(bool(quads))
    node, distance = _ray_node(bake=True, lib=Lib(counts=(n_rays, n_index))), _distance() if with_distance else None
    out = None if make_out else torch.ones((rows, LW, 4)).as_subclass(type(_fake((1,))))
    got = rig.run(node.render_lens, lens, cam, distance=distance, out=out, time=TIME, stream=stream, quads=quads)
    assert tuple(got.shape) == (rows, LW, 4) and got.dtype == F32 and got.is_contiguous() and (make_out or got is out)
    device = distance.device if with_distance else CUDA0
    assert rig.made == [(STREAM, CUDA0), (STREAM, device)] and rig.entered == 2      # render_lens's own context around lens_rays'
    raw, flags, rays = bytes(lens.native()), N.LENS_QUADS if quads else 0, rig.tensors[0]
    formed = [("atmo_lens_ray_counts", dict(lens=raw, flags=flags, n_rays=NO_COUNT, n_index=NO_COUNT)),
              ("atmo_lens_rays", dict(ctx=CTX, lens=raw, flags=flags, distance=distance.data_ptr() if with_distance else None,
                                      pitch=LW + 5 if with_distance else 0, rays=rays.data_ptr(), index=None if quads else rig.tensors[1].data_ptr(), stream=STREAM))]
    shade = dict(ctx=CTX, frame=_frame(node, cam, TIME), rays=rays.data_ptr(), stream=STREAM)
    if quads:
        shaded = rig.tensors[1]
        assert rig.seen == [("empty", (n_rays, 8), F32, True), ("empty", (n_rays, 4), F32, True)]
        shade.update(rgba=shaded.data_ptr(), n_quads=n_rays // 4, width=LW, first_quad=(BAND[0] // 2) * ((LW + 1) // 2))
        assert _calls(node) == formed + [BAKE, ("atmo_shade_ray_quads", shade)]
        assert torch.equal(_bits(got), _bits(quads_to_image(shaded, LW, rows)))
    else:      # row-major, through the tile index, into a zeroed image
        assert rig.seen == [("empty", (n_rays, 8), F32, True), ("empty", (n_index,), I32, True)] + ([("zeros", (rows, LW, 4), F32, True)] if make_out else [])
        shade.update(rgba=got.data_ptr(), n=rows * LW, width=LW, first=BAND[0] * LW, index=rig.tensors[1].data_ptr(), n_index=n_index)
        assert _calls(node) == formed + [BAKE, ("atmo_shade_rays_indexed", shade)]
        assert not got.any()


# ---- nothing to do -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_no_rays(rig):
    """ray_order and ray_list return before any entry point, the size query included; the shading calls and lens_rays hand the library its n = 0."""
    node, none = _ray_node(lib=Lib(without=RAY_ENTRIES[3:])), _fake((0, 8))
    order = rig.run(node.ray_order, none, stream=STREAM)
    index, listed = rig.run(node.ray_list, none, cull=True, stream=STREAM)
    assert tuple(order.shape) == tuple(index.shape) == (0,) and order.dtype == index.dtype == I32 and tuple(listed.shape) == (1,) and listed.dtype == I32
    assert int(listed[0]) == 0 and rig.seen == [("empty", (0,), I32, False), ("empty", (0,), I32, False), ("zeros", (1,), I32, False)]
    assert _calls(node) == [] and rig.made == [] and rig.entered == 0      # (and a library without the entry points is not noticed)
    out = rig.run(node.shade_rays, none, stream=STREAM)
    quads = rig.run(node.shade_ray_quads, none, width=3, stream=STREAM)
    assert tuple(out.shape) == tuple(quads.shape) == (0, 4)
    world = _frame(node, None, 0.0)
    assert _calls(node) == [("atmo_shade_rays", dict(ctx=CTX, frame=world, rays=none.data_ptr(), rgba=out.data_ptr(), n=0, width=1, first=0, stream=STREAM)),
                            ("atmo_shade_ray_quads", dict(ctx=CTX, frame=world, rays=none.data_ptr(), rgba=quads.data_ptr(), n_quads=0, width=3, first_quad=0,
                                                          stream=STREAM))]


@pytest.mark.parametrize("make_out", BOTH, ids=["out", "no_out"])
def test_no_rows_of_a_lens(rig, make_out):
    lens = Lens.equirect(LW, LH, rows=(4, 4))
    node, out = _ray_node(bake=True, lib=Lib(without=RAY_ENTRIES)), None if make_out else _fake((0, LW, 4))
    got = rig.run(node.render_lens, lens, out=out, stream=STREAM, quads=False)
    assert tuple(got.shape) == (0, LW, 4) and got.dtype == F32 and (make_out or got is out)
    assert rig.seen == ([("zeros", (0, LW, 4), F32, False)] if make_out else []) and _calls(node) == [] and rig.made == [] and node._bake_pending is True
    node = _ray_node()      # lens_rays itself asks for the counts and hands the library its empty band
    rays, index = rig.run(node.lens_rays, lens, tile_index=True, stream=STREAM)
    assert tuple(rays.shape) == (0, 8) and tuple(index.shape) == (0,) and [name for name, _ in _calls(node)] == ["atmo_lens_ray_counts", "atmo_lens_rays"]


# ---- refusals: the exception's class and full text, and which of two faults wins; nothing reaches the library --------------------------------------------------
def kind(what, dtype="float32", contiguous=True):
    return f"{what} must be a {'contiguous ' if contiguous else ''}CUDA {dtype} tensor"


RAYS_SHAPE, QUADS_SHAPE, OUT_SHAPE = "rays must have shape (n, 8)", "quads must have shape (n, 8)", "out must have shape (n, 4)"
INDEX_SHAPE = "index must have shape (m,)"
INTEGERS, QUAD_INTEGERS = "width and first must be integers", "width and first_quad must be integers"
RANGE = "width must be at least 1, first at least 0 and first + n at most 2^32"
QUAD_RANGE = "width must be at least 1, first_quad at least 0 and first_quad + n_quads at most 2^30"
OUT_ROWS, QUAD_OUT_ROWS = "out must have one row per ray: shape (n, 4)", "out must have one row per ray: shape (4 * n_quads, 4)"
FOUR_ROWS = "quads must have four rows per quad: shape (4 * n_quads, 8)"
TOO_MANY = "at most 2^28 rays"
COUNT_ONE = "count must have one element"
TILE_ROW_MAJOR = "the tile index is row-major only"
DISTANCE_SHAPE = "distance must have shape (lens.height, >= lens.width) with contiguous rows"
DEPTH_SHAPE = "depth must have shape (viewport_h, viewport_w)"


def missing(name, header, suffix=""):
    return f"libatmo_hip.so does not export {name} (include/{header}){suffix}; rebuild it"


def _huge(cols=8):
    """2^28 + 1 rows that take no memory: nothing looks at them before the count is refused."""
    return torch.empty(((1 << 28) + 1, cols), device="meta").as_subclass(type(_fake((1,))))


def _good():
    return dict(rays=_fake((12, 8)), out=_fake((12, 4)), index=_fake((5,), I32), count=_fake((1,), I32), cam=_cam())


def _t(shape, dtype=F32):
    return _fake(shape, dtype)


CPU = torch.zeros((12, 8))
# (id, method, positional arguments, keyword arguments, the entry points the library lacks, exception, message).  "rays" / "cam" ... are _good()'s.
# A row with two faults is named "<the one that wins>_before_<the other>": one such pair for every two adjacent checks.
REFUSALS = [
    # shade_rays: rays' kind, rays' shape, index's kind, index's shape, the integers, their range, out's kind, out's shape, out's rows, the symbol
    ("rays_cpu", "shade_rays", (CPU, "cam"), {}, (), TypeError, kind("rays")),
    ("rays_float16", "shade_rays", (_t((12, 8), torch.float16), "cam"), {}, (), TypeError, kind("rays")),
    ("rays_strided", "shade_rays", (_t((12, 16))[:, ::2], "cam"), {}, (), TypeError, kind("rays")),
    ("rays_numpy", "shade_rays", (np.zeros((12, 8), dtype=np.float32), "cam"), {}, (), TypeError, kind("rays")),
    ("rays_none", "shade_rays", (None, "cam"), {}, (), TypeError, kind("rays")),
    ("rays_kind_before_shape", "shade_rays", (_t((12, 7), torch.float64), "cam"), {}, (), TypeError, kind("rays")),
    ("rays_seven_columns", "shade_rays", (_t((12, 7)), "cam"), {}, (), ValueError, RAYS_SHAPE),
    ("rays_flat", "shade_rays", (_t((96,)), "cam"), {}, (), ValueError, RAYS_SHAPE),
    ("rays_shape_before_index_kind", "shade_rays", (_t((12, 8, 1)), "cam"), dict(index=[0, 1]), (), ValueError, RAYS_SHAPE),
    ("index_cpu", "shade_rays", ("rays", "cam"), dict(index=torch.zeros((5,), dtype=I32)), (), TypeError, kind("index", "int32")),
    ("index_strided", "shade_rays", ("rays", "cam"), dict(index=_t((10,), I32)[::2]), (), TypeError, kind("index", "int32")),
    ("index_kind_before_shape", "shade_rays", ("rays", "cam"), dict(index=_t((5, 1), torch.int64)), (), TypeError, kind("index", "int32")),
    ("index_shape_before_integers", "shade_rays", ("rays", "cam"), dict(index=_t((5, 1), I32), width=2.5), (), ValueError, INDEX_SHAPE),
    ("integers_before_range", "shade_rays", ("rays", "cam"), dict(width=2.5, first=-1), (), TypeError, INTEGERS),
    ("first_a_string", "shade_rays", ("rays", "cam"), dict(first="0"), (), TypeError, INTEGERS),
    ("width_zero_before_out_kind", "shade_rays", ("rays", "cam"), dict(width=0, out=torch.zeros((12, 4))), (), ValueError, RANGE),
    ("first_negative", "shade_rays", ("rays", "cam"), dict(first=-1), (), ValueError, RANGE),
    ("first_plus_n_past_2_32", "shade_rays", ("rays", "cam"), dict(first=2 ** 32 - 11), (), ValueError, RANGE),
    ("out_kind_before_shape", "shade_rays", ("rays", "cam"), dict(out=_t((12, 3), torch.float64)), (), TypeError, kind("out")),
    ("out_shape_before_rows", "shade_rays", ("rays", "cam"), dict(out=_t((11, 3))), (), ValueError, OUT_SHAPE),
    ("out_rows_before_symbol", "shade_rays", ("rays", "cam"), dict(out=_t((11, 4))), ("atmo_shade_rays",), ValueError, OUT_ROWS),
    ("no_shade_rays", "shade_rays", ("rays", "cam"), dict(out="out"), ("atmo_shade_rays",), RuntimeError, missing("atmo_shade_rays", "atmo_rays.h")),
    ("no_shade_rays_indexed", "shade_rays", ("rays", "cam"), dict(out="out", index="index"), ("atmo_shade_rays_indexed",), RuntimeError,
     missing("atmo_shade_rays_indexed", "atmo_ray_order.h")),
    # shade_ray_quads: quads' kind, shape, four rows a quad, the integers, their range, out's kind, out's shape, out's rows, the symbol
    ("quads_kind_before_shape", "shade_ray_quads", (_t((12, 7), torch.float64), "cam"), dict(width=6), (), TypeError, kind("quads")),
    ("quads_shape_before_four_rows", "shade_ray_quads", (_t((13, 7)), "cam"), dict(width=6), (), ValueError, QUADS_SHAPE),
    ("four_rows_before_integers", "shade_ray_quads", (_t((13, 8)), "cam"), dict(width=2.5), (), ValueError, FOUR_ROWS),
    ("quad_integers_before_range", "shade_ray_quads", ("rays", "cam"), dict(width=2.5, first_quad=-1), (), TypeError, QUAD_INTEGERS),
    ("quad_width_zero_before_out_kind", "shade_ray_quads", ("rays", "cam"), dict(width=0, out=torch.zeros((12, 4))), (), ValueError, QUAD_RANGE),
    ("first_quad_past_2_30", "shade_ray_quads", ("rays", "cam"), dict(width=6, first_quad=2 ** 30 - 2), (), ValueError, QUAD_RANGE),
    ("quad_out_kind_before_shape", "shade_ray_quads", ("rays", "cam"), dict(width=6, out=_t((12, 3), torch.float64)), (), TypeError, kind("out")),
    ("quad_out_shape_before_rows", "shade_ray_quads", ("rays", "cam"), dict(width=6, out=_t((8, 3))), (), ValueError, OUT_SHAPE),
    ("quad_out_rows_before_symbol", "shade_ray_quads", ("rays", "cam"), dict(width=6, out=_t((8, 4))), ("atmo_shade_ray_quads",), ValueError, QUAD_OUT_ROWS),
    ("no_shade_ray_quads", "shade_ray_quads", ("rays", "cam"), dict(width=6, out="out"), ("atmo_shade_ray_quads",), RuntimeError,
     missing("atmo_shade_ray_quads", "atmo_ray_quads.h")),
    # ray_order: rays' kind, shape, the count of rays, the symbols (the sort's before the size query's)
    ("order_kind_before_shape", "ray_order", (_t((12, 7), torch.float64),), {}, (), TypeError, kind("rays")),
    ("order_shape_before_too_many", "ray_order", (_huge(7),), {}, (), ValueError, RAYS_SHAPE),
    ("order_too_many_before_symbol", "ray_order", (_huge(),), {}, ("atmo_ray_order",), ValueError, TOO_MANY),
    ("no_ray_order", "ray_order", ("rays",), {}, ("atmo_ray_order", "atmo_ray_order_scratch_bytes"), RuntimeError, missing("atmo_ray_order", "atmo_ray_order.h")),
    ("no_ray_order_scratch_bytes", "ray_order", ("rays",), {}, ("atmo_ray_order_scratch_bytes",), RuntimeError,
     missing("atmo_ray_order_scratch_bytes", "atmo_ray_order.h")),
    # ray_list: rays' kind, shape, the count of rays, count's kind, count's size, (with the cull) out's kind, shape and rows, the symbols
    ("list_kind_before_shape", "ray_list", (_t((12, 7), torch.float64),), {}, (), TypeError, kind("rays")),
    ("list_shape_before_too_many", "ray_list", (_huge(7),), {}, (), ValueError, RAYS_SHAPE),
    ("list_too_many_before_count_kind", "ray_list", (_huge(), 5), {}, (), ValueError, TOO_MANY),
    ("count_cpu", "ray_list", ("rays", torch.zeros((1,), dtype=I32)), {}, (), TypeError, kind("count", "int32")),
    ("count_an_int", "ray_list", ("rays", 5), {}, (), TypeError, kind("count", "int32")),
    ("count_kind_before_size", "ray_list", ("rays", _t((2,), torch.int64)), {}, (), TypeError, kind("count", "int32")),
    ("count_size_before_out_kind", "ray_list", ("rays", _t((2,), I32)), dict(cull=True, out=torch.zeros((12, 4))), (), ValueError, COUNT_ONE),
    ("list_out_kind_before_shape", "ray_list", ("rays",), dict(cull=True, out=_t((12, 3), torch.float64)), (), TypeError, kind("out")),
    ("list_out_shape_before_rows", "ray_list", ("rays",), dict(cull=True, out=_t((11, 3))), (), ValueError, OUT_SHAPE),
    ("list_out_rows_before_symbol", "ray_list", ("rays",), dict(cull=True, out=_t((11, 4))), ("atmo_ray_list",), ValueError, OUT_ROWS),
    ("no_ray_list", "ray_list", ("rays",), {}, ("atmo_ray_list", "atmo_ray_list_scratch_bytes"), RuntimeError, missing("atmo_ray_list", "atmo_ray_list.h")),
    ("no_ray_list_scratch_bytes", "ray_list", ("rays",), {}, ("atmo_ray_list_scratch_bytes",), RuntimeError,
     missing("atmo_ray_list_scratch_bytes", "atmo_ray_list.h")),
    # camera_rays and camera_ray_quads: depth's kind, depth's shape, the symbol
    ("depth_kind_before_shape", "camera_rays", ("cam", torch.zeros((3, 3))), {}, (), TypeError, kind("depth")),
    ("depth_shape_before_symbol", "camera_rays", ("cam", _t((10, 25))), {}, ("atmo_debug_frame_rays",), ValueError, DEPTH_SHAPE),
    ("no_frame_rays", "camera_rays", ("cam", _t((10, 24))), {}, ("atmo_debug_frame_rays",), RuntimeError, missing("atmo_debug_frame_rays", "atmo_rays.h")),
    ("quads_depth_kind", "camera_ray_quads", ("cam", torch.zeros((10, 24))), {}, (), TypeError, kind("depth")),
    ("quads_depth_shape", "camera_ray_quads", ("cam", _t((24, 10))), {}, (), ValueError, DEPTH_SHAPE),
    ("quads_no_frame_rays", "camera_ray_quads", ("cam", _t((10, 24))), {}, ("atmo_debug_frame_rays",), RuntimeError,
     missing("atmo_debug_frame_rays", "atmo_rays.h")),
    # lens_rays: quads with the tile index, distance's kind, distance's shape, the symbols (the rays' before the counts')
    ("tile_index_before_distance_kind", "lens_rays", ("lens",), dict(quads=True, tile_index=True, distance=torch.zeros((LH, LW))), (), ValueError, TILE_ROW_MAJOR),
    ("distance_cpu", "lens_rays", ("lens",), dict(distance=torch.zeros((LH, LW))), (), TypeError, kind("distance", contiguous=False)),
    ("distance_kind_before_shape", "lens_rays", ("lens",), dict(distance=_t((LH + 1, LW), torch.float64)), (), TypeError, kind("distance", contiguous=False)),
    ("distance_a_row_short", "lens_rays", ("lens",), dict(distance=_t((LH - 1, LW))), (), ValueError, DISTANCE_SHAPE),
    ("distance_narrow", "lens_rays", ("lens",), dict(distance=_t((LH, LW - 1))), (), ValueError, DISTANCE_SHAPE),
    ("distance_every_other_texel", "lens_rays", ("lens",), dict(distance=_t((LH, 2 * LW))[:, ::2]), (), ValueError, DISTANCE_SHAPE),
    ("distance_flat", "lens_rays", ("lens",), dict(distance=_t((LH * LW,))), (), ValueError, DISTANCE_SHAPE),
    ("distance_shape_before_symbol", "lens_rays", ("lens",), dict(distance=_t((LH, LW, 1))), ("atmo_lens_rays",), ValueError, DISTANCE_SHAPE),
    ("no_lens_rays", "lens_rays", ("lens",), {}, ("atmo_lens_rays", "atmo_lens_ray_counts"), RuntimeError,
     missing("atmo_lens_rays", "atmo_lens.h", ": no lens rays")),
    ("no_lens_ray_counts", "lens_rays", ("lens",), {}, ("atmo_lens_ray_counts",), RuntimeError, missing("atmo_lens_ray_counts", "atmo_lens.h", ": no lens rays")),
    # render_lens: out's kind, out's shape, then lens_rays' own
    ("image_cpu", "render_lens", ("lens",), dict(quads=False, out=torch.zeros((5, LW, 4))), (), TypeError, kind("out")),
    ("image_kind_before_shape", "render_lens", ("lens",), dict(quads=False, out=_t((5, LW, 3), torch.float16)), (), TypeError, kind("out")),
    ("image_strided", "render_lens", ("lens",), dict(quads=True, out=_t((5, LW, 8))[:, :, ::2]), (), TypeError, kind("out")),
    ("image_shape_before_distance_kind", "render_lens", ("lens",), dict(quads=False, out=_t((LH, LW, 4)), distance=torch.zeros((LH, LW))), (), ValueError,
     f"out must have shape (5, {LW}, 4)"),
    ("image_distance_kind", "render_lens", ("lens",), dict(quads=True, distance=torch.zeros((LH, LW))), (), TypeError, kind("distance", contiguous=False)),
    ("image_no_lens_rays", "render_lens", ("lens",), dict(quads=None), ("atmo_lens_rays",), RuntimeError, missing("atmo_lens_rays", "atmo_lens.h", ": no lens rays")),
]
# ... and on a cloud node with cloud detail on: the detail entry points' header, behind the same checks
DETAIL_REFUSALS = [
    ("detail_out_rows_before_symbol", "shade_rays", ("rays", "cam"), dict(out=_t((11, 4))), ("atmo_shade_rays_detail",), ValueError, OUT_ROWS),
    ("no_shade_rays_detail", "shade_rays", ("rays", "cam"), dict(out="out"), ("atmo_shade_rays_detail",), RuntimeError,
     missing("atmo_shade_rays_detail", "atmo_ray_detail.h", ": no cloud detail for rays")),
    ("no_shade_rays_detail_with_an_index", "shade_rays", ("rays", "cam"), dict(out="out", index="index"), ("atmo_shade_rays_detail",), RuntimeError,
     missing("atmo_shade_rays_detail", "atmo_ray_detail.h", ": no cloud detail for rays")),
    ("no_shade_ray_quads_detail", "shade_ray_quads", ("rays", "cam"), dict(width=6, out="out"), ("atmo_shade_ray_quads_detail",), RuntimeError,
     missing("atmo_shade_ray_quads_detail", "atmo_ray_detail.h", ": no cloud detail for rays")),
]


def _refused(rig, node, method, args, kw, exc, message):
    good = dict(_good(), lens=_lens())
    pick = lambda v: good[v] if isinstance(v, str) and v in good else v      # noqa: E731
    with pytest.raises(exc) as e:
        rig.run(getattr(node, method), *[pick(a) for a in args], **{k: pick(v) for k, v in kw.items()}, stream=STREAM)
    assert type(e.value) is exc and str(e.value) == message
    assert node._lib.calls == []


@pytest.mark.parametrize("method,args,kw,without,exc,message", [pytest.param(*row[1:], id=f"{row[1]}-{row[0]}") for row in REFUSALS])
def test_a_bad_argument_is_refused(rig, method, args, kw, without, exc, message):
    _refused(rig, _ray_node(bake=True, lib=Lib(without=without)), method, args, kw, exc, message)


@pytest.mark.parametrize("method,args,kw,without,exc,message", [pytest.param(*row[1:], id=f"{row[1]}-{row[0]}") for row in DETAIL_REFUSALS])
def test_a_bad_argument_is_refused_on_a_detail_node(rig, method, args, kw, without, exc, message):
    _refused(rig, _ray_node(detail=True, bake=True, lib=Lib(without=without)), method, args, kw, exc, message)


def test_every_message_of_the_ray_methods_is_in_the_table():
    said = {row[6] for row in REFUSALS + DETAIL_REFUSALS}
    assert {kind("rays"), kind("quads"), kind("out"), kind("index", "int32"), kind("count", "int32"), kind("depth"), kind("distance", contiguous=False),
            RAYS_SHAPE, QUADS_SHAPE, OUT_SHAPE, INDEX_SHAPE, INTEGERS, QUAD_INTEGERS, RANGE, QUAD_RANGE, OUT_ROWS, QUAD_OUT_ROWS, FOUR_ROWS, TOO_MANY,
            COUNT_ONE, TILE_ROW_MAJOR, DISTANCE_SHAPE, DEPTH_SHAPE} <= said
    assert {row[6] for row in REFUSALS + DETAIL_REFUSALS if row[5] is RuntimeError} >= {
        missing(n, h, s) for n, h, s in [("atmo_shade_rays", "atmo_rays.h", ""), ("atmo_debug_frame_rays", "atmo_rays.h", ""),
                                         ("atmo_shade_ray_quads", "atmo_ray_quads.h", ""), ("atmo_shade_rays_indexed", "atmo_ray_order.h", ""),
                                         ("atmo_ray_order", "atmo_ray_order.h", ""), ("atmo_ray_order_scratch_bytes", "atmo_ray_order.h", ""),
                                         ("atmo_ray_list", "atmo_ray_list.h", ""), ("atmo_ray_list_scratch_bytes", "atmo_ray_list.h", ""),
                                         ("atmo_shade_rays_detail", "atmo_ray_detail.h", ": no cloud detail for rays"),
                                         ("atmo_shade_ray_quads_detail", "atmo_ray_detail.h", ": no cloud detail for rays"),
                                         ("atmo_lens_rays", "atmo_lens.h", ": no lens rays"), ("atmo_lens_ray_counts", "atmo_lens.h", ": no lens rays")]}
    assert len(RAY_ENTRIES) == 12
