"""GPU tests of the multi-view draw into packed and pitched colour targets (include/atmo_views_target.h): atmo_render_views_target against
atmo_render_target of every view on its own.  Every picture comparison is BIT-EXACT on the raw 16- / 8- / 32-bit patterns (np.array_equal; no tolerance):
the header's contract is that a view's bytes do not depend on the views drawn with it, on the order the tiles of the batch run in, nor on the batch at
all.  Every output sits inside a sentinel-filled buffer that is compared WHOLE: the guards in front of and behind it, and the 7 pixels of padding behind
every row of a pitched output, must come back untouched.  One test goes to the numpy statement of the formats (godot_atmosphere_shader_amd/targets.py),
so that the file is not only self-comparison."""
import numpy as np
import pytest
import torch

from common import demo_textures, has_clouds, kernel_flags, make_node
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T
from test_views_gpu import BIG, FAMILY_CASES, SMALL, SMALL_RECT

pytestmark = pytest.mark.gpu

KF_VIEWS = 2048
GUARD = 64                       # sentinel pixels in front of and behind every buffer
PAD = 7                          # sentinel pixels behind every row of a pitched buffer
FORMATS = ("rgba16f", "rgba8")
BYTE_FORMATS = ("rgba8", "rgba8_srgb", "bgra8", "bgra8_srgb", "a2b10g10r10")     # uint8 tensors, four bytes a pixel as they lie in memory
BITS = {"rgba16f": np.uint16, "rgba32f": np.uint32, **{f: np.uint8 for f in BYTE_FORMATS}}
SENTINEL = {"rgba16f": 0x5A5A, "rgba32f": 0x7FC5A5A5, **{f: 0xA5 for f in BYTE_FORMATS}}     # (0x7FC5A5A5: a NaN pattern no kernel produces)
PX_BYTES = {"rgba16f": 8, "rgba32f": 16, **{f: 4 for f in BYTE_FORMATS}}


class Buf:
    """A (rows, cols, 4) colour tensor of `fmt` whose rows are cols + pad pixels apart, inside a sentinel-filled allocation with GUARD pixels in front of
    and behind it.  `view` is what a draw gets; `bits()` is the whole allocation's raw patterns, (GUARD + rows * (cols + pad) + GUARD, 4)."""

    def __init__(self, rows, cols, fmt, pad=0, fill=None):
        self.rows, self.cols, self.fmt, self.pad = rows, cols, fmt, pad
        n = rows * (cols + pad)
        host = np.full((2 * GUARD + n, 4), SENTINEL[fmt], dtype=BITS[fmt])
        if fill is not None:
            host[GUARD:GUARD + n].reshape(rows, cols + pad, 4)[:, :cols] = fill
        self.whole = torch.from_numpy(host.view(T.DTYPES[T.format_id(fmt)])).cuda()
        self.view = self.whole[GUARD:GUARD + n].view(rows, cols + pad, 4)[:, :cols]
        assert self.view.shape == (rows, cols, 4) and (n == 0 or self.view.data_ptr() % PX_BYTES[fmt] == 0)

    def bits(self):
        return self.whole.detach().cpu().numpy().view(BITS[self.fmt])

    def picture(self, bits=None):
        bits = self.bits() if bits is None else bits
        return bits[GUARD:GUARD + self.rows * (self.cols + self.pad)].reshape(self.rows, self.cols + self.pad, 4)[:, :self.cols]

    def outside_intact(self, bits=None):
        """The guards and the padding behind every row still hold the sentinel."""
        bits = self.bits() if bits is None else bits
        n = self.rows * (self.cols + self.pad)
        body = bits[GUARD:GUARD + n].reshape(self.rows, self.cols + self.pad, 4)
        return bool(np.all(bits[:GUARD] == SENTINEL[self.fmt]) and np.all(bits[GUARD + n:] == SENTINEL[self.fmt])
                    and np.all(body[:, self.cols:] == SENTINEL[self.fmt]))


def _random_dst(shape, fmt, seed):
    """Pseudo-random destination bits: every finite half pattern / every byte / finite floats with alphas in [0, 1] are drawn from."""
    rng = np.random.default_rng(seed)
    if fmt in BYTE_FORMATS:
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    if fmt == "rgba32f":
        a = rng.uniform(-0.25, 2.0, size=shape).astype(np.float32)
        a[..., 3] = rng.uniform(0.0, 1.0, size=shape[:-1]).astype(np.float32)
        return a.view(np.uint32)
    allh = np.arange(65536, dtype=np.uint16)
    finite = allh[(allh & 0x7C00) != 0x7C00]
    return finite[rng.integers(0, finite.size, size=shape)]


def _depth(cam):
    return torch.from_numpy(S.depth_ground_sphere(cam)).cuda()


def _full(cams, rects):
    return [r or (0, 0, c.width, c.height) for c, r in zip(cams, rects)]


def _shape(cam, rect, composite):
    x0, y0, x1, y1 = rect
    return (cam.height, cam.width) if composite else (max(y1 - y0, 0), max(x1 - x0, 0))


def _single_draws(node, cams, depths, rects, fmt, pads, composite):
    """Every view on its own (atmo_render_target through node.render / node.render_composite) into the same kind of buffer: the whole buffers' bits."""
    want = []
    for i, (cam, depth, rect, full) in enumerate(zip(cams, depths, rects, _full(cams, rects))):
        rows, cols = _shape(cam, full, composite)
        buf = Buf(rows, cols, fmt, pads[i], _random_dst((rows, cols, 4), fmt, 100 + i) if composite else None)
        if rows and cols and full[2] > full[0] and full[3] > full[1]:
            if composite:
                node.render_composite(cam, depth, buf.view, rect=rect)
            else:
                node.render(cam, depth, out=buf.view, rect=rect)
        torch.cuda.synchronize()
        assert buf.outside_intact(), ("single draw wrote outside its pixels", i)
        want.append(buf.bits().copy())
    return want


def _batch_bufs(cams, rects, fmt, pads, composite):
    bufs = []
    for i, (cam, full) in enumerate(zip(cams, _full(cams, rects))):
        rows, cols = _shape(cam, full, composite)
        bufs.append(Buf(rows, cols, fmt, pads[i], _random_dst((rows, cols, 4), fmt, 100 + i) if composite else None))
    return bufs


def _check_batch(node, cams, depths, rects, fmt, pads, label, family="atmo_render_views_target_kernel<"):
    """Plain and composite: every view of one batch == its own atmo_render_target draw, bytes outside the pixels untouched."""
    for composite in (False, True):
        want = _single_draws(node, cams, depths, rects, fmt, pads, composite)
        single_name = node.kernel_name
        bufs = _batch_bufs(cams, rects, fmt, pads, composite)
        got = node.render_views(cams, depths, outs=[b.view for b in bufs], rects=rects, composite=composite)
        torch.cuda.synchronize()
        assert node.kernel_name.startswith(family), node.kernel_name
        assert kernel_flags(node) == int(single_name.split("<")[1].split(",")[0]) + KF_VIEWS, (node.kernel_name, single_name)
        assert node.kernel_name.split(",")[1].strip(" >") == single_name.split(",")[1].strip(" >"), (node.kernel_name, single_name)
        for i, buf in enumerate(bufs):
            bits = buf.bits()
            assert got[i] is buf.view
            assert buf.outside_intact(bits), (label, fmt, composite, "bytes outside view", i)
            assert np.array_equal(bits, want[i]), (label, fmt, composite, i)
            if buf.rows and buf.cols and _full(cams, rects)[i][2] > _full(cams, rects)[i][0] and _full(cams, rects)[i][3] > _full(cams, rects)[i][1]:
                before = _random_dst((buf.rows, buf.cols, 4), fmt, 100 + i) if composite else np.full((buf.rows, buf.cols, 4), SENTINEL[fmt], dtype=BITS[fmt])
                assert not np.array_equal(buf.picture(bits), before), (label, fmt, composite, i, "the view changes nothing")


def _two_cams():
    return [S.Camera.from_pose(*BIG, "P_space"), S.Camera.from_pose(*SMALL, "P_limb")]


# ---- 1. every kernel ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config,kw,sampler", FAMILY_CASES, ids=[f"{c}{'_direct%d' % kw['light_steps'] if kw else ''}_{s}" for c, kw, s in FAMILY_CASES])
def test_packed_views_equal_their_own_target_draws(config, kw, sampler):
    """Two views with different poses and sizes -- 251 x 141 whole and tight, 96 x 64 with an odd-origin partial rect and pitched -- in one launch, for
    every kernel of the family, RGBA16F and RGBA8, plain and composite over pseudo-random destination bits."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node(config, tex, sampler=sampler, **kw)
    cams = _two_cams()
    depths = [_depth(c) for c in cams]
    for fmt in FORMATS:
        _check_batch(node, cams, depths, [None, SMALL_RECT], fmt, [0, PAD], f"{config} {sampler}")
    if has_clouds(config):
        assert bool(kernel_flags(node) & 32) == (sampler == "declared")
    node.close()


# ---- 2. the numpy statement of the formats -------------------------------------------------------------------------------------------------------

def test_packed_views_are_the_encoded_float_views():
    """clouds_high_rm under the declared sampler: the plain batch == targets.encode(the float batch's output), the composite == targets.blend(float
    source, destination bits) -- a discarded fragment leaves its destination alone."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    cams = _two_cams()
    depths = [_depth(c) for c in cams]
    rects = [None, SMALL_RECT]
    src = [o.cpu().numpy() for o in node.render_views(cams, depths, rects=rects)]
    full_src = [o.cpu().numpy() for o in node.render_views(cams, depths)]             # the composite's sources: whole viewports
    cleared = make_node("clouds_high_rm", tex, target_cleared=True)
    nan_outs = [torch.full((c.height, c.width, 4), float("nan"), dtype=torch.float32, device="cuda") for c in cams]
    cleared.render_views(cams, depths, outs=nan_outs)
    torch.cuda.synchronize()
    discarded = [torch.isnan(o).all(dim=-1).cpu().numpy() for o in nan_outs]
    cleared.close()
    assert all(0.05 <= d.mean() <= 0.95 for d in discarded), [d.mean() for d in discarded]
    for fmt in FORMATS:
        outs = node.render_views(cams, depths, rects=rects, target=fmt)
        torch.cuda.synchronize()
        assert node.kernel_name.startswith("atmo_render_views_target_kernel<")
        for i in range(2):
            assert outs[i].dtype == {"rgba16f": torch.float16, "rgba8": torch.uint8}[fmt]
            assert np.array_equal(outs[i].cpu().numpy().view(BITS[fmt]), T.encode(src[i], fmt).view(BITS[fmt])), (fmt, "plain", i)
        dst = [_random_dst((c.height, c.width, 4), fmt, 7 + i) for i, c in enumerate(cams)]
        bufs = [Buf(c.height, c.width, fmt, PAD * i, d) for i, (c, d) in enumerate(zip(cams, dst))]
        node.render_views(cams, depths, outs=[b.view for b in bufs], rects=rects, composite=True)
        torch.cuda.synchronize()
        for i, (cam, rect) in enumerate(zip(cams, _full(cams, rects))):
            x0, y0, x1, y1 = rect
            blended = T.blend(full_src[i], dst[i].view(T.DTYPES[T.format_id(fmt)]), fmt).view(BITS[fmt])
            want = dst[i].copy()
            inside = np.zeros((cam.height, cam.width), dtype=bool)
            inside[y0:y1, x0:x1] = True
            write = inside & ~discarded[i]
            want[write] = blended[write]
            assert bufs[i].outside_intact() and np.array_equal(bufs[i].picture(), want), (fmt, "composite", i)
    node.close()


# ---- 3. split screen in one image ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_split_screen_halves_of_one_image(fmt):
    """One pitched 192 x 64 image, two 96 x 64 views with pixels = image and image + 96 pixels, pitch = the image's row: the layout the float batch has
    to refuse.  Plain and composite; each half == its own atmo_render_target draw into the same layout; bytes outside the image are untouched."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    cams = [S.Camera.from_pose(96, 64, "P_space"), S.Camera.from_pose(96, 64, "P_limb")]
    depths = [_depth(c) for c in cams]
    for composite in (False, True):
        fill = _random_dst((64, 192, 4), fmt, 31) if composite else None
        images = [Buf(64, 192, fmt, PAD, fill) for _ in range(2)]
        halves = [[img.view[:, :96], img.view[:, 96:]] for img in images]
        assert halves[0][1].data_ptr() == halves[0][0].data_ptr() + 96 * PX_BYTES[fmt] and halves[0][0].stride(0) == (192 + PAD) * 4
        for i in range(2):            # image 0: one draw per half
            (node.render_composite(cams[i], depths[i], halves[0][i]) if composite else node.render(cams[i], depths[i], out=halves[0][i]))
        torch.cuda.synchronize()
        node.render_views(cams, depths, outs=halves[1], composite=composite)       # image 1: one batch
        torch.cuda.synchronize()
        assert node.kernel_name.startswith("atmo_render_views_target_kernel<")
        want, got = images[0].bits(), images[1].bits()
        assert images[0].outside_intact(want) and images[1].outside_intact(got), (fmt, composite)
        assert np.array_equal(got, want), (fmt, composite)
        before = fill if composite else np.full((64, 192, 4), SENTINEL[fmt], dtype=BITS[fmt])
        for half in (slice(0, 96), slice(96, 192)):
            assert not np.array_equal(images[1].picture(got)[:, half], before[:, half]), (fmt, composite, "a half was not drawn")
    # ... and as two rects of ONE 192 x 64 viewport, composite: the same camera, one scene buffer
    cam = S.Camera.from_pose(192, 64, "P_space")
    depth = _depth(cam)
    fill = _random_dst((64, 192, 4), fmt, 32)
    images = [Buf(64, 192, fmt, PAD, fill) for _ in range(2)]
    rects = [(0, 0, 96, 64), (96, 0, 192, 64)]
    for r in rects:
        node.render_composite(cam, depth, images[0].view, rect=r)
    node.render_views([cam, cam], [depth, depth], outs=[images[1].view, images[1].view], rects=rects, composite=True)
    torch.cuda.synchronize()
    assert images[1].outside_intact() and np.array_equal(images[1].bits(), images[0].bits())
    node.close()


# ---- 4. RGBA32F ----------------------------------------------------------------------------------------------------------------------------------

def test_rgba32f_batches_are_the_float_batch():
    """RGBA32F targets go through the kernels of atmo_render_views: a tight batch is atmo_render_views byte for byte, a pitched one N x atmo_render_target."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    cams = _two_cams()
    depths = [_depth(c) for c in cams]
    rects = [None, SMALL_RECT]
    # pitched (and one tight view beside a pitched one): against the single target draws
    _check_batch(node, cams, depths, rects, "rgba32f", [PAD, PAD], "rgba32f pitched", family="atmo_render_views_kernel<")
    _check_batch(node, cams, depths, rects, "rgba32f", [0, PAD], "rgba32f tight + pitched", family="atmo_render_views_kernel<")
    # tight, through atmo_render_views_target itself (node.render_views hands tight float32 tensors to atmo_render_views)
    for composite in (False, True):
        fills = [_random_dst((*_shape(c, r, composite), 4), "rgba32f", 100 + i) if composite else None for i, (c, r) in enumerate(zip(cams, _full(cams, rects)))]
        a = [Buf(*_shape(c, r, composite), "rgba32f", 0, f) for c, r, f in zip(cams, _full(cams, rects), fills)]
        b = [Buf(*_shape(c, r, composite), "rgba32f", 0, f) for c, r, f in zip(cams, _full(cams, rects), fills)]
        node.render_views(cams, depths, outs=[x.view for x in a], rects=rects, composite=composite)
        torch.cuda.synchronize()
        float_name = node.kernel_name
        tgts = [N.AtmoTarget(x.view.data_ptr(), N.TARGET_RGBA32F, 0) for x in b]
        views = node.prepare_views_target(cams, [d.data_ptr() for d in depths], tgts, rects)
        node.render_views_target_prepared(views, 2, composite, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert node.kernel_name == float_name and float_name.startswith("atmo_render_views_kernel<")
        for x, y in zip(a, b):
            assert y.outside_intact() and np.array_equal(y.bits(), x.bits()), composite
    node.close()


# ---- 5. view counts ------------------------------------------------------------------------------------------------------------------------------

def test_packed_view_counts():
    """One view; eight small views with one empty and differing pitches; zero views."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    cam = S.Camera.from_pose(*BIG, "P_space")
    for fmt in FORMATS:
        _check_batch(node, [cam], [_depth(cam)], [(17, 9, 250, 141)], fmt, [PAD], "one view")
    poses = ["P_space", "P_ground", "P_limb", "P_clouds", "P_night", "P_space", "P_limb", "P_night"]
    sizes = [(96, 64), (80, 48), (64, 40), (112, 56), (96, 64), (48, 32), (72, 72), (96, 54)]
    cams = [S.Camera.from_pose(w, h, p) for (w, h), p in zip(sizes, poses)]
    rects = [None, (1, 3, 79, 47), None, (40, 20, 40, 50), None, (3, 3, 47, 31), None, (0, 1, 96, 53)]   # view 3 is empty
    depths = [_depth(c) for c in cams]
    for fmt in FORMATS:
        _check_batch(node, cams, depths, rects, fmt, [0, PAD, 1, 3, 2 * PAD, 0, 5, PAD], "eight views")
    assert node.render_views([], [], target="rgba16f") == []
    views = node.prepare_views_target([], [], [])
    node.render_views_target_prepared(views, 0)
    with pytest.raises(ValueError):
        node.render_views([cam] * 9, [_depth(cam)] * 9, target="rgba8")
    node.close()


# ---- 6. order independence -----------------------------------------------------------------------------------------------------------------------

def test_packed_pictures_do_not_depend_on_the_tile_order():
    """Two 640 x 360 clouds_high_rm views (3 600 tiles), a still camera, 16 RGBA16F batches into pitched outputs: every one is bit for bit the separate
    draws, the learnt order is in use by the end (feedback_stats), and the same run with atmo_set_tile_feedback(0) gives the same bytes."""
    tex = demo_textures(cube_n=64, shape_n=32)
    cams = [S.Camera.from_pose(640, 360, "P_space"), S.Camera.from_pose(640, 360, "P_limb")]
    depths = [_depth(c) for c in cams]
    fmt = "rgba16f"
    ref_node = make_node("clouds_high_rm", tex, tile_feedback=0)
    want = _single_draws(ref_node, cams, depths, [None, None], fmt, [PAD, PAD], False)
    ref_node.close()
    for feedback in (-1, 0):
        node = make_node("clouds_high_rm", tex, tile_feedback=feedback)
        before = node.feedback_stats()
        first = None
        for k in range(16):
            bufs = _batch_bufs(cams, [None, None], fmt, [PAD, PAD], False)
            node.render_views(cams, depths, outs=[b.view for b in bufs])
            torch.cuda.synchronize()
            got = [b.bits() for b in bufs]
            first = first or got
            for i in range(2):
                assert np.array_equal(got[i], first[i]) and np.array_equal(got[i], want[i]), (feedback, k, i)
        st = node.feedback_stats()
        print(f"\ntile_feedback {feedback}: {st}")
        if feedback == 0:
            assert st["ordered_draws"] == before["ordered_draws"] and st["sorts"] == before["sorts"]
        else:
            assert st["ordered_draws"] - before["ordered_draws"] >= 4 and st["sorts"] - before["sorts"] >= 1 and st["states"] == 1
        node.close()


# ---- 7. on the device: refusals and the staging ring ---------------------------------------------------------------------------------------------

def test_mixed_formats_are_refused_and_nothing_is_written():
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high", tex)
    cams = _two_cams()
    depths = [_depth(c) for c in cams]
    bufs = [Buf(BIG[1], BIG[0], "rgba16f", PAD), Buf(SMALL[1], SMALL[0], "rgba8", 0)]
    with pytest.raises(N.AtmoError) as ei:
        node.render_views(cams, depths, outs=[b.view for b in bufs])
    assert ei.value.code == N.ATMO_E_ARG and "view 1" in str(ei.value) and "one format per batch" in str(ei.value)
    torch.cuda.synchronize()
    for b in bufs:
        assert np.all(b.bits() == SENTINEL[b.fmt])
    # overlapping halves are refused on the device too, and nothing is written
    img = Buf(64, 192, "rgba8", 0)
    small = [S.Camera.from_pose(96, 64, "P_space"), S.Camera.from_pose(96, 64, "P_limb")]
    with pytest.raises(N.AtmoError) as ei:
        node.render_views(small, [_depth(c) for c in small], outs=[img.view[:, :96], img.view[:, 95:191]])
    assert ei.value.code == N.ATMO_E_ARG and "overlapping" in str(ei.value)
    torch.cuda.synchronize()
    assert np.all(img.bits() == SENTINEL["rgba8"])
    node.close()


def test_packed_views_refuse_graph_capture():
    """As atmo_render_views: on a capturing stream atmo_render_views_target returns ATMO_E_STATE and leaves the capture usable; outside a capture the
    batch works as before."""
    tex = demo_textures(cube_n=64, shape_n=32)
    cams = [S.Camera.from_pose(320, 180, "P_space"), S.Camera.from_pose(320, 180, "P_limb")]
    depths = [_depth(c) for c in cams]
    node = make_node("clouds_high", tex)
    refs = [node.render(c, d, target="rgba16f").clone() for c, d in zip(cams, depths)]
    torch.cuda.synchronize()
    outs = [torch.zeros_like(r) for r in refs]
    tgts = [N.AtmoTarget(o.data_ptr(), N.TARGET_RGBA16F, 0) for o in outs]
    views = node.prepare_views_target(cams, [d.data_ptr() for d in depths], tgts)
    frame = node.prepare_frame(cams[0])
    scratch = torch.zeros((180, 320, 4), dtype=torch.float32, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(N.AtmoError) as ei:
                node.render_views_target_prepared(views, 2, False, side.cuda_stream)
            assert ei.value.code == N.ATMO_E_STATE and "atmo_render_views_target" in str(ei.value)
            node.render_prepared(frame, depths[0].data_ptr(), scratch.data_ptr(), side.cuda_stream)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert scratch.any() and not outs[0].view(torch.int16).any() and not outs[1].view(torch.int16).any()
    node.render_views_target_prepared(views, 2, False, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for o, r in zip(outs, refs):
        assert torch.equal(o.view(torch.int16), r.view(torch.int16))
    node.close()


def test_packed_batches_can_be_enqueued_ahead():
    """20 RGBA8 batches with a new pose each, back to back without a host synchronisation, into 20 output sets: each equals its separate draws -- a
    staging slot of the per-view constants reused too early would shade a batch with a later batch's cameras; 20 wraps the ring of 16 slots."""
    tex = demo_textures(cube_n=64, shape_n=32)
    node = make_node("clouds_high_rm", tex)
    w, h, fmt = 160, 90, "rgba8"

    def cams_of(k):
        a = 0.05 * k
        return [S.Camera(w, h, (160.0 * np.sin(a), 10.0 + k, 160.0 * np.cos(a)), (0.0, 0.0, 0.0)),
                S.Camera(w, h, (160.0 * np.sin(a) + 3.0, 10.0 + k, 160.0 * np.cos(a)), (0.0, 0.0, 0.0))]

    batches = [cams_of(k) for k in range(20)]
    depths = [[_depth(c) for c in cams] for cams in batches]
    bufs = [[Buf(h, w, fmt, PAD * i) for i in range(2)] for _ in batches]
    torch.cuda.synchronize()
    for k, cams in enumerate(batches):              # no synchronisation in here
        node.render_views(cams, depths[k], outs=[b.view for b in bufs[k]])
    torch.cuda.synchronize()
    got = [[b.bits() for b in pair] for pair in bufs]
    for k, cams in enumerate(batches):
        want = _single_draws(node, cams, depths[k], [None, None], fmt, [0, PAD], False)
        for i in range(2):
            assert np.array_equal(got[k][i], want[i]), (k, i)
    assert not np.array_equal(got[0][0], got[1][0])   # the poses differ
    node.close()
