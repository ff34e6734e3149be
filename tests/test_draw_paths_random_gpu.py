"""GPU tests that hold every draw path to the single draw ON THE RANDOM SCENES of the fuzz (tests/random_scenes.py): packed and pitched targets, view
batches, depth sources, the far mode's box proxy, its batches and the planets of one frame.  Each of those paths is a separately compiled twin kernel that the
headers promise to be its own single draw bit for bit; the twins' own test files hold them to that on the demo scene only (a planet at the origin,
power-of-two textures, the compile-time step counts).  Here they get what the random scenes carry: cubemap faces and shape volumes that are no power of
two, an unset cubemap, run-time light-step counts, 12 / 16 / 32 view steps and 8 / 24 cloud steps, the fuzz's range of radius, density, sphere-depth
factor, shape inversion and coverage rotation, cameras inside the atmosphere, and a moved and rotated planet.

Every comparison is on bits (np.array_equal, no tolerance), and its reference is never the path under test: it is the existing single draw into float
RGBA (`render` / `render_composite`, which the oracle holds on these scenes: test_parity_random_scenes, and `test_single_draws_match_the_oracle` here
for the moved planets and the far cameras), or the numpy statement of a contract (targets.encode, targets.blend, depth_formats.decode).  Every buffer
lies between sentinel guards with a pitched pad behind each row (test_views_target_gpu.Buf).  tests/test_random_scenes_host.py proves on the CPU oracle
that the frames hold something; the `drawn` fixture asserts the same of the single draws.

Notation: N the seed's near camera (placed with the planet), F the far camera, F2 a second far camera, Rn the odd-origin partial rect."""
import ctypes as C

import numpy as np
import pytest
import torch

import proxy_geometry as G
import random_scenes as RS
from common import TOL
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import depth_formats as D
from godot_atmosphere_shader_amd import planet_atmosphere as PA
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T
from godot_atmosphere_shader_amd.planet_atmosphere import depth_source
from test_depth_gpu import CARRIER, DPAD, NEAR_FILL
from test_proxy_gpu import _check_composite, _pattern, _same_bits
from test_views_target_gpu import BITS, PAD, Buf, _random_dst

pytestmark = pytest.mark.gpu

KF_PROXY, KF_TARGET, KF_VIEWS, KF_DEPTH = 512, 1024, 2048, 4096
FORMATS = ("rgba32f", "rgba16f", "rgba8", "rgba8_srgb", "bgra8", "bgra8_srgb", "a2b10g10r10")     # the seven formats of targets.FORMATS, by value
assert sorted({T.FORMATS[f] for f in FORMATS}) == sorted(set(T.FORMATS.values())) and [T.FORMATS[f] for f in FORMATS] == sorted(T.FORMATS[f] for f in FORMATS)
DEPTH_FORMATS = ("d16", "x8d24", "d32f")
MIN_SHADED = 0.10          # what tests/test_random_scenes_host.py proves of the oracle's frames
# A scene with u_sphere_depth_factor = 1 takes the ground from the analytic sphere and none of it from the depth buffer (linear_depth * (1 - factor) +
# sphere * factor): no depth decoder can show in its frame.  Its depth-source draws are compared as they are, and once more with this factor, under which
# the buffer is read (tests/test_random_scenes_host.py::test_depth_sources_show_in_the_far_frame proves both statements on the oracle).
DEPTH_SOURCE_FACTOR = RS.DEPTH_SOURCE_FACTOR


def seed_formats(seed):
    """Two of the seven per seed, so that all seven occur over the list."""
    return FORMATS[seed % 7], FORMATS[(seed + 3) % 7]


def packed_format(seed):
    """The seed's packed byte format: the first of its two that is neither float format."""
    return [f for f in seed_formats(seed) if f not in ("rgba32f", "rgba16f")][0]


def _shaded(frame):
    return float(np.any(frame != 0.0, axis=-1).mean())


def _name(kernel_name):
    """("atmo_render_views_kernel", FLAGS, LSTEPS) of a kernel's name."""
    family, args = kernel_name.rstrip(">").split("<")
    args = [int(a) for a in args.split(",")]
    return family, args[0], args[1]


_launched = []          # the kernel names `_expect` has seen since the last `_report` (for the record in profiles/draw_paths_fuzz/)


def _report(what):
    print(f"{what}: {' '.join(sorted(set(_launched)))}")
    _launched.clear()


def _expect(kernel_name, family, base_name, extra_flags):
    """`kernel_name` names `family` with the flags of the single float draw's kernel plus the twin's, and the same light-step argument."""
    _launched.append(kernel_name)
    fam, flags, lsteps = _name(kernel_name)
    base_family, base_flags, base_lsteps = _name(base_name)
    assert base_family == "atmo_render_kernel", base_name
    assert (fam, flags, lsteps) == (family, base_flags + extra_flags, base_lsteps), (kernel_name, family, base_name, extra_flags)


def _target_flag(fmt):
    return 0 if fmt == "rgba32f" else KF_TARGET           # RGBA32F targets, tight or pitched, are drawn by the float kernels


def _family(views=False, proxy=False, fmt="rgba32f", depth=False):
    packed = "_target" if (depth or fmt != "rgba32f") else ""
    return f"atmo_render{'_views' if views else ''}{'_proxy' if proxy else ''}{'_depth' if depth else ''}{packed}_kernel"


def _flags(views=False, proxy=False, fmt="rgba32f", depth=False):
    return (KF_VIEWS if views else 0) + (KF_PROXY if proxy else 0) + ((KF_TARGET | KF_DEPTH) if depth else _target_flag(fmt))


class Scene:
    """A seed's scene on the device: the cameras, the depth buffers, one node per sampler with its single float draws (the references)."""

    def __init__(self, seed):
        self.seed = seed
        self.params, self.tex, self.M, self.N, self.sun, self.dN_np = RS.placed(seed)
        (self.F, self.dF_np), (self.F2, self.dF2_np) = RS.far_camera(seed), RS.far_camera(seed, 1)
        self.dN, self.dF, self.dF2 = (torch.from_numpy(d).cuda() for d in (self.dN_np, self.dF_np, self.dF2_np))
        self.Rn = RS.partial_rect(self.N)
        self.shader, self.ocfg, kw = RS.variant_of(seed, RS.VARIANTS_BATCH)
        self.draws = []          # (cubemap_lod, node, near float frame, far float frame, the single float draw's kernel name)
        for lod in RS.samplers(seed, self.tex):
            node = RS.make_node(self.params, self.tex, self.sun, self.N, self.shader, kw, lod, model=self.M)
            near = node.render(self.N, self.dN).cpu().numpy()
            far = node.render(self.F, self.dF).cpu().numpy()
            name = node.kernel_name
            declared = lod is None and len(RS.samplers(seed, self.tex)) == 2
            assert name.startswith("atmo_render_kernel<") and bool(_name(name)[1] & 32) == declared, (name, lod)
            self.draws.append((lod, node, near, far, name))

    def close(self):
        for _, node, *_ in self.draws:
            node.close()


@pytest.fixture(scope="module", params=RS.SEEDS)
def drawn(request):
    """One Scene per seed, shared by the families (pytest runs a seed's tests together); no family passes on nothing: both single draws shade at least a
    tenth of their pixels, which the host file proves of the oracle's frames (and the fuzz asserts the kernels' discard sets to be the oracle's)."""
    sc = Scene(request.param)
    for lod, _, near, far, _ in sc.draws:
        assert _shaded(near) >= MIN_SHADED and _shaded(far) >= MIN_SHADED, (sc.seed, lod, _shaded(near), _shaded(far))
    yield sc
    sc.close()


def _full(cam, rect):
    return rect or (0, 0, cam.width, cam.height)


def _view(dtype_bits, fmt):
    return dtype_bits.view(T.DTYPES[T.format_id(fmt)])


# ---- 1. packed targets ----------------------------------------------------------------------------------------------------------------------------------

def test_packed_targets_are_the_encoded_float_frame(drawn):
    """At N, two formats of the seven, tight and pitched, whole and with Rn: render(target=fmt) == targets.encode(the float frame),
    render_composite == targets.blend(the float frame, the scene's bytes) where the fragment was kept and inside the rect, the scene's bytes elsewhere."""
    sc = drawn
    cam, h, w = sc.N, sc.N.height, sc.N.width
    for lod, node, near, _, base in sc.draws:
        discarded = np.all(near == 0.0, axis=-1)
        for fmt in seed_formats(sc.seed):
            for pad in (0, PAD):
                for rect in (None, sc.Rn):
                    x0, y0, x1, y1 = _full(cam, rect)
                    label = (sc.seed, lod, fmt, pad, rect)
                    buf = Buf(y1 - y0, x1 - x0, fmt, pad)
                    node.render(cam, sc.dN, out=buf.view, rect=rect, target=fmt)
                    torch.cuda.synchronize()
                    _expect(node.kernel_name, _family(fmt=fmt), base, _flags(fmt=fmt))
                    assert buf.outside_intact(), label
                    assert np.array_equal(buf.picture(), T.encode(near[y0:y1, x0:x1], fmt).view(BITS[fmt])), label
                    dst = _random_dst((h, w, 4), fmt, 7 + sc.seed)
                    buf = Buf(h, w, fmt, pad, dst)
                    node.render_composite(cam, sc.dN, buf.view, rect=rect, target=fmt)
                    torch.cuda.synchronize()
                    _expect(node.kernel_name, _family(fmt=fmt), base, _flags(fmt=fmt))
                    want = dst.copy()
                    write = ~discarded
                    write[:y0], write[y1:], write[:, :x0], write[:, x1:] = False, False, False, False
                    want[write] = T.blend(near, _view(dst, fmt), fmt).view(BITS[fmt])[write]
                    assert buf.outside_intact(), label
                    assert np.array_equal(buf.picture(), want), label
                    assert not np.array_equal(want, dst), (label, "the composite changes nothing")
    _report(f"seed {sc.seed} packed targets {seed_formats(sc.seed)}")


# ---- 2. batches against their own single draws ----------------------------------------------------------------------------------------------------------

def _batch_equals_singles(node, cams, depths, rects, fmt, pads, proxy, label, single_depths=None):
    """Plain and composite: every view of ONE batch launch == its own single draw into the same kind of buffer (prefilled: what a draw leaves alone must
    survive), whole sentinel-guarded allocations compared.  `single_depths`: the depths of the single draws where `depths` are depth sources of the same
    values.  Returns [(the single draws' kernel name, the batch's)] for plain and composite."""
    names = []
    size = node.proxy_box_size(cams[0])
    box = dict(box_size=size) if proxy else {}
    single_depths = depths if single_depths is None else single_depths
    for composite in (False, True):
        shapes = [(c.height, c.width) if composite else (y1 - y0, x1 - x0) for c, (x0, y0, x1, y1) in ((c, _full(c, r)) for c, r in zip(cams, rects))]
        fills = [_random_dst((*shapes[i], 4), fmt, 100 + i) for i in range(len(cams))]
        want = []
        for i, (cam, depth, rect) in enumerate(zip(cams, single_depths, rects)):
            buf = Buf(*shapes[i], fmt, pads[i], fills[i])
            if composite:
                (node.render_proxy_composite if proxy else node.render_composite)(cam, depth, buf.view, rect=rect, target=fmt, **box)
            else:
                (node.render_proxy if proxy else node.render)(cam, depth, out=buf.view, rect=rect, target=fmt, **box)
            torch.cuda.synchronize()
            assert buf.outside_intact(), (label, "a single draw wrote outside its pixels", i)
            want.append(buf.bits().copy())
        single_name = node.kernel_name
        bufs = [Buf(*shapes[i], fmt, pads[i], fills[i]) for i in range(len(cams))]
        got = (node.render_views_proxy if proxy else node.render_views)(cams, depths, outs=[b.view for b in bufs], rects=rects, composite=composite,
                                                                         target=fmt, **box)
        torch.cuda.synchronize()
        names.append((single_name, node.kernel_name))
        for i, buf in enumerate(bufs):
            bits = buf.bits()
            assert got[i] is buf.view
            assert buf.outside_intact(bits), (label, fmt, composite, "bytes outside view", i)
            assert np.array_equal(bits, want[i]), (label, fmt, composite, i)
            assert not np.array_equal(buf.picture(bits), fills[i]), (label, fmt, composite, i, "the view changes nothing")
    return names


def test_view_batches_equal_their_own_draws(drawn):
    """render_views([N, N, F], rects=[None, Rn, None]): float, plain and composite, against `render` / `render_composite` -- the plain views are also the
    fixture's float frames --, then into one packed format of the seed and RGBA16F against `render(target=...)`."""
    sc = drawn
    cams, depths, rects = [sc.N, sc.N, sc.F], [sc.dN, sc.dN, sc.dF], [None, sc.Rn, None]
    x0, y0, x1, y1 = sc.Rn
    for lod, node, near, far, base in sc.draws:
        outs = node.render_views(cams, depths, rects=rects)
        torch.cuda.synchronize()
        _expect(node.kernel_name, "atmo_render_views_kernel", base, KF_VIEWS)
        for i, want in enumerate((near, near[y0:y1, x0:x1], far)):
            assert np.array_equal(outs[i].cpu().numpy().view(np.uint32), want.view(np.uint32)), (sc.seed, lod, "float batch", i)
        for fmt, pads in (("rgba32f", [0, 0, 0]), (packed_format(sc.seed), [PAD, 0, PAD]), ("rgba16f", [0, PAD, PAD])):
            for single, batch in _batch_equals_singles(node, cams, depths, rects, fmt, pads, False, (sc.seed, lod)):
                _expect(single, _family(fmt=fmt), base, _flags(fmt=fmt))
                _expect(batch, _family(views=True, fmt=fmt), base, _flags(views=True, fmt=fmt))
    _report(f"seed {sc.seed} view batches")


# ---- 3. the far mode ------------------------------------------------------------------------------------------------------------------------------------

def test_far_mode_is_the_single_draw_on_its_fragments(drawn):
    """At F: render_proxy / render_proxy_composite against render / render_composite on the passing and stable pixels of proxy_geometry.frame_masks
    (test_proxy_gpu._check_composite: unstable pixels excluded, at most 1e-3 of the covered ones); render_proxy(target=fmt) == the encoded float
    proxy frame; render_views_proxy([F, F2, F], rects=[None, None, Rn]) and its target form == each view's own proxy draw."""
    sc = drawn
    cam, h, w = sc.F, sc.F.height, sc.F.width
    cams, depths, rects = [sc.F, sc.F2, sc.F], [sc.dF, sc.dF2, sc.dF], [None, None, RS.partial_rect(sc.F)]
    for lod, node, _, far, base in sc.draws:
        assert abs(node.proxy_box_size(cam) - RS.proxy_box(sc.params, cam)) <= 1e-9 * RS.proxy_box(sc.params, cam)
        full, got, scene, passing = _check_composite(node, cam, sc.dF_np, seed=1 + sc.seed)
        _expect(node.kernel_name, "atmo_render_proxy_kernel", base, KF_PROXY)
        assert passing.sum() >= 300 and bool((got != scene).any()), (sc.seed, lod, int(passing.sum()))
        _, passing, unstable = G.frame_masks(cam, node.global_transform, node.proxy_box_size(cam), sc.dF_np)
        p, s = torch.from_numpy(passing).cuda(), torch.from_numpy(~unstable).cuda()
        fill = _pattern((h, w, 4), 7)
        out = node.render_proxy(cam, sc.dF, out=fill.clone())
        torch.cuda.synchronize()
        ref = torch.from_numpy(far).cuda()
        assert bool(_same_bits(out, ref)[p & s].all()) and bool(_same_bits(out, fill)[~p & s].all()), (sc.seed, lod)
        # the packed proxy draw is the encoded float proxy draw (both into zero-filled buffers: the pixels left alone encode as zeros)
        float_proxy = node.render_proxy(cam, sc.dF).cpu().numpy()
        assert float_proxy[passing & ~unstable].any()
        for fmt in seed_formats(sc.seed):
            buf = Buf(h, w, fmt, PAD, np.zeros((h, w, 4), dtype=BITS[fmt]))
            node.render_proxy(cam, sc.dF, out=buf.view, target=fmt)
            torch.cuda.synchronize()
            _expect(node.kernel_name, _family(proxy=True, fmt=fmt), base, _flags(proxy=True, fmt=fmt))
            assert buf.outside_intact() and np.array_equal(buf.picture(), T.encode(float_proxy, fmt).view(BITS[fmt])), (sc.seed, lod, fmt)
        for fmt, pads in (("rgba32f", [0, 0, 0]), (packed_format(sc.seed), [0, PAD, PAD])):
            for single, batch in _batch_equals_singles(node, cams, depths, rects, fmt, pads, True, (sc.seed, lod)):
                _expect(single, _family(proxy=True, fmt=fmt), base, _flags(proxy=True, fmt=fmt))
                _expect(batch, _family(views=True, proxy=True, fmt=fmt), base, _flags(views=True, proxy=True, fmt=fmt))
    _report(f"seed {sc.seed} far mode")


# ---- 4. depth sources -----------------------------------------------------------------------------------------------------------------------------------

def _texels(depth_np, fmt):
    """The depth quantised to `fmt`; x8d24 with a hashed top byte (as test_depth_gpu's decoder test hashes it: every byte value occurs)."""
    q = D.quantise(depth_np, fmt)
    if fmt == "x8d24":
        q = q | (((q * np.uint32(2654435761)) >> np.uint32(13)) << np.uint32(24))
    return q


def _pitched_source(texels, fmt):
    """A depth_source over a buffer DPAD texels wider than the viewport whose padding holds the near plane; (source, the buffer: keep it alive)."""
    whole = np.full((texels.shape[0], texels.shape[1] + DPAD), NEAR_FILL[fmt], dtype=texels.dtype)
    whole[:, :texels.shape[1]] = texels
    t = torch.from_numpy(whole.view(CARRIER[fmt])).cuda()
    return depth_source(t[:, :texels.shape[1]], fmt), t


def _depth_forms_equal_float_forms(sc, node, base, cam, depth_np, far_forms, label):
    """Every draw from a pitched depth source of the seed's texel format == the same draw from depth_formats.decode(texels) uploaded as tight floats,
    plain and composite, into the seed's packed format, pitched."""
    dfmt, fmt = DEPTH_FORMATS[sc.seed % 3], packed_format(sc.seed)
    texels = _texels(depth_np, dfmt)
    decoded = torch.from_numpy(D.decode(texels, dfmt)).cuda()
    src, _keep = _pitched_source(texels, dfmt)
    h, w = cam.height, cam.width
    Rn = RS.partial_rect(cam)
    single = lambda proxy: lambda d, bufs, comp: (                                                                     # noqa: E731
        ((node.render_proxy_composite if proxy else node.render_composite)(cam, d, bufs[0].view, target=fmt)) if comp else
        ((node.render_proxy if proxy else node.render)(cam, d, out=bufs[0].view, target=fmt)))
    batch = lambda proxy: lambda d, bufs, comp: (node.render_views_proxy if proxy else node.render_views)(             # noqa: E731
        [cam, cam], [d, d], outs=[b.view for b in bufs], rects=[None, Rn], composite=comp, target=fmt)
    forms = [("single", single(False), 1, dict())]
    if far_forms:
        forms += [("views", batch(False), 2, dict(views=True)), ("proxy", single(True), 1, dict(proxy=True)), ("views proxy", batch(True), 2, dict(views=True, proxy=True))]
    for what, draw, n, kind in forms:
        for composite in (False, True):
            shapes = [(h, w)] + ([(h, w) if composite else (Rn[3] - Rn[1], Rn[2] - Rn[0])] if n == 2 else [])
            fills = [_random_dst((*s, 4), fmt, 50 + i) for i, s in enumerate(shapes)]
            want = [Buf(*s, fmt, PAD, f) for s, f in zip(shapes, fills)]
            got = [Buf(*s, fmt, PAD, f) for s, f in zip(shapes, fills)]
            draw(decoded, want, composite)
            torch.cuda.synchronize()
            _expect(node.kernel_name, _family(fmt=fmt, **kind), base, _flags(fmt=fmt, **kind))
            draw(src, got, composite)
            torch.cuda.synchronize()
            _expect(node.kernel_name, _family(fmt=fmt, depth=True, **kind), base, _flags(fmt=fmt, depth=True, **kind))
            for i in range(n):
                assert want[i].outside_intact() and got[i].outside_intact(), (label, what, composite, i)
                assert np.array_equal(got[i].bits(), want[i].bits()), (label, what, dfmt, fmt, composite, i)
                assert not np.array_equal(got[i].picture(), fills[i]), (label, what, composite, i, "the draw changes nothing")


def test_depth_sources_equal_the_decoded_floats(drawn):
    """At F for every seed, at N too where N has ground in its depth buffer (seed % 3 != 0): D16 / X8D24 (hashed top byte) / pitched D32F by seed."""
    sc = drawn
    for lod, node, _, far, base in sc.draws:
        own = float(sc.params["u_sphere_depth_factor"])
        factors = [own] + ([DEPTH_SOURCE_FACTOR] if own == 1.0 else [])      # (the last one is the factor under which the depth buffer is read)
        try:
            for factor in factors:
                node.set("shader_params/u_sphere_depth_factor", factor)
                _depth_forms_equal_float_forms(sc, node, base, sc.F, sc.dF_np, True, (sc.seed, lod, "F", factor))
                if sc.seed % 3 != 0:
                    _depth_forms_equal_float_forms(sc, node, base, sc.N, sc.dN_np, False, (sc.seed, lod, "N", factor))
            # no decoder is tested on nothing: the frame from the D16-decoded floats differs from the far-plane frame on at least half of the ground
            q16 = D.quantise(sc.dF_np, "d16")
            ground = q16 != 0
            dec_frame = node.render(sc.F, torch.from_numpy(D.decode(q16, "d16")).cuda()).cpu().numpy()
            far_frame = node.render(sc.F, torch.from_numpy(S.depth_far(sc.F)).cuda()).cpu().numpy()
            differs = np.any(dec_frame.view(np.uint32) != far_frame.view(np.uint32), axis=-1)
            print(f"seed {sc.seed} sampler {lod}: sphere-depth factor {factors[-1]}: the D16 frame differs from the far-plane frame on "
                  f"{differs[ground].mean():.3f} of the ground")
            assert ground.mean() >= 0.05 and differs[ground].mean() >= 0.5, (sc.seed, lod, differs[ground].mean())
        finally:
            node.set("shader_params/u_sphere_depth_factor", own)
    _report(f"seed {sc.seed} depth sources {DEPTH_FORMATS[sc.seed % 3]}")


# ---- 5. one anchor to the oracle ------------------------------------------------------------------------------------------------------------------------

ANCHORS = [next(s for s in RS.SEEDS if s % 6 == v) for v in range(6)]       # the first seed of each variant


@pytest.mark.parametrize("seed", ANCHORS)
def test_single_draws_match_the_oracle(oracle32, seed):
    """The moved planets and the far cameras are new inputs for the single draw as well: `render` at F and at the placed N against the oracle, by
    test_parity_random_scenes' rule (identical zero and finite masks, error <= TOL absolute up to 1 and relative above), under both samplers where cloudy."""
    sc = Scene(seed)
    try:
        for lod, node, near, far, _ in sc.draws:
            lut = node.read_optical_depth() if "light_steps" not in sc.ocfg else None
            declared = lod is None and len(sc.draws) == 2
            for what, got, cam, depth in (("N", near, sc.N, sc.dN_np), ("F", far, sc.F, sc.dF_np)):
                want, hits = RS.oracle_render(oracle32, sc.params, sc.tex, sc.ocfg, declared, lut, cam, sc.sun, depth, model=sc.M)
                assert hits > 0 and _shaded(got) >= MIN_SHADED
                assert np.array_equal(np.all(got == 0.0, axis=-1), np.all(want == 0.0, axis=-1)), (seed, lod, what)
                finite = np.isfinite(want)
                assert np.array_equal(np.isfinite(got), finite), (seed, lod, what)
                err = np.abs(got - want)[finite] / np.maximum(1.0, np.abs(want[finite]))
                print(f"seed {seed} sampler {lod} {what}: {hits} hit rays, max err vs oracle {err.max():.3e}")
                assert err.max() <= TOL, (seed, lod, what, float(err.max()))
    finally:
        sc.close()


# ---- 6. the planets of one frame ------------------------------------------------------------------------------------------------------------------------

PW, PH = 320, 180
GROUPS = [RS.SEEDS[i:i + 3] for i in range(0, len(RS.SEEDS), 3)]      # list order, threes; the last group has two
DIAMETERS = (48.0, 64.0, 56.0)                                        # the atmosphere shells' diameters on screen, pixels: within 40 .. 90


def _planet_frame(group, overlap):
    """One 320 x 180 frame (camera at the origin looking down -z, fovy 40 degrees) and a position per planet: each at its own far-style distance, so that
    its shell is DIAMETERS[i] pixels wide whatever its radius, along x with a gap of 3 (R + H) of the larger neighbour between centres -- 1.5 of that
    neighbour's diameter on screen.  overlap: the middle planet's centre moves to half a radius from its left neighbour's, so that their rects overlap."""
    scenes = [RS.scene_of(s) for s in group]
    a = [sc[0]["u_planet_radius"] + sc[0]["u_atmosphere_height"] for sc in scenes]
    focal = 0.5 * PH / np.tan(np.radians(0.5 * RS.FAR_FOVY_DEG))
    dist = [2.0 * a[i] * focal / DIAMETERS[i] for i in range(len(group))]
    xs = [0.0]
    for i in range(1, len(group)):
        xs.append(xs[-1] + 1.5 * max(DIAMETERS[i - 1], DIAMETERS[i]))
    xs = [x - 0.5 * xs[-1] for x in xs]
    if overlap:
        xs[1] = xs[0] + 0.25 * DIAMETERS[0]
    pos = [np.array([xs[i] / focal * dist[i], 0.0, -dist[i]]) for i in range(len(group))]
    near = 0.05 * min(sc[0]["u_atmosphere_height"] for sc in scenes)
    cam = S.Camera(PW, PH, eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), fovy_deg=RS.FAR_FOVY_DEG, near=near, far=2.0 * max(d + r for d, r in zip(dist, a)))
    depth = np.maximum.reduce([S.depth_ground_sphere(cam, tuple(p.tolist()), sc[0]["u_planet_radius"]) for p, sc in zip(pos, scenes)])    # reverse-Z: the nearest wins
    return scenes, cam, pos, depth


def _launch_rect(node, cam):
    rect, tiles = (C.c_int * 4)(), C.c_int(-1)
    f = node.prepare_frame(cam)
    assert N.load().atmo_debug_proxy_launch_rect(node._ctx, C.byref(f), node.proxy_model(), C.c_float(node.proxy_box_size(cam)), rect, C.byref(tiles)) == N.ATMO_OK
    return tuple(rect), tiles.value


def _plan(rects, keys):
    """include/atmo_planets.h's plan for draws into one image: a draw's level is one more than the highest level of the earlier draws whose rects it
    overlaps; launches level by level, within a level one per key in the order of first appearance."""
    def touch(p, q):
        return p[0] < q[2] and q[0] < p[2] and p[1] < q[3] and q[1] < p[3]

    level = []
    for j, r in enumerate(rects):
        level.append(max([level[i] + 1 for i in range(j) if touch(rects[i], r)], default=0))
    launch_of, n = [-1] * len(rects), 0
    for lv in range(max(level) + 1):
        for first in range(len(rects)):
            if level[first] != lv or launch_of[first] >= 0:
                continue
            for i in range(first, len(rects)):
                if level[i] == lv and launch_of[i] < 0 and keys[i] == keys[first]:
                    launch_of[i] = n
            n += 1
    return launch_of, n, level


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=["-".join(str(s) for s in grp) for grp in GROUPS])
def test_planets_equal_the_sequential_proxy_composites(g):
    """Three seeds' planets (one context each) in one frame, listed back to front (draw_order): render_planets leaves every byte as the sequential
    render_proxy_composite(target=...) calls leave it, and plan_planets puts them in as many launches as the single draws' kernel names give distinct
    keys.  Second pass: the middle planet over its left neighbour's rect: two levels."""
    group = GROUPS[g]
    fmt = "rgba16f" if g == 0 else FORMATS[g % 7]
    for overlap in (False, True):
        scenes, cam, pos, depth_np = _planet_frame(group, overlap)
        depth = torch.from_numpy(depth_np).cuda()
        nodes = []
        for seed, (params, _, sun, tex), p in zip(group, scenes, pos):
            shader, _, kw = RS.variant_of(seed, RS.VARIANTS_BATCH)
            model = G.translation(*p)
            nodes.append(RS.make_node(params, tex, tuple((np.asarray(sun) + p).tolist()), cam, shader, kw, None, model=model))
        try:
            order = PA.draw_order(nodes, cam)
            rects = [_launch_rect(n, cam)[0] for n in order]
            for r in rects:
                assert 40 <= r[2] - r[0] <= 90 and 40 <= r[3] - r[1] <= 90 and 0 <= r[0] and r[2] <= PW, (group, rects)
            fill = _random_dst((PH, PW, 4), fmt, 43 + g)
            want, got = Buf(PH, PW, fmt, PAD, fill), Buf(PH, PW, fmt, PAD, fill)
            keys, before = [], fill
            for n in order:
                n.render_proxy_composite(cam, depth, want.view, target=fmt)
                torch.cuda.synchronize()
                keys.append(_name(n.kernel_name))
                assert keys[-1][0] == _family(proxy=True, fmt=fmt), n.kernel_name
                after = want.picture().copy()
                assert not np.array_equal(after, before), (group, "a planet's composite changes nothing")
                before = after
            draws = [(n, cam, depth, got.view, None, None, fmt) for n in order]
            launch_of, n_launches, level = _plan(rects, keys)
            if overlap:
                left, mid = order.index(nodes[0]), order.index(nodes[1])
                assert max(level) == 1 and level[max(left, mid)] == 1 and level[min(left, mid)] == 0, (group, rects, level)
            else:
                assert max(level) == 0 and n_launches == len(set(keys)), (group, rects, keys)
            assert PA.plan_planets(draws) == (launch_of, n_launches), (group, overlap, keys, rects)
            PA.render_planets(draws)
            torch.cuda.synchronize()
            for n, key in zip(order, keys):
                assert _name(n.kernel_name) == (_family(views=True, proxy=True, fmt=fmt), key[1] + KF_VIEWS, key[2]), (n.kernel_name, key)
            assert want.outside_intact() and got.outside_intact(), (group, overlap)
            assert np.array_equal(got.bits(), want.bits()), (group, overlap, fmt)
            print(f"planets {group} {fmt} overlap={overlap}: rects {rects}, launches {launch_of}, kernels {' '.join(sorted({n.kernel_name for n in order}))}")
        finally:
            for n in nodes:
                n.close()


def test_the_lists_of_this_file():
    """All seven formats occur over the list, as colour targets and -- the five byte formats -- under the depth sources; the anchors and the groups."""
    assert {f for s in RS.SEEDS for f in seed_formats(s)} == set(FORMATS)
    assert {packed_format(s) for s in RS.SEEDS} == set(FORMATS) - {"rgba32f", "rgba16f"}
    assert ANCHORS == [0, 7, 8, 3, 10, 5] and len(GROUPS) == 16 and len(GROUPS[-1]) == 2
