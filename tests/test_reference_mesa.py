"""A pin the author of this repository did not write: tests/golden/reference_exec_mesa.npz holds the outputs of the reference's shader text
compiled by MESA'S GLSL compiler and executed by llvmpipe (Mesa 23.2.1, the image's swrast_dri.so, driven headless through the DRI swrast
interface: tests/golden/mesa_glsl_runner.c, mesa_exec.py, make_mesa_vectors.py; report: profiles/round5/mesa_pin.txt).  The repository's own
interpreter (gdshader_vm.py) pins the oracle to 5e-7; this file checks that a third party's reading of the same text lands in the same place.

What bounds the agreement is llvmpipe's arithmetic, not the oracle's -- ulp-level choices the language leaves to the implementation, probed bit for bit
(profiles/round5/mesa_pin.txt section 12): mix is a + (b - a) t there (the stated convention here: the GLSL text's a (1 - t) + b t), normalize goes through
inversesqrt, dot sums in another order, exp is 1.1e-6 relative (18 ulp), pow 1e-6 (measured, stored in the fixture) -- so
  * the cloudless variants agree to 2e-5 (v2) / 5e-5 (v1: its products reach 1e14 before the clamp);
  * a cloud pixel's light is a product of up to 64 exponentials times an optical thickness of up to 250: most values agree to 1e-5, and the
    fp32-hypersensitive pixels (profiles/round4/fuzz_sensitive_pixels.txt: the fp32 ORACLE itself sits up to 2e-2 from the fp64 evaluation of
    the same text on them) move by up to 6e-3 -- with a correctly rounded exp substituted as well: any one-ulp difference moves them.  Bars: >= 97.5 %
    of a frame's values within 1e-4, none beyond 1e-2, and every pixel within 16 x (2e-5 + that pixel's own |fp32 oracle - fp64 oracle|): Mesa's
    deviation is explained, pixel by pixel, by fp32 sensitivity;
  * discard masks, the vertex-stage varyings and the LUT bake of the demo scene are compared EXACTLY (the bake: 65 536 of 65 536 texels bit-identical).

  -m "not gpu":  the CPU oracle against Mesa's vectors; the interpreter's vectors against Mesa's (tests/checks/reference_tree.py re-runs Mesa on a
                 reference checkout).
  -m gpu:        the HIP path through the C ABI against Mesa's vectors (small frames and whole rows at the BASELINE sizes, both cubemap samplers).
Nothing here needs Mesa or the reference at run time."""
import os
import sys

import numpy as np
import pytest

from common import make_node
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.planet_atmosphere import make_frame

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)

import reference_scenes as RS  # noqa: E402
from test_reference_exec import NODE_CONFIG  # noqa: E402

CLOUDLESS_BAR = {"planet_atmosphere_no_clouds": 2e-5, "planet_atmosphere_v1_no_clouds": 5e-5}
CLOUD_MAX, CLOUD_SHARE_BEYOND_1E4, SENS_FACTOR, SENS_BASE = 1e-2, 0.025, 16.0, 2e-5
# BASELINE-size rows (make_mesa_vectors.MESA_ROWS)
ROWS = [("planet_atmosphere_no_clouds", 1920, 1080, "P_space"), ("planet_atmosphere_clouds_high", 1920, 1080, "P_space"),
        ("planet_atmosphere_clouds_high", 1920, 1080, "P_clouds"), ("planet_atmosphere_clouds_high_rm", 3840, 2160, "P_space"),
        ("planet_atmosphere_clouds_high_rm", 3840, 2160, "P_clouds")]


def _cloudy(shader):
    return "clouds" in shader.replace("no_clouds", "")


def _samplers(shader):
    return ("lod0", "declared") if _cloudy(shader) else ("lod0",)


@pytest.fixture(scope="module")
def vm():
    return np.load(os.path.join(GOLDEN, "reference_exec.npz"))


@pytest.fixture(scope="module")
def mesa(vm):
    z = np.load(os.path.join(GOLDEN, "reference_exec_mesa.npz"))
    assert "llvmpipe" in str(z["mesa_info"]) and "Mesa" in str(z["mesa_info"])
    for k in ("crc_blue_noise", "crc_shape", "crc_cubemap", "crc_shape_full", "crc_cubemap_full"):  # the same texels as the interpreter's vectors
        assert int(z[k]) == int(vm[k]), k
    return z


@pytest.fixture(scope="module")
def textures():
    return dict(blue_noise=S.make_blue_noise(), shape=S.make_shape_texture(RS.SHAPE_N), cubemap=S.make_coverage_cubemap(RS.CUBE_N))


def _scene(sname):
    params, model = RS.scenes()[sname]
    return dict(params, u_world_to_model_matrix=S.col_major(np.linalg.inv(model))), model


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _check(got, want, shader, what, sens=None):
    """got: oracle or HIP; want: Mesa.  sens: per-pixel |fp32 oracle - fp64 oracle| (max over channels) where available."""
    assert np.array_equal(np.all(got == 0.0, axis=-1), np.all(want == 0.0, axis=-1)), f"{what}: discard sets differ"
    e = _rel(got, want)
    if not _cloudy(shader):
        assert e.max() <= CLOUDLESS_BAR[shader], f"{what}: {e.max():.3e}"
        return float(e.max())
    assert e.max() <= CLOUD_MAX, f"{what}: {e.max():.3e}"
    share = float(np.mean(e > 1e-4))
    assert share <= CLOUD_SHARE_BEYOND_1E4, f"{what}: {100 * share:.2f} % of the values beyond 1e-4"
    if sens is not None:
        ratio = e.max(-1) / (SENS_BASE + sens)
        assert ratio.max() <= SENS_FACTOR, f"{what}: a pixel deviates {ratio.max():.1f} x its own fp32 sensitivity"
    return float(e.max())


# ------------------------------------------------------------------------------------------------------ CPU
def test_llvmpipe_accuracy_is_what_the_bars_assume(mesa):
    acc = dict(zip([str(n) for n in mesa["accuracy_names"]], [float(v) for v in mesa["accuracy_values"]]))
    assert 2e-7 < acc["exp (relative)"] < 3e-6 and acc["pow(x, 1.7) (relative)"] < 3e-6 and acc["log2 (absolute)"] < 2e-6
    assert acc["sqrt (relative)"] < 1.3e-7 and acc["1 / x (relative)"] < 1.3e-7 and acc["inversesqrt (relative)"] < 2e-7


def test_mesa_and_the_interpreter_read_the_text_the_same_way(vm, mesa):
    """Fixture against fixture: two executors of the reference text, one of them Mesa's.  Discards and varyings exactly; the bake of the demo
    scene bit for bit, of the other scene to 4e-7 (an ulp or two of exp through the RGBA8 packing: the packed low byte differs, not the value)."""
    for sname in RS.scenes():
        for pose in RS.POSES:
            assert np.array_equal(mesa[f"planet_vs_{sname}_{pose}"], vm[f"planet_vs_{sname}_{pose}"])
            assert np.array_equal(mesa[f"sun_vs_{sname}_{pose}"], vm[f"sun_vs_{sname}_{pose}"])
            for shader in RS.VARIANTS:
                key = f"{sname}_{pose}_{shader}"
                assert np.array_equal(mesa[f"discard_{key}"], vm[f"discard_{key}"]), key
                _check(vm[f"rgba_{key}"], mesa[f"rgba_{key}"], shader, f"interpreter vs Mesa {key}")
    assert np.array_equal(mesa["lut_demo"].view(np.uint32), vm["lut_demo"].view(np.uint32))
    a, b = mesa["lut_alt"], vm["lut_alt"]
    assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)) <= 4e-7 and np.mean(a.view(np.uint32) == b.view(np.uint32)) > 0.7


@pytest.mark.parametrize("sname", list(RS.scenes()))
def test_oracle_bake_against_mesa(oracle32, mesa, sname):
    params, _ = _scene(sname)
    lut = oracle32.bake_optical_depth(params["u_planet_radius"], params["u_atmosphere_height"], params["u_density"])
    if sname == "demo":
        assert np.array_equal(lut.view(np.uint32), mesa["lut_demo"].view(np.uint32))   # 65 536 texels of Mesa's execution, bit for bit
    else:
        assert np.max(np.abs(lut - mesa[f"lut_{sname}"]) / np.maximum(np.abs(lut), 1e-30)) <= 4e-7


@pytest.mark.parametrize("shader", list(RS.VARIANTS))
@pytest.mark.parametrize("sname", list(RS.scenes()))
def test_oracle_against_mesa_fragments(oracle32, oracle64, vm, mesa, textures, sname, shader):
    params, model = _scene(sname)
    worst = 0.0
    for pose in RS.POSES:
        cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
        frame = make_frame(cam, model, S.DEMO_SUN_POSITION, 0.0)
        depth = vm[f"depth_{sname}_{pose}"]
        tex = dict(textures, optical_depth=vm[f"lut_{sname}"])
        got, _ = oracle32.render(params, tex, RS.VARIANTS[shader], frame, depth, nthreads=4)
        sens = None
        if _cloudy(shader):
            g64, _ = oracle64.render(params, tex, RS.VARIANTS[shader], frame, depth, nthreads=4)
            sens = _rel(got, g64.astype(np.float32)).max(-1)
        worst = max(worst, _check(got, mesa[f"rgba_{sname}_{pose}_{shader}"], shader, f"oracle vs Mesa {sname}/{pose}/{shader}", sens))
    print(f"\n{sname} {shader}: max |oracle - Mesa| over 5 poses = {worst:.3e}")


@pytest.mark.parametrize("steps", RS.VIEW_STEP_COUNTS)
def test_oracle_against_mesa_at_32_and_64_view_steps(oracle32, vm, mesa, textures, steps):
    params, model = _scene("demo")
    for pose in RS.POSES:
        cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
        got, _ = oracle32.render(params, dict(textures, optical_depth=vm["lut_demo"]), dict(RS.VARIANTS["planet_atmosphere_no_clouds"], view_steps=steps),
                                 make_frame(cam, model, S.DEMO_SUN_POSITION, 0.0), vm[f"depth_demo_{pose}"], nthreads=4)
        e = _rel(got, mesa[f"steps{steps}_rgba_{pose}"]).max()
        assert e <= 5e-5, f"{steps} view steps {pose}: {e:.3e}"   # measured 3.2e-5 at 64 steps: 64 exponentials of 18 ulp each


def test_double_precision_switch_against_mesa(oracle32, vm, mesa, textures):
    """#define DOUBLE_PRECISION (planet_atmosphere_main.gdshaderinc:25,118-125: the text writes to components of its mat4 parameter) compiled by Mesa."""
    params, model = _scene("demo")
    cam = RS.camera_from_fixture(vm, RS.W, RS.H, "P_limb")
    frame = make_frame(cam, model, S.DEMO_SUN_POSITION, 0.0)
    inv_view = np.array(frame["inv_view_matrix"], dtype=np.float64).copy()
    inv_view[12:15] *= -1.0
    got, _ = oracle32.render(params, dict(textures, optical_depth=vm["lut_demo"]), dict(RS.VARIANTS["planet_atmosphere_clouds"], double_precision=1),
                             dict(frame, inv_view_matrix=inv_view), vm["depth_demo_P_limb"])
    want = mesa["rgba_double_precision_P_limb_planet_atmosphere_clouds"]
    _check(got, want, "planet_atmosphere_clouds", "oracle vs Mesa, DOUBLE_PRECISION")
    _check(vm["rgba_double_precision_P_limb_planet_atmosphere_clouds"], want, "planet_atmosphere_clouds", "interpreter vs Mesa, DOUBLE_PRECISION")


def _rows_case(vm, mesa, shader, w, h, pose, sampler):
    from common import demo_textures
    key = f"rows_{sampler}_{w}x{h}_{pose}_{shader}"
    tex = demo_textures()
    assert S.checksum(tex["shape"]) == int(mesa["crc_shape_full"]) and S.checksum(tex["cubemap"]) == int(mesa["crc_cubemap_full"])
    cam = RS.camera_from_fixture(vm, w, h, pose)
    depth = S.depth_ground_sphere(cam)
    rows = [int(r) for r in mesa[f"which_{key}"]]
    assert np.array_equal(depth[rows], mesa[f"depth_{key}"])   # Mesa drew the whole frame over exactly this depth buffer
    return tex, cam, rows, depth, mesa[f"rgba_{key}"]


@pytest.mark.parametrize("case", [c + (s,) for c in ROWS for s in _samplers(c[0])], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-{c[4]}")
def test_oracle_against_mesa_at_baseline_sizes(oracle32, vm, mesa, case):
    """BASELINE.json configs[1..3] at their sizes: whole rows of frames llvmpipe drew in full, under the level-0 sampler and under the sampler the
    reference declares with MESA'S OWN level-of-detail selection (at these sizes 97-100 % of the coverage samples are magnified)."""
    shader, w, h, pose, sampler = case
    tex, cam, rows, depth, want = _rows_case(vm, mesa, shader, w, h, pose, sampler)
    params, _ = _scene("demo")
    cfg = RS.VARIANTS[shader]
    if sampler == "declared":
        tex, cfg = dict(tex, cubemap=oracle32.cubemap_mip_chain(tex["cubemap"])), dict(cfg, cube_lod=1)
    frame = make_frame(cam, np.eye(4), S.DEMO_SUN_POSITION, 0.0)
    got = np.stack([oracle32.render(params, dict(tex, optical_depth=vm["lut_demo"]), cfg, frame, depth, rect=(0, r, w, r + 1), nthreads=4)[0][0]
                    for r in rows])
    worst = _check(got, want, shader, f"oracle vs Mesa {case}")
    print(f"\n{case}: max |oracle - Mesa| = {worst:.3e} over {want.shape[0] * want.shape[1]} pixels")


@pytest.fixture(scope="module")
def fuzz():
    return np.load(os.path.join(GOLDEN, "reference_exec_fuzz.npz"))


@pytest.fixture(scope="module")
def mesa_fuzz():
    return np.load(os.path.join(GOLDEN, "reference_exec_mesa_fuzz.npz"))


def _check_fuzz(got, want, shader, what, sens):
    """The random scenes: other planet scales (R = 1 .. 637), density scales and step lengths -- the fp32 sensitivity of a frame varies by orders of
    magnitude between them (the v1 model's products reach 1e14; the fp32 oracle is 1e-1 from the fp64 one on seed 17), so the bar is the pixel's own:
    |x - Mesa| <= 64 x (2e-5 + |fp32 oracle - fp64 oracle|) where the sensitivity is known (CPU), a flat 2e-2 with <= 2.5 % beyond 1e-4 otherwise."""
    assert np.array_equal(np.all(got == 0.0, axis=-1), np.all(want == 0.0, axis=-1)), what
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    e = np.where(fin, np.abs(got - want) / np.maximum(1.0, np.abs(np.where(fin, want, 0.0))), 0.0)
    if sens is not None:
        ratio = e.max(-1) / (SENS_BASE + sens)
        if os.environ.get("MESA_PRINT_RATIO"):
            print(f"{what}: ratio {ratio.max():.1f} max err {e.max():.2e}")
        assert ratio.max() <= 64.0, f"{what}: a pixel deviates {ratio.max():.1f} x its own fp32 sensitivity"
    else:
        assert e.max() <= 2e-2 and np.mean(e > 1e-4) <= CLOUD_SHARE_BEYOND_1E4, f"{what}: {e.max():.3e}, {100 * np.mean(e > 1e-4):.2f} % beyond 1e-4"
    return float(e.max())


@pytest.mark.parametrize("k", range(RS.FUZZ_SEEDS))
def test_oracle_against_mesa_random_scenes(oracle32, oracle64, fuzz, mesa_fuzz, k):
    """The 24 random scenes of reference_exec_fuzz.npz (planets R = 1 .. 637, moved and rotated, cameras inside / outside the layer, cube sizes 17 .. 128,
    non-power-of-two shape volumes, an unbound cubemap) as Mesa drew them: three shader files per scene."""
    from test_reference_exec import _fuzz_case
    params, cam, sun, model, tex, depth = _fuzz_case(fuzz, k)
    lut = oracle32.bake_optical_depth(params["u_planet_radius"], params["u_atmosphere_height"], params["u_density"])
    frame = make_frame(cam, model, sun, 0.0)
    for shader in RS.fuzz_variants(k):
        got, _ = oracle32.render(params, dict(tex, optical_depth=lut), RS.VARIANTS[shader], frame, depth, nthreads=4)
        g64, _ = oracle64.render(params, dict(tex, optical_depth=lut), RS.VARIANTS[shader], frame, depth, nthreads=4)
        with np.errstate(all="ignore"):
            sens = np.nan_to_num(np.abs(got - g64.astype(np.float32)) / np.maximum(1.0, np.abs(got)), nan=0.0, posinf=0.0).max(-1)
        _check_fuzz(got, mesa_fuzz[f"rgba_{k}_{shader}"], shader, f"oracle vs Mesa, seed {k} {shader}", sens)


DIRECT_BAR = 5e-5   # 32 view steps x (3 exponentials + 8 light samples): measured 2.8e-5 (Mesa against the oracle, 1920x1080, every pixel)


def test_headline_configuration_against_mesa(oracle32, vm, mesa):
    """BASELINE.json's headline configuration -- 32 view x 8 light steps, the DIRECT light march bench.py's `value` is measured on -- has no shader file of
    its own in the reference: it is compute_atmosphere_v2 with the LUT fetch replaced by the quantity the LUT tabulates.  For Mesa that composition is 14
    lines of glue around the reference's own ray_sphere / get_atmosphere_density (mesa_exec.DIRECT_LIGHT_GLUE), spliced in front of the untouched
    compute_atmosphere_v2.  The oracle's direct mode against it: five poses, and BASELINE configs[1] at 1920x1080 as rows and as whole-frame block means."""
    params, model = _scene("demo")
    blue = S.make_blue_noise()
    cfg = dict(view_steps=32, light_steps=8)
    for pose in RS.POSES:
        cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
        got, _ = oracle32.render(params, dict(blue_noise=blue), cfg, make_frame(cam, model, S.DEMO_SUN_POSITION, 0.0), vm[f"depth_demo_{pose}"], nthreads=4)
        want = mesa[f"direct32x8_rgba_{pose}"]
        assert np.array_equal(np.all(got == 0.0, axis=-1), np.all(want == 0.0, axis=-1))
        assert np.abs(got - want).max() <= DIRECT_BAR, pose
    cam = RS.camera_from_fixture(vm, 1920, 1080, "P_space")
    got, hits = oracle32.render(params, dict(blue_noise=blue), cfg, make_frame(cam, np.eye(4), S.DEMO_SUN_POSITION, 0.0), S.depth_ground_sphere(cam), nthreads=8)
    rows = [int(r) for r in mesa["direct32x8_rows_which"]]
    assert np.abs(got[rows] - mesa["direct32x8_rows_rgba"]).max() <= DIRECT_BAR
    mean, kept = _block_means(got)
    assert np.array_equal(kept, mesa["direct32x8_blockkept"]) and int(kept.sum()) == hits
    err = float(np.abs(mean - mesa["direct32x8_blockmean"]).max())
    print(f"\nheadline configuration 1920x1080: {hits} fragments kept by the oracle and by Mesa, max |block mean: oracle - Mesa| = {err:.2e}")
    assert err <= 5e-6   # measured 1.4e-6


def test_blend_stage_against_mesa(oracle32, vm, mesa, textures):
    """The draw with the renderer's blend stage: llvmpipe's FIXED-FUNCTION blender in blend_mix state over a colour buffer of seeded
    noise.  Its result is src * a + dst * (1 - a) with the products rounded on their own, bit for bit, and a discarded fragment leaves the buffer
    untouched (checked when the vectors were made: profiles/round5/mesa_pin.txt section 14) -- which is what atmo_render_composite computes.  Here: the
    oracle's frame pushed through that equation against Mesa's blended frame."""
    from make_mesa_vectors import COMPOSITE, composite_scene
    params, model = _scene("demo")
    scene = composite_scene()
    for pose, shader in COMPOSITE:
        cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
        src, _ = oracle32.render(params, dict(textures, optical_depth=vm["lut_demo"]), RS.VARIANTS[shader], make_frame(cam, model, S.DEMO_SUN_POSITION, 0.0),
                                 vm[f"depth_demo_{pose}"], nthreads=4)
        disc = np.unpackbits(mesa[f"discard_demo_{pose}_{shader}"])[:RS.W * RS.H].reshape(RS.H, RS.W).astype(bool)
        a = src[..., 3:4]
        got = np.concatenate([src[..., :3] * a + scene[..., :3] * (np.float32(1.0) - a), a + scene[..., 3:] * (np.float32(1.0) - a)], axis=-1).astype(np.float32)
        got[disc] = scene[disc]
        want = mesa[f"composite_{pose}_{shader}"]
        assert np.array_equal(want[disc], scene[disc])
        e = np.abs(got - want)
        assert e.max() <= (1e-2 if _cloudy(shader) else 2e-5) and np.mean(e > 1e-4) <= CLOUD_SHARE_BEYOND_1E4, (pose, shader, e.max())


# whole frames, compactly: per 16 x 16 block the mean of every channel and the number of kept fragments of the frame llvmpipe drew -- EVERY pixel of the frame
# under test enters the comparison.  Bars: the largest block-mean deviation of the CPU oracle from Mesa, measured when the vectors were made, with headroom.
BLOCKS = [("planet_atmosphere_no_clouds", 1920, 1080, "lod0", 2e-6),            # measured 5.1e-7
          ("planet_atmosphere_clouds_high", 1920, 1080, "declared", 5e-4),      # 2.8e-4: one block holds a 3e-2 pixel of section 6
          ("planet_atmosphere_clouds_high_rm", 3840, 2160, "declared", 2e-4)]   # 6.6e-5


def _block_means(rgba):
    from make_mesa_vectors import block_means
    return block_means(rgba, np.all(rgba == 0.0, axis=-1))


def _blocks_case(vm, mesa, shader, w, h, sampler):
    from common import demo_textures
    tex = demo_textures()
    assert S.checksum(tex["shape"]) == int(mesa["crc_shape_full"]) and S.checksum(tex["cubemap"]) == int(mesa["crc_cubemap_full"])
    cam = RS.camera_from_fixture(vm, w, h, "P_space")
    key = f"{sampler}_{w}x{h}_P_space_{shader}"
    return tex, cam, S.depth_ground_sphere(cam), mesa[f"blockmean_{key}"], mesa[f"blockkept_{key}"]


@pytest.mark.parametrize("case", BLOCKS[:2], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}")
def test_oracle_whole_frame_blocks_against_mesa(oracle32, vm, mesa, case):
    """configs[1] and configs[2] at 1920x1080, every pixel (the 3840x2160 frame of configs[3] is left to the GPU test: a minute of oracle time)."""
    shader, w, h, sampler, bar = case
    tex, cam, depth, want_mean, want_kept = _blocks_case(vm, mesa, shader, w, h, sampler)
    params, _ = _scene("demo")
    cfg = RS.VARIANTS[shader]
    if sampler == "declared":
        tex, cfg = dict(tex, cubemap=oracle32.cubemap_mip_chain(tex["cubemap"])), dict(cfg, cube_lod=1)
    got, hits = oracle32.render(params, dict(tex, optical_depth=vm["lut_demo"]), cfg, make_frame(cam, np.eye(4), S.DEMO_SUN_POSITION, 0.0), depth, nthreads=8)
    mean, kept = _block_means(got)
    assert int(want_kept.sum()) == hits                      # Mesa kept exactly the fragments the oracle shades ...
    assert np.array_equal(kept, want_kept)                   # ... block by block (a kept fragment that evaluates to 0 would show here; none does)
    err = float(np.abs(mean - want_mean).max())
    print(f"\n{shader} {w}x{h} {sampler}: {want_kept.size} blocks, max |block mean: oracle - Mesa| = {err:.2e}")
    assert err <= bar


@pytest.fixture(scope="module")
def mesa_lod(mesa):
    z = np.load(os.path.join(GOLDEN, "reference_exec_mesa_lod.npz"))
    assert str(z["mesa_info"]) == str(mesa["mesa_info"]) and str(z["gallivm_perf"]) == str(mesa["gallivm_perf"])
    return z


@pytest.mark.parametrize("pose", RS.LOD_POSES)
@pytest.mark.parametrize("shader", RS.LOD_VARIANTS)
def test_minified_frames_differ_from_mesa_by_two_named_choices(oracle32, vm, mesa_lod, textures, pose, shader):
    """Round 6: the 12 frames of mesa_pin.txt section 5 -- 48 x 27, the demo scene, the sampler the reference DECLARES, the 64^2 cubemap
    MINIFIED 4-8x so that lambda > 0 matters -- were "recorded, not a test": llvmpipe and the stated convention differed on 9-15 % of the values by up to 0.33.
    What separates them is now named and tested: (i) llvmpipe takes the cube-map derivative by the quotient RULE, d(s / ma) = (ds ma - s dma) / ma^2 with the
    lane's own ma, where the stated convention takes the exact difference of the two projections, (ds ma - s dma) / (ma ma'); (ii) its level-of-detail unit takes
    log2 piecewise linear (exponent + mantissa - 1).  Both are legal (GLSL / Vulkan leave the derivative's precision and log2's to the implementation).  With the
    two substituted IN THE CHECKER (OracleConfig.lod_log2_fast = 4 | 1) the oracle reproduces llvmpipe's frames: max 1.6e-5 over every pixel from inside the layer
    and from the limb, and at pose P_space everything but (a) the LAST ROW of the odd-height frame, whose vertical quad partners are the rasteriser's helper pixels
    below the viewport (the stated convention gives them no derivative; llvmpipe shades them), and (b) one or two hypersensitive pixels per frame.
    The chain: HIP == stated convention on these very frames (test_reference_exec.py, the `lod_rgba_*` vectors, <= 1e-4; test below), stated convention + (i) +
    (ii) == llvmpipe: the HIP path's distance from a third-party executor on minified frames is attributed to two named implementation choices, each measured
    (profiles/round6/mesa_lod_rule.txt: either one alone does not close it)."""
    params, model = _scene("demo")
    cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
    frame = make_frame(cam, model, S.DEMO_SUN_POSITION, 0.0)
    depth = vm[f"depth_demo_{pose}"]
    tex = dict(textures, optical_depth=vm["lut_demo"], cubemap=oracle32.cubemap_mip_chain(textures["cubemap"]))
    want = mesa_lod[f"mesa_lod_rgba_{pose}_{shader}"]
    stated, _ = oracle32.render(params, tex, dict(RS.VARIANTS[shader], cube_lod=1), frame, depth, nthreads=4)
    both, _ = oracle32.render(params, tex, dict(RS.VARIANTS[shader], cube_lod=1, lod_log2_fast=5), frame, depth, nthreads=4)
    e_stated, e = _rel(stated, want), _rel(both, want)
    body, last = e[:RS.H - 1], e[RS.H - 1]
    print(f"\n{pose} {shader}: stated convention vs Mesa max {e_stated.max():.2e} ({100 * np.mean(e_stated > 1e-4):.2f} % beyond 1e-4); with llvmpipe's derivative form and "
          f"log2: rows 0..{RS.H - 2} max {body.max():.2e} ({100 * np.mean(body > 1e-4):.3f} %), last row max {last.max():.2e}")
    if pose == "P_space":
        assert np.mean(e_stated > 1e-4) > 0.05                         # the frames on which the conventions DO differ
        assert np.mean(body > 1e-4) <= 0.002 and body.max() <= 2e-3      # <= 2 pixels of 1 248, the worst 1.1e-3 (hypersensitive: |o32 - o64| there is larger)
        assert last.max() <= 0.1                                        # the helper row: recorded, not matched (see the docstring)
    else:
        assert e.max() <= 5e-5                                          # every pixel, the last row included: 1.6e-5 measured
        assert e_stated.max() > 10 * e.max()


# ------------------------------------------------------------------------------------------------------ GPU
def _gpu_render(node, cam, depth_np):
    import torch as _t
    out = node.render(cam, _t.from_numpy(np.ascontiguousarray(depth_np)).cuda())
    _t.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shader", list(RS.VARIANTS))
@pytest.mark.parametrize("sname", list(RS.scenes()))
def test_hip_against_mesa_fragments(vm, mesa, textures, sname, shader):
    params, model = _scene(sname)
    node = make_node(NODE_CONFIG[shader], textures, params, sampler="lod0")   # these frames: the text executed with the level-0 sampler
    node.global_transform = model
    worst = 0.0
    for pose in RS.POSES:
        cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
        node._process(0.0, cam, time=0.0)   # the node derives u_world_to_model_matrix from its transform, as planet_atmosphere.gd does
        node.set_shader_parameter("u_cloud_coverage_rotation", np.asarray(params["u_cloud_coverage_rotation"], dtype=np.float32))
        got = _gpu_render(node, cam, vm[f"depth_{sname}_{pose}"])
        worst = max(worst, _check(got, mesa[f"rgba_{sname}_{pose}_{shader}"], shader, f"HIP vs Mesa {sname}/{pose}/{shader}"))
    node.close()
    print(f"\n{sname} {shader}: max |HIP - Mesa| over 5 poses = {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("pose", RS.LOD_POSES)
def test_hip_is_the_stated_convention_on_the_minified_frames(oracle32, vm, textures, pose):
    """The other half of the chain of test_minified_frames_differ_from_mesa_by_two_named_choices: on the 12 minified frames the HIP kernels ARE the stated
    convention (oracle, cube_lod = 1) to 1e-4 -- so what separates them from llvmpipe there is what separates the stated convention from it."""
    params, model = _scene("demo")
    cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
    depth = vm[f"depth_demo_{pose}"]
    otex = dict(textures, optical_depth=vm["lut_demo"], cubemap=oracle32.cubemap_mip_chain(textures["cubemap"]))
    for shader in RS.LOD_VARIANTS:
        node = make_node(NODE_CONFIG[shader], textures, params)
        got = _gpu_render(node, cam, depth)
        assert int(node.kernel_name.split("<")[1].split(",")[0]) & 32, node.kernel_name
        node.close()
        want, _ = oracle32.render(params, otex, dict(RS.VARIANTS[shader], cube_lod=1), make_frame(cam, model, S.DEMO_SUN_POSITION, 0.0), depth, nthreads=8)
        err = float(_rel(got, want).max())
        print(f"\n{pose} {shader}: |HIP - stated convention| = {err:.3e}")
        assert err <= 1e-4, (pose, shader, err)


@pytest.mark.gpu
def test_hip_bake_against_mesa(mesa, textures):
    params, _ = _scene("demo")
    node = make_node("no_clouds_8", textures, params)
    lut = node.read_optical_depth()
    node.close()
    assert np.array_equal(lut.view(np.uint32), mesa["lut_demo"].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c + (s,) for c in ROWS for s in _samplers(c[0])], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-{c[4]}")
def test_hip_against_mesa_at_baseline_sizes(vm, mesa, case):
    """The product path draws the full 1920x1080 / 3840x2160 frame (default kernels <49, 0, 1> / <51, 0, 1> under the declared sampler); the rows of
    llvmpipe's full frame are compared."""
    shader, w, h, pose, sampler = case
    tex, cam, rows, depth, want = _rows_case(vm, mesa, shader, w, h, pose, sampler)
    params, _ = _scene("demo")
    node = make_node(NODE_CONFIG[shader], tex, params, sampler=sampler) if _cloudy(shader) else make_node(NODE_CONFIG[shader], tex, params)
    got = _gpu_render(node, cam, depth)[rows]
    name = node.kernel_name
    node.close()
    worst = _check(got, want, shader, f"HIP vs Mesa {case}")
    print(f"\n{case} {name}: max |HIP - Mesa| = {worst:.3e} over {want.shape[0] * want.shape[1]} pixels")


@pytest.mark.gpu
@pytest.mark.parametrize("case", BLOCKS, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}")
def test_hip_whole_frame_blocks_against_mesa(vm, mesa, case):
    """BASELINE configs[1], [2], [3] at their sizes with the library's default kernels: every pixel of the HIP frame, as 16 x 16 block means and kept-fragment
    counts, against the frame llvmpipe drew from the reference's text."""
    shader, w, h, sampler, bar = case
    tex, cam, depth, want_mean, want_kept = _blocks_case(vm, mesa, shader, w, h, sampler)
    params, _ = _scene("demo")
    node = make_node(NODE_CONFIG[shader], tex, params)   # default sampler = the declared one for the cloud variants
    got = _gpu_render(node, cam, depth)
    name = node.kernel_name
    node.close()
    mean, kept = _block_means(got)
    assert np.array_equal(kept, want_kept)
    err = float(np.abs(mean - want_mean).max())
    print(f"\n{shader} {w}x{h} {sampler} {name}: {want_kept.size} blocks ({w * h} pixels), max |block mean: HIP - Mesa| = {err:.2e}")
    assert err <= bar


@pytest.mark.gpu
def test_hip_headline_kernel_against_mesa(vm, mesa):
    """atmo_render_kernel<4, 8, 1> -- the kernel bench.py's `value` and `roofline` are measured on -- against the frames llvmpipe drew from the reference's
    functions composed into the headline configuration (test_headline_configuration_against_mesa): five poses at 48 x 27, and BASELINE configs[1] at
    1920x1080 as rows and as whole-frame block means (every pixel)."""
    from common import demo_textures
    params, model = _scene("demo")
    tex = demo_textures()
    node = make_node("no_clouds_32x8_direct", tex, params)
    assert node.kernel_name.startswith("atmo_render_kernel<4, 8, 1>"), node.kernel_name
    worst = 0.0
    for pose in RS.POSES:
        cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
        got = _gpu_render(node, cam, vm[f"depth_demo_{pose}"])
        want = mesa[f"direct32x8_rgba_{pose}"]
        assert np.array_equal(np.all(got == 0.0, axis=-1), np.all(want == 0.0, axis=-1))
        worst = max(worst, float(np.abs(got - want).max()))
    cam = RS.camera_from_fixture(vm, 1920, 1080, "P_space")
    got = _gpu_render(node, cam, S.depth_ground_sphere(cam))
    node.close()
    rows = [int(r) for r in mesa["direct32x8_rows_which"]]
    worst = max(worst, float(np.abs(got[rows] - mesa["direct32x8_rows_rgba"]).max()))
    mean, kept = _block_means(got)
    assert np.array_equal(kept, mesa["direct32x8_blockkept"])
    err = float(np.abs(mean - mesa["direct32x8_blockmean"]).max())
    print(f"\nheadline kernel <4, 8, 1>: max |HIP - Mesa| = {worst:.3e} (5 poses + 2 rows at 1920x1080); whole 1920x1080 frame, 8160 block means: {err:.2e}")
    assert worst <= 1e-4 and err <= 2e-5   # the kernel's own distance to the oracle is 1.6e-5 (regrouped sums, hardware exp2): TOL, not the oracle's bar


@pytest.mark.gpu
def test_hip_blend_stage_against_mesa(vm, mesa, textures):
    """atmo_render_composite (the draw with the blend stage) against llvmpipe's fixed-function blender over the same scene colours."""
    import torch
    from make_mesa_vectors import COMPOSITE, composite_scene
    params, model = _scene("demo")
    scene = composite_scene()
    for pose, shader in COMPOSITE:
        node = make_node(NODE_CONFIG[shader], textures, params, sampler="lod0") if _cloudy(shader) else make_node(NODE_CONFIG[shader], textures, params)
        cam = RS.camera_from_fixture(vm, RS.W, RS.H, pose)
        buf = torch.from_numpy(scene.copy()).cuda()
        node.render_composite(cam, torch.from_numpy(np.ascontiguousarray(vm[f"depth_demo_{pose}"])).cuda(), buf)
        torch.cuda.synchronize()
        node.close()
        got, want = buf.cpu().numpy(), mesa[f"composite_{pose}_{shader}"]
        disc = np.unpackbits(mesa[f"discard_demo_{pose}_{shader}"])[:RS.W * RS.H].reshape(RS.H, RS.W).astype(bool)
        assert np.array_equal(got[disc], scene[disc])          # discarded fragments: the scene, bit for bit, in both
        e = np.abs(got - want)
        print(f"\nblend stage {pose} {shader}: max |HIP - Mesa| = {e.max():.3e}")
        assert e.max() <= (1e-2 if _cloudy(shader) else 2e-5) and np.mean(e > 1e-4) <= CLOUD_SHARE_BEYOND_1E4


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(RS.FUZZ_SEEDS))
def test_hip_against_mesa_random_scenes(fuzz, mesa_fuzz, k):
    """The product path on the 24 random scenes against the frames Mesa drew from the reference's text."""
    from godot_atmosphere_shader_amd import PlanetAtmosphere, load_shader
    from godot_atmosphere_shader_amd.planet_atmosphere import LinearColor, _SOURCE_COLOR
    from test_reference_exec import _fuzz_case

    params, cam, sun, model, tex, depth = _fuzz_case(fuzz, k)
    for shader in RS.fuzz_variants(k):
        node = PlanetAtmosphere(blue_noise=tex["blue_noise"], cubemap_lod=False)  # these vectors: the text executed with the level-0 sampler
        node.custom_shader = load_shader(shader)
        node.planet_radius, node.atmosphere_height, node.sun_path = params["u_planet_radius"], params["u_atmosphere_height"], sun
        for name, v in params.items():
            if name in ("u_planet_radius", "u_atmosphere_height", "u_cloud_coverage_rotation", "u_world_to_model_matrix"):
                continue
            node.set(f"shader_params/{name}", LinearColor(v) if name in _SOURCE_COLOR else v)  # the fixture holds linear colours
        node.global_transform = model
        node._process(0.0, cam, time=0.0)
        node.set_shader_parameter("u_cloud_coverage_rotation", np.asarray(params["u_cloud_coverage_rotation"], dtype=np.float32))
        node.set_shader_parameter("u_cloud_shape_texture", tex["shape"])
        if tex["cubemap"] is not None:
            node.set_shader_parameter("u_cloud_coverage_cubemap", tex["cubemap"])
        got = _gpu_render(node, cam, depth)
        node.close()
        _check_fuzz(got, mesa_fuzz[f"rgba_{k}_{shader}"], shader, f"HIP vs Mesa, seed {k} {shader}", None)
