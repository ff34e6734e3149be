"""The render kernels at the edge step counts (tests/step_count_cases.py) against the fp32 oracle.  Needs an MI355X.

The host takes any view, cloud and light step count from 1 to 4096; the rest of the suite draws 8 / 12 / 16 / 32 / 64 view steps, 8 / 24 / 32 / 64 cloud
steps and 3 / 5 / 8 / 64 light steps.  Here: one step, odd counts, both sides of the 32 / 33 switch to KF_VIEW_POS (all fourteen of its instantiations),
the neighbours of the unrolled 8-step light march, odd counts under two lanes per ray -- on the demo scene at 113 x 67 (odd, no multiple of the tile), three
poses a case, every kernel named before its picture is compared.  tests/test_step_counts_host.py proves that the list covers this and that the oracle's
frames hold something; tests/test_reference_exec.py pins the oracle to the executed reference text at these counts (reference_exec_steps.npz)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import proxy_geometry as G
import random_scenes as RS
import step_count_cases as SC
import test_draw_paths_random_gpu as DP
from common import TOL, demo_params, demo_textures, make_node
from godot_atmosphere_shader_amd import depth_formats as D
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import targets as T
from test_reference_exec import GOLDEN, NODE_CONFIG, _lut_texel_geometry
from test_views_target_gpu import BITS, PAD, Buf

import reference_scenes as RSC  # noqa: E402  (tests/golden, on the path since test_reference_exec's import)

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared depth buffers are read only)


def _gpu_render(node, cam, depth_np, rect=None):
    out = node.render(cam, _dev(depth_np), rect=rect)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bar(case):
    """default and v1: the contract; reference order: test_reference_order_v2_atmosphere's; precision 0: what test_precise_cloud_mode holds it to."""
    return 1e-5 if case["precision"] == "reference" else TOL


def _zero(img):
    return np.all(img == 0.0, axis=-1)


# ---- a. every case against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_step_counts_match_the_oracle(oracle32, case):
    tex, params = demo_textures(), demo_params()
    want = SC.oracle_frames(oracle32, case)
    node = make_node(case["shader"], tex, params, **SC.node_kwargs(case))
    worst = 0.0
    try:
        for pose in SC.POSES:
            cam, depth = SC.camera_and_depth(pose)
            got = _gpu_render(node, cam, depth)
            assert node.kernel_name == case["kernel"], (node.kernel_name, case["kernel"])
            assert np.array_equal(_zero(got), _zero(want[pose])), pose
            assert np.array_equal(np.isfinite(got), np.isfinite(want[pose])), pose
            worst = max(worst, SC.rel_err(got, want[pose]))
    finally:
        node.close()
    print(f"\n{SC.case_id(case)}: {case['kernel']} max err vs oracle {worst:.3e} (bar {_bar(case):.0e})")
    assert worst <= _bar(case), f"{SC.case_id(case)} {case['kernel']}: {worst:.3e}"


# ---- b. two lanes per ray against one --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.SPLIT_CASES, ids=[SC.case_id(c) for c in SC.SPLIT_CASES])
def test_two_lanes_equal_one_lane(oracle32, case):
    """Level-0 forms: the view sums are regrouped (lane 0 marches (view_steps + 1) / 2 steps, lane 1 the rest -- none at one step -- folded in through
    exp(-V_A k)), the cloud samples interleaved: equal within 2e-5, the oracle within TOL, an odd rect the crop bit for bit
    (test_lane_split_two_equals_one's bars).  Declared-sampler forms <49, 0, 2> / <51, 0, 2>: the one-lane frame's bits."""
    tex, params = demo_textures(), demo_params()
    declared = bool(SC.kernel_args(case)[0] & 32)
    want = SC.oracle_frames(oracle32, case)
    one = make_node(case["shader"], tex, params, **SC.node_kwargs(case, lane_split=1))
    two = make_node(case["shader"], tex, params, **SC.node_kwargs(case))
    diff = err = 0.0
    try:
        for pose in SC.POSES:
            cam, depth = SC.camera_and_depth(pose)
            a, b = _gpu_render(one, cam, depth), _gpu_render(two, cam, depth)
            assert two.kernel_name == case["kernel"] and one.kernel_name == case["kernel"][:-len(", 2>")] + ", 1>", (one.kernel_name, two.kernel_name)
            if declared:
                assert np.array_equal(a, b), pose
                continue
            assert np.array_equal(_zero(a), _zero(b)), pose
            diff, err = max(diff, float(np.abs(a - b).max())), max(err, float(np.abs(b - want[pose]).max()))
            x0, y0, x1, y1 = rect = (7, 5, SC.W - 30, SC.H - 11)
            assert np.array_equal(_gpu_render(two, cam, depth, rect=rect), b[y0:y1, x0:x1]), pose
    finally:
        one.close()
        two.close()
    if declared:
        print(f"\n{SC.case_id(case)}: {case['kernel']} the one-lane frame's bits at every pose")
        return
    print(f"\n{SC.case_id(case)}: {case['kernel']} max |one - two| {diff:.3e}, two lanes vs oracle {err:.3e}")
    assert diff <= 2e-5 and err <= TOL


# ---- c. against the executed reference text ------------------------------------------------------------------------------------------------------------
def test_step_counts_match_the_executed_reference():
    """The HIP frame of every case of reference_exec_steps.npz (the reference's shader text, both step macros forced, the declared sampler) within TOL,
    the discard sets equal."""
    z, base = np.load(os.path.join(GOLDEN, "reference_exec_steps.npz")), np.load(os.path.join(GOLDEN, "reference_exec.npz"))
    tex = dict(blue_noise=S.make_blue_noise(), shape=S.make_shape_texture(RSC.SHAPE_N), cubemap=S.make_coverage_cubemap(RSC.CUBE_N))
    params = demo_params()
    for shader, view, cloud in RSC.STEP_CASES:
        kw = dict(view_steps=view) if cloud is None else dict(view_steps=view, cloud_steps=cloud)
        node = make_node(NODE_CONFIG[shader], tex, params, **kw)          # the library's default sampler: the declared one
        worst = 0.0
        try:
            for pose in RSC.STEP_POSES:
                cam = RSC.camera_from_fixture(base, RSC.W, RSC.H, pose)
                got = _gpu_render(node, cam, base[f"depth_demo_{pose}"])
                key = RSC.step_case_key(shader, view, cloud, pose)
                discarded = np.unpackbits(z[f"discard_{key}"])[:RSC.W * RSC.H].reshape(RSC.H, RSC.W).astype(bool)
                assert np.array_equal(_zero(got), discarded), key
                worst = max(worst, SC.rel_err(got, z[f"rgba_{key}"]))
            name = node.kernel_name
        finally:
            node.close()
        print(f"\n{shader} view {view} cloud {cloud}: {name} max err vs executed reference {worst:.3e}")
        assert worst <= TOL, (shader, view, cloud, worst)
        assert bool(DP._name(name)[1] & 128) == (view > 32 and "v1" not in shader), name


# ---- d. long cloudy marches on thin shells ---------------------------------------------------------------------------------------------------------------
THIN = [("planet_atmosphere_clouds_high_rm", dict(view_steps=v, cloud_steps=24, cloud_light_rm=1), dict(view_steps=v, cloud_steps=24)) for v in (64, 65)]
THIN += [("planet_atmosphere_v1_clouds", dict(view_steps=64, lite=1, cloud_steps=32), dict(view_steps=64))]


@pytest.mark.parametrize("seed", [13, 43, 55])
def test_long_cloudy_marches_on_thin_atmospheres(oracle32, seed):
    """KF_VIEW_POS exists because the default form's running position sum drifted on thin shells at 64 view steps -- measured on the cloudless kernel
    only.  Three of those thin random scenes (H / R 0.047 .. 0.064) under the cloudy forms: clouds_high_rm at 64 and 65 view steps, 24 cloud steps, both
    samplers (<179, 0, 1> / <147, 0, 1>), and v1_clouds at 64, which has no KF_VIEW_POS form.  test_parity_random_scenes' rule and bar."""
    assert seed in RS.SEEDS
    params, cam_kw, sun, tex = RS.scene_of(seed)
    cam = S.Camera(**cam_kw)
    depth = RS.near_depth(seed, cam, params["u_planet_radius"])
    assert tex["cubemap"] is not None
    for shader, ocfg, kw in THIN:
        for lod in (None, False):
            node = RS.make_node(params, tex, sun, cam, shader, kw, lod)
            try:
                got = _gpu_render(node, cam, depth)
                name = node.kernel_name
            finally:
                node.close()
            declared = lod is None
            flags = DP._name(name)[1]
            assert bool(flags & 32) == declared and bool(flags & 128) == ("v1" not in shader), name
            lut = None if ocfg.get("lite") else oracle32.bake_optical_depth(params["u_planet_radius"], params["u_atmosphere_height"], params["u_density"])
            want, hits = RS.oracle_render(oracle32, params, tex, ocfg, declared, lut, cam, sun, depth)
            assert hits > 0 and float((~_zero(want)).mean()) >= 0.06
            assert np.array_equal(_zero(got), _zero(want)) and np.array_equal(np.isfinite(got), np.isfinite(want)), (seed, name)
            err = SC.rel_err(got, want)
            print(f"\nseed {seed} {shader} {ocfg} {name}: max err vs oracle {err:.3e}")
            assert err <= TOL, f"seed {seed} {shader} {ocfg} {name}: {err:.3e}"


# ---- e. the light march beside its unrolled form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 7, 8, 9])
def test_light_probe_at_the_unrolled_forms_neighbours(oracle32, steps):
    """sun_od_direct through atmo_debug_marched_optical_depth at the LUT's texel-centre geometry: 8 steps is the unrolled form (closed-form q[j], no
    fmaxf on hh), every other count the run-time loop -- whose body never runs at 1 -- with an almost identical integral at 7 and 9.  Each against the
    oracle's march at the same count, by the bars test_hip_direct_light_march_against_the_reference_lut holds the 8-step form to."""
    params = demo_params()
    R, H, rho = params["u_planet_radius"], params["u_atmosphere_height"], params["u_density"]
    pos, d = _lut_texel_geometry(R, H)
    pos, d = np.ascontiguousarray(pos, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
    want = oracle32.marched_optical_depth(R, H, rho, pos, d, steps)
    node = make_node("no_clouds_32x8_direct", demo_textures(), params)
    got = np.empty(pos.shape[0], dtype=np.float32)
    try:
        rc = node._lib.atmo_debug_marched_optical_depth(node._ctx, pos.shape[0], pos.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), steps,
                                                        got.ctypes.data_as(C.c_void_p))
    finally:
        node.close()
    assert rc == 0 and np.isfinite(want).all() and want.max() > 0
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    err = np.abs(got - want)
    big = want >= 1e-3 * want.max()
    rel_big = float((err[big] / want[big]).max())
    abs_small = float(err[~big].max()) if (~big).any() else 0.0
    print(f"\nlight march, {steps} steps: max relative deviation {rel_big:.3e} over {int(big.sum())} texels >= 1e-3 max ({want.max():.3g}); "
          f"max absolute deviation below that {abs_small:.3e}")
    assert rel_big <= 2e-5
    assert abs_small <= 2e-5 * 1e-3 * want.max()


# ---- f. the twin kernels at odd counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(7, 5, 7), (1, 1, 1)], ids=lambda c: "v%d-c%d-l%d" % c)
def test_twins_carry_odd_step_counts(counts):
    """clouds_high_rm with direct light under the declared sampler (<55, 0, 1>): the view batch, the packed target, the far mode's proxy and a D16 depth
    source are separately compiled twins that take the step counts at run time -- each the single float draw (or targets.encode of it) bit for bit, in
    the manner of tests/test_draw_paths_random_gpu.py."""
    view, cloud, light = counts
    tex, params = demo_textures(), demo_params()
    node = make_node("clouds_high_rm", tex, params, view_steps=view, cloud_steps=cloud, light_mode="direct", light_steps=light)
    try:
        (c0, d0_np), (c1, d1_np) = SC.camera_and_depth("P_space"), SC.camera_and_depth("P_clouds")
        d0, d1 = _dev(d0_np), _dev(d1_np)
        f0, f1 = _gpu_render(node, c0, d0_np), _gpu_render(node, c1, d1_np)
        base = node.kernel_name
        assert base == "atmo_render_kernel<55, 0, 1>" and DP._shaded(f0) >= 0.3 and DP._shaded(f1) >= 0.3
        # two views in one launch
        outs = node.render_views([c0, c1], [d0, d1])
        torch.cuda.synchronize()
        DP._expect(node.kernel_name, "atmo_render_views_kernel", base, DP.KF_VIEWS)
        for got, want in zip(outs, (f0, f1)):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        # a packed target, pitched
        buf = Buf(SC.H, SC.W, "rgba8", PAD)
        node.render(c0, d0, out=buf.view, target="rgba8")
        torch.cuda.synchronize()
        DP._expect(node.kernel_name, DP._family(fmt="rgba8"), base, DP._flags(fmt="rgba8"))
        assert buf.outside_intact() and np.array_equal(buf.picture(), T.encode(f0, "rgba8").view(BITS["rgba8"]))
        # the far mode's proxy from a far camera: the single draw on the passing fragments, nothing elsewhere
        far = S.Camera(SC.W, SC.H, (31.0, 17.0, 420.0), (0.0, 0.0, 0.0))
        dfar_np = S.depth_ground_sphere(far)
        dfar = _dev(dfar_np)
        ffar = _gpu_render(node, far, dfar_np)
        _, passing, unstable = G.frame_masks(far, node.global_transform, node.proxy_box_size(far), dfar_np)
        assert passing.sum() >= 300 and ffar[passing & ~unstable].any()
        fill = DP._pattern((SC.H, SC.W, 4), 7)
        out = node.render_proxy(far, dfar, out=fill.clone())
        torch.cuda.synchronize()
        DP._expect(node.kernel_name, "atmo_render_proxy_kernel", base, DP.KF_PROXY)
        p, s = torch.from_numpy(passing).cuda(), torch.from_numpy(~unstable).cuda()
        assert bool(DP._same_bits(out, torch.from_numpy(ffar).cuda())[p & s].all()) and bool(DP._same_bits(out, fill)[~p & s].all())
        # a D16 depth source, pitched: the draw from the decoded floats
        texels = DP._texels(d0_np, "d16")
        src, _keep = DP._pitched_source(texels, "d16")
        want = _gpu_render(node, c0, D.decode(texels, "d16"))
        assert DP._shaded(want) >= 0.3 and not np.array_equal(want, np.zeros_like(want))
        got = node.render(c0, src)
        torch.cuda.synchronize()
        DP._expect(node.kernel_name, DP._family(depth=True), base, DP._flags(depth=True))
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        node.close()
        DP._report("\ntwins at (view, cloud, light) = %s" % (counts,))          # (prints the names, and leaves the other file's record clean)
