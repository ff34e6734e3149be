"""The inputs of tests/test_draw_paths_random_gpu.py and of the fuzz are worth drawing -- proved on the fp32 CPU oracle and in numpy, without a GPU, so
that no GPU test passes on nothing: for every seed of random_scenes.SEEDS the near frame (the seed's variant, depth and placement) and the far frame
shade at least a tenth of their pixels, the far camera sees ground that D16 quantisation moves, and the far mode's box has enough passing fragments and
next to no pixel on which fp32 may decide the fragment test either way; over the list every variant, the 17-texel cubemap, the unset cubemap and the
shape volumes that are no power of two occur often enough.  Last, the fuzz's own seeds: every always-run seed with an empty frame has a replacement.

The frames are at most 113 x 37 and are drawn once per session (the module's fixtures)."""
import numpy as np
import pytest

import proxy_geometry as G
import random_scenes as RS
from godot_atmosphere_shader_amd import depth_formats as D
from godot_atmosphere_shader_amd import scene as S

MIN_SHADED = 0.10


def shaded_share(frame):
    return float(np.any(frame != 0.0, axis=-1).mean())


def _lut(oracle, params, ocfg):
    if "light_steps" in ocfg:
        return None
    return oracle.bake_optical_depth(params["u_planet_radius"], params["u_atmosphere_height"], params["u_density"])


def oracle_frame(oracle, seed, params, tex, cam, sun, depth, model=None, table=RS.VARIANTS_BATCH):
    """The oracle's frame under the library's default sampler (declared where the scene has clouds and a cubemap)."""
    _, ocfg, _ = RS.variant_of(seed, table)
    declared = RS.samplers(seed, tex) != (None,)
    return RS.oracle_render(oracle, params, tex, ocfg, declared, _lut(oracle, params, ocfg), cam, sun, depth, model=model)[0]


@pytest.fixture(scope="module")
def frames(oracle32):
    """seed -> dict(near=shaded share of the placed near frame, far=... of the far frame, plus the far camera's inputs)."""
    out = {}
    for seed in RS.SEEDS:
        params, tex, M, cam, sun, depth = RS.placed(seed)
        fcam, fdepth = RS.far_camera(seed)
        out[seed] = dict(params=params, tex=tex, M=M, fcam=fcam, fdepth=fdepth, sun=sun,
                         near=shaded_share(oracle_frame(oracle32, seed, params, tex, cam, sun, depth, M)),
                         far=shaded_share(oracle_frame(oracle32, seed, params, tex, fcam, sun, fdepth, M)))
    return out


def test_the_list_is_the_issue_s():
    assert len(RS.SEEDS) == 47 and RS.SEEDS[:6] == [0, 3, 5, 7, 8, 9] and set(range(60)) - set(RS.SEEDS) == set(RS.DROPPED)
    assert RS.VARIANTS_BATCH[1][1]["view_steps"] == 32 and RS.VARIANTS[1][1]["view_steps"] == 64
    assert [v for i, v in enumerate(RS.VARIANTS_BATCH) if i != 1] == [v for i, v in enumerate(RS.VARIANTS) if i != 1]
    assert all(max(ocfg["view_steps"], kw.get("view_steps", 0)) <= 32 for _, ocfg, kw in RS.VARIANTS_BATCH)


def test_placement():
    """Even seeds stay where they are; odd seeds are moved rigidly, and the near camera and the sun move with the planet."""
    for seed in RS.SEEDS:
        params, cam_kw, sun, _ = RS.scene_of(seed)
        _, _, M, cam, psun, _ = RS.placed(seed)
        if seed % 2 == 0:
            assert np.array_equal(M, np.eye(4)) and psun == sun
            continue
        rot = M[:3, :3]
        assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(rot), 1.0) and np.allclose(rot[1], (0, 1, 0)) and M[:3, 3].any()
        # the camera's position in the planet's model space is the unplaced scene's
        eye_model = np.linalg.inv(M) @ np.append(cam.inv_view[:3, 3], 1.0)
        assert np.allclose(eye_model[:3], cam_kw["eye"], rtol=1e-9, atol=1e-9 * params["u_planet_radius"])
        assert np.allclose((np.linalg.inv(M) @ np.append(psun, 1.0))[:3], sun, rtol=1e-9)
    fcam, _ = RS.far_camera(RS.SEEDS[1])
    f2, _ = RS.far_camera(RS.SEEDS[1], 1)
    assert not np.allclose(fcam.inv_view, f2.inv_view) and (fcam.width, fcam.height) == (f2.width, f2.height)


def test_every_frame_shades_a_tenth_of_its_pixels(frames):
    for seed, f in frames.items():
        print(f"seed {seed}: near frame {f['near']:.3f} shaded, far frame {f['far']:.3f}")
    low = {s: (f["near"], f["far"]) for s, f in frames.items() if f["near"] < MIN_SHADED or f["far"] < MIN_SHADED}
    assert not low, low


def test_far_ground_and_its_d16_quantisation(frames):
    for seed, f in frames.items():
        depth = f["fdepth"]
        q = D.quantise(depth, "d16")
        ground = q != 0
        moved = (D.decode(q, "d16") != depth)[ground].mean()
        print(f"seed {seed}: ground on {ground.mean():.3f} of the far frame after D16, decoded != float on {moved:.3f} of it")
        assert ground.mean() >= 0.05, seed
        assert moved > 0.5, seed


def test_depth_sources_show_in_the_far_frame(oracle32, frames):
    """The oracle's far frame from the D16-decoded depth differs from its far-plane frame on at least half of the ground pixels -- for every seed whose
    scene reads the depth buffer.  A scene with u_sphere_depth_factor = 1 does not (the ground comes from the analytic sphere alone): there the two
    frames are the same bits, whatever the far camera's depth range, and the condition holds under the factor the GPU test's second pass of those
    seeds draws with (random_scenes.DEPTH_SOURCE_FACTOR).  No seed is dropped from the depth-source family."""
    analytic = []
    for seed, f in frames.items():
        q = D.quantise(f["fdepth"], "d16")
        ground = q != 0
        own = float(f["params"]["u_sphere_depth_factor"])
        sun = f["sun"]

        def differs(factor):
            params = dict(f["params"], u_sphere_depth_factor=factor)
            a = oracle_frame(oracle32, seed, params, f["tex"], f["fcam"], sun, D.decode(q, "d16"), f["M"])
            b = oracle_frame(oracle32, seed, params, f["tex"], f["fcam"], sun, S.depth_far(f["fcam"]), f["M"])
            return float(np.any(a.view(np.uint32) != b.view(np.uint32), axis=-1)[ground].mean())

        share = differs(own)
        if own == 1.0:
            assert share == 0.0, seed
            analytic.append(seed)
            share = differs(RS.DEPTH_SOURCE_FACTOR)
        print(f"seed {seed}: sphere-depth factor {own}: the D16 frame differs from the far-plane frame on {share:.3f} of the ground")
        assert share >= 0.5, (seed, own, share)
    print(f"u_sphere_depth_factor = 1 (depth buffer unread): {analytic}")
    assert 0 < len(analytic) < len(frames) // 2


def test_far_box_fragments(frames):
    for seed, f in frames.items():
        covered, passing, unstable = G.frame_masks(f["fcam"], f["M"], RS.proxy_box(f["params"], f["fcam"]), f["fdepth"])
        print(f"seed {seed}: {int(covered.sum())} covered, {int(passing.sum())} passing, {int(unstable.sum())} unstable")
        assert passing.sum() >= 300, seed
        assert unstable.sum() <= 1e-3 * covered.sum(), (seed, int(unstable.sum()), int(covered.sum()))


def test_what_the_list_covers():
    per_variant = [sum(1 for s in RS.SEEDS if s % 6 == v) for v in range(6)]
    assert min(per_variant) >= 6, per_variant
    cloudy = [s for s in RS.SEEDS if RS.is_cloud_variant(s)]
    cube17 = [s for s in cloudy if s % 4 == 2 and s % 5 != 4]
    no_cube = [s for s in cloudy if s % 5 == 4]
    npot_shape = [s for s in cloudy if s % 4 in (2, 3)]
    print(f"per variant {per_variant}; 17-texel cubemap {cube17}; no cubemap {no_cube}; 24^3 / 48^3 shape {npot_shape}")
    assert len(cube17) >= 5 and len(no_cube) >= 3 and len(npot_shape) >= 10
    for s in cube17:
        tex = RS.textures(s)
        assert tex["cubemap"].shape == (6, 17, 17) and RS.samplers(s, tex) == (None, False)
    for s in no_cube:
        assert RS.textures(s)["cubemap"] is None
    assert {RS.textures(s)["shape"].shape[0] for s in npot_shape[:4]} <= {24, 48}


def test_fuzz_seeds_with_empty_frames_have_replacements(oracle32):
    """The shaded share of every fuzz seed's oracle frame (as test_parity_random_scenes draws it: VARIANTS, identity placement), and the rule that picks
    the replacements, run again."""
    share = {}

    def shaded(seed):
        if seed not in share:
            params, cam_kw, sun, tex = RS.scene_of(seed)
            cam = S.Camera(**cam_kw)
            depth = RS.near_depth(seed, cam, params["u_planet_radius"])
            share[seed] = shaded_share(oracle_frame(oracle32, seed, params, tex, cam, sun, depth, table=RS.VARIANTS))
        return share[seed]

    for seed in RS.FUZZ_SEEDS:
        print(f"fuzz seed {seed}: {shaded(seed):.3f} shaded")
    empty = [s for s in RS.FUZZ_ALWAYS if shaded(s) == 0.0]
    assert empty, "the always-run seeds 1, 2, 4 and 6 look past their planets"
    listed = [s for s in RS.FUZZ_SEEDS if s not in RS.FUZZ_REPLACEMENTS.values()]
    want = {}
    for s in empty:
        want[s] = RS.fuzz_replacement(s, listed + list(want.values()), shaded)
    print(f"empty always-run frames {empty}: replacements {want}")
    assert RS.FUZZ_REPLACEMENTS == want
    assert all(r in RS.FUZZ_SEEDS for r in want.values()) and all(s in RS.FUZZ_SEEDS for s in range(12))
