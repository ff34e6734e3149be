"""The cloudless direct-light kernels against frames and light-march values recorded from the parent of the instruction diet (tests/golden/direct_diet,
made by make_direct_diet_golden.py there): the short exact prologue, the sure-miss test and the power-of-two folding in the 8-step light march are only
allowed to change the instruction stream, so every comparison here is BITWISE."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_diet")
sys.path.insert(0, GOLDEN)
import direct_diet_cases as DC  # noqa: E402
import make_direct_diet_golden as MK  # noqa: E402


@pytest.fixture(scope="module")
def textures():
    from godot_atmosphere_shader_amd.demo import demo_textures

    return demo_textures()


@pytest.mark.gpu
@pytest.mark.parametrize("stem,case", DC.frame_cases(), ids=[s for s, _ in DC.frame_cases()])
def test_frame_equals_the_parent_builds_bit_for_bit(textures, stem, case):
    """67 x 35 (partial tiles both ways) from P_space (silhouette inside the frame: hit and miss lanes, the sure-miss test live), P_limb, and from
    inside the shell (P_ground, P_shell: rc.miss_k <= 0, the sure-miss test off); stored discards and a cleared target (discards leave the sentinel);
    9 light steps (LSTEPS = 0), an RGBA8 target (KF_TARGET twin), a two-view batch (KF_VIEWS twin)."""
    want = np.load(os.path.join(GOLDEN, stem + ".npy"))
    got = MK.draw(case, textures)
    assert got.shape == want.shape and got.dtype == want.dtype
    differ = got.view(np.uint8) != want.view(np.uint8)
    print(f"{stem}: {int(differ.any(axis=-1).sum())} of {differ[..., 0].size} values differ in their bits")
    assert not differ.any()
    if case["cleared"]:   # the discard set itself: a cleared-target draw leaves exactly the recorded pixels alone
        assert np.array_equal((got == DC.SENTINEL).all(axis=-1), (want == DC.SENTINEL).all(axis=-1))


@pytest.mark.gpu
@pytest.mark.parametrize("stem,over,radius,height,steps", MK.light_cases(), ids=[c[0] for c in MK.light_cases()])
def test_light_march_equals_the_parent_builds_bit_for_bit(textures, stem, over, radius, height, steps):
    """sun_od_direct through atmo_debug_marched_optical_depth on the 4 096 inputs of direct_diet_cases.light_inputs: hh just below, at and just above 0,
    bdot of both signs, nearly cancelling chords, the bulk of the shell; on the demo planet with 8 and 9 steps, and with 8 steps on a planet of radius
    2^-45, where the squared light step is subnormal (and far below an ulp of r2 >= R^2)."""
    from godot_atmosphere_shader_amd.demo import demo_params

    pos, sun = DC.light_inputs(radius, height)
    want = np.load(os.path.join(GOLDEN, stem + ".npy"))
    got = MK.light_march(textures, demo_params(**over), pos, sun, steps)
    differ = got.view(np.uint32) != want.view(np.uint32)
    print(f"{stem}: {int(differ.sum())} of {differ.size} values differ in their bits")
    assert not differ.any(), f"first at input {int(np.argmax(differ))}: {got[differ][0]!r} against {want[differ][0]!r}"
