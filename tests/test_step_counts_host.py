"""What tests/step_count_cases.py covers, proved on the list itself and on the CPU oracle (no GPU): tests/test_step_counts_gpu.py can then only pass
on kernels that were launched, at the counts named, on frames that hold something."""
import numpy as np
import pytest

import step_count_cases as SC
from common import CONFIGS, SAMPLERS

KF_CLOUDS, KF_RM, KF_DIRECT, KF_LITE, KF_PRECISE, KF_CUBE_LOD, KF_ATMO_REF, KF_VIEW_POS = 1, 2, 4, 8, 16, 32, 64, 128
# launch_render's ATMO_VIEW_POS_CASE list, each | KF_VIEW_POS, LSTEPS 0, one lane per ray
VIEW_POS_FORMS = [0, 4, 1, 5, 3, 7, 17, 21, 19, 23, 49, 53, 51, 55]


def _values(key, where=lambda c: True):
    return {c[key] for c in SC.CASES if where(c)}


def test_all_fourteen_view_pos_instantiations_are_named():
    names = {c["kernel"] for c in SC.CASES}
    assert len(VIEW_POS_FORMS) == len(set(VIEW_POS_FORMS)) == 14
    for f in VIEW_POS_FORMS:
        assert f"atmo_render_kernel<{f | KF_VIEW_POS}, 0, 1>" in names, f
    # half of them at 33 view steps, half at 65
    at = {v: {SC.kernel_args(c)[0] for c in SC.CASES if c["view_steps"] == v and SC.kernel_args(c)[0] & KF_VIEW_POS} for v in (33, 65)}
    assert len(at[33]) >= 7 and len(at[65]) >= 7 and at[33] | at[65] == {f | KF_VIEW_POS for f in VIEW_POS_FORMS}


def test_every_edge_count_occurs():
    assert {1, 2, 3, 7, 31, 32, 33, 65} <= _values("view_steps")
    assert {1, 2, 3, 5, 33} <= _values("cloud_steps")
    assert {1, 2, 7, 8, 9} <= _values("light_steps")
    # ... where the issue asks for them: the cloudless v2 shader under both light modes, each light count paired with a view count
    for mode in ("lut", "direct"):
        assert {1, 2, 3, 7, 31, 32, 33, 65} <= _values("view_steps", lambda c: c["shader"] == "no_clouds_8" and c["light_mode"] == mode and c["precision"] == "default")
    assert {1, 2, 7, 8, 9} <= _values("light_steps", lambda c: c["shader"] == "no_clouds_8")
    by = {(c["view_steps"], c["light_steps"]): c["kernel"] for c in SC.CASES
          if c["shader"] == "no_clouds_8" and c["precision"] == "default" and c["lane_split"] == 0}
    assert by[32, 8].endswith("<4, 8, 1>") and by[33, 8] == "atmo_render_kernel<132, 0, 1>"
    # cloud steps on the three v2 cloud shaders under both samplers, view steps from 1, 3, 8, 33
    for shader in ("clouds", "clouds_high", "clouds_high_rm"):
        for sampler in SAMPLERS:
            mine = lambda c: c["shader"] == shader and c["sampler"] == sampler and c["precision"] == "default" and c["lane_split"] == 0   # noqa: E731
            assert {1, 2, 3, 5, 33} <= _values("cloud_steps", mine), (shader, sampler)
            assert _values("view_steps", lambda c: mine(c) and c["light_mode"] == "lut") <= {1, 3, 8, 33, 65}
    for shader, flags in (("clouds_high", 53), ("clouds_high_rm", 55)):
        assert {7, 8, 9} <= _values("light_steps", lambda c: c["shader"] == shader)
        names = {c["kernel"] for c in SC.CASES if c["shader"] == shader}
        assert {f"atmo_render_kernel<{flags}, 8, 1>", f"atmo_render_kernel<{flags}, 0, 1>"} <= names      # the TWIN's two forms under KF_CUBE_LOD
    # v1: 1, 3, 33 view steps; cloud steps 1 and 5
    for shader in ("v1_no_clouds", "v1_clouds", "v1_clouds_high"):
        assert {1, 3, 33} <= _values("view_steps", lambda c: c["shader"] == shader), shader
    for shader in ("v1_clouds", "v1_clouds_high"):
        assert {1, 5} <= _values("cloud_steps", lambda c: c["shader"] == shader), shader
    # reference order
    ref = [c for c in SC.CASES if c["precision"] == "reference"]
    for mode in ("lut", "direct"):
        assert {1, 3, 33} <= {c["view_steps"] for c in ref if c["shader"] == "no_clouds_8" and c["light_mode"] == mode}
    assert any(c["shader"] == "clouds_high_rm" and c["sampler"] == "declared" and (c["view_steps"], c["cloud_steps"]) == (33, 5) for c in ref)
    # two lanes per ray
    two = SC.SPLIT_CASES
    assert all(c["kernel"].endswith(", 2>") for c in two) and all(c["kernel"].endswith(", 1>") for c in SC.CASES if c["lane_split"] != 2)
    for shader in ("clouds", "clouds_high_rm", "v1_clouds"):
        assert {(v, k) for v in (1, 3, 7) for k in (1, 3, 5)} <= {(c["view_steps"], c["cloud_steps"]) for c in two if c["shader"] == shader and c["sampler"] == "lod0"}
    for mode in ("lut", "direct"):
        assert {1, 3, 7} <= {c["view_steps"] for c in two if c["shader"] == "no_clouds_8" and c["light_mode"] == mode}
    assert {7, 8} <= {c["light_steps"] for c in two if c["shader"] == "no_clouds_8"}
    for flags in (49, 51):
        assert {(3, 3), (3, 5)} <= {(c["view_steps"], c["cloud_steps"]) for c in two if c["kernel"] == f"atmo_render_kernel<{flags}, 0, 2>"}


def test_names_follow_the_hosts_rules():
    """Each written name against the rules of atmo_create, atmo_set_precision, launch_shape and render_kernel_name, bit by bit."""
    for c in SC.CASES:
        flags, lsteps, split = SC.kernel_args(c)
        cfg = CONFIGS[c["shader"]][1]
        lite, cloudy, v = bool(cfg.get("lite")), c["cloud_steps"] is not None, c["view_steps"]
        assert bool(flags & KF_LITE) == lite and bool(flags & KF_CLOUDS) == cloudy, c
        assert bool(flags & KF_RM) == bool(cfg.get("cloud_light_rm")), c
        assert bool(flags & KF_DIRECT) == (c["light_mode"] == "direct" and not lite), c
        assert bool(flags & KF_PRECISE) == ((cloudy or lite) and c["precision"] != "fast"), c
        assert bool(flags & KF_ATMO_REF) == (c["precision"] == "reference" and not lite), c
        assert bool(flags & KF_CUBE_LOD) == (cloudy and c["sampler"] == "declared" and c["precision"] != "fast"), c
        if v < 33:
            assert not flags & KF_VIEW_POS, c                                   # no name below 33 view steps carries bit 128
        elif not lite and not flags & KF_ATMO_REF:
            assert flags & KF_VIEW_POS, c                                       # every v2 name without bit 64 above 32 carries it
        else:
            assert not flags & KF_VIEW_POS, c                                   # KF_LITE and the reference order have no such form
        assert lsteps == (8 if flags & KF_DIRECT and c["light_steps"] == 8 and not flags & (KF_ATMO_REF | KF_VIEW_POS) else 0), c
        assert split == (2 if c["lane_split"] == 2 else 1), c
        if split == 2:
            assert not flags & (KF_VIEW_POS | KF_ATMO_REF) and (not flags & KF_CUBE_LOD or flags & ~KF_RM == 49), c
        assert 1 <= v <= 65 and (not cloudy or 1 <= c["cloud_steps"] <= 65) and c["light_steps"] <= 9, c


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_the_oracles_frames_hold_something(oracle32, case):
    """No case passes on black against black: the fp32 oracle shades at least 0.3 of every pose's pixels (the reference alone gives 0.35 at worst, at
    P_limb), and the P_clouds frame -- the pose that says something at one view step -- peaks above 0.5."""
    frames = SC.oracle_frames(oracle32, case)
    for pose in SC.POSES:
        img = frames[pose]
        assert img.shape == (SC.H, SC.W, 4) and np.isfinite(img).all()
        assert float(np.any(img != 0.0, axis=-1).mean()) >= 0.3, pose
    assert float(frames["P_clouds"].max()) > 0.5
    if case["cloud_steps"] is not None:
        # ... nor on a cloud march that contributes nothing: from inside the layer the clouds move more than half the pixels by over 1e-2, at one
        # cloud step too (measured: 0.655 of them at worst)
        bare = dict(case, shader="v1_no_clouds" if case["shader"].startswith("v1") else "no_clouds_8", cloud_steps=None)
        moved = np.abs(frames["P_clouds"] - SC.oracle_frames(oracle32, bare)["P_clouds"]).max(axis=-1) > 1e-2
        assert float(moved.mean()) >= 0.5
