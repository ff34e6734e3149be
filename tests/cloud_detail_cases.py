"""The cloud-detail fixture frames as ONE list (no GPU and no reference tree needed to import it): tests/golden/make_detail_vectors.py executes the
reference text for every case, tests/test_cloud_detail_host.py re-asserts on the committed file what the generator asserted, and
tests/test_cloud_detail_gpu.py draws every case and holds it to the file.

A case is one 48 x 27 frame of the demo scene drawn by a reference shader with `#define CLOUDS_ALWAYS_LOW_QUALITY` commented out
(include/atmo_cloud_detail.h), at a pose and a TIME, executed under both cubemap samplers: "declared" (linear-mipmap, implicit LOD from the 2 x 2 pixel
quads) and "lod0" (level 0).  `shape_n`: the size of the shape volume (24 is no power of two: the general wrap and the unfused p * n - 0.5);
`invert`: u_cloud_shape_invert where the case sets it (the demo scene's own value is 1).

The kernel names are WRITTEN here from render_kernel_name's format -- FLAGS as the sum of 1 clouds, 2 raymarched cloud light, 8 v1 (lite), 16 precise,
32 declared sampler, 8192 cloud detail -- never asked of the library."""
T1 = 37.5
SAMPLERS = ("declared", "lod0")
CH, RM, CL, V1CH = "planet_atmosphere_clouds_high", "planet_atmosphere_clouds_high_rm", "planet_atmosphere_clouds", "planet_atmosphere_v1_clouds_high"
# the binding's shader of each reference file (common.CONFIGS / demo.CONFIGS names)
NODE_SHADER = {CH: "clouds_high", RM: "clouds_high_rm", CL: "clouds", V1CH: "v1_clouds_high"}
_FLAGS = {CH: 17, RM: 19, CL: 17, V1CH: 25}


def _case(shader, pose, time, shape_n=32, invert=None):
    tag = ("" if shape_n == 32 else f"_shape{shape_n}") + ("" if invert is None else f"_invert{int(invert)}")
    return dict(shader=shader, pose=pose, time=float(time), shape_n=shape_n, invert=invert,
                name=f"{shader.replace('planet_atmosphere_', '')}_{pose}_t{time:g}{tag}")


CASES = [_case(CH, pose, t) for pose in ("P_space", "P_clouds", "P_limb") for t in (0.0, T1)]
# (P_clouds takes one side of alpha0 < 0.3 only, which is why it is no pose of the raymarched light)
CASES += [_case(RM, pose, t) for pose in ("P_space", "P_ground", "P_limb") for t in (0.0, T1)]
# The 24^3 frame stands at t = 12.25, the first substitute: at t = 37.5 one pixel of its level-0 frame changed when the literal 0.3 became 0.2999 / 0.3001
# (the generator's condition 4), so that time was replaced, not the bar.
T_SUBSTITUTE = 12.25
CASES += [_case(CL, "P_space", T1), _case(V1CH, "P_space", T1), _case(RM, "P_space", T_SUBSTITUTE, shape_n=24), _case(RM, "P_space", T1, invert=1.0)]
# One more: the demo scene's own u_cloud_shape_invert is 1, so the row above repeats clouds_high_rm P_space t = 37.5 with the value spelled
# out; this one draws the other branch (no inversion: the bounds of the early outs change sides).  At t = 12.25 for the reason the 24^3 frame is: at 37.5
# one pixel of its declared-sampler frame changed with the threshold.
CASES += [_case(RM, "P_space", T_SUBSTITUTE, invert=0.0)]


def key(case, sampler):
    return f"{case['name']}_{sampler}"


def kernel_name(case, sampler):
    return f"atmo_render_detail_kernel<{8192 + _FLAGS[case['shader']] + (32 if sampler == 'declared' else 0)}, 0>"


def is_rm(case):
    return case["shader"] == RM


def t0_twin(case):
    """The t = 0 case of the same shader, pose and scene, or None."""
    for c in CASES:
        if c["time"] == 0.0 and case["time"] != 0.0 and all(c[k] == case[k] for k in ("shader", "pose", "shape_n", "invert")):
            return c
    return None


def rel_err(got, want):
    """The project's 1e-4 rule: absolute up to |value| = 1, relative above (clouds are HDR)."""
    import numpy as np

    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
