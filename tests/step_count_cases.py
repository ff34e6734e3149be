"""The step counts at the edges of what the host accepts, as ONE list of cases (no GPU needed to import it): tests/test_step_counts_gpu.py draws
every case and holds it to the oracle, tests/test_step_counts_host.py proves what the list covers.

The host takes any view, cloud and light step count from 1 to 4096 (check_create_args, atmo_api.hip).  What changes with the count:
  view steps   > 32: a v2 context that is not in reference order gets KF_VIEW_POS (flag bit 128: launch_shape), fourteen instantiations of their own
               (launch_render's ATMO_VIEW_POS_CASE list), one lane per ray, the run-time light loop;
               odd, with two lanes per ray: lane 0 marches (view_steps + 1) / 2 steps and lane 1 the rest -- none at all at one step;
  cloud steps  odd, with two lanes per ray: the level-0 march interleaves the samples between the lanes;
  light steps  8 is the unrolled sun_od_direct<8> (LSTEPS 8 in the name), every other count the run-time loop sun_od_direct<0>, whose body never
               runs at 1.

A case is a dict: `shader` (a name of common.CONFIGS whose keywords are empty), `view_steps`, `cloud_steps` (None: a cloudless shader), `light_mode`
("lut" / "direct") and `light_steps` (0 under "lut"), `precision` ("default": precise clouds, the fast v2 march; "fast": atmo_set_precision 0, outside
the contract of atmo.h; "reference": atmo_set_precision 2), `sampler` (common.SAMPLERS), `lane_split` (0: the library's choice, one lane; 2) and `kernel`:
the name the draw must report.  The names are WRITTEN here, from launch_render's case list and render_kernel_name's format -- FLAGS as the sum of
  1 clouds, 2 raymarched cloud light, 4 direct light, 8 v1 (lite), 16 precise, 32 declared sampler, 64 reference order, 128 KF_VIEW_POS
-- never asked of the library: a host that picks another kernel fails the name before any picture is compared.

The list is a covering design, not the product of its axes; test_step_counts_host.py states what it must cover."""
import functools

import numpy as np

from common import CONFIGS, demo_frame, demo_params, demo_textures, oracle_inputs
from godot_atmosphere_shader_amd import scene as S

W, H = 113, 67          # odd, and no multiple of the 16 x 8 (8 x 8 under two lanes per ray) tile
POSES = ("P_space", "P_clouds", "P_limb")
LIT = "lut"


def _case(shader, view, cloud, light, kernel, precision="default", sampler="declared", lane_split=0):
    assert not CONFIGS[shader][2], shader          # (a config with keywords of its own would collide with the overrides)
    assert (cloud is not None) == bool(CONFIGS[shader][1].get("cloud_steps")), (shader, cloud)
    direct = light != LIT
    return dict(shader=shader, view_steps=view, cloud_steps=cloud, light_mode="direct" if direct else "lut", light_steps=light if direct else 0,
                precision=precision, sampler=sampler, lane_split=lane_split, kernel=f"atmo_render_kernel<{kernel}>")


NC, CL, CH, RM = "no_clouds_8", "clouds", "clouds_high", "clouds_high_rm"
V1, V1C, V1CH = "v1_no_clouds", "v1_clouds", "v1_clouds_high"

CASES = []

# ---- view steps 1, 2, 3, 7, 31, 32, 33, 65 on the cloudless v2 shader --------------------------------------------------------------------------------
# baked-LUT light
CASES += [_case(NC, v, None, LIT, "0, 0, 1") for v in (1, 2, 3, 7, 31, 32)]
CASES += [_case(NC, v, None, LIT, "128, 0, 1") for v in (33, 65)]
# direct light: every light-step count of 1, 2, 7, 8, 9; 32 -> 33 view steps at the unrolled count changes BOTH the family and the light loop
CASES += [
    _case(NC, 1, None, 1, "4, 0, 1"), _case(NC, 2, None, 2, "4, 0, 1"), _case(NC, 3, None, 7, "4, 0, 1"), _case(NC, 7, None, 9, "4, 0, 1"),
    _case(NC, 31, None, 8, "4, 8, 1"), _case(NC, 32, None, 8, "4, 8, 1"), _case(NC, 33, None, 8, "132, 0, 1"), _case(NC, 65, None, 9, "132, 0, 1"),
    _case(NC, 32, None, 7, "4, 0, 1"), _case(NC, 33, None, 1, "132, 0, 1"),
]

# ---- cloud steps 1, 2, 3, 5, 33 on the three v2 cloud shaders under both samplers; view steps from 1, 3, 8, 33 -----------------------------------------
# (33 view steps: KF_VIEW_POS forms 145 / 147 -- precise, level 0 -- and 177 / 179 -- declared sampler)
for cloud, view in ((1, 1), (2, 3), (3, 8), (5, 33), (33, 3)):
    vp = 128 if view > 32 else 0
    for shader, rm in ((CL, 0), (CH, 0), (RM, 2)):
        CASES.append(_case(shader, view, cloud, LIT, f"{49 + rm + vp}, 0, 1", sampler="declared"))
        CASES.append(_case(shader, view, cloud, LIT, f"{17 + rm + vp}, 0, 1", sampler="lod0"))
# ... with direct light at 7, 8 and 9 light steps: the TWIN families' LSTEPS 8 and 0 forms, under the declared sampler (53, 55) and at level 0 (21, 23)
CASES += [
    _case(CH, 3, 2, 7, "53, 0, 1"), _case(CH, 8, 3, 8, "53, 8, 1"), _case(CH, 1, 5, 9, "53, 0, 1"),
    _case(RM, 8, 5, 7, "55, 0, 1"), _case(RM, 3, 3, 8, "55, 8, 1"), _case(RM, 1, 1, 9, "55, 0, 1"),
    _case(CH, 3, 5, 8, "21, 8, 1", sampler="lod0"), _case(CH, 8, 1, 9, "21, 0, 1", sampler="lod0"),
    _case(RM, 1, 3, 8, "23, 8, 1", sampler="lod0"), _case(RM, 3, 33, 7, "23, 0, 1", sampler="lod0"),
    _case(CL, 3, 3, 7, "53, 0, 1"), _case(CL, 8, 5, 8, "21, 8, 1", sampler="lod0"),
]

# ---- the fourteen KF_VIEW_POS instantiations: seven at 33 view steps (128, 132, 129, 133, 145, 147, 177 -- three of them above) and seven at 65 -------
CASES += [
    # precision 0 (fast cloud density: level 0 only): 1, 3, 5, 7
    _case(CL, 33, 3, LIT, "129, 0, 1", precision="fast", sampler="lod0"), _case(CL, 33, 5, 7, "133, 0, 1", precision="fast", sampler="lod0"),
    _case(RM, 65, 5, LIT, "131, 0, 1", precision="fast", sampler="lod0"), _case(RM, 65, 3, 8, "135, 0, 1", precision="fast", sampler="lod0"),
    # precise, level 0: 17 and 19 at 33 above; 21 and 23 (direct light; the unrolled count takes the loop here)
    _case(CH, 65, 5, 8, "149, 0, 1", sampler="lod0"), _case(RM, 65, 33, 9, "151, 0, 1", sampler="lod0"),
    # the declared sampler: 49 at 33 above; 51, 53, 55 at 65
    _case(RM, 65, 33, LIT, "179, 0, 1"), _case(CH, 65, 3, 7, "181, 0, 1"), _case(RM, 65, 5, 8, "183, 0, 1"),
    _case(CL, 65, 2, LIT, "177, 0, 1"), _case(CL, 65, 1, LIT, "145, 0, 1", sampler="lod0"),
]
# ... and precision 0 below the switch: the forms test_precise_cloud_mode draws at 8 view steps only
CASES += [_case(CL, 1, 1, LIT, "1, 0, 1", precision="fast", sampler="lod0"), _case(RM, 3, 5, 9, "7, 0, 1", precision="fast", sampler="lod0")]

# ---- the v1 shaders: 1, 3, 33 view steps (KF_LITE has no KF_VIEW_POS form: bit 128 stays clear), cloud steps 1 and 5 ---------------------------------------
CASES += [_case(V1, v, None, LIT, "24, 0, 1") for v in (1, 3, 33)]
CASES += [
    _case(V1C, 1, 1, LIT, "57, 0, 1"), _case(V1C, 3, 5, LIT, "25, 0, 1", sampler="lod0"), _case(V1C, 33, 1, LIT, "25, 0, 1", sampler="lod0"),
    _case(V1C, 33, 5, LIT, "57, 0, 1"),
    _case(V1CH, 1, 5, LIT, "25, 0, 1", sampler="lod0"), _case(V1CH, 3, 1, LIT, "57, 0, 1"), _case(V1CH, 33, 5, LIT, "25, 0, 1", sampler="lod0"),
    _case(V1CH, 33, 1, LIT, "57, 0, 1"),
]

# ---- reference-order mode (bit 64): one launch shape, the run-time light loop, no KF_VIEW_POS ------------------------------------------------------------
CASES += [_case(NC, v, None, LIT, "64, 0, 1", precision="reference") for v in (1, 3, 33)]
CASES += [_case(NC, v, None, ls, "68, 0, 1", precision="reference") for v, ls in ((1, 1), (3, 8), (33, 7))]
CASES += [_case(RM, 33, 5, LIT, "115, 0, 1", precision="reference")]

# ---- two lanes per ray, level-0 sampler: view steps 1, 3, 7 crossed with cloud steps 1, 3, 5; light steps 7 and 8 for the direct form ------------------------
for v in (1, 3, 7):
    CASES.append(_case(NC, v, None, LIT, "0, 0, 2", lane_split=2))
    CASES.append(_case(NC, v, None, 7, "4, 0, 2", lane_split=2))
    CASES.append(_case(NC, v, None, 8, "4, 8, 2", lane_split=2))
    for c in (1, 3, 5):
        CASES.append(_case(CL, v, c, LIT, "17, 0, 2", sampler="lod0", lane_split=2))
        CASES.append(_case(RM, v, c, LIT, "19, 0, 2", sampler="lod0", lane_split=2))
        CASES.append(_case(V1C, v, c, LIT, "25, 0, 2", sampler="lod0", lane_split=2))
# ---- two lanes per ray, declared sampler: the two forms the library draws a frame's heavy tiles with ------------------------------------------------------
CASES += [_case(CH, 3, c, LIT, "49, 0, 2", lane_split=2) for c in (3, 5)]
CASES += [_case(RM, 3, c, LIT, "51, 0, 2", lane_split=2) for c in (3, 5)]


def case_id(case):
    light = "lut" if case["light_mode"] == "lut" else f"l{case['light_steps']}"
    cloud = "" if case["cloud_steps"] is None else f"-c{case['cloud_steps']}"
    extra = ("" if case["precision"] == "default" else "-" + case["precision"]) + ("-2lanes" if case["lane_split"] == 2 else "")
    sampler = f"-{case['sampler']}" if case["cloud_steps"] is not None else ""
    return f"{case['shader']}-v{case['view_steps']}{cloud}-{light}{sampler}{extra}"


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS), sorted(i for i in IDS if IDS.count(i) > 1)
SPLIT_CASES = [c for c in CASES if c["lane_split"] == 2]


def kernel_args(case):
    """(FLAGS, LSTEPS, SPLIT) of the case's kernel name."""
    return tuple(int(a) for a in case["kernel"].rstrip(">").split("<")[1].split(","))


def node_kwargs(case, lane_split=None):
    """The keywords of common.make_node (behind the shader name, the textures and the parameters) that make the case's context."""
    kw = dict(sampler=case["sampler"], view_steps=case["view_steps"], light_mode=case["light_mode"], light_steps=case["light_steps"],
              lane_split=case["lane_split"] if lane_split is None else lane_split)
    if case["cloud_steps"] is not None:
        kw["cloud_steps"] = case["cloud_steps"]
    if case["precision"] == "fast":
        kw["precise_clouds"] = False
    if case["precision"] == "reference":
        kw["precise_atmosphere"] = True
    return kw


def oracle_config(case):
    """The oracle's step-count config of the case: the shader's own (demo.CONFIGS) with the counts overridden."""
    cfg = dict(CONFIGS[case["shader"]][1], view_steps=case["view_steps"])
    if case["cloud_steps"] is not None:
        cfg["cloud_steps"] = case["cloud_steps"]
    if case["light_mode"] == "direct" and not cfg.get("lite"):
        cfg["light_steps"] = case["light_steps"]
    return cfg


@functools.lru_cache(maxsize=None)
def camera_and_depth(pose):
    cam = S.Camera.from_pose(W, H, pose)
    depth = S.depth_ground_sphere(cam)
    depth.setflags(write=False)
    return cam, depth


_frames = {}


def oracle_frames(oracle, case):
    """{pose: the fp32 oracle's W x H frame of the demo scene} for the case; computed once per (step counts, sampler) and shared between the tests --
    the precision mode, the lanes per ray and the kernel are the library's business, not the oracle's.  Read only.  The LUT is the oracle's own bake
    (the device's is held to it bit for bit: test_bake_bit_exact)."""
    cfg = oracle_config(case)
    declared = case["sampler"] == "declared"
    key = (tuple(sorted(cfg.items())), declared and case["cloud_steps"] is not None)
    if key not in _frames:
        params, tex = demo_params(), demo_textures()
        uses_lut = not cfg.get("lite") and not cfg.get("light_steps")
        lut = _lut(oracle) if uses_lut else None
        ocfg, otex = oracle_inputs(oracle, cfg, tex, lut, declared=declared)
        out = {}
        for pose in POSES:
            cam, depth = camera_and_depth(pose)
            img, _ = oracle.render(params, otex, ocfg, demo_frame(cam), depth, nthreads=8)
            img.setflags(write=False)
            out[pose] = img
        _frames[key] = out
    return _frames[key]


_luts = {}


def _lut(oracle):
    if id(oracle) not in _luts:
        p = demo_params()
        _luts[id(oracle)] = oracle.bake_optical_depth(p["u_planet_radius"], p["u_atmosphere_height"], p["u_density"])
    return _luts[id(oracle)]


def rel_err(got, want):
    """test_parity_random_scenes' rule on the finite values: absolute up to 1, relative above (clouds are HDR)."""
    finite = np.isfinite(want)
    if not finite.any():
        return 0.0
    return float((np.abs(got[finite] - want[finite]) / np.maximum(1.0, np.abs(want[finite]))).max())
