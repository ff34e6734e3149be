#!/usr/bin/env python3
"""Records tests/golden/direct_diet/*.npy on the GPU with the library that is loaded -- run it with the PARENT commit's build (tools/ab_build_commit.sh
parent <commit>, then ATMO_HIP_LIB=.../libatmo_hip_parent.so): the frames and light-march values a bit-identical change of the direct-light kernels
must reproduce.

    ATMO_HIP_LIB=$PWD/godot_atmosphere_shader_amd/libatmo_hip_parent.so python tests/golden/direct_diet/make_direct_diet_golden.py [out dir]"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
import direct_diet_cases as DC  # noqa: E402


def draw(case, textures, device=0):
    """The frame(s) of one case as numpy arrays ((35, 67, 4) float32 or uint8; a views case: the views stacked on a new first axis)."""
    import torch

    from godot_atmosphere_shader_amd import scene as S
    from godot_atmosphere_shader_amd.demo import demo_params, make_node

    extra = dict(target_cleared=True) if case["cleared"] else {}
    node = make_node("no_clouds_32x8_direct", textures, demo_params(), device=device, **extra)
    if "light_steps" in case:
        node.close()
        from godot_atmosphere_shader_amd.demo import CONFIGS
        from godot_atmosphere_shader_amd.planet_atmosphere import PlanetAtmosphere

        kw = dict(CONFIGS["no_clouds_32x8_direct"][2], light_steps=case["light_steps"])
        node = _node_with(PlanetAtmosphere, kw, textures, demo_params(), device, extra)
    poses = case["views"] if "views" in case else (case["pose"],)
    cams = [S.Camera.from_pose(DC.W, DC.H, DC.POSES[p]) for p in poses]
    depths = [torch.from_numpy(S.depth_ground_sphere(c)).to(f"cuda:{device}") for c in cams]
    dtype = torch.uint8 if case.get("target") else torch.float32
    fill = 64 if case.get("target") else DC.SENTINEL
    outs = [torch.full((DC.H, DC.W, 4), fill, dtype=dtype, device=f"cuda:{device}") for _ in cams]
    if "views" in case:
        node.render_views(cams, depths, outs)
    else:
        node.render(cams[0], depths[0], outs[0], target=case.get("target"))
    torch.cuda.synchronize()
    got = np.stack([o.cpu().numpy() for o in outs]) if "views" in case else outs[0].cpu().numpy()
    node.close()
    return got


def _node_with(cls, kw, textures, params, device, extra):
    """make_node for a configuration that demo.CONFIGS does not list (another light-step count)."""
    from godot_atmosphere_shader_amd import demo, scene as S
    from godot_atmosphere_shader_amd.planet_atmosphere import _SOURCE_COLOR, LinearColor, load_shader

    node = cls(device=device, blue_noise=textures["blue_noise"], **kw, **extra)
    node.custom_shader = load_shader(demo.CONFIGS["no_clouds_32x8_direct"][0])
    node.planet_radius = params["u_planet_radius"]
    node.atmosphere_height = params["u_atmosphere_height"]
    node.sun_path = S.DEMO_SUN_POSITION
    for k, v in params.items():
        if k in ("u_planet_radius", "u_atmosphere_height", "u_cloud_coverage_rotation", "u_world_to_model_matrix"):
            continue
        node.set(f"shader_params/{k}", LinearColor(v) if k in _SOURCE_COLOR else v)
    node._process(0.0, None, time=0.0)
    return node


def light_march(textures, params, pos, sun, steps, device=0):
    from godot_atmosphere_shader_amd.demo import make_node

    node = make_node("no_clouds_32x8_direct", textures, params, device=device)
    got = np.empty(pos.shape[0], dtype=np.float32)
    rc = node._lib.atmo_debug_marched_optical_depth(node._ctx, pos.shape[0], pos.ctypes.data_as(C.c_void_p), sun.ctypes.data_as(C.c_void_p), steps,
                                                    got.ctypes.data_as(C.c_void_p))
    node.close()
    assert rc == 0
    return got


def light_cases():
    """[(file stem, params overrides, radius, height, light steps)]"""
    from godot_atmosphere_shader_amd import scene as S

    small = DC.SMALL_PLANET
    return [("light_demo_8", {}, S.DEMO_PLANET_RADIUS, S.DEMO_ATMOSPHERE_HEIGHT, 8), ("light_demo_9", {}, S.DEMO_PLANET_RADIUS, S.DEMO_ATMOSPHERE_HEIGHT, 9),
            ("light_small_8", small, small["u_planet_radius"], small["u_atmosphere_height"], 8)]


if __name__ == "__main__":
    from godot_atmosphere_shader_amd.demo import demo_params, demo_textures

    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out, exist_ok=True)
    textures = demo_textures()
    for stem, case in DC.frame_cases():
        a = draw(case, textures)
        np.save(os.path.join(out, stem + ".npy"), a)
        print(f"{stem}: {a.shape} {a.dtype}, {int((a.reshape(-1, 4) != 0).any(axis=1).sum())} non-zero pixels", flush=True)
    for stem, over, radius, height, steps in light_cases():
        pos, sun = DC.light_inputs(radius, height)
        v = light_march(textures, demo_params(**over), pos, sun, steps)
        np.save(os.path.join(out, stem + ".npy"), v)
        print(f"{stem}: {int(np.isfinite(v).sum())} finite, {int((v == 0).sum())} zero, max {np.nanmax(v):.4g}", flush=True)
