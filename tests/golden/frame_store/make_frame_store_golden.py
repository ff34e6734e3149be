#!/usr/bin/env python3
"""Records tests/golden/frame_store/*.npz on the GPU with the library that is loaded -- run it with the PARENT commit's build (tools/ab_build_commit.sh
parent <commit>, then ATMO_HIP_LIB=.../libatmo_hip_parent.so): the frames that a change of the float-frame store's cache bits must reproduce bit for bit.
Drawn twice (two runs into two directories), the files must come out the same.

    ATMO_HIP_LIB=$PWD/godot_atmosphere_shader_amd/libatmo_hip_parent.so python tests/golden/frame_store/make_frame_store_golden.py [out dir]

The cases, for this script and for tests/test_frame_store_gpu.py.  Frames are 67 x 35 (partial 16 x 8 tiles both ways), filled with SENTINEL before the
draw, from P_space (the silhouette inside the frame: hit and miss lanes, the sure-miss store live) and P_shell (the camera inside the shell: the exact
prologue's discard store).  The geometric-order twin runs only on launches of 512 tiles and more from outside the shell: 371 x 171 (24 x 22 tiles), P_space."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

W, H = 67, 35
GEO_W, GEO_H = 371, 171
SENTINEL = 0.25
POSES = {
    "P_space": "P_space",
    "P_shell": dict(eye=(20.0, 103.0, 10.0), target=(60.0, 60.0, 130.0)),   # 105.4 from the centre: inside the shell (108), above the ground
}
# kind -> (demo configuration, PlanetAtmosphere keywords): the kernel families that store float frames
KINDS = {
    "direct": ("no_clouds_32x8_direct", {}),                      # atmo_render_kernel<4, 8, 1>
    "geo": ("no_clouds_32x8_direct", {}),                         # ... <4 | KF_GEO, 8, 1>: a context's first draw, 512 tiles or more
    "lut8": ("no_clouds_8", {}),                                  # <0, 0, 1>, 8 view steps
    "clouds": ("clouds", {}),                                     # a cloud kernel under the declared sampler (the mip chain of the demo cubemap)
    "views": ("no_clouds_32x8_direct", {}),                       # atmo_render_views_kernel: P_space and P_shell in one launch
    "proxy": ("no_clouds_32x8_direct", {}),                       # atmo_render_proxy: the box's passing fragments only
    "composite": ("no_clouds_32x8_direct", {}),                   # render_composite twice over one destination
}


def cases():
    """[(file stem, kind, pose)]; pose None = the kind's own (views: both poses; geo: P_space)."""
    out = []
    for kind in ("direct", "lut8", "clouds", "proxy", "composite"):
        for pose in POSES:
            out.append((f"{kind}_{pose}", kind, pose))
    out.append(("geo_P_space", "geo", "P_space"))
    out.append(("views_space_shell", "views", None))
    return out


def camera(pose, w=W, h=H):
    from godot_atmosphere_shader_amd import scene as S

    return S.Camera.from_pose(w, h, POSES[pose])


def depth_of(cam, device=0):
    import torch

    from godot_atmosphere_shader_amd import scene as S

    return torch.from_numpy(S.depth_ground_sphere(cam)).to(f"cuda:{device}")


def node_of(kind, textures, device=0, **extra):
    from godot_atmosphere_shader_amd.demo import demo_params, make_node

    cfg, kw = KINDS[kind]
    return make_node(cfg, textures, demo_params(), device=device, **kw, **extra)


def scene_colour(h=H, w=W):
    """The destination of the composite case: a fixed gradient, every channel different, alpha below one."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return np.stack([x / np.float32(w), y / np.float32(h), np.float32(0.5) + np.float32(0.25) * (x + y) / np.float32(w + h),
                     np.full_like(x, np.float32(0.75))], axis=-1).astype(np.float32)


def draw(kind, pose, textures, device=0):
    """The frame(s) of one case as a float32 array ((H, W, 4); views: (2, H, W, 4)), and the node's feedback_stats after the draw."""
    import torch

    dev = f"cuda:{device}"
    node = node_of(kind, textures, device)
    try:
        if kind == "views":
            cams = [camera(p) for p in POSES]
            outs = [torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device=dev) for _ in cams]
            node.render_views(cams, [depth_of(c, device) for c in cams], outs)
            torch.cuda.synchronize()
            return np.stack([o.cpu().numpy() for o in outs]), node.feedback_stats()
        w, h = (GEO_W, GEO_H) if kind == "geo" else (W, H)
        cam = camera(pose, w, h)
        depth = depth_of(cam, device)
        if kind == "composite":
            out = torch.from_numpy(scene_colour()).to(dev)
            node.render_composite(cam, depth, out)
            node.render_composite(cam, depth, out)   # over what the first composite wrote
        else:
            out = torch.full((h, w, 4), SENTINEL, dtype=torch.float32, device=dev)
            (node.render_proxy if kind == "proxy" else node.render)(cam, depth, out)
        torch.cuda.synchronize()
        return out.cpu().numpy(), node.feedback_stats()
    finally:
        node.close()


if __name__ == "__main__":
    from godot_atmosphere_shader_amd.demo import demo_textures

    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out_dir, exist_ok=True)
    textures = demo_textures()
    for stem, kind, pose in cases():
        a, stats = draw(kind, pose, textures)
        np.savez_compressed(os.path.join(out_dir, stem + ".npz"), frame=a)
        px = a.reshape(-1, 4)
        print(f"{stem}: {a.shape} {a.dtype}, {int((px == SENTINEL).all(axis=1).sum())} sentinel pixels, {int((px == 0).all(axis=1).sum())} zero pixels, "
              f"ordered_draws {stats.get('ordered_draws')}", flush=True)
