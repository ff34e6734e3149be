"""Cost of the far-mode proxy draw (include/atmo_scene.h) against the fullscreen composite on the MI355X.

  python tools/proxy_probe.py --out profiles/proxy/proxy_probe.json

Cases (1920 x 1080, demo planet R = 100, H = 8, empty scene depth):
  footprint  one far planet whose box covers about 1 / 10 / 40 % of the frame: atmo_render_proxy_composite against atmo_render_composite, per family;
  overhead   a box covering the whole viewport: the fragment test's cost over the fullscreen draw;
  scene6     six planets: one frame drawn with draw_atmospheres against six fullscreen composites.
Each pair is timed as interleaved A/B rounds (device events around `reps` draws); medians are reported.  Prints one JSON object."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures, make_node  # noqa: E402
from godot_atmosphere_shader_amd.planet_atmosphere import draw_atmospheres  # noqa: E402

FAMILIES = ["no_clouds_8", "no_clouds_32x8_direct", "clouds_high", "clouds_high_rm", "v1_clouds_high"]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(fa, fb, reps, rounds):
    for _ in range(3):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    return dict(proxy_ms=round(ma, 5), full_ms=round(mb, 5), ratio=round(ma / mb, 4), spread_proxy=round((max(ta) - min(ta)) / ma, 4),
                spread_full=round((max(tb) - min(tb)) / mb, 4))


def cam_at(dist, w, h, fovy=75.0):
    return S.Camera(w, h, (0.0, 0.0, dist), (0.0, 0.0, 0.0), fovy_deg=fovy, far=max(800.0, 4.0 * dist))


def dist_for_fraction(frac, w, h, box, fovy=75.0):
    """Camera distance at which the box's front face (edge `box`) covers about `frac` of the frame."""
    t = math.tan(math.radians(fovy) / 2.0)
    side_px = math.sqrt(frac * w * h)                  # the face's square in pixels
    return box / 2.0 + box * h / (2.0 * t * side_px)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    from godot_atmosphere_shader_amd import _native as N

    w, h = args.width, args.height
    tex = demo_textures()
    res = dict(build_id=N.load().atmo_build_id().decode(), width=w, height=h, reps=args.reps, rounds=args.rounds, footprint={}, overhead={})
    for fam in FAMILIES:
        node = make_node(fam, tex)
        node.global_transform = np.eye(4)
        box = node.proxy_box_size(cam_at(1000.0, w, h))
        for frac in (0.01, 0.10, 0.40):
            cam = cam_at(dist_for_fraction(frac, w, h, box), w, h)
            depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
            scene = torch.rand((h, w, 4), device="cuda")
            r = ab(lambda: node.render_proxy_composite(cam, depth, scene), lambda: node.render_composite(cam, depth, scene), args.reps, args.rounds)
            res["footprint"][f"{fam}@{int(frac * 100)}%"] = r
            print(fam, frac, r, flush=True)
        # the whole viewport inside the box's silhouette (its front face one unit in front of the camera), the planet in view: every pixel runs the
        # fragment test and then the same shading as the fullscreen draw
        cam = cam_at(420.0, w, h)
        depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
        scene = torch.rand((h, w, 4), device="cuda")
        big = 2.0 * (420.0 - 1.0)
        r = ab(lambda: node.render_proxy_composite(cam, depth, scene, box_size=big), lambda: node.render_composite(cam, depth, scene), args.reps, args.rounds)
        res["overhead"][fam] = r
        print("overhead", fam, r, flush=True)
        node.close()
    # six planets, all in far mode, spread over the view
    cam = S.Camera(w, h, (0.0, 0.0, 900.0), (0.0, 0.0, 0.0), far=6000.0)
    nodes = []
    for k, (fam, pos) in enumerate([("clouds_high", (0.0, 0.0, 0.0)), ("no_clouds_8", (300.0, 120.0, -400.0)), ("clouds", (-350.0, -80.0, -200.0)),
                                    ("v1_no_clouds", (150.0, -200.0, -1200.0)), ("clouds_high_rm", (-500.0, 250.0, -1800.0)), ("no_clouds_8", (700.0, 0.0, -2500.0))]):
        node = make_node(fam, tex)
        node.global_transform = np.eye(4)
        node.global_transform[:3, 3] = pos
        node._process(camera=cam, time=0.0)
        nodes.append(node)
    depth = torch.zeros((h, w), device="cuda")
    scene = torch.rand((h, w, 4), device="cuda")

    def fullscreen():
        for n in nodes:
            n.render_composite(cam, depth, scene)
    r = ab(lambda: draw_atmospheres(nodes, cam, depth, scene), fullscreen, max(args.reps // 4, 2), args.rounds)
    res["scene6"] = dict(r, modes=[n._mode for n in nodes])
    print("scene6", r, flush=True)
    for n in nodes:
        n.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
