"""Cost of drawing several far-mode views in one launch (include/atmo_views_proxy.h) against drawing them one after another with the single proxy draws
(include/atmo_scene.h, atmo_target.h), on the MI355X.

  tools/ab_build_commit.sh pre <parent commit>          # the baseline arm's library: godot_atmosphere_shader_amd/libatmo_hip_pre.so
  python tools/views_proxy_probe.py --out profiles/views/views_proxy_probe.json

Arms, in ONE process (both libraries loaded side by side, as tools/views_target_probe.py does, whose helpers this tool imports), timed as interleaved A/B
rounds with device events around `reps` frames; medians are reported:
  seq    the baseline library (--baseline, default libatmo_hip_pre.so; without it: this build) drawing the N views with N atmo_render_proxy_composite
         calls ("float") or N atmo_render_proxy_target calls, RGBA16F composite ("rgba16f"), on one stream;
  batch  atmo_render_views_proxy / atmo_render_views_proxy_target of this build, one call.
Every view blends into its own viewport-sized image, both arms from the same destination bits and the same number of times, so the images can be
compared at the end.  Cases, on a still camera: a stereo pair, 2 x 1920 x 1080, 420 units from the demo planet (its box covers about a sixth of each
picture), for no_clouds_8, no_clouds_32x8_direct, clouds_high and clouds_high_rm; and the six 512 x 512 faces of a probe at (300, 200, 250), 90 degrees
each: the box lands in three of them, the other three have no tile.  Per frame = all N views.  Prints one JSON object."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from godot_atmosphere_shader_amd import _native as N  # noqa: E402
from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures  # noqa: E402
from views_target_probe import FAMILIES, ab, load_both, node_on  # noqa: E402


def stereo_cameras(w, h):
    return [S.Camera(w, h, (31.0 + dx, 17.0, 420.0), (31.0 + dx, 17.0, 0.0)) for dx in (-0.3, 0.3)]


def probe_cameras(n):
    eye = np.array((300.0, 200.0, 250.0))
    faces = [((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, -1)), ((0, -1, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))]
    return [S.Camera(n, n, tuple(eye), tuple(eye + np.array(d, dtype=np.float64)), up=tuple(float(x) for x in u), fovy_deg=90.0) for d, u in faces]


def scene_images(cams, seed, half):
    """Two identical sets of scene images (finite colours, alphas in [0, 1]): float32, or RGBA16F."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for c in cams:
        img = rng.uniform(0.0, 1.0, size=(c.height, c.width, 4)).astype(np.float16 if half else np.float32)
        a.append(torch.from_numpy(img).cuda())
        b.append(torch.from_numpy(img).cuda())
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline", default=os.path.join(ROOT, "godot_atmosphere_shader_amd", "libatmo_hip_pre.so"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--families", default=",".join(FAMILIES))
    args = ap.parse_args()
    cur, pre = load_both(args.baseline)
    tex = demo_textures()
    res = dict(build_id=cur.atmo_build_id().decode(), baseline_build_id=(pre or cur).atmo_build_id().decode(), baseline="parent library" if pre else "this build",
               reps=args.reps, rounds=args.rounds, cases={})
    stream = torch.cuda.current_stream().cuda_stream
    seq_lib = pre or cur
    for fam in args.families.split(","):
        seq_node, batch_node = node_on(seq_lib, cur, fam, tex), node_on(cur, cur, fam, tex)
        for node in (seq_node, batch_node):
            node.global_transform = np.eye(4)
        cases = [("stereo 2x1920x1080", stereo_cameras(1920, 1080))]
        if fam == "clouds_high_rm":
            cases.append(("probe 6x512x512", probe_cameras(512)))
        for label, cams in cases:
            n = len(cams)
            size = batch_node.proxy_box_size(cams[0])
            model = batch_node.proxy_model()
            depths = [torch.from_numpy(S.depth_ground_sphere(c)).cuda() for c in cams]
            frames = [seq_node.prepare_frame(c) for c in cams]
            seq_node._bake_if_needed(stream)
            batch_node._bake_if_needed(stream)
            for form in ("float", "rgba16f"):
                outs_a, outs_b = scene_images(cams, 5, form == "rgba16f")
                if form == "float":
                    views = batch_node.prepare_views(cams, [d.data_ptr() for d in depths], [o.data_ptr() for o in outs_b])

                    def seq(k):
                        for f, d, o in zip(frames, depths, outs_a):
                            N.check(seq_node._ctx, seq_lib.atmo_render_proxy_composite(seq_node._ctx, C.byref(f), model, C.c_float(size), C.c_void_p(d.data_ptr()),
                                                                                       C.c_void_p(o.data_ptr()), C.c_void_p(stream)))

                    def batch(k):
                        batch_node.render_views_proxy_prepared(views, n, model, size, True, stream)
                else:
                    tgts_a = [N.AtmoTarget(o.data_ptr(), N.TARGET_RGBA16F, 0) for o in outs_a]
                    views = batch_node.prepare_views_target(cams, [d.data_ptr() for d in depths], [N.AtmoTarget(o.data_ptr(), N.TARGET_RGBA16F, 0) for o in outs_b])

                    def seq(k):
                        for f, d, t in zip(frames, depths, tgts_a):
                            N.check(seq_node._ctx, seq_lib.atmo_render_proxy_target(seq_node._ctx, C.byref(f), model, C.c_float(size), C.c_void_p(d.data_ptr()),
                                                                                    C.byref(t), 1, C.c_void_p(stream)))

                    def batch(k):
                        batch_node.render_views_proxy_target_prepared(views, n, model, size, True, stream)
                r = ab(seq, batch, args.reps, args.rounds, warm=4)
                torch.cuda.synchronize()
                bits = torch.int16 if form == "rgba16f" else torch.int32
                r["identical"] = all(torch.equal(a.view(bits), b.view(bits)) for a, b in zip(outs_a, outs_b))
                r["batch_kernel"] = batch_node.kernel_name
                first, grid, rects = (C.c_int * (n + 1))(), (C.c_int * (2 * n))(), (C.c_int * (4 * n))()
                fviews = batch_node.prepare_views(cams, [0] * n, [0] * n)
                N.check(batch_node._ctx, cur.atmo_debug_views_proxy_layout(batch_node._ctx, fviews, n, model, C.c_float(size), first, grid, rects))
                r["tiles_per_view"] = [first[i + 1] - first[i] for i in range(n)]
                res["cases"][f"{fam} {label} {form}"] = r
                print(fam, label, form, r, flush=True)
        seq_node.close()
        batch_node.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
