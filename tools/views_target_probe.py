"""Cost of drawing several views into packed colour targets in one launch (include/atmo_views_target.h) against drawing them one after another with
atmo_render_target, on the MI355X.

  tools/ab_build_commit.sh pre <parent commit>          # the baseline arm's library: godot_atmosphere_shader_amd/libatmo_hip_pre.so
  python tools/views_target_probe.py --out profiles/views/views_target_probe.json

Arms, in ONE process (both libraries loaded side by side), timed as interleaved A/B rounds with device events around `reps` frames; medians are reported:
  seq    the baseline library (--baseline, default libatmo_hip_pre.so; without it: this build) drawing the N views with N atmo_render_target calls on one
         stream, tile feedback on;
  batch  atmo_render_views_target of this build, one call.
Targets are RGBA16F composites (what a swapchain host does): each view blends into its own viewport-sized image, both arms from the same destination bits
and the same number of times, so the images can be compared at the end.  Cases, on a still camera: 2 x 1920 x 1080 (a stereo pair) and 8 x 1280 x 720
(eight poses), for no_clouds_8, no_clouds_32x8_direct, clouds_high and clouds_high_rm; and panning by 1 degree per frame: 2 x 1920 x 1080 clouds_high_rm
(empty scene depth).  Per frame = all N views.  Prints one JSON object."""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from godot_atmosphere_shader_amd import _native as N  # noqa: E402
from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures, make_node  # noqa: E402

FAMILIES = ["no_clouds_8", "no_clouds_32x8_direct", "clouds_high", "clouds_high_rm"]
EYE = S.POSES["P_space"]["eye"]


def load_both(baseline):
    """(this build's library, the baseline library or None): two CDLLs in one process (ctypes loads RTLD_LOCAL: each resolves its own kernels)."""
    cur = N.load()
    if not baseline or not os.path.exists(baseline):
        return cur, None
    keep_path, keep_env = N.LIB_PATH, os.environ.get("ATMO_HIP_LIB")
    N.LIB_PATH, N._lib = baseline, None
    os.environ["ATMO_HIP_LIB"] = baseline      # an A/B library may lack the newest entry points
    try:
        pre = N.load()
    finally:
        N.LIB_PATH, N._lib = keep_path, cur
        if keep_env is None:
            del os.environ["ATMO_HIP_LIB"]
        else:
            os.environ["ATMO_HIP_LIB"] = keep_env
    return cur, pre


def node_on(lib, cur, fam, tex):
    """demo.make_node on the given library."""
    N._lib = lib
    try:
        return make_node(fam, tex)
    finally:
        N._lib = cur


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        fn(k)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(fa, fb, reps, rounds, warm=14):
    for k in range(warm):          # the tile orders settle: two unmeasured draws, four recording ones, a sort picked up by a later call
        fa(k); fb(k)
        torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    return dict(seq_ms=round(ma, 5), batch_ms=round(mb, 5), batch_over_seq=round(mb / ma, 4), spread_seq=round((max(ta) - min(ta)) / ma, 4),
                spread_batch=round((max(tb) - min(tb)) / mb, 4))


def still_cameras(n, w, h):
    if n == 2:       # a stereo pair: eyes 0.6 units apart
        return [S.Camera.from_pose(w, h, dict(eye=(EYE[0] + dx, EYE[1], EYE[2]), target=(EYE[0] + dx, EYE[1], 0.0))) for dx in (-0.3, 0.3)]
    poses = ["P_space", "P_limb", "P_night", "P_ground", "P_clouds", "P_space", "P_limb", "P_night"]
    return [S.Camera.from_pose(w, h, p) for p in poses[:n]]


def pan_cameras(w, h, steps):
    """[step][eye]: a stereo pair turning by 1 degree per frame about the vertical axis, forth and back."""
    out = []
    for k in list(range(steps)) + list(range(steps - 2, 0, -1)):
        a = math.radians(k - steps / 2.0)
        out.append([S.Camera(w, h, (EYE[0] + dx, EYE[1], EYE[2]), (EYE[0] + dx + EYE[2] * math.sin(a), EYE[1], EYE[2] - EYE[2] * math.cos(a))) for dx in (-0.3, 0.3)])
    return out


def scene_images(n, w, h, seed):
    """Two identical sets of n RGBA16F scene images: finite colours, alphas in [0, 1]."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, size=(n, h, w, 4)).astype(np.float16)
    return [torch.from_numpy(a[i]).cuda() for i in range(n)], [torch.from_numpy(a[i]).cuda() for i in range(n)]


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
               target="rgba16f composite", reps=args.reps, rounds=args.rounds, still={}, pan={})
    stream = torch.cuda.current_stream().cuda_stream

    def target_of(t):
        return N.AtmoTarget(t.data_ptr(), N.TARGET_RGBA16F, 0)

    for fam in args.families.split(","):
        seq_node, batch_node = node_on(pre or cur, cur, fam, tex), node_on(cur, cur, fam, tex)
        seq_lib = pre or cur

        def draw_single(frame, depth_ptr, tgt):
            N.check(seq_node._ctx, seq_lib.atmo_render_target(seq_node._ctx, C.byref(frame), C.c_void_p(depth_ptr), C.byref(tgt), 1, C.c_void_p(stream)))

        for n, w, h in ((2, 1920, 1080), (8, 1280, 720)):
            cams = still_cameras(n, w, h)
            depths = [torch.from_numpy(S.depth_ground_sphere(c)).cuda() for c in cams]
            outs_a, outs_b = scene_images(n, w, h, 5)
            frames = [seq_node.prepare_frame(c) for c in cams]
            tgts_a = [target_of(o) for o in outs_a]
            views = batch_node.prepare_views_target(cams, [d.data_ptr() for d in depths], [target_of(o) for o in outs_b])
            seq_node._bake_if_needed(stream)

            def seq(k):
                for f, d, t in zip(frames, depths, tgts_a):
                    draw_single(f, d.data_ptr(), t)

            def batch(k):
                batch_node.render_views_target_prepared(views, n, True, stream)
            r = ab(seq, batch, args.reps, args.rounds)
            torch.cuda.synchronize()
            r["identical"] = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(outs_a, outs_b))
            r["batch_kernel"] = batch_node.kernel_name
            r["batch_feedback"] = batch_node.feedback_stats()
            res["still"][f"{fam} {n}x{w}x{h}"] = r
            print(fam, n, w, h, r, flush=True)
        if fam == "clouds_high_rm":
            w, h = 1920, 1080
            steps = pan_cameras(w, h, 16)
            depth = torch.zeros((h, w), device="cuda")
            outs_a, outs_b = scene_images(2, w, h, 6)
            frames = [[seq_node.prepare_frame(c) for c in pair] for pair in steps]
            tgts_a = [target_of(o) for o in outs_a]
            views = [batch_node.prepare_views_target(pair, [depth.data_ptr()] * 2, [target_of(o) for o in outs_b]) for pair in steps]

            def seq_pan(k):
                for f, t in zip(frames[k % len(steps)], tgts_a):
                    draw_single(f, depth.data_ptr(), t)

            def batch_pan(k):
                batch_node.render_views_target_prepared(views[k % len(steps)], 2, True, stream)
            r = ab(seq_pan, batch_pan, len(steps), args.rounds, warm=len(steps))
            torch.cuda.synchronize()
            r["identical"] = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(outs_a, outs_b))
            res["pan"][f"{fam} 2x{w}x{h} 1deg/frame"] = r
            print("pan", fam, r, flush=True)
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
