"""Cost of drawing a frame's far planets with ONE atmo_render_planets call (include/atmo_planets.h) against drawing them one after another with
atmo_render_proxy_target, on the MI355X.

  tools/ab_build_commit.sh pre <parent commit>          # the baseline arm's library: godot_atmosphere_shader_amd/libatmo_hip_pre.so
  python tools/planets_probe.py --out profiles/planets/planets_probe.json

Arms, in ONE process (both libraries loaded side by side, as tools/views_target_probe.py does, whose helpers this tool imports), timed as interleaved A/B
rounds with device events around `reps` frames; medians and each arm's min .. max are reported:
  seq    the baseline library (--baseline, default libatmo_hip_pre.so; without it: this build) making N atmo_render_proxy_target calls, RGBA16F
         composites, on one stream, in list order;
  batch  ONE atmo_render_planets call of this build on the same list.
Both arms blend into their own 1920 x 1080 RGBA16F image from the same bits and the same number of times; the images are compared at the end (asserted).
Cases, a still camera 900 units in front of a 3 x 2 grid of demo planets (each box about 150 x 150 pixels, none touching another): six planets of
no_clouds_8, of no_clouds_32x8_direct, of clouds_high, of clouds_high_rm; three clouds_high beside three no_clouds_8 (two launches); and a planet with a
moon in front (two draws that touch: two launches).  Every planet is a context of its own.

THE GATE (six planets of clouds_high, the case the call exists for): the batch's median lies below the sequential arm's by more than the sum of the two
arms' spreads (max - min over the rounds) -- a difference inside the spreads is not a win.  Reported as "gate"; every other row is reported as measured.
Prints one JSON object."""
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
from godot_atmosphere_shader_amd import planet_atmosphere as PA  # noqa: E402
from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures  # noqa: E402
from views_target_probe import load_both, node_on, timed  # noqa: E402

W, H = 1920, 1080
GRID = [(x, y, 0.0) for y in (330.0, -330.0) for x in (-800.0, 0.0, 800.0)]
GATE_CASE = "6 x clouds_high"


def ab(fa, fb, reps, rounds, warm=4):
    for k in range(warm):
        fa(k); fb(k)
        torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    return dict(seq_ms=round(ma, 5), seq_min_ms=round(min(ta), 5), seq_max_ms=round(max(ta), 5), batch_ms=round(mb, 5), batch_min_ms=round(min(tb), 5),
                batch_max_ms=round(max(tb), 5), batch_over_seq=round(mb / ma, 4),
                beyond_spreads=bool(ma - mb > (max(ta) - min(ta)) + (max(tb) - min(tb))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline", default=os.path.join(ROOT, "godot_atmosphere_shader_amd", "libatmo_hip_pre.so"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    cur, pre = load_both(args.baseline)
    seq_lib = pre or cur
    tex = demo_textures()
    cam = S.Camera(W, H, (0.0, 0.0, 900.0), (0.0, 0.0, 0.0), far=5000.0)
    stream = torch.cuda.current_stream().cuda_stream
    res = dict(build_id=cur.atmo_build_id().decode(), baseline_build_id=seq_lib.atmo_build_id().decode(), baseline="parent library" if pre else "this build",
               target="rgba16f composite 1920x1080", reps=args.reps, rounds=args.rounds, cases={})
    six = lambda fam: [(fam, pos, None) for pos in GRID]                                                       # noqa: E731
    cases = [("6 x no_clouds_8", six("no_clouds_8")), ("6 x no_clouds_32x8_direct", six("no_clouds_32x8_direct")), (GATE_CASE, six("clouds_high")),
             ("6 x clouds_high_rm", six("clouds_high_rm")),
             ("3 x clouds_high + 3 x no_clouds_8", [("clouds_high" if k % 2 == 0 else "no_clouds_8", pos, None) for k, pos in enumerate(GRID)]),
             ("planet + moon in front", [("clouds_high", (0.0, 0.0, 0.0), None), ("clouds_high", (40.0, 25.0, 450.0), (45.0, 5.0))])]
    ok = True
    for label, planets in cases:
        pairs = []
        for fam, pos, size in planets:
            pair = [node_on(seq_lib, cur, fam, tex), node_on(cur, cur, fam, tex)]
            for node in pair:
                if size is not None:
                    node.planet_radius, node.atmosphere_height = size
                node.global_transform = np.eye(4)
                node.global_transform[:3, 3] = pos
                node._process(camera=cam, time=0.0)
                node._bake_if_needed(stream)
            pairs.append(pair)
        depth = torch.from_numpy(np.maximum.reduce([S.depth_ground_sphere(cam, pos, n[0].planet_radius) for (_, pos, _), n in zip(planets, pairs)])).cuda()
        img = np.random.default_rng(5).uniform(0.0, 1.0, size=(H, W, 4)).astype(np.float16)
        out_a, out_b = torch.from_numpy(img).cuda(), torch.from_numpy(img).cuda()
        tgt_a = N.AtmoTarget(out_a.data_ptr(), N.TARGET_RGBA16F, 0)
        singles = [(a._ctx, a.prepare_frame(cam), a.proxy_model(), C.c_float(a.proxy_box_size(cam))) for a, _ in pairs]
        draws = [(b, cam, depth, out_b, None, None, None) for _, b in pairs]
        arr = PA.prepare_planets(draws)
        launch_of, n_launches = PA.plan_planets(draws)

        def seq(k):
            for ctx, f, model, size in singles:
                N.check(ctx, seq_lib.atmo_render_proxy_target(ctx, C.byref(f), model, size, C.c_void_p(depth.data_ptr()), C.byref(tgt_a), 1, C.c_void_p(stream)))

        def batch(k):
            PA.render_planets_prepared(arr, len(draws), stream)
        r = ab(seq, batch, args.reps, args.rounds)
        torch.cuda.synchronize()
        r["identical"] = bool(torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)))
        r["changed_pixels"] = int((out_b.cpu().numpy().view(np.uint16) != img.view(np.uint16)).any(axis=-1).sum())
        r["launch_of"], r["launches"] = launch_of, n_launches
        r["batch_kernels"] = sorted({b.kernel_name for _, b in pairs})
        if label == GATE_CASE:
            r["gate"] = "pass" if r["beyond_spreads"] else "FAIL"
        ok = ok and r["identical"] and r["changed_pixels"] > 1000
        res["cases"][label] = r
        print(label, r, flush=True)
        for pair in pairs:
            for node in pair:
                node.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    assert ok, "the two arms' images differ, or nothing was drawn"


if __name__ == "__main__":
    main()
