"""Cost of a reduced-resolution draw (include/atmo_reduced.h) on the MI355X: atmo_render_reduced_target at scale 2 and 4 against atmo_render_depth_target of
the SAME library -- the full-resolution draw is the yardstick, and its kernels are the ones every earlier commit shipped (tools/isa_diff.py).

    python tools/reduced_probe.py --out profiles/reduced/reduced_probe.json

Per case (config, size; pose P_space, a tight D32 depth buffer, composite into RGBA16F) the arms are timed INTERLEAVED -- every round times each arm once,
device events around `reps` calls through the C entry points (one ctypes call per draw):
  full, full2     atmo_render_depth_target, twice: full2 / full is the run-to-run spread of the yardstick against itself
  reduced_s2, reduced_s4   atmo_render_reduced_target: the depth reduction, the low draw, the upsample
  pick_s2, up_s2, pick_s4, up_s4   the two passes alone (atmo_reduced_depth, atmo_reduced_upsample on the buffers the whole call left)
after warm-up draws, four frame-paced draws (the tile order settles) and 25 ms of sustained work.  Reported per arm: the median, minimum and maximum of
the rounds (ms per call), the ratios reduced / full, and what the two passes move in bytes (the depth read once by each pass, the low depth written and
read, the low frame read, the target read and written) over their time.  Prints one JSON object; --table prints the markdown table of a saved one."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("clouds_high", 1920, 1080), ("clouds_high_rm", 1920, 1080), ("clouds_high", 3840, 2160), ("clouds_high_rm", 3840, 2160), ("no_clouds_8", 1920, 1080)]
TOLERANCE = 0.1


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def pass_bytes(w, h, s):
    """(bytes the reduction moves, bytes the upsample moves) for a D32 depth and an RGBA16F composite: each pixel's depth once per pass, the low depth
    written / read once, the low frame read once, the target read and written."""
    lw, lh = (w + s - 1) // s, (h + s - 1) // s
    return 4 * w * h + 4 * lw * lh, 4 * w * h + 4 * lw * lh + 16 * lw * lh + 2 * 8 * w * h


def probe(config, w, h, reps, rounds):
    import numpy as np
    import torch

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd import reduced as R
    from godot_atmosphere_shader_amd import scene as S
    from godot_atmosphere_shader_amd.demo import demo_textures, make_node

    node = make_node(config, demo_textures())
    lib = R.bind(node._lib)
    cam = S.Camera.from_pose(w, h, "P_space")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    node._bake_if_needed(stream.value)
    g = torch.Generator(device="cpu").manual_seed(3)
    scene = torch.rand((h, w, 4), generator=g, dtype=torch.float32).to(torch.float16).cuda()
    target = N.AtmoTarget(scene.data_ptr(), N.TARGET_RGBA16F, 0)
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    src = N.AtmoDepth(depth.data_ptr(), N.DEPTH_D32_SFLOAT, 0)
    nf = node.prepare_frame(cam)

    def check(rc):
        if rc != N.ATMO_OK:
            raise RuntimeError(lib.atmo_last_error_string(node._ctx).decode())

    def full():
        check(lib.atmo_render_depth_target(node._ctx, C.byref(nf), C.byref(src), C.byref(target), 1, stream))

    arms, keep = {"full": full}, []
    for s in (2, 4):
        depth_floats, nbytes = R.scratch_layout(w, h, s)
        scratch = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
        opt = R.AtmoReduced(s, TOLERANCE)
        low_depth, low_rgba = C.c_void_p(scratch.data_ptr()), C.c_void_p(scratch.data_ptr() + 4 * depth_floats)
        keep.append((scratch, opt))
        arms[f"reduced_s{s}"] = (lambda o=opt, sc=scratch: check(lib.atmo_render_reduced_target(node._ctx, C.byref(nf), C.byref(src), C.byref(o),
                                                                                                  C.c_void_p(sc.data_ptr()), C.byref(target), 1, stream)))
        arms[f"pick_s{s}"] = (lambda s=s, ld=low_depth: check(lib.atmo_reduced_depth(node._ctx, C.byref(nf), C.byref(src), s, ld, stream)))
        arms[f"up_s{s}"] = (lambda o=opt, ld=low_depth, lc=low_rgba: check(lib.atmo_reduced_upsample(node._ctx, C.byref(nf), C.byref(src), C.byref(o), ld, lc,
                                                                                                      C.byref(target), 1, stream)))
    arms["full2"] = full
    for fn in arms.values():                      # warm-up (the whole calls run before their passes: the scratch holds a drawn low frame)
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(4):                            # frame-paced draws: the tile order settles
        for fn in arms.values():
            fn()
            torch.cuda.synchronize()
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.025:
        for fn in arms.values():
            for _ in range(8):
                fn()
        torch.cuda.synchronize()
    samples = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            samples[k].append(timed(torch, fn, reps))
    res = {k: dict(median_ms=round(float(np.median(v)), 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5)) for k, v in samples.items()}
    res["spread_full2_over_full"] = round(res["full2"]["median_ms"] / res["full"]["median_ms"], 4)
    for s in (2, 4):
        res[f"reduced_s{s}"]["vs_full"] = round(res[f"reduced_s{s}"]["median_ms"] / res["full"]["median_ms"], 4)
        for arm, nbytes in zip((f"pick_s{s}", f"up_s{s}"), pass_bytes(w, h, s)):
            res[arm]["bytes"] = nbytes
            res[arm]["gb_per_s"] = round(nbytes / (res[arm]["median_ms"] * 1e-3) / 1e9, 1)
    res["kernel"] = node.kernel_name
    node.close()
    return res


def table(doc):
    rows = ["| config | size | full draw ms | s = 2 ms | s = 2 / full | s = 4 ms | s = 4 / full | reduction s2 / s4 us | upsample s2 / s4 us | verdict |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for key, r in doc["results"].items():
        config, size = key.rsplit("@", 1)
        r2, r4 = r["reduced_s2"], r["reduced_s4"]
        verdict = "wins at both scales" if max(r2["vs_full"], r4["vs_full"]) < 1.0 else "LOSES at both scales" if min(r2["vs_full"], r4["vs_full"]) >= 1.0 else \
            "wins at s = 4 only" if r4["vs_full"] < 1.0 else "wins at s = 2 only"
        rows.append(f"| {config} | {size} | {r['full']['median_ms']:.4f} | {r2['median_ms']:.4f} | {r2['vs_full']:.3f} | {r4['median_ms']:.4f} | {r4['vs_full']:.3f} | "
                    f"{1e3 * r['pick_s2']['median_ms']:.1f} / {1e3 * r['pick_s4']['median_ms']:.1f} | {1e3 * r['up_s2']['median_ms']:.1f} / {1e3 * r['up_s4']['median_ms']:.1f} | {verdict} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--table", default=None, help="print the markdown table of a saved result and exit")
    args = ap.parse_args()
    if args.table:
        with open(args.table) as f:
            print(table(json.loads(f.read())))
        return
    import torch

    from godot_atmosphere_shader_amd import _native as N

    res = dict(build_id=N.load().atmo_build_id().decode(), device=torch.cuda.get_device_name(0), pose="P_space", depth="d32f", target="rgba16f composite",
               depth_tolerance=TOLERANCE, reps=args.reps, rounds=args.rounds, results={})
    for config, w, h in CASES:
        r = probe(config, w, h, args.reps, args.rounds)
        res["results"][f"{config}@{w}x{h}"] = r
        print(config, w, h, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(table(res))


if __name__ == "__main__":
    main()
