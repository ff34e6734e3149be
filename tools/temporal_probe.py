"""Cost of a temporal draw (include/atmo_temporal.h) on the MI355X: atmo_render_temporal_target at scale 2 and 4 against atmo_render_reduced_target at the
same scale and atmo_render_depth_target of the SAME library -- whose kernels are the ones every earlier commit shipped (tools/isa_diff.py).

    python tools/temporal_probe.py --out profiles/temporal/temporal_probe.json

Per case (config, size; pose P_space, a tight D32 depth buffer, composite into RGBA16F) the arms are timed INTERLEAVED -- every round times each arm once,
device events around `reps` calls through the C entry points (one ctypes call per draw):
  full, full2              atmo_render_depth_target, twice: full2 / full is the run-to-run spread of the yardstick against itself
  reduced_s2, reduced_s4   atmo_render_reduced_target
  temporal_s2, temporal_s4 atmo_render_temporal_target: the phase depth, the low draw, the resolve.  Every call advances the phase and swaps the two
                           histories; the previous camera is the current one a 1-degree orbit back, so most pixels take the bilinear path
  resolve_s2, resolve_s4   atmo_temporal_resolve alone on the buffers the whole call left;  up_s2, up_s4: atmo_reduced_upsample alone
  copy_resolve, copy_up    a device-to-device copy that reads and writes as many bytes as that pass reads and writes together
after warm-up draws, four frame-paced draws (the tile order settles) and 25 ms of sustained work.  Reported per arm: the median, minimum and maximum of
the rounds (ms per call), the ratios to the full and the reduced draw, and each pass's time over its copy's.  Prints one JSON object; --table prints the
markdown tables of a saved one."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from reduced_probe import pass_bytes, timed  # noqa: E402

CASES = [("clouds_high", 1920, 1080), ("clouds_high_rm", 1920, 1080), ("no_clouds_8", 1920, 1080), ("clouds_high", 3840, 2160),
         ("clouds_high_rm", 3840, 2160), ("no_clouds_8", 3840, 2160)]
TOLERANCE = 0.1


def resolve_bytes(w, h, s):
    """What the resolve moves for a D32 depth and an RGBA16F composite: each pixel's depth, the previous history (21 B a pixel) and the low frame with
    its depth read; the current history (21 B) written, the target read and written."""
    lw, lh = (w + s - 1) // s, (h + s - 1) // s
    return (4 + 21) * w * h + 20 * lw * lh + 21 * w * h + 2 * 8 * w * h


def probe(config, w, h, reps, rounds):
    import numpy as np
    import torch

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd import reduced as R
    from godot_atmosphere_shader_amd import scene as S
    from godot_atmosphere_shader_amd import temporal as TP
    from godot_atmosphere_shader_amd.demo import demo_textures, make_node

    node = make_node(config, demo_textures())
    lib = TP.bind(R.bind(node._lib))
    cam = S.Camera.from_pose(w, h, "P_space")
    a = np.radians(-1.0)                                       # the previous camera: a 1-degree orbit back
    rot = np.eye(4)
    rot[0, 0], rot[0, 2], rot[2, 0], rot[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    prev = S.Camera.from_pose(w, h, "P_space")
    prev.inv_view = rot @ cam.inv_view
    prev.view = np.linalg.inv(prev.inv_view)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    node._bake_if_needed(stream.value)
    g = torch.Generator(device="cpu").manual_seed(3)
    scene = torch.rand((h, w, 4), generator=g, dtype=torch.float32).to(torch.float16).cuda()
    target = N.AtmoTarget(scene.data_ptr(), N.TARGET_RGBA16F, 0)
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    src = N.AtmoDepth(depth.data_ptr(), N.DEPTH_D32_SFLOAT, 0)
    nf = node.prepare_frame(cam)
    fd = node.make_frame(cam)
    prev_clip, prev_inv = TP.prev_clip_from_view(fd, prev), S.col_major(prev.inv_projection)

    def check(rc):
        if rc != N.ATMO_OK:
            raise RuntimeError(lib.atmo_last_error_string(node._ctx).decode())

    def full():
        check(lib.atmo_render_depth_target(node._ctx, C.byref(nf), C.byref(src), C.byref(target), 1, stream))

    def copier(nbytes):
        a_, b_ = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        return lambda: b_.copy_(a_)

    arms, keep = {"full": full}, []
    for s in (2, 4):
        depth_floats, nbytes = R.scratch_layout(w, h, s)
        scratch = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
        low_depth, low_rgba = C.c_void_p(scratch.data_ptr()), C.c_void_p(scratch.data_ptr() + 4 * depth_floats)
        ropt = R.AtmoReduced(s, TOLERANCE)
        hist = [torch.zeros(TP.history_layout(w, h)[2], dtype=torch.uint8, device="cuda") for _ in range(2)]
        opts = [TP.options(s, p, TOLERANCE, 0.1, None, False, prev_clip, prev_inv) for p in TP.phase_sequence(s)]
        first = TP.options(s, 0, TOLERANCE, 0.1, None, True)
        state = dict(frame=0)
        keep.append((scratch, ropt, hist, opts, first))
        check(lib.atmo_render_temporal_target(node._ctx, C.byref(nf), C.byref(src), C.byref(first), C.c_void_p(scratch.data_ptr()), None,
                                              C.c_void_p(hist[1].data_ptr()), C.byref(target), 1, stream))

        def temporal(s=s, sc=scratch, hist=hist, opts=opts, state=state):
            f = state["frame"]
            state["frame"] = f + 1
            check(lib.atmo_render_temporal_target(node._ctx, C.byref(nf), C.byref(src), C.byref(opts[f % (s * s)]), C.c_void_p(sc.data_ptr()),
                                                  C.c_void_p(hist[(f + 1) & 1].data_ptr()), C.c_void_p(hist[f & 1].data_ptr()), C.byref(target), 1, stream))

        def resolve(s=s, hist=hist, opts=opts, ld=low_depth, lc=low_rgba, state=state):
            f = state["frame"]
            state["frame"] = f + 1
            check(lib.atmo_temporal_resolve(node._ctx, C.byref(nf), C.byref(src), C.byref(opts[f % (s * s)]), ld, lc,
                                            C.c_void_p(hist[(f + 1) & 1].data_ptr()), C.c_void_p(hist[f & 1].data_ptr()), C.byref(target), 1, stream))

        arms[f"reduced_s{s}"] = (lambda o=ropt, sc=scratch: check(lib.atmo_render_reduced_target(node._ctx, C.byref(nf), C.byref(src), C.byref(o),
                                                                                                  C.c_void_p(sc.data_ptr()), C.byref(target), 1, stream)))
        arms[f"up_s{s}"] = (lambda o=ropt, ld=low_depth, lc=low_rgba: check(lib.atmo_reduced_upsample(node._ctx, C.byref(nf), C.byref(src), C.byref(o), ld, lc,
                                                                                                      C.byref(target), 1, stream)))
        arms[f"copy_up_s{s}"] = copier(pass_bytes(w, h, s)[1])
        arms[f"temporal_s{s}"] = temporal
        arms[f"resolve_s{s}"] = resolve
        arms[f"copy_resolve_s{s}"] = copier(resolve_bytes(w, h, s))
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
        t = res[f"temporal_s{s}"]
        t["vs_full"] = round(t["median_ms"] / res["full"]["median_ms"], 4)
        t["vs_reduced"] = round(t["median_ms"] / res[f"reduced_s{s}"]["median_ms"], 4)
        res[f"reduced_s{s}"]["vs_full"] = round(res[f"reduced_s{s}"]["median_ms"] / res["full"]["median_ms"], 4)
        for arm, copy, nbytes in ((f"resolve_s{s}", f"copy_resolve_s{s}", resolve_bytes(w, h, s)), (f"up_s{s}", f"copy_up_s{s}", pass_bytes(w, h, s)[1])):
            res[arm]["bytes"] = nbytes
            res[arm]["gb_per_s"] = round(nbytes / (res[arm]["median_ms"] * 1e-3) / 1e9, 1)
            res[arm]["over_copy"] = round(res[arm]["median_ms"] / res[copy]["median_ms"], 3)
        ages = keep[s // 2 - 1][2][0].cpu().numpy()[TP.history_layout(w, h)[1]:][: w * h]       # what the last calls left: how much of it the filter made
        res[f"temporal_s{s}"]["history_fallback_share"] = round(float((ages == 255).mean()), 4)
    res["kernel"] = node.kernel_name
    node.close()
    return res


def verdict(vs_full, vs_reduced):
    a = "wins against the full draw" if vs_full < 1.0 else "LOSES against the full draw"
    return a + (", costs %.2f x the reduced draw" % vs_reduced)


def table(doc):
    rows = ["| config | size | full ms | reduced s2 ms | temporal s2 ms | s2 / full | s2 / reduced | reduced s4 ms | temporal s4 ms | s4 / full | s4 / reduced | verdict |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for key, r in doc["results"].items():
        config, size = key.rsplit("@", 1)
        t2, t4 = r["temporal_s2"], r["temporal_s4"]
        v = "s2 " + verdict(t2["vs_full"], t2["vs_reduced"]) + "; s4 " + verdict(t4["vs_full"], t4["vs_reduced"])
        rows.append(f"| {config} | {size} | {r['full']['median_ms']:.4f} | {r['reduced_s2']['median_ms']:.4f} | {t2['median_ms']:.4f} | {t2['vs_full']:.3f} | "
                    f"{t2['vs_reduced']:.3f} | {r['reduced_s4']['median_ms']:.4f} | {t4['median_ms']:.4f} | {t4['vs_full']:.3f} | {t4['vs_reduced']:.3f} | {v} |")
    rows += ["", "| config | size | resolve s2 / s4 us | its copy us | resolve / copy | upsample s2 / s4 us | its copy us | upsample / copy |", "|---|---|---|---|---|---|---|---|"]
    for key, r in doc["results"].items():
        config, size = key.rsplit("@", 1)
        us = lambda k: 1e3 * r[k]["median_ms"]
        rows.append(f"| {config} | {size} | {us('resolve_s2'):.1f} / {us('resolve_s4'):.1f} | {us('copy_resolve_s2'):.1f} / {us('copy_resolve_s4'):.1f} | "
                    f"{r['resolve_s2']['over_copy']:.2f} / {r['resolve_s4']['over_copy']:.2f} | {us('up_s2'):.1f} / {us('up_s4'):.1f} | "
                    f"{us('copy_up_s2'):.1f} / {us('copy_up_s4'):.1f} | {r['up_s2']['over_copy']:.2f} / {r['up_s4']['over_copy']:.2f} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--table", default=None, help="print the markdown tables of a saved result and exit")
    args = ap.parse_args()
    if args.table:
        with open(args.table) as f:
            print(table(json.loads(f.read())))
        return
    import torch

    from godot_atmosphere_shader_amd import _native as N

    res = dict(build_id=N.load().atmo_build_id().decode(), device=torch.cuda.get_device_name(0), pose="P_space", depth="d32f", target="rgba16f composite",
               depth_tolerance=TOLERANCE, history_tolerance=0.1, previous_camera="a 1-degree orbit back", reps=args.reps, rounds=args.rounds, results={})
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
