"""Cost of drawing into a packed colour target (include/atmo_target.h) on the MI355X: the RGBA16F / RGBA8 draws against the float draws, and against what a
host does without them -- convert its buffer to float4, composite, convert back.

  python tools/target_probe.py --out profiles/targets/target_probe.json

Per workload (shipped8 = no_clouds_8, headline = no_clouds_32x8_direct, clouds_high, clouds_high_rm; pose P_space, the demo scene) and size, these arms are timed
INTERLEAVED in one process -- every round times each arm once, with device events around `reps` draws enqueued through the C entry points (one ctypes call per
draw in every arm):
  a_plain / a_comp          atmo_render / atmo_render_composite (float4)
  b16_plain / b16_comp      atmo_render_target, RGBA16F
  b8_plain / b8_comp        atmo_render_target, RGBA8_UNORM
  c16_comp / c8_comp        the host's way today: torch converts the RGBA16F / RGBA8 buffer to float4, atmo_render_composite, torch converts back
Reported per arm: the median, minimum and maximum of the rounds (ms per draw); b / a ratios beside the spread of a's own samples ((max - min) / median).
Prints one JSON object."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from godot_atmosphere_shader_amd import _native as N  # noqa: E402
from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures, make_node  # noqa: E402

WORKLOADS = [("shipped8", "no_clouds_8"), ("headline", "no_clouds_32x8_direct"), ("clouds_high", "clouds_high"), ("clouds_high_rm", "clouds_high_rm")]
SIZES = [(1920, 1080), (3840, 2160)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def probe(node, cam, depth, reps, rounds):
    h, w = cam.height, cam.width
    lib, ctx = node._lib, node._ctx
    nf = node.prepare_frame(cam)
    node._bake_if_needed(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dptr = C.c_void_p(depth.data_ptr())
    g = torch.Generator(device="cpu").manual_seed(3)
    scene32 = torch.rand((h, w, 4), generator=g, dtype=torch.float32).cuda()
    scene16, scene8 = scene32.to(torch.float16), (scene32 * 255.0).round().to(torch.uint8)
    out32 = torch.empty_like(scene32)
    out16, out8 = torch.empty_like(scene16), torch.empty_like(scene8)
    tmp32 = torch.empty_like(scene32)

    def check(rc):
        if rc != N.ATMO_OK:
            raise RuntimeError(lib.atmo_last_error_string(ctx).decode())

    def target_draw(tensor, fmt, composite):
        t = N.AtmoTarget(tensor.data_ptr(), fmt, 0)
        return lambda: check(lib.atmo_render_target(ctx, C.byref(nf), dptr, C.byref(t), composite, stream))

    def host_way(packed):
        def fn():
            if packed.dtype == torch.uint8:
                torch.div(packed, 255.0, out=tmp32)
            else:
                tmp32.copy_(packed)
            check(lib.atmo_render_composite(ctx, C.byref(nf), dptr, C.c_void_p(tmp32.data_ptr()), stream))
            if packed.dtype == torch.uint8:
                packed.copy_(tmp32.clamp(0.0, 1.0).mul_(255.0).round_())
            else:
                packed.copy_(tmp32)
        return fn

    arms = {
        "a_plain": lambda: check(lib.atmo_render(ctx, C.byref(nf), dptr, C.c_void_p(out32.data_ptr()), stream)),
        "a_comp": lambda: check(lib.atmo_render_composite(ctx, C.byref(nf), dptr, C.c_void_p(scene32.data_ptr()), stream)),
        "b16_plain": target_draw(out16, N.TARGET_RGBA16F, 0),
        "b16_comp": target_draw(scene16, N.TARGET_RGBA16F, 1),
        "b8_plain": target_draw(out8, N.TARGET_RGBA8_UNORM, 0),
        "b8_comp": target_draw(scene8, N.TARGET_RGBA8_UNORM, 1),
        "c16_comp": host_way(scene16.clone()),
        "c8_comp": host_way(scene8.clone()),
    }
    for _ in range(12):   # warm-up: clocks, caches, and the tile order settles (one feedback state serves every arm: same grid, same stream)
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
    samples = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            samples[k].append(timed(fn, reps))
    res = {}
    for k, v in samples.items():
        med = float(np.median(v))
        res[k] = dict(median_ms=round(med, 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5), spread=round((max(v) - min(v)) / med, 4))
    for b, a in (("b16_plain", "a_plain"), ("b8_plain", "a_plain"), ("b16_comp", "a_comp"), ("b8_comp", "a_comp")):
        res[b]["vs_float"] = round(res[b]["median_ms"] / res[a]["median_ms"], 4)
    for c, b in (("c16_comp", "b16_comp"), ("c8_comp", "b8_comp")):
        res[c]["vs_packed"] = round(res[c]["median_ms"] / res[b]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    args = ap.parse_args()
    tex = demo_textures()
    res = dict(build_id=N.load().atmo_build_id().decode(), device=torch.cuda.get_device_name(0), pose="P_space", reps=args.reps, rounds=args.rounds, results={})
    for name, config in WORKLOADS:
        if args.only and name not in args.only.split(","):
            continue
        for w, h in SIZES:
            cam = S.Camera.from_pose(w, h, "P_space")
            depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
            node = make_node(config, tex)
            r = probe(node, cam, depth, args.reps, args.rounds)
            r["kernels"] = node.kernel_name
            node.close()
            res["results"][f"{name}@{w}x{h}"] = r
            print(name, f"{w}x{h}", json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
