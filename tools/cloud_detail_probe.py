"""What the detail fetch costs (include/atmo_cloud_detail.h) on the MI355X: clouds_high and clouds_high_rm at 1920 x 1080, pose P_space, under both
cubemap samplers, cloud detail off against on.

    python tools/cloud_detail_probe.py [--out profiles/cloud_detail/cloud_detail_probe.json] [--reps 20] [--rounds 3]

ONE process, one context per workload and sampler; the two arms are timed INTERLEAVED -- every round times `off` (the context's usual kernel, tile-order
feedback as shipped), then `on` (atmo_render_detail_kernel, row-major), then `off` again (off2: off2 / off is the run-to-run spread of an arm against
itself), device events around `reps` draws through the binding, after warm-up draws of both arms (the feedback's order settles within them).  TIME
advances by a sixtieth of a second per draw in both arms (it is dead with detail off).  Reported per arm: the median, minimum and maximum of the rounds
(ms per draw), on / off, and the kernel each arm reported.  Prints one JSON object.  Needs a device: there is no CPU figure.

    python tools/cloud_detail_probe.py --table target [--out profiles/cloud_detail/detail_target_probe.json] [--reps 20] [--rounds 5]

The TARGET table (include/atmo_detail_target.h), cloud detail on in every arm, the same workloads, samplers, viewport and pose, rounds interleaved: `base`,
the float detail draw (atmo_render: float4 pixels, float depth) -- the baseline of every ratio --; `f32_d32`, `f16_d32`, `srgb_d16`:
atmo_render_detail_target into RGBA32F from D32, RGBA16F from D32, RGBA8_SRGB from D16; `batch2`: two 960 x 1080 views -- the halves of one RGBA16F image
and one D32 image -- in one atmo_render_views_detail_target; `singles2`: the same two views as two atmo_render_detail_target draws; `base2`: the baseline
once more (base2 / base is the run-to-run spread of an arm against itself); `base_d16`: the float detail draw handed a tight float buffer of the DECODED
D16 values -- sixteen bits lose this pose's far ground (profiles/depth/README.md), so the D16 picture is another picture than `base`'s and `srgb_d16` is
like for like against this arm only.  All through the binding."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures, make_node  # noqa: E402

WORKLOADS = ["clouds_high", "clouds_high_rm"]
SAMPLERS = {"declared": None, "lod0": False}   # PlanetAtmosphere's cubemap_lod
W, H = 1920, 1080


def timed(node, cam, depth, out, reps, t0):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        node.render(cam, depth, out=out, time=t0 + i / 60.0)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


TARGET_ARMS = ("base", "f32_d32", "f16_d32", "srgb_d16", "base_d16", "batch2", "singles2", "base2")


def target_table(args):
    from godot_atmosphere_shader_amd import depth_formats as D
    from godot_atmosphere_shader_amd.planet_atmosphere import depth_source

    tex = demo_textures()
    cam = S.Camera.from_pose(W, H, "P_space")
    half = [S.Camera.from_pose(W // 2, H, "P_space"), S.Camera.from_pose(W // 2, H, "P_space")]
    depth_np = S.depth_ground_sphere(cam)
    depth = torch.from_numpy(depth_np).cuda()
    d16 = depth_source(torch.from_numpy(D.quantise(depth_np, "d16").view("int16")).cuda(), "d16")
    depth_d16 = torch.from_numpy(D.decode(D.quantise(depth_np, "d16"), "d16")).cuda()
    d32 = depth_source(depth)
    d32_halves = [depth_source(depth[:, :W // 2]), depth_source(depth[:, W // 2:])]
    out32 = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out16 = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
    out8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    out16_halves = [out16[:, :W // 2], out16[:, W // 2:]]

    def draws(node, arm, t):
        if arm in ("base", "base2"):
            node.render(cam, depth, out=out32, time=t)
        elif arm == "base_d16":
            node.render(cam, depth_d16, out=out32, time=t)
        elif arm == "f32_d32":
            node.render(cam, d32, out=out32, time=t)
        elif arm == "f16_d32":
            node.render(cam, depth, out=out16, time=t)
        elif arm == "srgb_d16":
            node.render(cam, d16, out=out8, time=t, target="rgba8_srgb")
        elif arm == "batch2":
            node.render_views(half, d32_halves, out16_halves, time=t)
        else:
            for c, d, o in zip(half, d32_halves, out16_halves):
                node.render(c, d, out=o, time=t)

    def timed_arm(node, arm, reps, t0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            draws(node, arm, t0 + i / 60.0)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    result = {"table": "target", "viewport": [W, H], "pose": "P_space", "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
              "rows": []}
    for workload in WORKLOADS:
        for sampler, lod in SAMPLERS.items():
            node = make_node(workload, tex, cubemap_lod=lod, cloud_detail=True)
            names, arms = {}, {a: [] for a in TARGET_ARMS}
            try:
                for arm in TARGET_ARMS[:-1]:
                    timed_arm(node, arm, args.warmup, 0.0)
                    names[arm] = node.kernel_name
                for r in range(args.rounds):
                    for arm in TARGET_ARMS:
                        arms[arm].append(timed_arm(node, arm, args.reps, 1.0 + r))
            finally:
                node.close()
            med = {a: sorted(v)[len(v) // 2] for a, v in arms.items()}
            row = {"workload": workload, "sampler": sampler, "kernels": names,
                   "ms": {a: {"median": med[a], "min": min(v), "max": max(v)} for a, v in arms.items()},
                   "over_base": {a: med[a] / med["base"] for a in TARGET_ARMS}, "batch2_over_singles2": med["batch2"] / med["singles2"],
                   "srgb_d16_over_base_d16": med["srgb_d16"] / med["base_d16"]}
            result["rows"].append(row)
            print(f"{workload:16s} {sampler:9s} " + "  ".join(f"{a} {med[a]:.4f} ({row['over_base'][a]:.3f} x)" for a in TARGET_ARMS), file=sys.stderr, flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", choices=["switch", "target"], default="switch")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=24)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cloud_detail_probe.py measures on a device; none is visible")
    if args.table == "target":
        return emit(target_table(args), args)
    tex = demo_textures()
    cam = S.Camera.from_pose(W, H, "P_space")
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    result = {"viewport": [W, H], "pose": "P_space", "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "rows": []}
    for workload in WORKLOADS:
        for sampler, lod in SAMPLERS.items():
            node = make_node(workload, tex, cubemap_lod=lod)
            names, arms = {}, {"off": [], "on": [], "off2": []}
            try:
                for on in (False, True):
                    node.cloud_detail = on
                    timed(node, cam, depth, out, args.warmup, 0.0)
                    names["on" if on else "off"] = node.kernel_name
                for r in range(args.rounds):
                    for arm in ("off", "on", "off2"):
                        node.cloud_detail = arm == "on"
                        arms[arm].append(timed(node, cam, depth, out, args.reps, 1.0 + r))
            finally:
                node.close()
            med = {a: sorted(v)[len(v) // 2] for a, v in arms.items()}
            row = {"workload": workload, "sampler": sampler, "kernels": names,
                   "ms": {a: {"median": med[a], "min": min(v), "max": max(v)} for a, v in arms.items()},
                   "on_over_off": med["on"] / med["off"], "off2_over_off": med["off2"] / med["off"]}
            result["rows"].append(row)
            print(f"{workload:16s} {sampler:9s} off {med['off']:.4f} ms  on {med['on']:.4f} ms  ({row['on_over_off']:.3f} x)  off again {med['off2']:.4f} ms "
                  f"({row['off2_over_off']:.3f} x)   {names['off']} -> {names['on']}", file=sys.stderr, flush=True)
    emit(result, args)


def emit(result, args):
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
