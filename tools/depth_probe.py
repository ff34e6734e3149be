"""Cost of reading the renderer's own depth buffer (include/atmo_depth.h) on the MI355X: the depth-source draws against the parent commit's float-depth draw,
and against what a D24 host does without them -- a conversion pass into a float copy in front of every draw.

  tools/ab_build_commit.sh pre <parent commit>
  ATMO_HIP_LIB=godot_atmosphere_shader_amd/libatmo_hip_pre.so python tools/depth_probe.py --out profiles/depth/depth_probe.json

ONE process holds both libraries: ATMO_HIP_LIB names the parent's (arms a, a2 and b draw with it), the in-tree library draws arm c.  Per workload
(no_clouds_32x8_direct = the headline, no_clouds_8, clouds_high, clouds_high_rm; pose P_space, 1920 x 1080, composite into RGBA16F) the arms are timed
INTERLEAVED -- every round times each arm once, device events around `reps` draws through the C entry points (one ctypes call per draw):
  a, a2       the parent's atmo_render_target on a tight float depth, twice: a2 / a is the run-to-run spread of (a) against itself
  b           the parent's draw behind the conversion pass `(d & 0xFFFFFF).float() / 16777215` into a preallocated float buffer
  c_x8d24, c_d16, c_d32f_pitched   atmo_render_depth_target on the buffer as it is
  a_d16, b_d16   (a) and (b) for the D16 buffer: 16 bits lose the far ground of this pose (its codes round to 0, the far plane), so the D16 picture has
                 more sky behind the limb to march than the float picture -- c_d16 is held against the parent's draw of the SAME picture (the decoded
                 floats) and against the D16 conversion pass, not against (a)
after bench.py's priming (warm-up draws, four frame-paced draws, 25 ms of sustained work).  Reported per arm: the median, minimum and maximum of the
rounds (ms per draw); c / a and c / b ratios.  Prints one JSON object."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from godot_atmosphere_shader_amd import _native as N  # noqa: E402
from godot_atmosphere_shader_amd import depth_formats as D  # noqa: E402
from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures, make_node  # noqa: E402

WORKLOADS = ["no_clouds_32x8_direct", "no_clouds_8", "clouds_high", "clouds_high_rm"]
W, H = 1920, 1080
PITCH_PAD = 64   # texels of padding per row of the pitched d32f arm


def load_both():
    """(the parent's library, the in-tree library): N.load() once per path."""
    parent_path = os.environ.get("ATMO_HIP_LIB")
    if not parent_path:
        raise SystemExit("ATMO_HIP_LIB must name the parent commit's library (tools/ab_build_commit.sh pre <parent>)")
    parent = N.load()
    os.environ.pop("ATMO_HIP_LIB")
    N._lib, N.LIB_PATH = None, os.path.join(ROOT, "godot_atmosphere_shader_amd", "libatmo_hip.so")
    return parent, N.load()


def node_of(lib, config, tex):
    N._lib = lib   # PlanetAtmosphere binds whichever library is loaded when it is made
    return make_node(config, tex)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def probe(parent_node, new_node, cam, depth_np, reps, rounds):
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for node in (parent_node, new_node):
        node._bake_if_needed(stream.value)
    g = torch.Generator(device="cpu").manual_seed(3)
    scene = torch.rand((H, W, 4), generator=g, dtype=torch.float32).to(torch.float16).cuda()
    target = N.AtmoTarget(scene.data_ptr(), N.TARGET_RGBA16F, 0)
    depth = torch.from_numpy(depth_np).cuda()
    words = torch.from_numpy(D.quantise(depth_np, "x8d24").view(np.int32)).cuda()
    codes = torch.from_numpy(D.quantise(depth_np, "d16").view(np.int16)).cuda()
    pitched = torch.zeros((H, W + PITCH_PAD), dtype=torch.float32, device="cuda")
    pitched[:, :W] = depth
    converted = torch.empty((H, W), dtype=torch.float32, device="cuda")
    masked = torch.empty((H, W), dtype=torch.int32, device="cuda")
    decoded16 = torch.from_numpy(D.decode(D.quantise(depth_np, "d16"), "d16")).cuda()
    codes32 = torch.empty((H, W), dtype=torch.int32, device="cuda")
    frames = {id(n): n.prepare_frame(cam) for n in (parent_node, new_node)}

    def check(node, rc):
        if rc != N.ATMO_OK:
            raise RuntimeError(node._lib.atmo_last_error_string(node._ctx).decode())

    def float_draw(node, tensor):
        nf, ptr = frames[id(node)], C.c_void_p(tensor.data_ptr())
        return lambda: check(node, node._lib.atmo_render_target(node._ctx, C.byref(nf), ptr, C.byref(target), 1, stream))

    def depth_draw(tensor, fmt, pitch):
        nf, d = frames[id(new_node)], N.AtmoDepth(tensor.data_ptr(), fmt, pitch)
        return lambda: check(new_node, new_node._lib.atmo_render_depth_target(new_node._ctx, C.byref(nf), C.byref(d), C.byref(target), 1, stream))

    draw_converted = float_draw(parent_node, converted)

    def host_way():   # what a D24 host pays today: the conversion pass, then the draw on the float copy
        torch.bitwise_and(words, 0xFFFFFF, out=masked)
        converted.copy_(masked)
        converted.div_(16777215.0)
        draw_converted()

    def host_way_d16():
        codes32.copy_(codes)
        torch.bitwise_and(codes32, 0xFFFF, out=codes32)
        converted.copy_(codes32)
        converted.div_(65535.0)
        draw_converted()

    arms = {
        "a": float_draw(parent_node, depth),
        "b": host_way,
        "a_d16": float_draw(parent_node, decoded16),
        "b_d16": host_way_d16,
        "c_x8d24": depth_draw(words, N.DEPTH_X8_D24_UNORM, 0),
        "c_d16": depth_draw(codes, N.DEPTH_D16_UNORM, 0),
        "c_d32f_pitched": depth_draw(pitched, N.DEPTH_D32_SFLOAT, 4 * (W + PITCH_PAD)),
        "a2": float_draw(parent_node, depth),
    }
    # bench.py's priming: warm-up draws, four frame-paced draws (the tile order settles), 25 ms of sustained work
    for fn in arms.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(4):
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
            samples[k].append(timed(fn, reps))
    res = {}
    for k, v in samples.items():
        med = float(np.median(v))
        res[k] = dict(median_ms=round(med, 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5))
    res["spread_a2_over_a"] = round(res["a2"]["median_ms"] / res["a"]["median_ms"], 4)
    for k, a, b in (("c_x8d24", "a", "b"), ("c_d16", "a_d16", "b_d16"), ("c_d32f_pitched", "a", "b")):
        res[k]["vs_a"] = round(res[k]["median_ms"] / res[a]["median_ms"], 4)
        res[k]["vs_b"] = round(res[k]["median_ms"] / res[b]["median_ms"], 4)
    res["b"]["vs_a"] = round(res["b"]["median_ms"] / res["a"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    args = ap.parse_args()
    parent, new = load_both()
    tex = demo_textures()
    cam = S.Camera.from_pose(W, H, "P_space")
    depth_np = S.depth_ground_sphere(cam)
    res = dict(parent_build_id=parent.atmo_build_id().decode(), build_id=new.atmo_build_id().decode(), device=torch.cuda.get_device_name(0), pose="P_space",
               size=[W, H], reps=args.reps, rounds=args.rounds, results={})
    for config in WORKLOADS:
        if args.only and config not in args.only.split(","):
            continue
        parent_node, new_node = node_of(parent, config, tex), node_of(new, config, tex)
        r = probe(parent_node, new_node, cam, depth_np, args.reps, args.rounds)
        r["kernels"] = [parent_node.kernel_name, new_node.kernel_name]
        parent_node.close()
        new_node.close()
        res["results"][config] = r
        print(config, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
