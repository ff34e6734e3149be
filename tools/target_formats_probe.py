"""Cost of the sRGB, BGRA and 10-bit colour targets (include/atmo_target.h, formats 16 .. 19) on the MI355X.

  tools/ab_build_commit.sh pre <parent commit>          # the baseline arm's library: godot_atmosphere_shader_amd/libatmo_hip_pre.so
  python tools/target_formats_probe.py --out profiles/targets/target_formats_probe.json

Two questions, per workload (shipped8 = no_clouds_8, headline = no_clouds_32x8_direct; pose P_space, the demo scene, 1920 x 1080):
  1. Do the formats that existed pay for the new ones?  The RGBA16F / RGBA8_UNORM plain and composite draws of this build against the same draws of the
     PARENT commit's library, loaded side by side (--baseline).  Gate: this build's median is not above the parent's by more than the parent arm's own
     spread, (max - min) / median of its rounds.
  2. What do the new formats cost?  Each against RGBA8_UNORM of this build, and its composite against the host's way for that format: torch decodes the
     buffer to float4 with the contract's own tables, atmo_render_composite, torch encodes.  Gate: the packed composite is faster than the host's way.
All arms are timed INTERLEAVED in one process: every round times each arm once, with device events around `reps` draws enqueued through the C entry points.
Reported per arm: median, minimum, maximum of the rounds (ms per draw) and the spread.  Prints one JSON object."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from godot_atmosphere_shader_amd import _native as N  # noqa: E402
from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd import targets as T  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures  # noqa: E402
from target_probe import timed  # noqa: E402
from views_target_probe import load_both, node_on  # noqa: E402

WORKLOADS = [("shipped8", "no_clouds_8"), ("headline", "no_clouds_32x8_direct")]
NEW = [("srgb8", N.TARGET_RGBA8_SRGB), ("bgra8", N.TARGET_BGRA8_UNORM), ("bgra8_srgb", N.TARGET_BGRA8_SRGB), ("rgb10a2", N.TARGET_A2B10G10R10_UNORM)]


class HostWay:
    """decode -> float4 composite -> encode in torch, by the contract of targets.py (the tables for sRGB; rint of the fp32 product for UNORM)."""

    def __init__(self, fmt, packed, composite):
        self.fmt, self.packed, self.composite = fmt, packed, composite
        self.tmp = torch.empty(packed.shape, dtype=torch.float32, device=packed.device)
        self.decode_table = torch.from_numpy(T.SRGB_DECODE.copy()).to(packed.device)
        self.thresh = torch.from_numpy(T.SRGB_THRESH[1:].copy()).to(packed.device)
        self.srgb = fmt in (T.RGBA8_SRGB, T.BGRA8_SRGB)
        self.order = [2, 1, 0, 3] if fmt in (T.BGRA8, T.BGRA8_SRGB) else None

    def __call__(self):
        p, tmp = self.packed, self.tmp
        if self.fmt == T.A2B10G10R10:
            w = p.view(torch.int32)[..., 0]
            for c in range(3):
                torch.div((w >> (10 * c)) & 1023, 1023.0, out=tmp[..., c])
            torch.div((w >> 30) & 3, 3.0, out=tmp[..., 3])
        else:
            q = p[..., self.order] if self.order else p
            if self.srgb:
                tmp[..., :3] = self.decode_table[q[..., :3].long()]
                torch.div(q[..., 3], 255.0, out=tmp[..., 3])
            else:
                torch.div(q, 255.0, out=tmp)
        self.composite(tmp)
        c = tmp.nan_to_num_(0.0).clamp_(0.0, 1.0)
        if self.fmt == T.A2B10G10R10:
            rgb = c[..., :3].mul(1023.0).round_().to(torch.int32)
            a = c[..., 3].mul(3.0).round_().to(torch.int32)
            p.view(torch.int32)[..., 0] = rgb[..., 0] | (rgb[..., 1] << 10) | (rgb[..., 2] << 20) | (a << 30)
            return
        out = torch.empty_like(p)
        if self.srgb:
            out[..., :3] = torch.bucketize(c[..., :3].contiguous(), self.thresh, right=True)
            out[..., 3] = c[..., 3].mul(255.0).round_()
        else:
            out.copy_(c.mul_(255.0).round_())
        p.copy_(out[..., self.order] if self.order else out)


def probe(cur_node, pre_node, cam, depth, reps, rounds):
    h, w = cam.height, cam.width
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dptr = C.c_void_p(depth.data_ptr())
    g = torch.Generator(device="cpu").manual_seed(3)
    scene32 = torch.rand((h, w, 4), generator=g, dtype=torch.float32).cuda()
    scene16, scene8 = scene32.to(torch.float16), (scene32 * 255.0).round().to(torch.uint8)

    def draws(node):
        lib, ctx, nf = node._lib, node._ctx, node.prepare_frame(cam)
        node._bake_if_needed(0)

        def check(rc):
            if rc != N.ATMO_OK:
                raise RuntimeError(lib.atmo_last_error_string(ctx).decode())

        def target_draw(tensor, fmt, composite):
            t = N.AtmoTarget(tensor.data_ptr(), fmt, 0)
            return lambda: check(lib.atmo_render_target(ctx, C.byref(nf), dptr, C.byref(t), composite, stream))

        def float_composite(tensor):
            check(lib.atmo_render_composite(ctx, C.byref(nf), dptr, C.c_void_p(tensor.data_ptr()), stream))

        return target_draw, float_composite

    arms = {}
    for tag, node in (("cur", cur_node), ("pre", pre_node)):
        if node is None:
            continue
        target_draw, _ = draws(node)
        arms[f"{tag}_b16_plain"] = target_draw(torch.empty_like(scene16), N.TARGET_RGBA16F, 0)
        arms[f"{tag}_b16_comp"] = target_draw(scene16.clone(), N.TARGET_RGBA16F, 1)
        arms[f"{tag}_b8_plain"] = target_draw(torch.empty_like(scene8), N.TARGET_RGBA8_UNORM, 0)
        arms[f"{tag}_b8_comp"] = target_draw(scene8.clone(), N.TARGET_RGBA8_UNORM, 1)
    target_draw, float_composite = draws(cur_node)
    for name, fmt in NEW:
        arms[f"{name}_plain"] = target_draw(torch.empty_like(scene8), fmt, 0)
        arms[f"{name}_comp"] = target_draw(scene8.clone(), fmt, 1)
        arms[f"{name}_host_comp"] = HostWay(fmt, scene8.clone(), float_composite)
    for _ in range(12):   # warm-up: clocks, caches, and the tile order settles
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
    # Order inside a round: every parent arm next to this build's arm of the same draw, which of the two goes first alternating from round to round, so
    # that neither is always the one behind the other kind of work; an untimed draw in front of each pair (the arm before it may have been a host's way,
    # a dozen torch kernels over the whole image).
    samples = {k: [] for k in arms}
    pairs = [k[4:] for k in arms if k.startswith("pre_")]
    rest = [k for k in arms if not k.startswith(("cur_", "pre_"))]
    for r in range(rounds):
        for k in pairs:
            arms[f"cur_{k}"]()
            for tag in (("cur", "pre") if r % 2 == 0 else ("pre", "cur")):
                samples[f"{tag}_{k}"].append(timed(arms[f"{tag}_{k}"], reps))
        for k in ([] if pairs else [k for k in arms if k.startswith("cur_")]) + rest:
            samples[k].append(timed(arms[k], reps))
    res = {}
    for k, v in samples.items():
        med = float(np.median(v))
        res[k] = dict(median_ms=round(med, 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5), spread=round((max(v) - min(v)) / med, 4))
    gates = dict(existing_formats_do_not_pay=True, packed_beats_host_way=True, failed=[])
    if pre_node is not None:
        for k in ("b16_plain", "b16_comp", "b8_plain", "b8_comp"):
            ratio = res[f"cur_{k}"]["median_ms"] / res[f"pre_{k}"]["median_ms"]
            res[f"cur_{k}"]["vs_parent"] = round(ratio, 4)
            if ratio - 1.0 > res[f"pre_{k}"]["spread"]:
                gates["existing_formats_do_not_pay"] = False
                gates["failed"].append(f"cur_{k}")
    for name, _ in NEW:
        for kind in ("plain", "comp"):
            res[f"{name}_{kind}"]["vs_rgba8"] = round(res[f"{name}_{kind}"]["median_ms"] / res[f"cur_b8_{kind}"]["median_ms"], 4)
        res[f"{name}_host_comp"]["vs_packed"] = round(res[f"{name}_host_comp"]["median_ms"] / res[f"{name}_comp"]["median_ms"], 4)
        if not res[f"{name}_comp"]["median_ms"] < res[f"{name}_host_comp"]["median_ms"]:
            gates["packed_beats_host_way"] = False
            gates["failed"].append(f"{name}_comp")
    res["gates"] = gates
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline", default=os.path.join(ROOT, "godot_atmosphere_shader_amd", "libatmo_hip_pre.so"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    cur, pre = load_both(args.baseline)
    tex = demo_textures()
    w, h = (int(x) for x in args.size.split("x"))
    res = dict(build_id=cur.atmo_build_id().decode(), baseline_build_id=pre.atmo_build_id().decode() if pre else None, device=torch.cuda.get_device_name(0),
               pose="P_space", reps=args.reps, rounds=args.rounds, results={})
    for name, config in WORKLOADS:
        cam = S.Camera.from_pose(w, h, "P_space")
        depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
        cur_node = node_on(cur, cur, config, tex)
        pre_node = node_on(pre, cur, config, tex) if pre else None
        r = probe(cur_node, pre_node, cam, depth, args.reps, args.rounds)
        cur_node.close()
        if pre_node is not None:
            pre_node.close()
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
