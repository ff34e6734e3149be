"""What shading caller-supplied rays costs (include/atmo_rays.h) on the MI355X, per kernel family: atmo_shade_rays on the camera rays of the 1920 x 1080
P_space frame against the like-for-like draw, and the same rays once more in a fixed random order.

    python tools/rays_probe.py [--out profiles/rays/rays_probe.json] [--reps 20] [--rounds 3]

ONE process, one context per family; three arms timed INTERLEAVED, every round in the order render, rays, shuffled, render2:
  render    atmo_render of the frame with atmo_set_sampler_lod 0 and atmo_set_tile_feedback 0 -- row-major, level 0: the draw the ray kernels are held to
            bit for bit (tests/test_rays_gpu.py), so what differs is the lane mapping (64 consecutive rays of a row against a 16 x 4 pixel block), 32 more
            bytes read per ray, and the planet centre (and the clouds' origin) in VGPRs instead of SGPRs;
  rays      atmo_shade_rays on camera_rays(frame), width = 1920;
  shuffled  the same rays in a fixed random permutation (seed 1), width = n: what a bounce-ray queue looks like -- the rays of a wave no longer march in step;
  render2   render again: render2 / render is the run-to-run spread of an arm against itself.
Device events around `reps` calls through the binding (one event pair around the K launches), after priming as bench.py does: warm-up calls of every arm,
then ~25 ms of draws so that the clocks are the sustained ones.  Reported per arm: the median, minimum and maximum of the rounds (ms per call), the ratios
of the medians, and the kernel each arm reported.  Prints one JSON object.  Needs a device: there is no CPU figure.

The QUADS table (--table quads, or both: the default), for the three cloud families under the DECLARED sampler (include/atmo_ray_quads.h), same frame, same
timing, every round in the order render, quads, rays, render2:
  render    atmo_render under the default, declared sampler (a chain bound) with atmo_set_tile_feedback 0: the draw the quad kernels are held to bit for bit
            (tests/test_ray_quads_gpu.py); a wave there is a 16 x 4 pixel block, here a 32 x 2 strip (16 quads of a quad row);
  quads     atmo_shade_ray_quads on camera_ray_quads(frame), width = 1920;
  rays      the level-0 atmo_shade_rays of the same frame's rays, for scale (another picture: level 0);
  render2   render again.
`bits_equal_render`: the quads' picture, put back into rows, is the render arm's.

The ORDER table (--table order; include/atmo_ray_order.h), all seven families under the level-0 sampler, same frame, same timing, every round in the order
rays, shuffled, order, indexed, indexed_id, order_indexed:
  rays           the frame's order, plain (width = 1920);
  shuffled       the fixed permutation, plain (width = n): the queue the order is for;
  order          atmo_ray_order alone on the shuffled queue, scratch and index allocated once;
  indexed        atmo_shade_rays_indexed on the shuffled queue through the device's order;
  indexed_id     the coherent queue through the identity: what the indirection costs by itself;
  order_indexed  order, then indexed, back to back in one timed call: the sum as a queue's owner pays it.
The plain arms run the parent commit's instructions (tools/isa_diff.py is the proof), so no second library is needed.  `bits_equal`, per arm: rays -- the
render frame's; shuffled -- its own second run's; order -- ray_order.ray_order of the same rays in numpy; indexed and order_indexed -- the shuffled arm's;
indexed_id -- the rays arm's.  `order_plus_indexed_ms` is the sum of the two medians, `below_shuffled_range` whether it and the order_indexed median lie
below the MINIMUM of the shuffled arm's rounds.

The LIST table (--table list --rounds 5; include/atmo_ray_list.h), the ORDER table's shuffled queue from P_space and from P_limb, same timing.  Per pose,
once (the list does not depend on the family): atmo_ray_list alone for each flag combination (list_0, list_order, list_cull, list_order_cull) against
atmo_ray_order of the same queue (order), every ray live; `parity`: whether list_order's median lies inside order's min-max range widened by 5 %.  Per
pose and family, every round in the order shuffled, order_indexed, cull_indexed, order_cull_indexed, eighth_plain, eighth_list, tail:
  shuffled            the plain atmo_shade_rays of the queue;
  order_indexed       atmo_ray_order, then atmo_shade_rays_indexed;
  cull_indexed        atmo_ray_list(CULL), then atmo_shade_rays_indexed over the capacity;
  order_cull_indexed  atmo_ray_list(ORDER | CULL), then the same;
  eighth_plain        the plain call on the first capacity / 8 rays: what a host that read the count back would launch;
  eighth_list         *count = capacity / 8: atmo_ray_list(ORDER | CULL) and the indexed call, both over the whole capacity;
  tail                the indexed call through a list of END entries alone: one index load per thread and nothing else.
The baselines are kernels this library shares with its parent byte for byte (tools/isa_diff.py).  `bits_equal`: every list arm's picture against the
shuffled arm's (eighth_list: against eighth_plain's, on the live rows).

The DETAIL table (--table detail --rounds 5; include/atmo_ray_detail.h), the three cloud families with atmo_set_cloud_detail 1, the frame from P_space and
from P_limb, same timing.  Two contexts per pose and family, atmo_set_tile_feedback 0; every round in the order of DETAIL_ARMS:
  render, rays             level-0 context: the detail draw (atmo_render_detail_kernel) and atmo_shade_rays_detail on the camera's rays in order;
  shuffled                 the plain detail call on the fixed shuffled queue;
  list_indexed             atmo_ray_list(ORDER | CULL), then the indexed detail call;
  order_indexed            atmo_ray_order, then the indexed detail call;
  render_off, rays_off     the same context with the switch off: atmo_render_kernel and atmo_shade_rays_kernel, for the on / off ratios;
  render_q, quads          declared-sampler context: the detail draw and atmo_shade_ray_quads_detail on the camera's quads;
  render_q_off, quads_off  the same with the switch off;
  render2                  the level-0 detail draw again: the run-to-run spread.
The pixel-side kernels are the parent commit's byte for byte (tools/isa_diff.py).  `bits_equal`: rays and quads against their draws, the two list arms
against the shuffled arm.

The LENS table (--table lens --rounds 5; include/atmo_lens.h), 2048 x 1024 (the cube face 1448 x 1448, as many rays within 0.03 %), same timing, every
entry the median of the interleaved rounds.  `generator`: per lens, atmo_lens_rays alone -- row-major (`rows`), row-major with the tile index (`tiles`)
and in quad order (`quads`) -- beside the 32 B / ray write floor at 6.2 TB/s (`floor_ms`; the tile index adds 4 B an entry).  `panorama`: per pose
(P_space: 13 % of the sphere is the planet; P_clouds: the eye inside the cloud layer, every ray hits the shell) and family (clouds_high, clouds_high_rm, lut;
the default sampler, a chain bound) the equirect's rays shaded three ways: `plain` = atmo_shade_rays row by row, `tiles` = the same rays through the
tile index (atmo_shade_rays_indexed), `quads` = atmo_shade_ray_quads (the declared sampler: another picture; null for lut, which has no texture call).
`bits_equal`: the tile arm against the plain arm."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_textures, make_node  # noqa: E402

# label -> (demo configuration, PlanetAtmosphere keywords)
FAMILIES = {
    "lut": ("no_clouds_32_lut", {}),
    "direct8": ("no_clouds_32x8_direct", {}),
    "direct5": ("no_clouds_8", dict(view_steps=32, light_mode="direct", light_steps=5)),
    "clouds_high": ("clouds_high", {}),
    "clouds_high_rm": ("clouds_high_rm", {}),
    "v1_no_clouds": ("v1_no_clouds", {}),
    "v1_clouds": ("v1_clouds", {}),
}
W, H = 1920, 1080
ARMS = ("render", "rays", "shuffled", "render2")
QUAD_FAMILIES = ("clouds_high", "clouds_high_rm", "v1_clouds")
QUAD_ARMS = ("render", "quads", "rays", "render2")
ORDER_ARMS = ("rays", "shuffled", "order", "indexed", "indexed_id", "order_indexed")


def order_rows(args, tex, cam, depth, frame, out, perm):
    """The ORDER table's rows (the module's docstring)."""
    import ctypes as C

    import numpy as np

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd import ray_order as R

    n = H * W
    rows = []
    identity = torch.arange(n, dtype=torch.int32, device="cuda")
    out2 = torch.empty_like(out)
    for label in args.families.split(","):
        config, kw = FAMILIES[label]
        node = make_node(config, tex, cubemap_lod=False, tile_feedback=0, **kw)   # atmo_set_sampler_lod 0, atmo_set_tile_feedback 0
        try:
            rays = node.camera_rays(cam, depth)
            shuffled = rays[perm].contiguous()
            need = C.c_size_t()
            N.check(node._ctx, node._lib.atmo_ray_order_scratch_bytes(n, C.byref(need)))
            scratch = torch.empty(((need.value + 3) // 4,), dtype=torch.int32, device="cuda")
            index = torch.empty((n,), dtype=torch.int32, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream

            def order():
                N.check(node._ctx, node._lib.atmo_ray_order(node._ctx, shuffled.data_ptr(), n, index.data_ptr(), scratch.data_ptr(), need.value, stream))

            def indexed():
                node.shade_rays(shuffled, cam, out=out2, index=index)

            def both():
                order()
                indexed()

            calls = {"rays": lambda: node.shade_rays(rays, cam, width=W, out=out), "shuffled": lambda: node.shade_rays(shuffled, cam, out=out),
                     "order": order, "indexed": indexed, "indexed_id": lambda: node.shade_rays(rays, cam, width=W, out=out2, index=identity),
                     "order_indexed": both}
            names = {}
            for arm in ORDER_ARMS:
                timed(calls[arm], args.warmup)
                names[arm] = node.kernel_name
            # the pictures, outside the timing
            bits = lambda t: t.view(torch.int32)   # noqa: E731
            equal = {}
            node.render(cam, depth, out=frame)
            calls["rays"]()
            plain = out.clone()
            equal["rays"] = bool(torch.equal(bits(frame.reshape(-1, 4)), bits(plain)))
            calls["shuffled"]()
            plain_shuffled = out.clone()
            calls["shuffled"]()
            equal["shuffled"] = bool(torch.equal(bits(out), bits(plain_shuffled)))
            index.fill_(-1)
            order()
            torch.cuda.synchronize()
            equal["order"] = bool(np.array_equal(index.cpu().numpy().astype(np.int64), R.ray_order(shuffled.cpu().numpy())))
            out2.fill_(float("nan"))
            indexed()
            equal["indexed"] = bool(torch.equal(bits(out2), bits(plain_shuffled)))
            out2.fill_(float("nan"))
            calls["indexed_id"]()
            equal["indexed_id"] = bool(torch.equal(bits(out2), bits(plain)))
            out2.fill_(float("nan"))
            index.fill_(-1)
            both()
            equal["order_indexed"] = bool(torch.equal(bits(out2), bits(plain_shuffled)))
            t_warm = time.perf_counter()
            while time.perf_counter() - t_warm < 0.025:   # sustained clocks
                calls["rays"]()
                torch.cuda.synchronize()
            arms = {a: [] for a in ORDER_ARMS}
            for _ in range(args.rounds):
                for arm in ORDER_ARMS:
                    arms[arm].append(timed(calls[arm], args.reps))
        finally:
            node.close()
        med = {a: sorted(v)[len(v) // 2] for a, v in arms.items()}
        total = med["order"] + med["indexed"]
        row = {"family": label, "kernels": names, "bits_equal": equal,
               "ms": {a: {"median": med[a], "min": min(v), "max": max(v)} for a, v in arms.items()},
               "shuffled_over_rays": med["shuffled"] / med["rays"], "indexed_over_rays": med["indexed"] / med["rays"],
               "indexed_id_over_rays": med["indexed_id"] / med["rays"], "order_plus_indexed_ms": total,
               "order_plus_indexed_over_shuffled": total / med["shuffled"], "order_indexed_over_shuffled": med["order_indexed"] / med["shuffled"],
               "below_shuffled_range": bool(total < min(arms["shuffled"]) and med["order_indexed"] < min(arms["shuffled"]))}
        rows.append(row)
        print(f"{label:15s} rays {med['rays']:.4f}  shuffled {med['shuffled']:.4f} ({min(arms['shuffled']):.4f} - {max(arms['shuffled']):.4f})  order "
              f"{med['order']:.4f}  indexed {med['indexed']:.4f}  indexed_id {med['indexed_id']:.4f}  order + indexed {total:.4f} (one call: "
              f"{med['order_indexed']:.4f}) ms = {row['order_plus_indexed_over_shuffled']:.3f} x shuffled  below its range: {row['below_shuffled_range']}  "
              f"bits equal: {equal}  {names['indexed']}", file=sys.stderr, flush=True)
    return rows


LIST_ALONE = ("order", "list_0", "list_order", "list_cull", "list_order_cull")
LIST_ARMS = ("shuffled", "order_indexed", "cull_indexed", "order_cull_indexed", "eighth_plain", "eighth_list", "tail")


def list_rows(args, tex, out, perm):
    """The LIST table's rows (the module's docstring)."""
    import ctypes as C

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame

    n = H * W
    stats = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}   # noqa: E731
    bits = lambda t: t.view(torch.int32)   # noqa: E731
    poses = []
    out2 = torch.empty_like(out)
    for pose in ("P_space", "P_limb"):
        cam = S.Camera.from_pose(W, H, pose)
        depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
        entry = {"pose": pose, "rows": []}
        for label in args.families.split(","):
            config, kw = FAMILIES[label]
            node = make_node(config, tex, cubemap_lod=False, tile_feedback=0, **kw)
            try:
                shuffled = node.camera_rays(cam, depth)[perm].contiguous()
                need = C.c_size_t()
                N.check(node._ctx, node._lib.atmo_ray_list_scratch_bytes(n, C.byref(need)))
                scratch = torch.empty(((need.value + 3) // 4,), dtype=torch.int32, device="cuda")
                index = torch.empty((n,), dtype=torch.int32, device="cuda")
                ends = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                listed = torch.zeros((1,), dtype=torch.int32, device="cuda")
                full = torch.tensor([n], dtype=torch.int32, device="cuda")
                eighth = torch.tensor([n // 8], dtype=torch.int32, device="cuda")
                nf = _to_native_frame(node.make_frame(cam, 0.0))
                stream = torch.cuda.current_stream().cuda_stream

                def order():
                    N.check(node._ctx, node._lib.atmo_ray_order(node._ctx, shuffled.data_ptr(), n, index.data_ptr(), scratch.data_ptr(), need.value, stream))

                def build(flags, count=full, rgba=out2):
                    N.check(node._ctx, node._lib.atmo_ray_list(node._ctx, C.byref(nf), shuffled.data_ptr(), count.data_ptr(), n, flags, rgba.data_ptr(),
                                                               index.data_ptr(), listed.data_ptr(), scratch.data_ptr(), need.value, stream))

                def indexed(through=index):
                    node.shade_rays(shuffled, cam, out=out2, index=through)

                def pair(first):
                    first()
                    indexed()

                if not entry.get("list_alone"):   # the list alone, once per pose
                    alone = {"order": order, "list_0": lambda: build(0), "list_order": lambda: build(1), "list_cull": lambda: build(2),
                             "list_order_cull": lambda: build(3)}
                    for arm in LIST_ALONE:
                        timed(alone[arm], args.warmup)
                    t = {a: [] for a in LIST_ALONE}
                    for _ in range(args.rounds):
                        for arm in LIST_ALONE:
                            t[arm].append(timed(alone[arm], args.reps))
                    entry["list_alone"] = {a: stats(v) for a, v in t.items()}
                    lo, hi = min(t["order"]) / 1.05, max(t["order"]) * 1.05
                    entry["parity"] = bool(lo <= entry["list_alone"]["list_order"]["median"] <= hi)
                    build(3)
                    torch.cuda.synchronize()
                    entry["listed_order_cull"] = int(listed.item())
                calls = {"shuffled": lambda: node.shade_rays(shuffled, cam, out=out), "order_indexed": lambda: pair(order),
                         "cull_indexed": lambda: pair(lambda: build(2)), "order_cull_indexed": lambda: pair(lambda: build(3)),
                         "eighth_plain": lambda: node.shade_rays(shuffled[:n // 8], cam, width=n, out=out[:n // 8]),
                         "eighth_list": lambda: pair(lambda: build(3, eighth)), "tail": lambda: indexed(ends)}
                for arm in LIST_ARMS:
                    timed(calls[arm], args.warmup)
                # the pictures, outside the timing
                equal = {}
                calls["shuffled"]()
                plain = out.clone()
                for arm in ("order_indexed", "cull_indexed", "order_cull_indexed"):
                    out2.fill_(float("nan"))
                    calls[arm]()
                    equal[arm] = bool(torch.equal(bits(out2), bits(plain)))
                out2.fill_(float("nan"))
                calls["eighth_list"]()
                equal["eighth_list"] = bool(torch.equal(bits(out2[:n // 8]), bits(plain[:n // 8])) and torch.isnan(out2[n // 8:]).all())
                t_warm = time.perf_counter()
                while time.perf_counter() - t_warm < 0.025:   # sustained clocks
                    calls["shuffled"]()
                    torch.cuda.synchronize()
                arms = {a: [] for a in LIST_ARMS}
                for _ in range(args.rounds):
                    for arm in LIST_ARMS:
                        arms[arm].append(timed(calls[arm], args.reps))
            finally:
                node.close()
            med = {a: sorted(v)[len(v) // 2] for a, v in arms.items()}
            row = {"family": label, "bits_equal": equal, "ms": {a: stats(v) for a, v in arms.items()},
                   **{f"{a}_over_shuffled": med[a] / med["shuffled"] for a in ("order_indexed", "cull_indexed", "order_cull_indexed")},
                   "eighth_list_over_plain": med["eighth_list"] / med["eighth_plain"]}
            entry["rows"].append(row)
            print(f"{pose} {label:15s} " + "  ".join(f"{a} {med[a]:.4f}" for a in LIST_ARMS) + f"  bits equal: {equal}", file=sys.stderr, flush=True)
        print(f"{pose} list alone: " + "  ".join(f"{a} {v['median']:.4f} ({v['min']:.4f} - {v['max']:.4f})" for a, v in entry["list_alone"].items()) +
              f"  parity: {entry['parity']}  listed under ORDER | CULL: {entry['listed_order_cull']} of {n}", file=sys.stderr, flush=True)
        poses.append(entry)
    return poses


DETAIL_FAMILIES = ("clouds_high", "clouds_high_rm", "v1_clouds")
DETAIL_ARMS = ("render", "rays", "shuffled", "list_indexed", "order_indexed", "render_off", "rays_off", "render_q", "quads", "render_q_off", "quads_off",
               "render2")


def detail_rows(args, tex, out, perm):
    """The DETAIL table's rows (the module's docstring)."""
    import ctypes as C

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame
    from godot_atmosphere_shader_amd.ray_quads import quads_to_image

    n = H * W
    stats = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}   # noqa: E731
    bits = lambda t: t.view(torch.int32)   # noqa: E731
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(out)
    poses = []
    for pose in ("P_space", "P_limb"):
        cam = S.Camera.from_pose(W, H, pose)
        depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
        entry = {"pose": pose, "rows": []}
        for label in [f for f in args.families.split(",") if f in DETAIL_FAMILIES]:
            config, kw = FAMILIES[label]
            node = make_node(config, tex, cubemap_lod=False, tile_feedback=0, cloud_detail=True, **kw)   # level 0
            qnode = make_node(config, tex, tile_feedback=0, cloud_detail=True, **kw)                     # the declared sampler, a chain bound
            try:
                rays = node.camera_rays(cam, depth)
                shuffled = rays[perm].contiguous()
                quads = qnode.camera_ray_quads(cam, depth)
                qout = torch.empty((quads.shape[0], 4), dtype=torch.float32, device="cuda")
                need = C.c_size_t()
                N.check(node._ctx, node._lib.atmo_ray_list_scratch_bytes(n, C.byref(need)))
                scratch = torch.empty(((need.value + 3) // 4,), dtype=torch.int32, device="cuda")
                index = torch.empty((n,), dtype=torch.int32, device="cuda")
                listed = torch.zeros((1,), dtype=torch.int32, device="cuda")
                full = torch.tensor([n], dtype=torch.int32, device="cuda")
                nf = _to_native_frame(node.make_frame(cam, 0.0))
                stream = torch.cuda.current_stream().cuda_stream

                def order():
                    N.check(node._ctx, node._lib.atmo_ray_order(node._ctx, shuffled.data_ptr(), n, index.data_ptr(), scratch.data_ptr(), need.value, stream))

                def build():
                    N.check(node._ctx, node._lib.atmo_ray_list(node._ctx, C.byref(nf), shuffled.data_ptr(), full.data_ptr(), n, 3, out2.data_ptr(),
                                                               index.data_ptr(), listed.data_ptr(), scratch.data_ptr(), need.value, stream))

                def pair(first):
                    first()
                    node.shade_rays(shuffled, cam, out=out2, index=index)

                calls = {"render": lambda: node.render(cam, depth, out=frame), "rays": lambda: node.shade_rays(rays, cam, width=W, out=out),
                         "shuffled": lambda: node.shade_rays(shuffled, cam, out=out), "list_indexed": lambda: pair(build),
                         "order_indexed": lambda: pair(order), "render_q": lambda: qnode.render(cam, depth, out=frame),
                         "quads": lambda: qnode.shade_ray_quads(quads, cam, width=W, out=qout)}
                for arm, on in (("render_off", "render"), ("rays_off", "rays"), ("render_q_off", "render_q"), ("quads_off", "quads")):
                    calls[arm] = calls[on]
                calls["render2"] = calls["render"]

                def switch(arm):   # outside the timing: a host call
                    node.cloud_detail = qnode.cloud_detail = not arm.endswith("_off")

                names = {}
                for arm in DETAIL_ARMS:
                    switch(arm)
                    timed(calls[arm], args.warmup)
                    names[arm] = (qnode if arm in ("render_q", "quads", "render_q_off", "quads_off") else node).kernel_name
                # the pictures, outside the timing
                switch("render")
                equal = {}
                calls["render"]()
                calls["rays"]()
                equal["rays"] = bool(torch.equal(bits(frame.reshape(-1, 4)), bits(out)))
                calls["render_q"]()
                calls["quads"]()
                equal["quads"] = bool(torch.equal(bits(frame), bits(quads_to_image(qout, W, H))))
                calls["shuffled"]()
                plain = out.clone()
                for arm in ("list_indexed", "order_indexed"):
                    out2.fill_(float("nan"))
                    calls[arm]()
                    equal[arm] = bool(torch.equal(bits(out2), bits(plain)))
                t_warm = time.perf_counter()
                while time.perf_counter() - t_warm < 0.025:   # sustained clocks
                    calls["render"]()
                    torch.cuda.synchronize()
                arms = {a: [] for a in DETAIL_ARMS}
                for _ in range(args.rounds):
                    for arm in DETAIL_ARMS:
                        switch(arm)
                        arms[arm].append(timed(calls[arm], args.reps))
            finally:
                node.close()
                qnode.close()
            med = {a: sorted(v)[len(v) // 2] for a, v in arms.items()}
            row = {"family": label, "kernels": names, "bits_equal": equal, "ms": {a: stats(v) for a, v in arms.items()},
                   "rays_over_render": med["rays"] / med["render"], "quads_over_render_q": med["quads"] / med["render_q"],
                   "shuffled_over_rays": med["shuffled"] / med["rays"], "list_indexed_over_shuffled": med["list_indexed"] / med["shuffled"],
                   "order_indexed_over_shuffled": med["order_indexed"] / med["shuffled"],
                   "on_over_off": {a: med[a] / med[a + "_off"] for a in ("render", "rays", "render_q", "quads")},
                   "render2_over_render": med["render2"] / med["render"]}
            entry["rows"].append(row)
            print(f"{pose} {label:15s} " + "  ".join(f"{a} {med[a]:.4f}" for a in DETAIL_ARMS) + f"  rays / render {row['rays_over_render']:.3f}  quads / render_q "
                  f"{row['quads_over_render_q']:.3f}  on / off {({a: round(v, 3) for a, v in row['on_over_off'].items()})}  bits equal: {equal}  "
                  f"{names['rays']} / {names['quads']} / {names['order_indexed']}", file=sys.stderr, flush=True)
        poses.append(entry)
    return poses


LENS_W, LENS_H, LENS_FACE = 2048, 1024, 1448
LENS_FAMILIES = ("clouds_high", "clouds_high_rm", "lut")
LENS_ORDERS = ("rows", "tiles", "quads")
WRITE_TBPS = 6.2   # plain stores, MI355X


def lens_rows(args, tex):
    """The LENS table (the module's docstring)."""
    import math

    from godot_atmosphere_shader_amd.lens import Lens

    def medians(calls, warm, graphs=False):
        """ms per call of every arm, the rounds interleaved.  graphs: a call replays a captured graph of args.reps launches -- device time, no host between"""
        for call in calls.values():
            timed(call, 2 if graphs else args.warmup)
        t_warm = time.perf_counter()
        while time.perf_counter() - t_warm < 0.025:   # sustained clocks
            warm()
            torch.cuda.synchronize()
        arms = {a: [] for a in calls}
        for _ in range(args.rounds):
            for arm, call in calls.items():
                arms[arm].append(timed(call, 1) / args.reps if graphs else timed(call, args.reps))
        return {a: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for a, v in arms.items()}

    lenses = {"equirect": Lens.equirect(LENS_W, LENS_H), "fisheye": Lens.fisheye(LENS_W, LENS_H, fov=math.radians(180.0)),
              "octahedral": Lens.octahedral(LENS_W, LENS_H), "cube_face": Lens.cube_face(LENS_FACE, 5)}
    result = {"generator": [], "panorama": []}
    node = make_node(FAMILIES["lut"][0], tex, tile_feedback=0)
    try:
        import ctypes as C

        from godot_atmosphere_shader_amd import _native as N

        # the generator alone is some tens of microseconds: each arm is a captured graph of args.reps calls into buffers of its own
        calls, keep = {}, []
        side = torch.cuda.Stream()
        for name, lens in lenses.items():
            for order in LENS_ORDERS:
                n_rays, n_index = lens.counts(order == "quads")
                rays = torch.empty((n_rays, 8), dtype=torch.float32, device="cuda")
                index = torch.empty((n_index,), dtype=torch.int32, device="cuda") if order == "tiles" else None
                nl, graph = lens.native(), torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(graph, stream=side):   # one stream, no parallel branches
                        for _ in range(args.reps):
                            N.check(node._ctx, node._lib.atmo_lens_rays(node._ctx, C.byref(nl), N.LENS_QUADS if order == "quads" else 0, None, 0,
                                                                        C.c_void_p(rays.data_ptr()), C.c_void_p(index.data_ptr()) if index is not None else None,
                                                                        C.c_void_p(side.cuda_stream)))
                torch.cuda.synchronize()
                keep.append((rays, index, graph))
                calls[f"{name}/{order}"] = graph.replay
        ms = medians(calls, calls["equirect/rows"], graphs=True)
        for name, lens in lenses.items():
            n_rows, n_index = lens.counts(False)
            n_quads = lens.counts(True)[0]
            floor = {"rows": 32 * n_rows, "tiles": 32 * n_rows + 4 * n_index, "quads": 32 * n_quads}
            row = {"lens": name, "size": [lens.width, lens.height], "ms": {o: ms[f"{name}/{o}"] for o in LENS_ORDERS},
                   "floor_ms": {o: floor[o] / (WRITE_TBPS * 1e9) for o in LENS_ORDERS}}
            result["generator"].append(row)
            print(f"{name:11s} " + "  ".join(f"{o} {row['ms'][o]['median']:.4f} ms (floor {row['floor_ms'][o]:.4f})" for o in LENS_ORDERS), file=sys.stderr, flush=True)
    finally:
        node.close()
    lens = lenses["equirect"]
    for pose in ("P_space", "P_clouds"):
        cam = S.Camera.from_pose(LENS_W, LENS_H, pose)   # of the camera the rays take the view matrix: the eye and its orientation
        for label in LENS_FAMILIES:
            config, kw = FAMILIES[label]
            node = make_node(config, tex, tile_feedback=0, **kw)   # the default sampler: declared, a chain bound
            try:
                rays, index = node.lens_rays(lens, tile_index=True)
                out = torch.empty((rays.shape[0], 4), dtype=torch.float32, device="cuda")
                out2 = torch.zeros_like(out)
                calls = {"plain": lambda: node.shade_rays(rays, cam, width=LENS_W, out=out),
                         "tiles": lambda: node.shade_rays(rays, cam, width=LENS_W, out=out2, index=index)}
                if label != "lut":
                    quads = node.lens_rays(lens, quads=True)
                    qout = torch.empty((quads.shape[0], 4), dtype=torch.float32, device="cuda")
                    calls["quads"] = lambda: node.shade_ray_quads(quads, cam, width=LENS_W, out=qout)
                names = {}
                for arm, call in calls.items():
                    call()
                    names[arm] = node.kernel_name
                torch.cuda.synchronize()
                same = bool(torch.equal(out.view(torch.int32), out2.view(torch.int32)))
                hit = float((out != 0).any(dim=1).float().mean())
                ms = medians(calls, calls["plain"])
            finally:
                node.close()
            row = {"pose": pose, "family": label, "kernels": names, "bits_equal": same, "shaded": hit, "ms": {a: ms.get(a) for a in ("plain", "tiles", "quads")},
                   "tiles_over_plain": ms["tiles"]["median"] / ms["plain"]["median"],
                   "quads_over_plain": ms["quads"]["median"] / ms["plain"]["median"] if "quads" in ms else None}
            result["panorama"].append(row)
            print(f"{pose} {label:15s} " + "  ".join(f"{a} {v['median']:.4f} ({v['min']:.4f} - {v['max']:.4f})" for a, v in ms.items()) +
                  f"  tiles / plain {row['tiles_over_plain']:.3f}  shaded {hit:.3f}  bits equal: {same}", file=sys.stderr, flush=True)
    return result


def timed(call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--families", default=",".join(FAMILIES))
    ap.add_argument("--table", choices=("rays", "quads", "both", "order", "list", "detail", "lens"), default="both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rays_probe.py measures on a device; none is visible")
    tex = demo_textures()
    if args.table == "lens":
        result = {"reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "lens": lens_rows(args, tex)}
        text = json.dumps(result)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
        print(text)
        return
    cam = S.Camera.from_pose(W, H, "P_space")
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.empty((H * W, 4), dtype=torch.float32, device="cuda")
    perm = torch.randperm(H * W, generator=torch.Generator().manual_seed(1)).cuda()
    result = {"viewport": [W, H], "pose": "P_space", "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "rows": []}
    if args.table == "order":
        result["order_rows"] = order_rows(args, tex, cam, depth, frame, out, perm)
    if args.table == "list":
        result["list_poses"] = list_rows(args, tex, out, perm)
    if args.table == "detail":
        result["detail_poses"] = detail_rows(args, tex, out, perm)
    for label in args.families.split(",") if args.table in ("rays", "both") else ():
        config, kw = FAMILIES[label]
        node = make_node(config, tex, cubemap_lod=False, tile_feedback=0, **kw)   # atmo_set_sampler_lod 0, atmo_set_tile_feedback 0
        try:
            rays = node.camera_rays(cam, depth)
            shuffled = rays[perm].contiguous()
            calls = {"render": lambda: node.render(cam, depth, out=frame), "rays": lambda: node.shade_rays(rays, cam, width=W, out=out),
                     "shuffled": lambda: node.shade_rays(shuffled, cam, out=out)}
            calls["render2"] = calls["render"]
            names = {}
            for arm in ("render", "rays", "shuffled"):
                timed(calls[arm], args.warmup)
                names[arm] = node.kernel_name
            # the picture is the same in all three arms: checked once, outside the timing
            node.render(cam, depth, out=frame)
            node.shade_rays(rays, cam, width=W, out=out)
            same = bool(torch.equal(frame.reshape(-1, 4).view(torch.int32), out.view(torch.int32)))
            t_warm = time.perf_counter()
            while time.perf_counter() - t_warm < 0.025:   # sustained clocks
                calls["render"]()
                torch.cuda.synchronize()
            arms = {a: [] for a in ARMS}
            for _ in range(args.rounds):
                for arm in ARMS:
                    arms[arm].append(timed(calls[arm], args.reps))
        finally:
            node.close()
        med = {a: sorted(v)[len(v) // 2] for a, v in arms.items()}
        row = {"family": label, "kernels": names, "bits_equal_render": same,
               "ms": {a: {"median": med[a], "min": min(v), "max": max(v)} for a, v in arms.items()},
               "rays_over_render": med["rays"] / med["render"], "shuffled_over_rays": med["shuffled"] / med["rays"],
               "render2_over_render": med["render2"] / med["render"]}
        result["rows"].append(row)
        print(f"{label:15s} render {med['render']:.4f} ms  rays {med['rays']:.4f} ms ({row['rays_over_render']:.3f} x)  shuffled {med['shuffled']:.4f} ms "
              f"({row['shuffled_over_rays']:.3f} x rays)  render again {med['render2']:.4f} ms ({row['render2_over_render']:.3f} x)  bits equal: {same}  "
              f"{names['render']} / {names['rays']}", file=sys.stderr, flush=True)
    if args.table in ("quads", "both"):
        from godot_atmosphere_shader_amd.ray_quads import quads_to_image

        result["quad_rows"] = []
        for label in [f for f in args.families.split(",") if f in QUAD_FAMILIES]:
            config, kw = FAMILIES[label]
            node = make_node(config, tex, tile_feedback=0, **kw)   # the default sampler: declared, a chain bound; atmo_set_tile_feedback 0
            try:
                rays = node.camera_rays(cam, depth)
                quads = node.camera_ray_quads(cam, depth)
                qout = torch.empty((quads.shape[0], 4), dtype=torch.float32, device="cuda")
                calls = {"render": lambda: node.render(cam, depth, out=frame), "quads": lambda: node.shade_ray_quads(quads, cam, width=W, out=qout),
                         "rays": lambda: node.shade_rays(rays, cam, width=W, out=out)}
                calls["render2"] = calls["render"]
                names = {}
                for arm in ("render", "quads", "rays"):
                    timed(calls[arm], args.warmup)
                    names[arm] = node.kernel_name
                node.render(cam, depth, out=frame)
                node.shade_ray_quads(quads, cam, width=W, out=qout)
                same = bool(torch.equal(frame.view(torch.int32), quads_to_image(qout, W, H).view(torch.int32)))
                t_warm = time.perf_counter()
                while time.perf_counter() - t_warm < 0.025:   # sustained clocks
                    calls["render"]()
                    torch.cuda.synchronize()
                arms = {a: [] for a in QUAD_ARMS}
                for _ in range(args.rounds):
                    for arm in QUAD_ARMS:
                        arms[arm].append(timed(calls[arm], args.reps))
            finally:
                node.close()
            med = {a: sorted(v)[len(v) // 2] for a, v in arms.items()}
            row = {"family": label, "kernels": names, "bits_equal_render": same,
                   "ms": {a: {"median": med[a], "min": min(v), "max": max(v)} for a, v in arms.items()},
                   "quads_over_render": med["quads"] / med["render"], "rays_over_render": med["rays"] / med["render"],
                   "render2_over_render": med["render2"] / med["render"]}
            result["quad_rows"].append(row)
            print(f"{label:15s} render {med['render']:.4f} ms  quads {med['quads']:.4f} ms ({row['quads_over_render']:.3f} x)  level-0 rays {med['rays']:.4f} ms "
                  f"({row['rays_over_render']:.3f} x)  render again {med['render2']:.4f} ms ({row['render2_over_render']:.3f} x)  bits equal: {same}  "
                  f"{names['render']} / {names['quads']}", file=sys.stderr, flush=True)
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
