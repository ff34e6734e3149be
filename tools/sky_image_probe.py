"""Cost of the sky-image calls (include/atmo_sky_image.h) on the MI355X.

    python tools/sky_image_probe.py --out profiles/sky_image/sky_image_probe.json

Three groups, each timed INTERLEAVED -- every round times each arm once, device events around `reps` runs of the arm -- medians over the rounds:
  resolve   atmo_sky_image_resolve through the C entry point on random rows, row-major and ATMO_LENS_QUADS, into RGBA16F and RGBA8_SRGB, for an equirect
            2048 x 1024 lens and one 512 x 512 cube face; beside two device-to-device copies: one WITH THE RESOLVE'S TRAFFIC (a copy of (16 + pixel
            size) / 2 bytes a pixel reads and writes together what the resolve reads plus writes) and one OF ALL ITS BYTES (16 + pixel size a pixel,
            twice the traffic: the form tools/sky_sh_probe.py measures the projection against)
  mips      the full chain of 6 x 512 x 512 and of 2048 x 1024 (RGBA16F and RGBA8_SRGB): one atmo_sky_image_mips call (fused: five levels a launch);
            the same chain as one call per level pair (n_levels = 2: the level-at-a-time form); a copy of level 0's bytes
  image     PlanetAtmosphere.render_sky_image (RGBA16F, premultiplied, mips) beside the shading alone (`_shade_lens` per lens), per node
The C calls are single ctypes calls, so their figures hold the host's launch rate as a floor (a few microseconds per call).  Prints one JSON object and
the markdown tables; --table prints the tables of a saved one.  No oracle is imported."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INSIDE = (20.0, 99.0, 5.0)       # radius 100, height 8: inside the atmosphere, under the clouds
NODES = ("no_clouds_8", "clouds_high")
IMAGES = ("equirect 2048x1024", "cube 6x512x512")
FORMATS = ("rgba16f", "rgba8_srgb")


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(torch, arms, reps, rounds):
    import numpy as np

    for fn, _ in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (fn, scale) in arms.items():
            samples[k].append(timed(torch, fn, max(int(reps * scale), 2)))
    return {k: dict(median_us=round(1e3 * float(np.median(v)), 2), min_us=round(1e3 * min(v), 2), max_us=round(1e3 * max(v), 2)) for k, v in samples.items()}


def lenses_of(image):
    from godot_atmosphere_shader_amd.lens import Lens

    return [Lens.equirect(2048, 1024, origin=INSIDE)] if image.startswith("equirect") else [Lens.cube_face(512, f, origin=INSIDE) for f in range(6)]


def torch_dtype(torch, fmt):
    return torch.float16 if fmt == "rgba16f" else torch.uint8


def probe_resolve(node, reps, rounds):
    import torch

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd import sky_image as SI
    from godot_atmosphere_shader_amd import targets as T

    lib = SI.bind(node._lib)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for image in IMAGES:
        lens = lenses_of(image)[0]      # one lens: the panorama, or one face
        nl, pixels = lens.native(), lens.width * lens.height
        rows = {q: torch.rand((lens.counts(q)[0], 4), dtype=torch.float32, device="cuda") for q in (False, True)}
        arms, keep = {}, []
        for fmt in FORMATS:
            px = T.PIXEL_BYTES[T.format_id(fmt)]
            dst = torch.zeros((lens.height, lens.width, 4), dtype=torch_dtype(torch, fmt), device="cuda")
            tgt = N.AtmoTarget(dst.data_ptr(), T.format_id(fmt), 0)
            a, b = torch.zeros((pixels * (16 + px) // 2,), dtype=torch.uint8, device="cuda"), torch.empty((pixels * (16 + px) // 2,), dtype=torch.uint8, device="cuda")
            a2, b2 = torch.zeros((pixels * (16 + px),), dtype=torch.uint8, device="cuda"), torch.empty((pixels * (16 + px),), dtype=torch.uint8, device="cuda")
            keep += [dst, tgt, a, b, a2, b2]
            for q in (False, True):
                def call(q=q, tgt=tgt):
                    rc = lib.atmo_sky_image_resolve(node._ctx, C.byref(nl), SI.QUADS if q else 0, C.c_void_p(rows[q].data_ptr()), C.byref(tgt), stream)
                    if rc != N.ATMO_OK:
                        raise RuntimeError(lib.atmo_last_error_string(node._ctx).decode())
                arms[f"{fmt} {'quads' if q else 'row-major'}"] = (call, 1.0)
            arms[f"{fmt} copy"] = (lambda a=a, b=b: b.copy_(a), 1.0)
            arms[f"{fmt} copy of all bytes"] = (lambda a=a2, b=b2: b.copy_(a), 1.0)
        res = interleaved(torch, arms, reps, rounds)
        for fmt in FORMATS:
            for order in ("row-major", "quads"):
                res[f"{fmt} {order}"]["over_copy"] = round(res[f"{fmt} {order}"]["median_us"] / res[f"{fmt} copy"]["median_us"], 3)
                res[f"{fmt} {order}"]["over_copy_of_all_bytes"] = round(res[f"{fmt} {order}"]["median_us"] / res[f"{fmt} copy of all bytes"]["median_us"], 3)
        res["pixels"] = pixels
        out[image if image.startswith("equirect") else "cube face 512x512"] = res
    return out


def probe_mips(node, reps, rounds):
    import torch

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd import sky_image as SI
    from godot_atmosphere_shader_amd import targets as T

    lib = SI.bind(node._lib)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for name, (layers, h, w) in (("6x512x512", (6, 512, 512)), ("2048x1024", (1, 1024, 2048))):
        n = SI.level_count(w, h)
        for fmt in FORMATS:
            f = T.format_id(fmt)
            levels = [torch.zeros((layers,) + SI.level_size(w, h, l)[::-1] + (4,), dtype=torch_dtype(torch, fmt), device="cuda") for l in range(n)]
            if fmt == "rgba16f":
                levels[0].copy_(torch.rand(levels[0].shape, device="cuda"))
            else:
                levels[0].copy_(torch.randint(0, 256, levels[0].shape, device="cuda", dtype=torch.uint8))
            arr = (SI.AtmoSkyLevel * n)(*[SI.AtmoSkyLevel(t.data_ptr(), 0, 0, 0) for t in levels])
            pairs = [(SI.AtmoSkyLevel * 2)(arr[l], arr[l + 1]) for l in range(n - 1)]
            copy_dst = torch.empty_like(levels[0])

            def check(rc):
                if rc != N.ATMO_OK:
                    raise RuntimeError(lib.atmo_last_error_string(node._ctx).decode())

            def fused():
                check(lib.atmo_sky_image_mips(node._ctx, arr, n, f, w, h, layers, stream))

            def by_level():
                for l, pair in enumerate(pairs):
                    wl, hl = SI.level_size(w, h, l)
                    check(lib.atmo_sky_image_mips(node._ctx, pair, 2, f, wl, hl, layers, stream))

            fused()
            torch.cuda.synchronize()
            want = [t.clone() for t in levels]
            for t in levels[1:]:
                t.zero_()
            by_level()
            torch.cuda.synchronize()
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(want, levels))
            res = interleaved(torch, {"fused": (fused, 1.0), "level at a time": (by_level, 1.0), "copy of level 0": (lambda: copy_dst.copy_(levels[0]), 1.0)},
                              reps, rounds)
            res.update(levels=n, launches_fused=-(-(n - 1) // SI.LEVELS_PER_LAUNCH), launches_level_at_a_time=n - 1, same_bytes=bool(same),
                       level0_bytes=levels[0].numel() * levels[0].element_size(),
                       fused_over_copy=round(res["fused"]["median_us"] / res["copy of level 0"]["median_us"], 3),
                       fused_over_level_at_a_time=round(res["fused"]["median_us"] / res["level at a time"]["median_us"], 3))
            out[f"{name} {fmt}"] = res
    return out


def probe_image(config, reps, rounds):
    import torch

    from godot_atmosphere_shader_amd.demo import demo_textures, make_node

    node = make_node(config, demo_textures())
    out = {}
    quads = node._shades_ray_quads()
    for image in IMAGES:
        lenses = lenses_of(image)

        def shade():
            for lens in lenses:
                node._shade_lens(lens, None, None, 0.0, None, quads)

        res = interleaved(torch, {"shade": (shade, 0.1), "render_sky_image": (lambda: node.render_sky_image(lenses), 0.1)}, reps, rounds)
        res.update(order="quads" if quads else "row-major, tile index", kernel=node.kernel_name,
                   image_over_shade=round(res["render_sky_image"]["median_us"] / res["shade"]["median_us"], 4),
                   difference_us=round(res["render_sky_image"]["median_us"] - res["shade"]["median_us"], 1))
        out[image] = res
    node.close()
    return out


def tables(doc):
    lines = ["| image | format | order | resolve us | copy with its traffic us | resolve / that | copy of all its bytes us | resolve / that |", "|---|---|---|---|---|---|---|---|"]
    for image, r in doc["resolve"].items():
        for fmt in FORMATS:
            for order in ("row-major", "quads"):
                a = r[f"{fmt} {order}"]
                lines.append(f"| {image} | {fmt} | {order} | {a['median_us']:.1f} | {r[fmt + ' copy']['median_us']:.1f} | {a['over_copy']:.2f} | "
                             f"{r[fmt + ' copy of all bytes']['median_us']:.1f} | {a['over_copy_of_all_bytes']:.2f} |")
    lines += ["", "| image | levels | fused us (launches) | level at a time us (launches) | copy of level 0 us | fused / copy | fused / level at a time | same bytes |",
              "|---|---|---|---|---|---|---|---|"]
    for key, r in doc["mips"].items():
        lines.append(f"| {key} | {r['levels']} | {r['fused']['median_us']:.1f} ({r['launches_fused']}) | {r['level at a time']['median_us']:.1f} "
                     f"({r['launches_level_at_a_time']}) | {r['copy of level 0']['median_us']:.1f} | {r['fused_over_copy']:.2f} | "
                     f"{r['fused_over_level_at_a_time']:.2f} | {r['same_bytes']} |")
    lines += ["", "| node | image | order | shading us | render_sky_image us | image / shading | difference us |", "|---|---|---|---|---|---|---|"]
    for config, per in doc["image"].items():
        for image, r in per.items():
            lines.append(f"| {config} | {image} | {r['order']} | {r['shade']['median_us']:.1f} | {r['render_sky_image']['median_us']:.1f} | "
                         f"{r['image_over_shade']:.3f} | {r['difference_us']:.1f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--table", default=None, help="print the markdown tables of a saved result and exit")
    args = ap.parse_args()
    if args.table:
        with open(args.table) as f:
            print(tables(json.loads(f.read())))
        return
    import torch

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd.demo import demo_textures, make_node

    res = dict(build_id=N.load().atmo_build_id().decode(), device=torch.cuda.get_device_name(0), origin=INSIDE, reps=args.reps, rounds=args.rounds)
    node = make_node("no_clouds_8", demo_textures())
    res["resolve"] = probe_resolve(node, args.reps, args.rounds)
    print("resolve", json.dumps(res["resolve"]), flush=True)
    res["mips"] = probe_mips(node, args.reps, args.rounds)
    print("mips", json.dumps(res["mips"]), flush=True)
    node.close()
    res["image"] = {}
    for config in NODES:
        res["image"][config] = probe_image(config, args.reps, args.rounds)
        print("image", config, json.dumps(res["image"][config]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(tables(res))


if __name__ == "__main__":
    main()
