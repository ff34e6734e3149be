"""Cost of the sky-as-light calls (include/atmo_sky_sh.h) on the MI355X, beside the shading of the same image and a copy of the bytes the projection reads.

    python tools/sky_sh_probe.py --out profiles/sky_sh/sky_sh_probe.json

Per case (a node, an image: one 2048 x 1024 equirect lens, or six 512 x 512 cube faces; every ray starts inside the atmosphere) the arms are timed
INTERLEAVED -- every round times each arm once, device events around `reps` runs of the arm -- and the medians over the rounds are reported:
  solid     atmo_lens_solid_angles, once per lens, through the C entry point
  project   atmo_sky_sh9, once per lens (ACCUMULATE behind the first), through the C entry point, on the arrays the shading left
  copy      one device-to-device copy of as many bytes as the projection reads: 16 + 16 + 4 per ray
  shade     the shading of the image as ambient_sh9 shades it (lens rays, then the ray entry point: quads under a declared sampler, else the tile index)
  ambient   PlanetAtmosphere.ambient_sh9: shade + solid + project, allocations included
`solid`, `project` and `copy` are single ctypes / torch calls per lens, so their figures hold the host's launch rate as a floor (a few microseconds per
call).  Prints one JSON object and the markdown table; --table prints the table of a saved one.  No oracle is imported."""
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


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def lenses_of(image):
    from godot_atmosphere_shader_amd.lens import Lens

    return [Lens.equirect(2048, 1024, origin=INSIDE)] if image.startswith("equirect") else [Lens.cube_face(512, f, origin=INSIDE) for f in range(6)]


def probe(config, image, reps, rounds):
    import numpy as np
    import torch

    from godot_atmosphere_shader_amd import _native as N
    from godot_atmosphere_shader_amd import sky_sh as SH
    from godot_atmosphere_shader_amd.demo import demo_textures, make_node

    node = make_node(config, demo_textures())
    lib = SH.bind(node._lib)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lenses = lenses_of(image)
    quads = node._shades_ray_quads()
    flags = N.LENS_QUADS if quads else 0
    out = torch.zeros((SH.FLOATS,), dtype=torch.float32, device="cuda")
    work, n_total = [], 0
    for lens in lenses:      # the arrays the two C calls work on: shaded once, here
        rays, shaded = node._shade_lens(lens, None, None, 0.0, None, quads)
        n = int(rays.shape[0])
        weights = torch.empty((n,), dtype=torch.float32, device="cuda")
        scratch = torch.empty((max(SH.scratch_bytes(n) // 4, 4),), dtype=torch.float32, device="cuda")
        work.append((lens.native(), rays, shaded, weights, scratch, n))
        n_total += n
    src = torch.zeros((36 * n_total,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def check(rc):
        if rc != N.ATMO_OK:
            raise RuntimeError(lib.atmo_last_error_string(node._ctx).decode())

    def solid():
        for nl, _, _, weights, _, _ in work:
            check(lib.atmo_lens_solid_angles(node._ctx, C.byref(nl), flags, C.c_void_p(weights.data_ptr()), stream))

    def project():
        for i, (_, rays, shaded, weights, scratch, n) in enumerate(work):
            check(lib.atmo_sky_sh9(node._ctx, C.c_void_p(rays.data_ptr()), C.c_void_p(shaded.data_ptr()), C.c_void_p(weights.data_ptr()), n,
                                   SH.ACCUMULATE if i else 0, C.c_void_p(scratch.data_ptr()), SH.scratch_bytes(n), C.c_void_p(out.data_ptr()), stream))

    def shade():
        for lens in lenses:
            node._shade_lens(lens, None, None, 0.0, None, quads)

    arms = {"solid": solid, "project": project, "copy": lambda: dst.copy_(src), "shade": shade, "ambient": lambda: node.ambient_sh9(lenses)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            samples[k].append(timed(torch, fn, reps if k in ("solid", "project", "copy") else max(reps // 10, 2)))
    res = {k: dict(median_ms=round(float(np.median(v)), 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5)) for k, v in samples.items()}
    sh = out.cpu().numpy()
    res.update(rays=n_total, order="quads" if quads else "row-major, tile index", bytes_read=36 * n_total, kernel=node.kernel_name,
               project_over_copy=round(res["project"]["median_ms"] / res["copy"]["median_ms"], 3),
               project_over_shade=round(res["project"]["median_ms"] / res["shade"]["median_ms"], 4),
               project_gb_per_s=round(36 * n_total / (res["project"]["median_ms"] * 1e-3) / 1e9, 1),
               copy_gb_per_s=round(2 * 36 * n_total / (res["copy"]["median_ms"] * 1e-3) / 1e9, 1),
               solid_angle=float(sh[36]), l00=[float(v) for v in sh[0:4]])
    node.close()
    return res


def table(doc):
    rows = ["| node | image | rays | solid angles us | projection us | copy of its bytes us | projection / copy | shading us | projection / shading | ambient_sh9 us |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for key, r in doc["results"].items():
        config, image = key.split("@", 1)
        us = lambda arm: f"{1e3 * r[arm]['median_ms']:.1f}"   # noqa: E731
        rows.append(f"| {config} | {image} | {r['rays']} | {us('solid')} | {us('project')} | {us('copy')} | {r['project_over_copy']:.2f} | {us('shade')} | "
                    f"{r['project_over_shade']:.4f} | {us('ambient')} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--table", default=None, help="print the markdown table of a saved result and exit")
    args = ap.parse_args()
    if args.table:
        with open(args.table) as f:
            print(table(json.loads(f.read())))
        return
    import torch

    from godot_atmosphere_shader_amd import _native as N

    res = dict(build_id=N.load().atmo_build_id().decode(), device=torch.cuda.get_device_name(0), origin=INSIDE, reps=args.reps, rounds=args.rounds, results={})
    for config in NODES:
        for image in IMAGES:
            r = probe(config, image, args.reps, args.rounds)
            res["results"][f"{config}@{image}"] = r
            print(config, image, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(table(res))


if __name__ == "__main__":
    main()
