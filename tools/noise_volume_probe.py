"""Cost of generating the cloud shape volume on the device (include/atmo_noise_volume.h) on the MI355X.

  python tools/noise_volume_probe.py --out profiles/noise_volume/probe.json

Per size (64^3, 128^3, 256^3; 4 octaves, gain 0.5, 8 lattice cells per side at octave 0) and per (normalize, seamless): device time of one generation,
from ONE event pair around K back-to-back atmo_generate_noise_volume calls on one stream (bind = 0, no read-back: the calls only enqueue), after a
warm-up of the same calls.  The added cost of bind -- atmo_set_texture's re-layout kernel, and the float copy of the footprints up to 64^3 -- is measured
separately: the same K calls with bind = 1 on a clouds_high context, minus the bind = 0 arm of the same round.  Rounds alternate the arms; reported
are the median, minimum and maximum over the rounds, in microseconds per call.  Also the wall time of scene.make_shape_texture(64) on this machine's
host: the float64 numpy volume every cloud test and bench.py upload, which the generator stands in for.  Prints one JSON object."""
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
from godot_atmosphere_shader_amd import scene as S  # noqa: E402

SIZES = {64: 400, 128: 100, 256: 25}    # n: K calls inside one event pair
OCTAVES, GAIN, SEED, CELLS = 4, 0.5, 7, 8


def timed_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    lib = N.load()
    ctx = C.c_void_p()
    N.check(None, lib.atmo_create(0, N.VARIANT_CLOUDS_HIGH, 8, 64, N.LIGHT_LUT, 0, C.byref(ctx)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(build_id=lib.atmo_build_id().decode(), device=torch.cuda.get_device_name(0), octaves=OCTAVES, gain=GAIN, cells=CELLS,
               rounds=args.rounds, unit="us per call", results={})

    def call(desc, bind):
        def fn():
            N.check(ctx, lib.atmo_generate_noise_volume(ctx, C.byref(desc), bind, None, stream))
        return fn

    for n, reps in SIZES.items():
        arms = {}
        for normalize in (1, 0):
            for seamless in (1, 0):
                desc = N.AtmoNoiseVolume(n, SEED, CELLS / n, OCTAVES, GAIN, (C.c_float * 3)(0.0, 0.0, 0.0), seamless, 0, normalize)
                key = f"{'normalize' if normalize else 'raw'}_{'seamless' if seamless else 'plain'}"
                arms[key] = call(desc, 0)
                if normalize and seamless:
                    arms[key + "_bind"] = call(desc, 1)
        for fn in arms.values():      # warm-up: code objects, the buffers of this size, the clocks
            for _ in range(max(reps // 4, 8)):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                samples[k].append(timed_us(fn, reps))
        r = {k: dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in samples.items()}
        added = [b - a for a, b in zip(samples["normalize_seamless"], samples["normalize_seamless_bind"])]
        r["bind_added"] = dict(median=round(float(np.median(added)), 2), min=round(min(added), 2), max=round(max(added), 2))
        r["calls_per_event_pair"] = reps
        res["results"][str(n)] = r
        print(n, json.dumps(r), flush=True)
    lib.atmo_destroy(ctx)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        S.make_shape_texture(64)
        walls.append(time.perf_counter() - t0)
    res["host_make_shape_texture_64_wall_s"] = dict(median=round(float(np.median(walls)), 4), min=round(min(walls), 4), max=round(max(walls), 4))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
