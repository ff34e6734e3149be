#!/usr/bin/env python3
"""Benchmark of the atmosphere raymarch hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Both forms work for N > 1: typed WITHOUT a launcher (no WORLD_SIZE in the environment), `python bench.py --gpus N` starts the second
command itself as a CHILD process -- before this process has imported torch or touched the GPU (self_launch below; never an exec) --
passes its output through and exits with its code.

A "step" is one pass of the hot path over one synthetic frame: BASELINE.json configs[1],
`planet_atmosphere_no_clouds` at 1920x1080 with 32 view steps x 8 light steps (direct light mode), demo
scene, pose P_space, analytic ground-sphere depth buffer, all inputs resident in HBM before the timed
region.  With N > 1 every rank shades its own viewport (weak scaling, BASELINE configs[4] shape: one
viewport per GPU on an orbit of camera poses).  The path has no exchange step, so frames stay resident in
each GPU's HBM (like the inputs); `value` includes ONE RCCL gather of every rank's last frame to rank 0 inside the
timed region (--gather final, the default: north_star's "final RCCL gather"); --gather every gathers EVERY frame
(two in flight, overlapped with the next render; root ingress over xGMI then sets the step time; the default of
--shard bands, where a frame only exists once it is assembled), --gather none skips the collective; with --full the other
modes' rates are measured in further loops and reported beside it (SURVEY.md 8e asks for with and without), and at
N > 1 the headline run is followed by BASELINE configs[4] (one 3840x2160 clouds_high_rm viewport per GPU).

A plain run does what the headline needs and no more: set up, warm up, time the K steps, write --dump-outputs if given, print the
line.  --full adds everything else this file measures, each in runs of its own after the headline: the sustained pass and isolated
launches, the tile-feedback-off rate, the --also extras, the CPU baseline and the hit fraction (N = 1), the other gather modes and
configs[4] (N > 1).

Output: rank 0 prints ONE compact JSON line (<= 6 KB: compact_record) as the LAST line of stdout -- the record the
driver parses -- and writes everything measured (every extra's roofline blocks, notes, motion cells) to
bench_detail.json (ATMO_BENCH_DETAIL overrides the path; profiles/round<N>/bench_default.json is a committed copy).

Other workloads (--workload): lut32 (reference-exact LUT light, 32 view steps), shipped8 (the shipped
no_clouds shader), clouds_high, clouds_high_rm; --width/--height select the framebuffer (3840x2160 for 4K).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BYTES_PER_RAY = 20          # 16 B RGBA32F store + 4 B depth load
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s
TIMING_EVERY = 4            # N > 1 only: HIP events bracket every 4th launch (the render stream also waits for gathers there)
FRAMES_IN_FLIGHT = 2        # --motion loops: the host stays at most this many frames ahead of the GPU (a swap chain's depth)
SUSTAINED_MS = 50.0         # N = 1: a second, longer timed pass of at least this much GPU time (visible to an outside sampler)
N_SIMD = 1024               # 256 CUs x 4 SIMDs
SPEC_CLOCK_GHZ = 2.4
# VALU issue costs, shader cycles per wave64 instruction on one SIMD.
#   "spec": cdna_hip_programming.md / MI355X_MICROARCH.md -- v_fma_f32 2 cycles (SIMD-32), transcendentals quarter rate.
#   "measured": tools/valu_issue.hip (s_memtime cycles, 8 waves per SIMD), profiles/round2/valu_issue*_mi355x.jsonl:
#      fast class 2.2 (v_fma/mul/add_f32 on VGPR/constant operands, mov, and/or/xor, lshr, add_u32), slow class 4.1 (any
#      SGPR operand, max/min/med3, cvt, floor/fract, cmp, cndmask, lshl, 3-operand integer ops, cube, DPP, v_pk_*_f32),
#      transcendental 8.1, and the ~3 fast ops issued after a transcendental do not pair: +6 cycles per isolated
#      transcendental, +3.4 per transcendental when they are issued in clusters of 4-8 as the shipped kernels do (pattern
#      tests "exp x1, fma x7" 3.69 vs "exp x4, fma x28" 3.36 cycles per instruction).  Slow ops run on one 16-lane pipe
#      while another wave's fast ops use the second: a mix costs max(4.1 S, 2.2 (S + F)).
ISSUE_SPEC = {"valu": 2.0, "trans": 8.0}
ISSUE_MEASURED = {"fast": 2.2, "slow": 4.1, "trans": 8.1, "poison_cycles_per_trans": 3.4}
PROFILE_DIR = "profiles/round6"  # no fallback to earlier rounds: "clouds_high" meant the LOD-0 sampler there
COMPACT_LIMIT = 6144         # bytes of the final stdout line (the driver keeps the last 8 KB of stdout)
DUMP_LIMIT_BYTES = 64 * 10**6  # --dump-outputs: a larger frame is written as a seeded sample of its pixels


def pmc_summary(workload, w, h):
    """rocprofv3 PMC results for the same bench command line (tools/profile.sh -> tools/summarize_pmc.py; collected in their
    own runs, never beside tracing), committed under profiles/round<N>/pmc_<workload>_<W>x<H>.json.  None when this
    workload/size has not been profiled."""
    path = f"{PROFILE_DIR}/pmc_{workload}_{w}x{h}.json"
    if not os.path.exists(os.path.join(ROOT, path)):
        return None
    with open(os.path.join(ROOT, path)) as f:
        d = json.load(f)
    c = {k: v["mean_per_launch"] for k, v in d.get("pmc_per_launch", {}).items()}
    out = {"source": path, "counters": c, "profiled_kernel_ns": d.get("kernel_stats", {}).get("avg_ns"), "build_id": d.get("build_id")}
    if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
        out["hbm_bytes"] = (c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0
    # these numbers are read from a committed file, not measured in this run -- they are the timed kernels' only if the library that was
    # profiled is the library loaded now (same sources, same flags: build.source_id compiled in as atmo_build_id)
    out["stale"] = out["build_id"] is None or out["build_id"] != loaded_build_id()
    return out


_BUILD_ID = None


def loaded_build_id():
    global _BUILD_ID
    if _BUILD_ID is None:
        try:
            from godot_atmosphere_shader_amd import _native
            _BUILD_ID = _native.load().atmo_build_id().decode()
        except Exception:  # an A/B library from before round 6 has no stamp: never equal to a profile's
            _BUILD_ID = "unknown"
    return _BUILD_ID


def valu_roofline(pmc, kernel_avg_ms):
    """The resource that actually binds: VALU instruction issue.  Dynamic instruction counts per launch from the PMC
    passes (SQ_INSTS_VALU and its class counters, calibrated on single-opcode kernels: tools/calibrate_counters.sh),
    priced twice: at the guide's rates ("spec") and with the measured issue model.  Returns None without counters."""
    if pmc is None or pmc.get("stale") or "SQ_INSTS_VALU" not in pmc["counters"] or not kernel_avg_ms:
        return None   # (no counters, or counters of another build: instruction counts of other kernels say nothing about these)
    c = pmc["counters"]
    n, t = c["SQ_INSTS_VALU"], c.get("SQ_INSTS_VALU_TRANS_F32", 0.0)
    # fast class upper bound: every f32 FMA/ADD/MUL (the counters cannot see SGPR operands) + the half of INT32 that is
    # add/sub; everything else that is not transcendental is slow class (cvt, cmp, cndmask, max/min, floor, cube, shifts ...)
    have_classes = "SQ_INSTS_VALU_FMA_F32" in c
    fast = (c["SQ_INSTS_VALU_FMA_F32"] + c["SQ_INSTS_VALU_ADD_F32"] + c["SQ_INSTS_VALU_MUL_F32"] + 0.5 * c.get("SQ_INSTS_VALU_INT32", 0.0)) if have_classes else (n - t)
    fast = min(fast, n - t)
    slow = n - t - fast
    m = ISSUE_MEASURED
    cyc_spec = ISSUE_SPEC["valu"] * (n - t) + ISSUE_SPEC["trans"] * t
    cyc_meas = (m["trans"] + m["poison_cycles_per_trans"]) * t + max(m["slow"] * slow, m["fast"] * (slow + fast))
    # Both floors are priced at the 2.4 GHz maximum -- the smallest floor, hence the most conservative fraction.  (Until late in round 6 the measured floor used
    # the clock of the PROFILED run, GRBM_GUI_ACTIVE / 8 / the counter pass's kernel time: on most boxes that estimate sits above 2.4 GHz and was capped, on a box
    # whose counter passes ran at 2.2 GHz it priced the floor at 2.2 and compared it with a kernel time measured at full clocks -- fractions of 1.03 and 1.17.
    # The estimate is still reported, as sustained_clock_ghz_of_the_counter_pass.)
    clock = SPEC_CLOCK_GHZ
    pass_clock = None
    if c.get("GRBM_GUI_ACTIVE") and pmc.get("profiled_kernel_ns"):
        pass_clock = c["GRBM_GUI_ACTIVE"] / 8.0 / pmc["profiled_kernel_ns"]
    floor_spec_ms = cyc_spec / (N_SIMD * SPEC_CLOCK_GHZ * 1e9) * 1e3
    floor_meas_ms = cyc_meas / (N_SIMD * clock * 1e9) * 1e3
    cyc_strict = m["trans"] * t + max(m["slow"] * slow, m["fast"] * (slow + fast))  # no pairing penalty after transcendentals
    floor_strict_ms = cyc_strict / (N_SIMD * clock * 1e9) * 1e3
    return {
        "bound": "valu-issue",
        "valu_wave_insts_per_launch": n,
        "class_wave_insts_per_launch": {"fast_upper_bound": fast, "slow": slow, "transcendental": t} if have_classes else None,
        "achieved_winst_per_s": n / (kernel_avg_ms * 1e-3),
        "cycles_per_winst_per_simd_achieved": kernel_avg_ms * 1e-3 * N_SIMD * clock * 1e9 / n,
        "issue_floor_spec_ms": floor_spec_ms,
        "issue_floor_measured_ms": floor_meas_ms,
        "frac_vs_spec": floor_spec_ms / kernel_avg_ms,
        "frac_vs_measured": floor_meas_ms / kernel_avg_ms,
        "issue_floor_measured_no_pairing_penalty_ms": floor_strict_ms,
        "frac_vs_measured_no_pairing_penalty": floor_strict_ms / kernel_avg_ms,
        "sustained_clock_ghz": clock,
        "sustained_clock_ghz_of_the_counter_pass": pass_clock,
        "issue_costs": {"spec": ISSUE_SPEC, "measured": ISSUE_MEASURED,
                        "source": "tools/valu_issue.hip -> profiles/round2/valu_issue_mi355x.jsonl, valu_issue_set2_mi355x.jsonl; "
                                  "class counters calibrated in profiles/round2/counter_calibration.txt"},
        "note": "frac_vs_spec prices every non-transcendental op at 2 cycles (unreachable: half of the ISA issues in 4); "
                "frac_vs_measured uses the per-class costs this chip sustains, including +3.4 cycles per transcendental for "
                "the fast-class ops that do not pair right after one (measured on clusters of 4-8); kernels that issue them in "
                "longer clusters pay that less often, so this figure can reach 1.0-1.05 (direct light at 3840x2160) -- "
                "frac_vs_measured_no_pairing_penalty drops the term and is a strict floor; the rest is the drain at the end of "
                "a draw (tools/wave_timeline.py) and lane divergence",
    }


def hbm_roofline(kernel_avg_ms, launches, launch_rays, pmc, isolated_ms=None):
    achieved = (BYTES_PER_RAY * launch_rays / (kernel_avg_ms * 1e-3) / 1e9) if kernel_avg_ms else None
    return {
        "bound": "hbm",
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": None if achieved is None else achieved / HBM_PEAK_GBS,
        "traffic": None if pmc is None else pmc.get("hbm_bytes"),
        "traffic_source": None if pmc is None else pmc["source"] + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, bytes per launch)",
        # true: the committed counters were collected on a library built from other sources than the one timed here (or carry no stamp)
        "traffic_stale": None if pmc is None else bool(pmc.get("stale")),
        "traffic_build_id": None if pmc is None else pmc.get("build_id"),
        "build_id": loaded_build_id(),
        "kernel_avg_ms": kernel_avg_ms or None,
        "kernel_launches_timed": launches,
        "kernel_timing": "ONE pair of HIP events on the launch stream around the whole run of K un-bracketed launches of the timed "
                         "region, elapsed / K (launches are back to back, so this is the kernel's duration in steady state "
                         "including the ~1 us hand-over between consecutive launches; it cannot exceed ms_per_step)",
        "kernel_isolated_ms": isolated_ms,
        "kernel_isolated_note": None if isolated_ms is None else
                                "mean of 8 launches each bracketed by its own event pair after the timed region (untimed): a "
                                "bracketed launch starts on a drained GPU and runs ~2-4 % longer than one in a back-to-back run",
        "algorithmic_bytes_per_launch": BYTES_PER_RAY * launch_rays,
        "note": "path is VALU-issue-bound, not HBM-bound (20 B/ray); see valu_roofline and DESIGN.md",
    }


def print_final_line(rec):
    """The compact record as the LAST line of stdout: whatever native libraries have buffered on C stdio (RCCL prints its version banner
    there when a communicator is created, and the C buffer is flushed at exit, i.e. AFTER everything Python printed) is flushed first."""
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    sys.stdout.flush()
    print(json.dumps(rec), flush=True)


def write_detail(result):
    """Everything measured, as one JSON document: bench_detail.json in the working directory (ATMO_BENCH_DETAIL overrides; '' = skip).
    Returns the path written, or None (a read-only working directory must not fail the bench)."""
    path = os.environ.get("ATMO_BENCH_DETAIL", "bench_detail.json")
    if not path:
        return None
    try:
        with open(path, "w") as f:
            json.dump(result, f)
        rel = os.path.relpath(path)
        return path if rel.startswith("..") else rel
    except OSError:
        return None


def dump_outputs(directory, rgba):
    """--dump-outputs: the (h, w, 4) float32 frame the last timed step drew, as DIR/rgba.npy -- what a caller of the render path receives, so
    that two builds can be compared output for output (the inputs are synthetic and seeded: the same arguments give the same inputs).
    A frame above DUMP_LIMIT_BYTES is written as its pixels at a fixed seeded sample of positions (the same for every run of that size)."""
    import numpy as np

    a = rgba.cpu().numpy()
    if a.nbytes > DUMP_LIMIT_BYTES:
        px = a.reshape(-1, a.shape[-1])
        n = DUMP_LIMIT_BYTES // 2 // px[0].nbytes
        a = px[np.sort(np.random.default_rng(0).choice(px.shape[0], n, replace=False))]
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "rgba.npy"), a)


def _r(x, digits=6):
    """Floats rounded to `digits` significant digits (the compact line carries numbers, not their float64 noise)."""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{digits}g}")


def _pick(d, keys):
    return {k: _r(d[k]) for k in keys if d is not None and k in d}


def compact_record(result, detail_path=None):
    """The final stdout line: the contract's keys, the two roofline blocks reduced to their numbers, the CPU baseline, and every extra
    as name -> [Mrays/s, HBM fraction] -- no prose, <= COMPACT_LIMIT bytes whatever --also holds (round 3's full line was 41.7 KB and the
    driver, which keeps the last 8 KB of stdout, could not parse it: BENCH_r03.parsed = null).  The detail goes to write_detail()."""
    rec = {k: _r(result[k]) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "timed_region_ms",
                                      "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "ranks", "backend", "shard_mode",
                                      "gather_mode", "stub") if k in result}
    cfg = result.get("config", {})
    c = _pick(cfg, ("width", "height", "kernel", "hit_fraction", "gather", "shard", "mrays_per_s_feedback_off", "mrays_per_s_no_gather",
                    "mrays_per_s_final_gather", "mrays_per_s_gather_every", "gather_ms_in_timed_region"))
    c = {k: v for k, v in c.items() if v is not None}
    c["workload"] = str(cfg.get("workload", ""))[:200]
    if isinstance(c.get("shard"), str):
        c["shard"] = c["shard"][:160]
    rec["config"] = c
    rec["roofline"] = _pick(result.get("roofline"), ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_avg_ms",
                                                     "algorithmic_bytes_per_launch", "traffic_stale", "build_id"))
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        rec["roofline"].setdefault(k, None)
    if result.get("valu_roofline"):
        rec["valu_roofline"] = _pick(result["valu_roofline"], ("frac_vs_spec", "frac_vs_measured"))
    if result.get("cpu_baseline"):
        rec["cpu_baseline"] = _pick(result["cpu_baseline"], ("value", "unit", "cores", "kind"))
        rec["cpu_baseline"]["sample"] = str(result["cpu_baseline"].get("sample", ""))[:120]
    extra = {}
    for name, e in (result.get("extra") or {}).items():
        if not isinstance(e, dict):
            continue
        if "Mrays/s" in e:
            rf = e.get("roofline") or {}
            frac = rf.get("frac")
            if frac is None:  # entries without a roofline block (two viewports): the same 20 B per ray
                frac = e["Mrays/s"] * 1e6 * BYTES_PER_RAY / 1e9 / HBM_PEAK_GBS
            extra[name] = [_r(e["Mrays/s"], 5), _r(frac, 4)]
        elif "Mtexels/s" in e:
            extra[name] = [_r(e["Mtexels/s"], 5), _r(e.get("hbm_GBps", 0.0) / HBM_PEAK_GBS, 4)]
        elif any(isinstance(v, dict) and "feedback_on" in v for v in e.values()):  # bench_motion: cells by camera motion
            for motion, row in e.items():
                if isinstance(row, dict) and "feedback_on" in row:
                    on = row["feedback_on"]
                    extra[f"{name}/{motion}"] = [_r(on["Mrays/s"], 5), _r((on.get("roofline") or {}).get("frac"), 4)]
        elif any(k.startswith("Mrays/s_") for k in e):  # configs[4]: rates by gather mode
            extra[name] = {k: _r(v, 5) for k, v in e.items() if k.startswith("Mrays/s_")}
    if extra:
        rec["extra"] = extra
        rec["extra_columns"] = ["Mrays/s (Mtexels/s for noise_cubemap)", "fraction of the 8 TB/s HBM roofline at 20 B/ray"]
    if detail_path:
        rec["detail"] = detail_path
    # whatever --also holds, the line stays under the limit: drop extras from the end until it fits
    while len(json.dumps(rec)) > COMPACT_LIMIT and rec.get("extra"):
        rec["extra"].pop(next(reversed(rec["extra"])))
        rec["extra_truncated"] = True
    return rec


WORKLOADS = {
    # name: (godot_atmosphere_shader_amd.demo.CONFIGS key, description)
    "direct32x8": ("no_clouds_32x8_direct", "planet_atmosphere_no_clouds, 32 view x 8 light steps (direct light march)"),
    "lut32": ("no_clouds_32_lut", "planet_atmosphere_no_clouds, 32 view steps, baked-LUT light (reference algorithm)"),
    "shipped8": ("no_clouds_8", "planet_atmosphere_no_clouds as shipped: 8 view steps, baked-LUT light"),
    "clouds": ("clouds", "planet_atmosphere_clouds: 8 view, 32 cloud steps"),
    "clouds_high": ("clouds_high", "planet_atmosphere_clouds_high: 8 view, 64 cloud steps, NoiseCubemap coverage"),
    "clouds_high_rm": ("clouds_high_rm", "planet_atmosphere_clouds_high_rm: 8 view, 64 cloud x 6 light steps"),
    # the fast cloud mode (atmo_set_precision 0): fused density expression, error grows with u_cloud_density_scale
    "clouds_high_fast": ("clouds_high", "planet_atmosphere_clouds_high, FAST cloud mode: 8 view, 64 cloud steps"),
    "clouds_high_rm_fast": ("clouds_high_rm", "planet_atmosphere_clouds_high_rm, FAST cloud mode: 8 view, 64 cloud x 6 light steps"),
    "v1_no_clouds": ("v1_no_clouds", "planet_atmosphere_v1_no_clouds (ATMOSPHERE_LITE): 16 view steps"),
    "v1_clouds_high": ("v1_clouds_high", "planet_atmosphere_v1_clouds_high (ATMOSPHERE_LITE): 16 view, 64 cloud steps"),
}


def CONFIGS_HAS_CLOUDS(config_name):
    from godot_atmosphere_shader_amd.demo import CONFIGS
    return bool(CONFIGS[config_name][1].get("cloud_steps"))


def node_kwargs(workload):
    return dict(precise_clouds=False) if workload.endswith("_fast") else {}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="direct32x8", choices=sorted(WORKLOADS))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pose", default="P_space")
    ap.add_argument("--sampler", default="declared", choices=["declared", "lod0"],
                    help="cloud workloads: how the coverage cubemap is sampled -- 'declared' (default: the linear-mipmap sampler the reference "
                         "declares, implicit LOD from the 2x2 pixel quad; the library's default since round 4) or 'lod0' (level 0 only, "
                         "atmo_set_sampler_lod 0: every cloud number of rounds 1-3)")
    ap.add_argument("--motion", default="", help="orbit:<deg/frame> or pan:<deg/frame>: a new camera pose every step (N = 1); "
                    "all frames and depth buffers are prepared before the timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="N>1: torch.distributed backend; nccl (= RCCL, default) on MI355X.  gloo exists for the CPU test of the launch path "
                         "(tests/test_host_logic.py) and is accepted only together with --stub-renderer")
    ap.add_argument("--stub-renderer", action="store_true",
                    help="TEST SWITCH, N>1 only: no kernel, no GPU -- every 'frame' is a torch fill on the CPU, so that self_launch, the rendezvous, "
                         "the barrier/max-over-ranks timing and the gathers can be run where there is no MI355X.  The line it prints says "
                         "\"stub\": true and data \"stub\"; its `value` is not a measurement of anything")
    ap.add_argument("--band-cost", default="measured", choices=["measured", "analytic"],
                    help="--shard bands: cut the viewport by MEASURED per-row costs (rank 0 draws the frame once through "
                         "atmo_measure_tile_costs and broadcasts the cuts; default) or by the analytic estimate cloud_row_cost")
    ap.add_argument("--gather", default=None, choices=["final", "none-then-final", "every", "none"],
                    help="N>1 (default: 'final' with --shard viewports, 'every' with --shard bands -- a banded frame only exists once it is "
                         "assembled): 'final' (= 'none-then-final', north_star's \"final RCCL gather\") = frames stay in "
                         "the HBM of the GPU that rendered them, one gather of every rank's last frame to rank 0 INSIDE the timed region; "
                         "'every' = RCCL gather of EVERY frame to rank 0, two in flight, overlapped with the next render (root ingress "
                         "over xGMI then sets the step time; round 2's default); 'none' = no collective.  Whatever the mode, the other two "
                         "rates are measured in further loops and reported as config.mrays_per_s_no_gather / _final_gather / _gather_every.")
    ap.add_argument("--shard", default="viewports", choices=["viewports", "bands", "tiles"],
                    help="N>1: 'viewports' = one full viewport per GPU (weak scaling, default); 'bands' = ONE viewport cut "
                         "into hit-balanced row bands, one per GPU, gathered in place into the frame on rank 0 (strong scaling); "
                         "'tiles' = ONE viewport's 16-row tile strips dealt to the GPUs longest-processing-time-first by measured cost, "
                         "each GPU draws its tiles in one launch (atmo_render_tiles), strips gathered into the frame on rank 0 every frame")
    ap.add_argument("--lanes", type=int, default=0, choices=[0, 1, 2],
                    help="--shard tiles: lanes per ray of every rank's draw (atmo_set_lane_split; 2 halves the longest wavefronts of a share -- "
                         "what bounds a strong-scaled cloud frame -- for 13-29 %% more work; LOD-0 sampler only)")
    ap.add_argument("--also", default="lut32,shipped8,clouds_high,clouds_high_rm,direct32x8@3840x2160,clouds_high_rm@3840x2160,"
                                      "clouds_high@lod0,clouds_high_rm@lod0,clouds_high_rm@lod0@3840x2160,"
                                      "clouds_high_rm@1280x720,clouds_high_rm@1280x720@nosplit,clouds_high_rm@P_limb,clouds_high_rm@P_limb@nosplit,"
                                      "direct32x8@moving,clouds_high_rm@moving,"
                                      "direct32x8@reforder,shipped8@cleared,lut32@cleared,noise_cubemap,direct32x8+2vp",
                    help="comma-separated extra workloads (name[@lod0][@reforder][@cleared][@nosplit][@P_pose][@WxH], name@moving, name+2vp) timed at N=1 after the headline and reported under "
                         "'extra', each with its own roofline blocks: the reference-exact LUT mode and the shipped 8-step shader "
                         "(SURVEY.md 8d), BASELINE configs[2] (clouds_high 1080p) and configs[3] (clouds_high_rm 3840x2160); '' to skip.  "
                         "name+2vp goes LAST: after two contexts have drawn concurrently on two extra streams, later single-stream draws of the "
                         "same process measure 10-20 %% slower (profiles/round4/bench_order_effect.txt)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: the sustained pass and isolated launches, the tile-feedback-off rate, the "
                         "--also extras, the CPU baseline, the hit fraction, at N > 1 the other gather modes and BASELINE configs[4], with --shard "
                         "tiles the loop without the collective and the assembled-frame check.  Off: set up, warm up, time --steps steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="N = 1: after the timed steps, write the frame the last timed step drew to DIR/rgba.npy (float32, height x width x 4; "
                         f"above {DUMP_LIMIT_BYTES // 10**6} MB a fixed seeded sample of its pixels, pixels x 4)")
    return ap.parse_args()


def usable_cores():
    """Cores this process may actually use: the affinity mask capped by the cgroup CPU quota (the GPU box exposes
    256 logical CPUs but limits the container to 16 CPUs' worth of time; more threads than that only get throttled)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            if q > 0:
                cores = max(1, min(cores, q // per))
        except (OSError, ValueError):
            pass
    return cores


def cpu_baseline(config_name, params, textures, cam, depth_np, lut, lod0=False):
    """The oracle (a port of the GDShader, not the reference itself: Godot is a GPU-only path) timed on this
    host's cores over one full frame of the same workload (same cubemap sampler as the timed kernels)."""
    from godot_atmosphere_shader_amd.demo import CONFIGS as DEMO_CONFIGS, demo_frame
    from oracle.oracle import Oracle

    cores = usable_cores()
    o = Oracle("f32_fast")
    tex = dict(textures, optical_depth=lut)
    CONFIGS = {config_name: (None, dict(DEMO_CONFIGS[config_name][1]))}
    if CONFIGS[config_name][1].get("cloud_steps") and not lod0:
        CONFIGS[config_name][1]["cube_lod"] = 1
        tex["cubemap"] = o.cubemap_mip_chain(textures["cubemap"])
    frame = demo_frame(cam)
    w, h = cam.width, cam.height
    # bounded sample: every 4th 8-row band of the frame when the full frame would take too long
    t0 = time.perf_counter()
    _, _ = o.render(params, tex, CONFIGS[config_name][1], frame, depth_np, rect=(0, h // 2 - 4, w, h // 2 + 4), nthreads=cores)
    probe = time.perf_counter() - t0
    est_full = probe * h / 8.0
    if est_full <= 30.0:
        rect = (0, 0, w, h)
        sample = f"1 full {w}x{h} frame"
    else:
        rows = max(8, int(h * 20.0 / est_full) // 8 * 8)
        y0 = (h - rows) // 2
        rect = (0, y0, w, y0 + rows)
        sample = f"rows {y0}..{y0 + rows} of one {w}x{h} frame"
    reps, dt, hits = 0, 0.0, 0
    t0 = time.perf_counter()
    while dt < 2.0 and reps < 200:  # repeat the sample until the wall time is measurable on a many-core host
        _, hits = o.render(params, tex, CONFIGS[config_name][1], frame, depth_np, rect=rect, nthreads=cores)
        reps += 1
        dt = time.perf_counter() - t0
    rays = (rect[2] - rect[0]) * (rect[3] - rect[1])
    return {"value": reps * rays / dt / 1e6, "unit": "Mrays/s", "cores": cores, "kind": "port",
            "sample": f"{reps} x {sample}, {o.precision} build of oracle/atmo_oracle.c, {dt:.2f} s wall, "
                      f"{dt * cores:.0f} core-seconds",
            "hit_fraction": hits / rays}


def bench_noise_cubemap(resolution=256):
    """the NoiseCubemap generator (noise_cubemap.gd:101-140, 'really slow' on the CPU) as a kernel,
    demo-scene settings (resolution 256, scale (100,200,100)); CPU figure = the oracle's scalar loop on one core."""
    from godot_atmosphere_shader_amd import NoiseCubemap, SeededValueNoise
    from oracle.oracle import Oracle

    nz = SeededValueNoise(seed=11, frequency=0.03, fractal_octaves=4, fractal_gain=0.5)
    res = NoiseCubemap(noise=nz, resolution=resolution, scale=(100.0, 200.0, 100.0))
    times = []
    for _ in range(20):
        res._request_update()
        res.process_deferred()
        times.append(res.last_kernel_ms)
    res.close()
    texels = 6 * resolution * resolution
    k_ms = sorted(times)[len(times) // 2]
    o = Oracle("f32")
    t0 = time.perf_counter()
    o.noise_cubemap(resolution, 11, 0.03, 4, 0.5, (100.0, 200.0, 100.0))
    cpu_s = time.perf_counter() - t0
    return {"workload": f"NoiseCubemap 6x{resolution}^2 L8, 4 octaves", "kernel_ms_median": k_ms,
            "Mtexels/s": texels / (k_ms * 1e-3) / 1e6,
            "algorithmic_bytes": texels, "hbm_GBps": texels / (k_ms * 1e-3) / 1e9,
            "cpu_oracle_1core_Mtexels/s": texels / cpu_s / 1e6}


def depth_ground_sphere_torch(torch, S, cam, device):
    """scene.depth_ground_sphere evaluated on the GPU in float64 (the --motion loops need a depth buffer per pose)."""
    import numpy as np
    w, h = cam.width, cam.height
    f64 = torch.float64
    xs = (torch.arange(w, device=device, dtype=f64) + 0.5) / w * 2.0 - 1.0
    ys = (torch.arange(h, device=device, dtype=f64) + 0.5) / h * 2.0 - 1.0
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    # plain elementwise arithmetic (no matmul: a per-pose GEMM / GEMV would put rocBLAS kernels at the top of the default command's profile)
    near_z = 1.0 if cam.reverse_z else 0.0
    ip = np.asarray(cam.inv_projection, dtype=np.float64)
    vx, vy, vz, vw = (gx * float(ip[k, 0]) + gy * float(ip[k, 1]) + (near_z * float(ip[k, 2]) + float(ip[k, 3])) for k in range(4))
    dx, dy, dz = vx / vw, vy / vw, vz / vw
    inv_len = torch.rsqrt(dx * dx + dy * dy + dz * dz)
    dx, dy, dz = dx * inv_len, dy * inv_len, dz * inv_len
    c = (cam.view @ np.array([0.0, 0.0, 0.0, 1.0]))[:3]
    bq = -(dx * float(c[0]) + dy * float(c[1]) + dz * float(c[2]))
    hh = S.DEMO_PLANET_RADIUS ** 2 - (float(c @ c) - bq * bq)
    hit = hh >= 0.0
    t = -bq - torch.sqrt(torch.where(hit, hh, torch.zeros_like(hh)))
    hit = hit & (t > cam.near)
    zv = dz * t
    p = cam.projection
    zc, wc = p[2, 2] * zv + p[2, 3], p[3, 2] * zv + p[3, 3]
    far = 0.0 if cam.reverse_z else 1.0
    return torch.where(hit, zc / torch.where(hit, wc, torch.ones_like(wc)), torch.full_like(zc, far)).to(torch.float32).contiguous()


MOTION_PAN_RANGE_DEG = 25.0


def parse_motion(text):
    """'orbit:1' / 'pan:0.5' -> (kind, degrees per frame); '' or 'static' -> None."""
    if not text or text == "static":
        return None
    kind, _, deg = text.partition(":")
    if kind not in ("orbit", "pan") or not deg:
        raise SystemExit("--motion takes orbit:<deg/frame> or pan:<deg/frame>")
    return kind, float(deg)


def motion_cameras(S, w, h, motion, n, base_pose="P_space"):
    """n camera poses, one per frame, `deg` degrees apart (planet_atmosphere.gd:285-341 writes the per-frame uniforms of a
    flying camera, demo/avatar.gd + demo/mouse_look.gd):
      orbit  the demo camera revolves around the planet's axis at its own distance, looking at the centre: the terminator
             and the cloud pattern sweep across a disc that stays where it is on the screen;
      pan    the demo camera stays where it is and yaws (mouse look): the whole disc slides across the screen, back and forth
             within +-25 degrees (1 degree = 14.4 pixels at 1920x1080, i.e. about one 16-pixel tile per degree)."""
    import math
    import numpy as np
    kind, deg = motion
    base = S.POSES[base_pose]
    eye0 = np.asarray(base["eye"], dtype=np.float64)
    cams = []
    for k in range(n):
        if kind == "orbit":
            a = math.radians(deg * k)
            r = float(np.hypot(eye0[0], eye0[2]))
            a0 = math.atan2(eye0[0], eye0[2])
            eye = (r * math.sin(a0 + a), float(eye0[1]), r * math.cos(a0 + a))
            pose = dict(eye=eye, target=(0.0, 0.0, 0.0))
        else:
            x = deg * k / MOTION_PAN_RANGE_DEG  # triangle wave of amplitude 1, slope +-1 per unit
            tri = 1.0 - abs((x + 1.0) % 4.0 - 2.0)
            a = math.radians(MOTION_PAN_RANGE_DEG * tri)
            fwd = np.asarray(base["target"], dtype=np.float64) - eye0
            dist = float(np.linalg.norm(fwd))
            fwd /= dist
            ca, sa = math.cos(a), math.sin(a)
            f2 = np.array([ca * fwd[0] + sa * fwd[2], fwd[1], -sa * fwd[0] + ca * fwd[2]])
            pose = dict(eye=tuple(eye0), target=tuple(eye0 + f2 * dist))
        cams.append(S.Camera.from_pose(w, h, pose))
    return cams


def pingpong(i, n):
    """0, 1, ..., n-1, n-2, ..., 1, 0, 1, ...: a pose sequence replayed without a jump."""
    if n <= 1:
        return 0
    m = i % (2 * n - 2)
    return m if m < n else 2 * n - 2 - m


class TimedRun:
    """What time_workload measured: wall seconds of the K-step timed region (host clock, synchronised on both sides), the
    HIP-event time of the same K launches, an isolated-launch figure, and the sustained pass."""
    def __init__(self):
        self.dt = 0.0
        self.steps = 0
        self.event_ms = 0.0
        self.isolated_ms = None
        self.sustained = None
        self.out = None
        self.last = None   # keep_last: a copy of the frame the last of the K timed steps drew

    @property
    def kernel_avg_ms(self):
        return self.event_ms / self.steps if self.steps else 0.0


def time_workload(torch, node, cam, depth, steps, warmup, out=None, sequence=None, sustained=False, isolated=True, keep_last=False):
    """Single-GPU timed loop.  `sequence`: None (the same frame every step) or a list of (native frame, depth tensor), one
    camera pose per step, replayed ping-pong (--motion); the host then stays at most FRAMES_IN_FLIGHT frames ahead of the GPU,
    like a swap chain, instead of enqueueing the whole run at once."""
    if out is None:
        out = torch.empty((cam.height, cam.width, 4), dtype=torch.float32, device=depth.device)
    stream = torch.cuda.current_stream().cuda_stream
    optr = out.data_ptr()
    if sequence is None:
        sequence = [(node.prepare_frame(cam), depth)]
    seq = [(fr, d.data_ptr()) for fr, d in sequence]
    nseq = len(seq)
    paced = nseq > 1
    ring = [torch.cuda.Event() for _ in range(FRAMES_IN_FLIGHT)] if paced else None
    counter = [0]

    def draw(n):
        for _ in range(n):
            i = counter[0]
            fr, dptr = seq[pingpong(i, nseq)]
            if paced:
                ev = ring[i % FRAMES_IN_FLIGHT]
                if i >= FRAMES_IN_FLIGHT:
                    ev.synchronize()
                node.render_prepared(fr, dptr, optr, stream)
                ev.record()
            else:
                node.render_prepared(fr, dptr, optr, stream)
            counter[0] = i + 1

    # W untimed steps; whatever W is, the context is primed outside the timed region (lazy LUT bake, feedback buffers,
    # and -- after the synchronisation -- the first heaviest-first tile order): two untimed draws at least
    draw(warmup)
    torch.cuda.synchronize()
    # A frame loop synchronises once per frame (present); the static loop does not, so a context would keep the tile order
    # of its first, cold draws for as long as the host runs ahead of the GPU.  Four more untimed draws, paced like frames,
    # let the heaviest-first order settle before the timed region (atmo_set_tile_feedback; NOTES.md).
    for _ in range(4):
        draw(1)
        torch.cuda.synchronize()
    # ... and the GPU needs ~20 ms of sustained work to reach its sustained clocks in a fresh process (a 20-step run measured
    # 8 % below a 200-step run otherwise: BENCH_r01 vs README in round 1): keep drawing, untimed, until that much has run
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.025:
        draw(8)
        torch.cuda.synchronize()

    def timed(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if os.environ.get("ATMO_BENCH_LAZY_EVENTS") != "1":
            # torch creates the hipEvent behind an Event at its first record(): inside the region that is host time in front of the first launch with the GPU
            # idle (round 6: the K = 20 region carried ~40 us beyond its kernels).  Record both once, outside, so the region's own records reuse them.
            e0.record()
            e1.record()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()  # on torch's current stream = the stream the kernels are launched on
        draw(n)
        e1.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, e0.elapsed_time(e1)

    run = TimedRun()
    run.dt, run.event_ms = timed(steps)
    run.steps = steps
    run.out = out
    if keep_last:   # before the sustained pass and the isolated launches draw into `out` again (another pose under --motion)
        run.last = out.clone()
    if sustained:
        n2 = max(steps, int(SUSTAINED_MS / max(run.dt / steps * 1e3, 1e-3)) + 1)
        dt2, ev2 = timed(n2)
        run.sustained = {"steps": n2, "timed_region_ms": dt2 * 1e3, "ms_per_step": dt2 / n2 * 1e3, "kernel_avg_ms": ev2 / n2,
                         "Mrays/s": cam.width * cam.height * n2 / dt2 / 1e6,
                         "note": f"second timed pass of >= {SUSTAINED_MS:.0f} ms right after the K-step region (same loop, same "
                                 "measurement), long enough for an outside GPU-activity sampler to see"}
    if isolated:
        node.set_timing(True, every=1)
        draw(8)
        torch.cuda.synchronize()
        n, ms = node.get_timing()
        node.set_timing(False)
        run.isolated_ms = ms / n if n else None
    return run


def timed_loop_distributed(torch, dist, render_into, h, w, device, steps, warmup, gather_mode, timing=None, bands=None):
    """The N > 1 timed region (also run on CPU/gloo by tests/test_distributed_gloo.py with a stub renderer).

    `render_into(buf)` enqueues one frame into the (h, w, 4) float32 tensor `buf`.  W untimed warm-up steps, then
    EXACTLY `steps` steps bracketed by barrier + device synchronisation on both sides (every rank reads its clock after ITS device
    has drained and before the closing barrier -- an RCCL barrier is a ~0.1 ms collective of its own, 5 % of a 20-step region, and the
    maximum over ranks already is the time the slowest rank needed); returns (max over ranks of the elapsed seconds, kernel launches,
    kernel ms) -- the last two from `timing = (start, read)` when given.
    gather_mode: "final" (only the last frame is gathered to rank 0, inside the timed region), "every", "none"."""
    from godot_atmosphere_shader_amd.sharding import FrameGather

    is_cuda = device.type == "cuda"

    def sync():
        if is_cuda:
            torch.cuda.synchronize()

    gather = None if gather_mode == "none" else FrameGather(h, w, device, dst=0, depth=2, bands=bands)
    rows = h if bands is None else bands[dist.get_rank()][1] - bands[dist.get_rank()][0]
    scratch = torch.empty((max(rows, 1), w, 4), dtype=torch.float32, device=device)[:rows]

    def step(last):
        # "final": frames stay resident in this GPU's HBM; only the last one is gathered.  "every": each frame.
        if gather is None or (gather_mode == "final" and not last):
            render_into(scratch)
        else:
            buf, slot = gather.next_send_buffer()
            render_into(buf)
            gather.submit(slot)

    if gather is not None:  # set up the communicator / p2p channels outside the timed region whatever W is
        buf, slot = gather.next_send_buffer()
        buf.zero_()
        gather.submit(slot)
        gather.finish()
    for i in range(warmup):
        step(i == warmup - 1)
    if gather is not None:
        gather.finish()
    sync()
    dist.barrier()
    sync()
    if timing is not None:
        timing[0]()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i == steps - 1)
    result = gather.finish() if gather is not None else None
    sync()
    dt = time.perf_counter() - t0  # this rank's K steps (+ its part of the gather) are complete; the MAX over ranks below is the job's time
    dist.barrier()
    sync()
    launches, kernel_ms = timing[1]() if timing is not None else (0, 0.0)
    tmax = torch.tensor([dt], dtype=torch.float64, device=device)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    timed_loop_distributed.last_gathered = result  # (world, h, w, 4) on rank 0 in gather modes, for tests
    return float(tmax.item()), launches, kernel_ms


def cut_bands_measured(torch, dist, device, world, rank, measure, repeats=3):
    """Row bands of equal MEASURED cost for `world` ranks: rank 0 calls `measure()` (per-row costs of the whole frame,
    PlanetAtmosphere.measure_row_costs; the last of `repeats` measurements counts: clocks and caches warm), cuts, and broadcasts the cuts
    -- every rank must use the same cuts, and measured costs differ from GPU to GPU."""
    from godot_atmosphere_shader_amd.sharding import balanced_row_bands

    cuts = torch.zeros(world + 1, dtype=torch.int64, device=device)
    if rank == 0:
        for _ in range(repeats):
            row_cost = measure()
        b = balanced_row_bands(row_cost, world)
        cuts.copy_(torch.tensor([b[0][0]] + [x[1] for x in b], dtype=torch.int64))
    dist.broadcast(cuts, src=0)
    c = [int(v) for v in cuts.tolist()]
    return [(c[k], c[k + 1]) for k in range(world)]


def cloud_row_cost(np, S, cam, cloudy):
    """Per-row cost estimate for band balancing: pixels whose ray hits the atmosphere shell count 1; for the cloud
    variants a pixel whose ray also crosses the cloud shell (between the ground sphere and the cloud-top sphere: the
    gate of render_clouds, clouds:263-278) counts CLOUD_WEIGHT more (64 cloud steps against 8 view steps)."""
    d = cam.pixel_view_dirs()
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    c = (cam.view @ np.array([0.0, 0.0, 0.0, 1.0]))[:3]
    bq = d @ c
    q2 = c @ c - bq * bq
    R, H = S.DEMO_PLANET_RADIUS, S.DEMO_ATMOSPHERE_HEIGHT
    hit = ((R + H) ** 2 - q2 >= 0)
    cost = hit.astype(np.float64)
    if cloudy:
        top = R + S.DEMO_SHADER_PARAMS["u_cloud_top"] * H
        cost += CLOUD_WEIGHT * (top ** 2 - q2 >= 0)
    return cost.sum(axis=1) + 0.02 * cam.width  # + a small per-row cost for the miss pixels


CLOUD_WEIGHT = 8.0


def run_workload(torch, S, name, w, h, pose, steps, warmup, textures, params, local_rank, with_frame_stats=True,
                 motion=None, node_extra=None, sampler=None, env=None):
    """One single-GPU workload: returns the result dictionary of an `extra` entry (rate, kernel time, both rooflines).
    motion: None or (kind, degrees per frame): a new camera pose every step (time_workload); node_extra: PlanetAtmosphere
    keyword arguments (tile_feedback=0 ...); sampler: None / "declared" (the library's default) or "lod0" -- the coverage cubemap's sampler."""
    import numpy as np  # noqa: F401
    from godot_atmosphere_shader_amd.demo import make_node

    config_name, desc = WORKLOADS[name]
    kw = dict(node_kwargs(name), **(node_extra or {}))
    if sampler == "lod0":
        kw["cubemap_lod"] = False
    elif os.environ.get("ATMO_BENCH_EXPLICIT_SAMPLER") == "1":
        kw["cubemap_lod"] = CONFIGS_HAS_CLOUDS(config_name)   # tools/ab_bench.sh: the same kernels, selected in the way libraries built before round 4 understand too
    saved = {k: os.environ.get(k) for k in (env or {})}   # A/B switches the library reads once, in atmo_create (ATMO_HEAVY_SPLIT=0 ...)
    os.environ.update(env or {})
    try:
        node = make_node(config_name, textures, params, device=local_rank, **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    cam = S.Camera.from_pose(w, h, pose)
    sequence = None
    if motion is not None:
        cams = motion_cameras(S, w, h, motion, max(64, min(steps, 128 if w * h > 4000000 else 256)), pose)
        sequence = [(node.prepare_frame(c), depth_ground_sphere_torch(torch, S, c, torch.device("cuda", local_rank))) for c in cams]
        depth = sequence[0][1]
    else:
        depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    run = time_workload(torch, node, cam, depth, steps, warmup, sequence=sequence)
    kernel_avg_ms = run.kernel_avg_ms
    pmc_name = name + ("@lod0" if sampler == "lod0" else "")
    ref_order = bool((node_extra or {}).get("precise_atmosphere"))
    pmc = pmc_summary(pmc_name, w, h) if (pose == "P_space" and motion is None and not ref_order) else None
    res = {"workload": f"{desc}{workload_suffix(config_name, sampler)}; {w}x{h}; demo scene, pose {pose}"
                       + ("; atmosphere march in the reference's operation order (atmo_set_precision 2: validation mode)" if ref_order else "")
                       + ("; discarded fragments store nothing (atmo_set_target_cleared 1)" if (node_extra or {}).get("target_cleared") else "")
                       + ("; heavy tiles NOT drawn on two lanes per ray (ATMO_HEAVY_SPLIT=0)" if (env or {}).get("ATMO_HEAVY_SPLIT") == "0" else "")
                       + ("" if motion is None else f", camera motion {motion[0]} {motion[1]:g} deg/frame, a new pose every step, "
                                                    f"{len(sequence)} poses replayed ping-pong, host at most {FRAMES_IN_FLIGHT} frames ahead"),
           "Mrays/s": w * h * steps / run.dt / 1e6,
           "ms_per_step": run.dt / steps * 1e3, "timed_region_ms": run.dt * 1e3, "steps": steps, "kernel_avg_ms": kernel_avg_ms or None,
           "kernel": node.kernel_name,
           "roofline": hbm_roofline(kernel_avg_ms, steps, w * h, pmc, run.isolated_ms), "valu_roofline": valu_roofline(pmc, kernel_avg_ms)}
    if with_frame_stats:
        res["hit_fraction"] = float((run.out.abs().sum(dim=-1) > 0).float().mean().item())
    res["feedback_stats"] = node.feedback_stats()
    res["split_stats"] = node.split_stats()   # draws whose heaviest tiles went to the two-lanes-per-ray kernel, tiles in the last such draw
    node.close()
    del run, depth, sequence
    return res


def workload_suffix(config_name, sampler):
    """States which sampler a cloud number is for (the reference declares a linear-mipmap samplerCube, cloud_funcs.gdshaderinc:15,45)."""
    from godot_atmosphere_shader_amd.demo import CONFIGS
    if not CONFIGS[config_name][1].get("cloud_steps"):
        return ""
    if sampler == "lod0":
        return "; coverage cubemap sampled at LOD 0 (atmo_set_sampler_lod 0)"
    return "; coverage cubemap sampled as declared (linear-mipmap, implicit LOD)"


def bench_motion(torch, S, name, w, h, steps, warmup, textures, params, local_rank,
                 motions=(None, ("orbit", 0.1), ("orbit", 1.0), ("orbit", 5.0), ("pan", 1.0))):
    """The same workload with the camera still and moving, tile-order feedback on and off (the feedback's gain was
    only ever measured on a redrawn frame).  Every loop is paced like a swap chain (time_workload), the static one too."""
    out = {}
    for motion in motions:
        key = "static" if motion is None else f"{motion[0]}:{motion[1]:g}"
        row = {}
        for fb in (1, 0):
            # the paced loops are host-driven (at most FRAMES_IN_FLIGHT frames ahead): a host hiccup of a few ms in a 10 ms region once
            # showed up as a 2.5x slower cell.  Each cell is the faster of two runs (both rates are kept in the line).
            runs = [run_workload(torch, S, name, w, h, "P_space", steps, warmup, textures, params, local_rank, with_frame_stats=False,
                                 motion=motion if motion is not None else ("orbit", 0.0), node_extra=dict(tile_feedback=fb)) for _ in range(2)]
            r = max(runs, key=lambda x: x["Mrays/s"])
            r["Mrays/s_both_runs"] = [x["Mrays/s"] for x in runs]
            rf = r["roofline"]
            row["feedback_on" if fb else "feedback_off"] = {
                "Mrays/s": r["Mrays/s"], "Mrays/s_both_runs": r["Mrays/s_both_runs"], "ms_per_step": r["ms_per_step"], "kernel_avg_ms": r["kernel_avg_ms"],
                "roofline": {k: rf[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_avg_ms", "algorithmic_bytes_per_launch")},
                "feedback_stats": r["feedback_stats"]}
        row["gain"] = row["feedback_on"]["Mrays/s"] / row["feedback_off"]["Mrays/s"] - 1.0
        out[key] = row
    out["workload"] = (f"{WORKLOADS[name][1]}; {w}x{h}; demo scene, camera still / orbiting / panning (bench.motion_cameras), "
                       f"{steps} timed steps each (the faster of two runs per cell), host at most {FRAMES_IN_FLIGHT} frames ahead")
    return out


def bench_two_viewports(torch, S, name, w, h, steps, warmup, textures, params, local_rank):
    """Two independent viewports of the same size drawn concurrently on two streams by two contexts (the single-GPU form of
    BASELINE configs[4]'s "independent viewports"): how much of the chip one 1920x1080 draw leaves idle.  Reported
    next to the one-viewport rate, never instead of it."""
    from godot_atmosphere_shader_amd.demo import make_node

    config_name, desc = WORKLOADS[name]
    cams = [S.Camera.from_pose(w, h, "P_space"), S.Camera.from_pose(w, h, S.orbit_pose(1, 8))]
    nodes, frames, depths, outs, streams = [], [], [], [], []
    for cam in cams:
        node = make_node(config_name, textures, params, device=local_rank, **node_kwargs(name))
        nodes.append(node)
        frames.append(node.prepare_frame(cam))
        depths.append(torch.from_numpy(S.depth_ground_sphere(cam)).cuda())
        outs.append(torch.empty((h, w, 4), dtype=torch.float32, device="cuda"))
        streams.append(torch.cuda.Stream())

    def loop(n):
        for _ in range(n):
            for k in range(2):
                nodes[k].render_prepared(frames[k], depths[k].data_ptr(), outs[k].data_ptr(), streams[k].cuda_stream)

    loop(warmup)
    torch.cuda.synchronize()
    for _ in range(4):  # same untimed priming as time_workload: tile order, then sustained clocks
        loop(1)
        torch.cuda.synchronize()
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.025:
        loop(4)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for node in nodes:
        node.close()
    return {"workload": f"2 x ({desc}; {w}x{h}), two contexts on two streams, poses P_space and orbit 1/8",
            "Mrays/s": 2 * w * h * steps / dt / 1e6, "ms_per_pair": dt / steps * 1e3, "steps": steps}


def self_launch(args):
    """`python bench.py --gpus N` typed as is (N > 1, no launcher: WORLD_SIZE unset): start
        python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free port> bench.py <same arguments>
    as a CHILD process, pass its stdout through line by line (rank 0's JSON record stays the last line), and exit with its code.  Called
    before torch is imported: this process never touches the GPU, and nothing is ever exec'ed (a process that has initialised HIP must not
    replace itself; the N ranks are fresh interpreters).  Returns when there is nothing to launch."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    import subprocess

    if not args.stub_renderer:
        # fail before N interpreters are started (counting devices does not initialise the GPU on this image; is_available / any HIP call would)
        import torch
        have = torch.cuda.device_count()
        if have < args.gpus:
            raise SystemExit(f"bench.py needs an MI355X per rank: --gpus {args.gpus}, but this node shows {have} GPU(s) (there is no CPU fallback)")

    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
            sock.bind(("127.0.0.1", 0))
            port = str(sock.getsockname()[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: no launcher in the environment, starting " + " ".join(cmd), file=sys.stderr, flush=True)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))  # dmabuf IPC: RCCL needs it on this pool
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, bufsize=1, env=env)
    try:
        for line in proc.stdout:
            sys.stdout.write(line)
            sys.stdout.flush()
        rc = proc.wait()
    except BaseException:
        proc.terminate()   # the exact child this process started, never a pattern
        proc.wait()
        raise
    raise SystemExit(rc)


class StubNode:
    """--stub-renderer (test switch): stands where the PlanetAtmosphere node stands in the N > 1 paths of main(); draws nothing."""
    kernel_name = "none (--stub-renderer)"

    def __init__(self, rank):
        self.rank = rank
        self.draws = 0

    def prepare_frame(self, cam, rect=None):
        from types import SimpleNamespace
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, cam.width, cam.height)
        return SimpleNamespace(x0=x0, y0=y0, x1=x1, y1=y1)

    def draw(self, buf):
        self.draws += 1
        buf.fill_(float(self.rank + 1))

    def set_timing(self, on, every=1):
        pass

    def get_timing(self):
        return 0, 0.0

    def close(self):
        pass


def main():
    args = parse_args()
    if args.stub_renderer and args.gpus < 2:
        raise SystemExit("--stub-renderer tests the N > 1 launch path: give --gpus 2 or more")
    if (args.backend == "gloo") != bool(args.stub_renderer):
        raise SystemExit("--backend gloo and --stub-renderer go together (a test of the launch path on a host without a GPU); the product path is RCCL")
    if args.dump_outputs and (args.gpus > 1 or os.environ.get("ATMO_BENCH_FORCE_DIST") == "1"):
        raise SystemExit("--dump-outputs is a single-GPU option (--gpus 1)")
    self_launch(args)
    if args.gather is None:
        args.gather = "every" if args.shard == "bands" else "final"
    if args.gather == "none-then-final":
        args.gather = "final"
    import numpy as np
    import torch

    from godot_atmosphere_shader_amd.demo import demo_params, demo_textures, make_node
    from godot_atmosphere_shader_amd import scene as S

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with --nproc-per-node {args.gpus}")
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    stub = bool(args.stub_renderer)
    if not stub:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False (there is no CPU fallback)")
        if local_rank >= torch.cuda.device_count():
            raise SystemExit(f"--gpus {args.gpus}: rank {rank} has no GPU (this node shows {torch.cuda.device_count()})")
        torch.cuda.set_device(local_rank)
    dist = None
    force_dist = os.environ.get("ATMO_BENCH_FORCE_DIST") == "1"  # exercise the RCCL path with a 1-rank group
    if world > 1 or force_dist:
        import torch.distributed as dist
        if stub:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    multi = world > 1 or force_dist
    if stub and (args.shard == "tiles" or not multi):
        raise SystemExit("--stub-renderer covers --shard viewports and --shard bands at N > 1")

    def sync():
        if not stub:
            torch.cuda.synchronize()

    w, h = args.width, args.height
    config_name, desc = WORKLOADS[args.workload]
    textures = demo_textures()
    params = demo_params()
    strong = args.shard == "bands" and multi
    if args.shard == "tiles" and multi:
        return main_tile_strips(args, torch, dist, S, textures, params, config_name, desc, world, rank, local_rank)
    pose = args.pose if (world == 1 or rank == 0 or strong) else S.orbit_pose(rank, world)
    cam = S.Camera.from_pose(w, h, pose)
    depth_np = S.depth_ground_sphere(cam)
    device = torch.device("cpu") if stub else torch.device("cuda", local_rank)
    depth = torch.from_numpy(depth_np).to(device)
    cloudy = bool(__import__("godot_atmosphere_shader_amd.demo", fromlist=["CONFIGS"]).CONFIGS[config_name][1].get("cloud_steps"))
    lod0 = args.sampler == "lod0" and cloudy
    explicit = os.environ.get("ATMO_BENCH_EXPLICIT_SAMPLER") == "1"   # tools/ab_bench.sh against libraries built before round 4
    node = StubNode(rank) if stub else make_node(
        config_name, textures, params, device=local_rank,
        **dict(node_kwargs(args.workload), **(dict(cubemap_lod=False) if lod0 else (dict(cubemap_lod=cloudy) if explicit else {}))))
    rays = w * h

    # ---- timed region ---------------------------------------------------------------------------------
    bands = None
    no_gather_rate = None
    dt_ng = None
    run = None
    motion = parse_motion(args.motion)
    if motion is not None and multi:
        raise SystemExit("--motion is a single-GPU mode")
    if not multi:
        sequence = None
        if motion is not None:
            cams = motion_cameras(S, w, h, motion, max(64, min(args.steps, 256)), args.pose)
            sequence = [(node.prepare_frame(c), depth_ground_sphere_torch(torch, S, c, device)) for c in cams]
        run = time_workload(torch, node, cam, depth, args.steps, args.warmup, sequence=sequence, sustained=args.full, isolated=args.full,
                            keep_last=bool(args.dump_outputs))
        dt_max, launches, kernel_ms = run.dt, run.steps, run.event_ms
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, run.last)
            run.last = None
        gather_mode = "none (single GPU)"
    else:
        if strong:
            # ONE frame in row bands of equal WORK.  Measured: rank 0 draws the whole frame once and reads back what every tile
            # cost (atmo_measure_tile_costs), sums per pixel row, cuts, and broadcasts the cuts (every rank must use the same);
            # analytic (--band-cost analytic): shell hits per row, cloud-shell hits weighted (cloud_row_cost).
            from godot_atmosphere_shader_amd.sharding import balanced_row_bands, band_rect
            if args.band_cost == "measured" and not stub:
                bands = cut_bands_measured(torch, dist, device, world, rank, lambda: node.measure_row_costs(cam, depth))
            else:
                bands = balanced_row_bands(cloud_row_cost(np, S, cam, "cloud" in config_name), world)
            frame = node.prepare_frame(cam, rect=band_rect(w, bands[rank]))
        else:
            frame = node.prepare_frame(cam)
        stream = 0 if stub else torch.cuda.current_stream().cuda_stream

        def render_into(buf):
            if buf.numel():
                if stub:
                    node.draw(buf)
                else:
                    node.render_prepared(frame, depth.data_ptr(), buf.data_ptr(), stream)

        # untimed, before the W warm-up steps of the timed loop: frame-paced draws so the tile order settles, then ~25 ms
        # of work so the GPU is at its sustained clocks (see time_workload)
        prime = torch.empty((max(1, frame.y1 - frame.y0), max(1, frame.x1 - frame.x0), 4), dtype=torch.float32, device=device)
        for _ in range(4):
            render_into(prime)
            sync()
        t_warm = time.perf_counter()
        while time.perf_counter() - t_warm < 0.025:
            for _ in range(8):
                render_into(prime)
            sync()
        del prime
        node_timing = (lambda: node.set_timing(True, every=TIMING_EVERY), node.get_timing)
        dt_max, launches, kernel_ms = timed_loop_distributed(
            torch, dist, render_into, h, w, device, args.steps, args.warmup, args.gather, node_timing, bands=bands)
        node.set_timing(False)
        gather_mode = {"none": "no collective",
                       "final": "one RCCL gather of each rank's last frame to rank 0, inside the timed region",
                       "every": "RCCL gather of every frame to rank 0, 2 frames in flight, inside the timed region"}[args.gather]
        # the rates WITHOUT the gather and with only the FINAL gather next to the headline mode's (same loop)
        final_gather_rate = None
        scale = 1 if strong else world
        if args.full and args.gather != "none":
            dt_ng, _, _ = timed_loop_distributed(torch, dist, render_into, h, w, device, args.steps, max(2, args.warmup // 4),
                                                 "none", None, bands=bands)
            no_gather_rate = scale * rays * args.steps / dt_ng / 1e6
        if args.full and args.gather != "final":
            dt_fg, _, _ = timed_loop_distributed(torch, dist, render_into, h, w, device, args.steps, max(2, args.warmup // 4),
                                                 "final", None, bands=bands)
            final_gather_rate = scale * rays * args.steps / dt_fg / 1e6
        every_gather_rate = None
        if args.full and args.gather != "every":
            dt_eg, _, _ = timed_loop_distributed(torch, dist, render_into, h, w, device, args.steps, max(2, args.warmup // 4),
                                                 "every", None, bands=bands)
            every_gather_rate = scale * rays * args.steps / dt_eg / 1e6

    result = None
    if rank == 0:
        value = (1 if strong else world) * rays * args.steps / dt_max / 1e6
        if no_gather_rate is None and (not multi or args.gather == "none"):
            no_gather_rate = value
        pmc = None if (strong or args.pose != "P_space" or motion is not None) else pmc_summary(args.workload + ("@lod0" if lod0 else ""), w, h)
        kernel_avg_ms = kernel_ms / launches if launches else 0.0
        launch_rays = rays if not strong else w * (bands[0][1] - bands[0][0])  # rank 0's kernel shades its band only
        hit_fraction = None
        if stub:
            pmc, hit_fraction = None, 0.0
        elif args.full:
            frame_img = node.render(cam, depth)
            torch.cuda.synchronize()
            hit_fraction = float((frame_img.abs().sum(dim=-1) > 0).float().mean().item())
            del frame_img
        result = {
            "metric": f"Mrays/s, {args.workload} at {w}x{h}" + ("; 32 view x 8 light steps" if args.workload == "direct32x8" else "")
                      + "; % HBM roofline" + (f"; gather {args.gather}" if multi else ""),
            "value": value,
            "unit": "Mrays/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt_max / args.steps * 1e3,
            "timed_region_ms": dt_max * 1e3,
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "stub" if stub else "synthetic",
            "stub": stub,
            # what ran: the process group's rank count and backend (nccl = RCCL), how frames were sharded and gathered (short forms; the prose is in config)
            "ranks": dist.get_world_size() if dist is not None else 1,
            "backend": dist.get_backend() if dist is not None else None,
            "shard_mode": args.shard if multi else None,
            "gather_mode": args.gather if multi else None,
            "config": {
                "workload": ("STUB RENDERER, no kernel ran (test of the launch path): " if stub else "")
                            + f"{desc}{workload_suffix(config_name, 'lod0' if lod0 else None)}; {w}x{h}; demo scene, pose {args.pose}"
                            + ("" if world == 1 or strong else f" on rank 0, orbit poses on ranks 1..{world - 1}; one viewport per GPU"),
                "width": w, "height": h, "rays_per_step_per_gpu": rays if not strong else None,
                "hit_fraction": hit_fraction,
                "mrays_per_s_hit_only": None if hit_fraction is None else value * hit_fraction,
                "gather": gather_mode,
                "mrays_per_s_no_gather": no_gather_rate,
                "mrays_per_s_final_gather": (value if args.gather == "final" else final_gather_rate) if multi else None,
                "mrays_per_s_gather_every": (value if args.gather == "every" else every_gather_rate) if multi else None,
                # what the collective adds to the K-step region (the same loop with and without it): one gather of a frame per rank in
                # "final" mode -- a constant, so its share of `value` shrinks with K
                "gather_ms_in_timed_region": ((dt_max - dt_ng) * 1e3 if dt_ng is not None else None),
                "shard": (f"one viewport in row bands of equal {args.band_cost} cost: " + str(bands)) if strong else "one viewport per GPU",
                "kernel": node.kernel_name,
            },
            "roofline": hbm_roofline(kernel_avg_ms, launches, launch_rays, pmc, None if run is None else run.isolated_ms),
        }
        if multi:
            result["roofline"]["kernel_timing"] = f"HIP events around every {TIMING_EVERY}th launch of the timed region, on the launch stream (rank 0)"
        if run is not None and run.sustained is not None:
            result["sustained_pass"] = run.sustained
        if motion is not None:
            result["config"]["motion"] = (f"{motion[0]} {motion[1]:g} deg/frame, a new camera pose every step ({len(sequence)} poses, ping-pong), "
                                          f"host at most {FRAMES_IN_FLIGHT} frames ahead of the GPU")
        vr = valu_roofline(pmc, kernel_avg_ms)
        if vr is not None:
            result["valu_roofline"] = vr
    node.close()

    # the conservative figure beside the headline: the same workload in row-major tile order (atmo_set_tile_feedback 0) -- what a panning
    # camera gets on the cloudless kernels (profiles/round3/ab_tile_feedback_motion.txt)
    if args.full and not multi and rank == 0 and motion is None and args.also.strip(", "):  # (not in the single-workload runs of tools/profile.sh: --also "")
        r_off = run_workload(torch, S, args.workload, w, h, args.pose, args.steps, args.warmup, textures, params, local_rank,
                             with_frame_stats=False, node_extra=dict(tile_feedback=0), sampler="lod0" if lod0 else None)
        result["config"]["mrays_per_s_feedback_off"] = r_off["Mrays/s"]

    # ---- extras ----------------------------------------------------------------------------------------
    if args.full and not multi and args.also and rank == 0:
        extra = {}
        ex_steps, ex_warm = max(10, args.steps // 4), max(3, args.warmup // 4)
        for item in [x for x in args.also.split(",") if x]:
            if item == "noise_cubemap":
                extra[item] = bench_noise_cubemap()
                continue
            name, *opts = item.split("@")
            if name.endswith("+2vp"):
                extra[item] = bench_two_viewports(torch, S, name[:-4], w, h, ex_steps, ex_warm, textures, params, local_rank)
                continue
            if "moving" in opts:
                extra[item] = bench_motion(torch, S, name, w, h, max(64, ex_steps), ex_warm, textures, params, local_rank)
                continue
            ew, eh, sampler, node_extra, epose, env = w, h, None, None, args.pose, None
            for o in opts:
                if o == "lod0":
                    sampler = "lod0"
                elif o == "nosplit":   # ATMO_HEAVY_SPLIT=0: every tile with one lane per ray (the A/B of round 5's heavy-tile split)
                    env = {"ATMO_HEAVY_SPLIT": "0"}
                elif o.startswith("P_"):
                    epose = o
                elif o == "reforder":  # atmo_set_precision 2: the v2 march in the reference's operation order (validation mode)
                    node_extra = dict(precise_atmosphere=True)
                elif o == "cleared":  # atmo_set_target_cleared 1: discarded fragments store nothing (the shader's `discard`)
                    node_extra = dict(target_cleared=True)
                else:
                    ew, eh = (int(v) for v in o.split("x"))
            extra[item] = run_workload(torch, S, name, ew, eh, epose, ex_steps, ex_warm, textures, params, local_rank, sampler=sampler,
                                       node_extra=node_extra, env=env)
        result["extra"] = extra
    if args.full and multi and not strong and args.workload == "direct32x8" and os.environ.get("ATMO_BENCH_NO_CONFIG4") != "1":
        # BASELINE.json configs[4]: independent 3840x2160 clouds_high_rm viewports, one per GPU, gathered to rank 0 over xGMI
        c4 = bench_config4(torch, dist, S, textures, params, local_rank, rank, world, max(5, args.steps // 8), 2, stub=stub)
        if rank == 0:
            result.setdefault("extra", {})["config4_clouds_high_rm_3840x2160"] = c4

    if rank == 0:
        if args.full and not multi and not args.no_cpu_baseline:
            from godot_atmosphere_shader_amd.demo import CONFIGS
            ocfg = CONFIGS[config_name][1]
            lut = None
            if not (ocfg.get("lite") or ocfg.get("light_steps")):
                n2 = make_node(config_name, textures, params, device=local_rank)
                lut = n2.read_optical_depth()
                n2.close()
            result["cpu_baseline"] = cpu_baseline(config_name, params, textures, cam, depth_np, lut, lod0)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print_final_line(compact_record(result, write_detail(result)))


def main_tile_strips(args, torch, dist, S, textures, params, config_name, desc, world, rank, local_rank):
    """--shard tiles: ONE viewport, its 16-row tile strips dealt to the ranks longest-processing-time-first by MEASURED tile costs (rank 0
    measures, everybody gets the costs by broadcast and computes the same deal); every step each rank draws its tiles in one launch, heaviest
    first (atmo_render_tiles), and the strips are gathered into the frame on rank 0 (a frame only exists once it is assembled: the gather
    of every frame is inside the timed region).  Strong scaling; `value` = the viewport's rays per second of assembled frames."""
    import numpy as np
    from godot_atmosphere_shader_amd.demo import make_node
    from godot_atmosphere_shader_amd.sharding import STRIP_TILE_ROWS, StripGather, heavy_tiles, lpt_strips

    w, h = args.width, args.height
    device = torch.device("cuda", local_rank)
    cam = S.Camera.from_pose(w, h, args.pose)
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    lod0 = args.sampler == "lod0" and CONFIGS_HAS_CLOUDS(config_name)
    node = make_node(config_name, textures, params, device=local_rank,
                     **dict(node_kwargs(args.workload), **(dict(cubemap_lod=False) if lod0 else {}), **(dict(lane_split=args.lanes) if args.lanes else {})))
    shape = torch.zeros(4, dtype=torch.int64, device=device)
    if rank == 0:
        for _ in range(3):  # the last of three measurements counts (clocks and caches warm)
            cost, tw, th = node.measure_tile_costs(cam, depth)
        shape.copy_(torch.tensor([cost.shape[0], cost.shape[1], tw, th]))
    dist.broadcast(shape, src=0)
    ty, tx, tw, th = (int(v) for v in shape.tolist())
    cost_t = torch.zeros((ty, tx), dtype=torch.int64, device=device)
    if rank == 0:
        cost_t.copy_(torch.from_numpy(cost.astype(np.int64)))
    dist.broadcast(cost_t, src=0)
    strips, tiles = lpt_strips(cost_t.cpu().numpy(), world)
    my_tiles = torch.from_numpy(tiles[rank].astype(np.int32)).to(device)
    # round 5: a share of one frame is as long as its heaviest wavefront from two GPUs on -- its heavy tiles go on two lanes per ray beside the rest
    # (atmo_render_tiles_split; the declared-sampler cloud kernels, bit-identical; elsewhere the library ignores the count)
    my_heavy = heavy_tiles(cost_t.cpu().numpy().reshape(-1)[tiles[rank]]) if not args.lanes else 0
    g = StripGather(h, w, strips, STRIP_TILE_ROWS * th, device, dst=0)
    frame = node.prepare_frame(cam)
    stream = torch.cuda.current_stream().cuda_stream
    target = g.render_target()

    def draw():
        node.render_tiles_prepared(frame, depth.data_ptr(), target.data_ptr(), my_tiles.data_ptr(), my_tiles.numel(), stream, n_heavy=my_heavy)

    def loop(n, gather):
        for _ in range(n):
            draw()
            if gather:
                g.gather()

    def timed(n, gather):
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        loop(n, gather)
        e1.record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        dist.barrier()
        tmax = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        return float(tmax.item()), e0.elapsed_time(e1)

    loop(max(2, args.warmup), True)
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.025:   # sustained clocks (see time_workload)
        loop(8, False)
        torch.cuda.synchronize()
    dt, _ = timed(args.steps, True)
    dt_ng = per_rank = identical = None
    if args.full:
        dt_ng, ev_ng = timed(args.steps, False)
        # what every rank's launch took, without the collective (HIP events around its K un-bracketed launches)
        per_rank = torch.zeros(world, dtype=torch.float64, device=device)
        per_rank[rank] = ev_ng / args.steps
        dist.all_reduce(per_rank)
        if rank == 0:
            assembled = g.gather()
            want = node.render(cam, depth)
            torch.cuda.synchronize()
            identical = bool(torch.equal(assembled, want))
        else:
            g.gather()
    result = None
    if rank == 0:
        rays = w * h
        value = rays * args.steps / dt / 1e6
        k_ms = None if per_rank is None else float(per_rank.max().item())
        slowest = 0 if per_rank is None else int(per_rank.argmax().item())
        result = {
            "metric": f"Mrays/s, {args.workload} at {w}x{h}; % HBM roofline; one viewport in tile strips over {world} GPUs, gather every",
            "value": value, "unit": "Mrays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "timed_region_ms": dt * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "ranks": dist.get_world_size(), "backend": dist.get_backend(), "shard_mode": "tiles", "gather_mode": "every",
            "config": {"workload": f"{desc}{workload_suffix(config_name, 'lod0' if lod0 else None)}; {w}x{h}; demo scene, pose {args.pose}",
                       "width": w, "height": h, "kernel": node.kernel_name, "gather": "strips of every frame gathered into the frame on rank 0, inside the timed region",
                       "shard": f"{len(strips[0]) and sum(len(s) for s in strips)} strips of {STRIP_TILE_ROWS * th} rows dealt LPT by measured cost: "
                                f"{[len(s) for s in strips]} strips per rank, {[int(t.size) for t in tiles]} tiles",
                       "mrays_per_s_no_gather": None if dt_ng is None else rays * args.steps / dt_ng / 1e6, "mrays_per_s_gather_every": value,
                       "gather_ms_in_timed_region": None if dt_ng is None else (dt - dt_ng) * 1e3,
                       "kernel_ms_per_rank": None if per_rank is None else [float(v) for v in per_rank.tolist()],
                       "assembled_frame_equals_single_gpu_frame": identical},
            "roofline": hbm_roofline(k_ms, args.steps, int(tiles[slowest].size) * tw * th, None),
        }
        if per_rank is not None:
            result["roofline"]["kernel_timing"] = "HIP events around the K un-bracketed tile-list launches of the slowest rank (loop without the collective)"
    node.close()
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print_final_line(compact_record(result, write_detail(result)))
    return result


def bench_config4(torch, dist, S, textures, params, local_rank, rank, world, steps, warmup, stub=False):
    """BASELINE.json configs[4]: `world` independent 3840x2160 planet_atmosphere_clouds_high_rm viewports (orbit poses), one
    per GPU; weak scaling, three rates: one final gather of every rank's last frame to rank 0 inside the timed region (north_star), every
    frame gathered to rank 0 (132.7 MB per rank per frame over xGMI), and no collective."""
    from godot_atmosphere_shader_amd.demo import make_node

    w, h = (3840, 2160) if not stub else (96, 54)   # the stub (CPU test of the launch path) keeps the shape of the loop, not the size
    pose = "P_space" if rank == 0 else S.orbit_pose(rank, world)
    cam = S.Camera.from_pose(w, h, pose)
    device = torch.device("cpu") if stub else torch.device("cuda", local_rank)
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).to(device)
    node = StubNode(rank) if stub else make_node("clouds_high_rm", textures, params, device=local_rank)
    frame = node.prepare_frame(cam)
    stream = 0 if stub else torch.cuda.current_stream().cuda_stream

    def render_into(buf):
        if stub:
            node.draw(buf)
        else:
            node.render_prepared(frame, depth.data_ptr(), buf.data_ptr(), stream)

    prime = torch.empty((h, w, 4), dtype=torch.float32, device=device)
    for _ in range(6):  # frame-paced, untimed: lets the heaviest-first tile order settle (see time_workload)
        render_into(prime)
        if not stub:
            torch.cuda.synchronize()
    del prime
    out = {}
    for mode in ("final", "every", "none"):
        timing = (lambda: node.set_timing(True, every=TIMING_EVERY), node.get_timing)
        dt, launches, kernel_ms = timed_loop_distributed(torch, dist, render_into, h, w, device, steps, warmup, mode, timing)
        node.set_timing(False)
        out[{"final": "Mrays/s_final_gather", "every": "Mrays/s_gather_every_frame", "none": "Mrays/s_no_gather"}[mode]] = world * w * h * steps / dt / 1e6
        out["ms_per_step_" + mode] = dt / steps * 1e3
        out["kernel_avg_ms_rank0"] = kernel_ms / launches if launches else None
    out.update(workload=("STUB RENDERER: " if stub else "") + f"planet_atmosphere_clouds_high_rm, {w}x{h}, one viewport per GPU x {world}", steps=steps, n_gpus=world,
               kernel=node.kernel_name, scaling="weak")
    node.close()
    return out


if __name__ == "__main__":
    main()
