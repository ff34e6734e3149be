#!/usr/bin/env python3
"""Times one variant of the headline direct-light kernel <4, 8, 1> with its view loop on each of the eight 4-byte positions of a 32-byte block of the
instruction stream, against the parent commit's library, so that no A/B of a change in front of the loop is confounded by where the loop lands
(profiles/round6/ab_loop_phase.txt: one position in eight is fast, the other seven cost +8.5 ... +11 %).

    python tools/phase_sweep.py build <tag> [-DFLAG=...]    no GPU: libatmo_hip_<tag>_p0.so ... _p7.so (-DATMO_LOOP_PAD=0..7 on top of the flags, at most four
                                                            builds at a time), each loop's position read back with tools/loop_phase.py, and a job script
    python tools/phase_sweep.py job <out.sh> <tag>...       no GPU: ONE job for several tags built before (all their libraries interleaved in every round)
    python tools/phase_sweep.py table <dir>                 the table of a finished job: per library the loop position, the rounds, the median, against the parent

The job times every library and the parent's (libatmo_hip_parent.so: tools/ab_build_commit.sh parent <commit>) with bench.py, interleaved inside each of
ROUNDS rounds (default 3; results under $OUT, default phase_sweep_out/<tags>; the job lands in $JOB_DIR, default the working directory).  Every bench.py run is a step under its own `timeout -k 10`, the steps are chained with &&: the job ends at the first fault,
abort or time-out and starts nothing after it.  WORKLOAD="--workload ... --width ..." times another case than the default one."""
import concurrent.futures
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "godot_atmosphere_shader_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_phase  # noqa: E402

PADS = range(8)
HEADLINE = "atmo_render_kernelILi4ELi8ELi1E"


def lib_of(name):
    return os.path.join(PKG, f"libatmo_hip_{name}.so")


def phase_of(name):
    rows = loop_phase.view_loops(lib_of(name), HEADLINE)
    assert len(rows) == 1, (name, rows)
    return rows[0][2], rows[0][3]   # header mod 32, loop bytes


def build(tag, flags):
    def one(pad):
        subprocess.run([os.path.join(ROOT, "tools", "ab_build.sh"), f"{tag}_p{pad}", f"-DATMO_LOOP_PAD={pad}", *flags], check=True, capture_output=True)
        return pad

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:   # four hipcc at a time
        list(pool.map(one, PADS))
    for pad in PADS:
        phase, size = phase_of(f"{tag}_p{pad}")
        print(f"{tag}_p{pad}: ATMO_LOOP_PAD={pad}  view loop {size} bytes, header {phase:2d} bytes into its 32-byte block")
    phases = sorted(phase_of(f"{tag}_p{pad}")[0] for pad in PADS)
    assert phases == list(range(0, 32, 4)), f"{tag}: the eight pads do not cover the eight positions: {phases}"


def write_job(path, tags):
    names = ["parent"] + [f"{t}_p{pad}" for t in tags for pad in PADS]
    for n in names:
        assert os.path.exists(lib_of(n)), f"{lib_of(n)}: build it first"
    out = "phase_sweep_out/" + "_".join(tags)
    lines = ["#!/bin/bash", "# written by tools/phase_sweep.py: interleaved rounds, one bench.py run per step, the chain ends at the first failing step",
             "set -u", "[ -f bench.py ] || { echo 'run it from the repository root'; exit 2; }", f"OUT=${{OUT:-{out}}}", "mkdir -p $OUT", 'WORKLOAD=${WORKLOAD:-}', "true \\"]
    for r in range(1, int(os.environ.get("ROUNDS", "3")) + 1):
        for n in names:
            lines.append(f"&& timeout -k 10 120 env ATMO_HIP_LIB=$PWD/godot_atmosphere_shader_amd/libatmo_hip_{n}.so ATMO_BENCH_DETAIL= "
                         f"python bench.py $WORKLOAD --no-cpu-baseline --also '' > $OUT/{n}.r{r}.json 2> $OUT/{n}.r{r}.err \\")
    lines += ["&& echo SWEEP_COMPLETE", "rc=$?", "python tools/phase_sweep.py table $OUT | tee $OUT/table.txt", "exit $rc"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    os.chmod(path, 0o755)
    print(f"wrote {path}: {len(names)} libraries x {os.environ.get('ROUNDS', '3')} rounds")


def table(d):
    runs = {}
    for fn in sorted(os.listdir(d)):
        m = re.match(r"(.+)\.r(\d+)\.json$", fn)
        if not m:
            continue
        try:
            with open(os.path.join(d, fn)) as f:
                j = json.loads(f.readline())
            runs.setdefault(m.group(1), []).append((j["roofline"]["kernel_avg_ms"], j["value"]))
        except (ValueError, KeyError):
            print(f"{fn}: no result line (the step failed)")
    if "parent" not in runs:
        return
    pm = statistics.median(t for t, _ in runs["parent"])
    pt = [t for t, _ in runs["parent"]]
    print(f"parent spread (max - min) {max(pt) - min(pt):.5f} ms = {100 * (max(pt) - min(pt)) / pm:.2f} % of its median")
    for n in sorted(runs, key=lambda n: (n != "parent", n)):
        ts = [t for t, _ in runs[n]]
        try:
            ph = "%2d" % phase_of(n)[0]
        except Exception:
            ph = " ?"
        med = statistics.median(ts)
        print(f"{n:24s} phase {ph}  kernel_avg_ms median {med:.5f} ({100 * (med / pm - 1):+6.2f} % vs parent)  rounds {' '.join('%.5f' % t for t in ts)}"
              f"  value median {statistics.median(v for _, v in runs[n]):.4g}")


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "build" and len(sys.argv) >= 3:
        build(sys.argv[2], sys.argv[3:])
        write_job(os.path.join(os.environ.get("JOB_DIR", "."), f"phase_sweep_{sys.argv[2]}.sh"), [sys.argv[2]])
    elif cmd == "job" and len(sys.argv) >= 4:
        write_job(sys.argv[2], sys.argv[3:])
    elif cmd == "table" and len(sys.argv) == 3:
        table(sys.argv[2])
    else:
        sys.exit(__doc__)
