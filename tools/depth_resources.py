#!/usr/bin/env python3
"""Static check of the depth-source kernels (atmo_render[_views][_proxy]_depth_target_kernel<FLAGS | KF_DEPTH, LSTEPS[, SPLIT]>, include/atmo_depth.h)
against their packed-target twins (the kernel of the same name without `depth_`, FLAGS without KF_DEPTH), in the ISA hipcc emits -- no GPU needed.  The
DepthConsts of these kernels is a kernel argument of its own (the batches: eight of them by value, indexed by the wave-uniform view number) and the depth
sample is one load in the prologue; what must hold for that to cost nothing is what tools/views_target_resources.py asks of the packed batches (whose
parsing this tool shares through tools/views_resources.py):

  - no stack frame (ScratchSize 0) -- a per-lane copy of a constants struct would be one;
  - inside loops, exactly as many vector memory loads as the twin has (its texture fetches): the depth load sits in the prologue, not in a loop, and the
    DepthConsts fields arrive through scalar loads;
  - the VGPR count on the occupancy step of the twin, or a better one;
  - no more SGPR spilling than the twin: v_readlane_b32 / v_writelane_b32 (how hipcc spills scalars) at most SPILL_SLACK more than the twin's.  The first
    form of the depth load -- the division inside a three-way branch -- cost the single-draw cloud kernels 200-300 of them and clouds_high a factor 1.85
    (profiles/depth/README.md, 3).

    python tools/depth_resources.py [--markdown] [-DFLAG ...]      exit code 0 = every kernel passes; one line (or table row) per kernel
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from views_resources import HIPCC_FLAGS, SRC, kernels, vgpr_waves  # noqa: E402

KF_DEPTH = 4096
# Lane reads a kernel may have beyond its twin's.  Chosen, not derived: the shipped build's largest difference is 21 (<5139, 0, 1>: 62 against 41; the next
# is 14), the failure this check exists for was 150-300 beyond the twin in sixteen kernels.  24 passes the former and catches the latter with a factor of
# six to spare; a build that fails here by a few reads has to be measured (tools/depth_probe.py), not waved through by raising the number.
SPILL_SLACK = 24
_NAME = re.compile(r"_ZN4atmo\d+(atmo_render(_views)?(_proxy)?_depth_target_kernel)ILi(\d+)ELi(\d+)E(?:Li(\d+)E)?E")


def table(asm_text: str):
    """[(kernel name, flags, lsteps, split or None, the kernel's numbers, the packed-target twin's numbers, [what fails])], sorted."""
    ks = kernels(asm_text)
    for m in re.finditer(r"^(_ZN4atmo\w+):[^\n]*\n(.*?)\.Lfunc_end", asm_text, re.S | re.M):   # (the bodies once more: views_resources.kernels keeps the counts only)
        ks[m.group(1)]["spill_reads"] = len(re.findall(r"^\s*v_readlane_b32", m.group(2), re.M))
    rows = []
    for name, k in ks.items():
        m = _NAME.match(name)
        if not m:
            continue
        kernel, flags, lsteps, split = m.group(1), int(m.group(4)), int(m.group(5)), m.group(6)
        twin_kernel = kernel.replace("_depth_target", "_target")
        twin_args = f"ILi{flags - KF_DEPTH}ELi{lsteps}E" + (f"Li{split}E" if split else "") + "E"
        twin = next((v for n, v in ks.items() if n.startswith(f"_ZN4atmo{len(twin_kernel)}{twin_kernel}{twin_args}")), None)
        bad = []
        if not flags & KF_DEPTH:
            bad.append("no KF_DEPTH in its flags")
        if twin is None:
            bad.append("no packed-target twin")
        else:
            if vgpr_waves(k["vgprs"]) < vgpr_waves(twin["vgprs"]):
                bad.append(f"VGPRs {k['vgprs']} = {vgpr_waves(k['vgprs'])} waves, the twin's {twin['vgprs']} = {vgpr_waves(twin['vgprs'])}")
            if k["loop_vector"] != twin["loop_vector"]:
                bad.append(f"{k['loop_vector']} vector loads inside loops, the twin has {twin['loop_vector']}")
            if k["spill_reads"] > twin["spill_reads"] + SPILL_SLACK:
                bad.append(f"{k['spill_reads']} SGPR spill reads, the twin has {twin['spill_reads']}")
        if k["scratch"]:
            bad.append(f"ScratchSize {k['scratch']}")
        rows.append((kernel, flags, lsteps, int(split) if split else None, k, twin, bad))
    return sorted(rows, key=lambda r: (r[0], r[1], r[2], r[3] or 0))


def main(argv):
    markdown = "--markdown" in argv
    argv = [a for a in argv if a != "--markdown"]
    out = os.path.join(tempfile.mkdtemp(prefix="depthres_"), "k.s")
    subprocess.run(["hipcc"] + HIPCC_FLAGS + [SRC, "-o", out] + argv, check=True, stderr=subprocess.DEVNULL)
    rows = table(open(out).read())
    if markdown:
        print("| kernel | `<FLAGS, LSTEPS[, SPLIT]>` | VGPRs (waves) | twin VGPRs (waves) | SGPRs | twin SGPRs | vector loads in loops | twin | SGPR spill reads | twin | scratch |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
    ok = bool(rows)
    for kernel, flags, lsteps, split, k, twin, bad in rows:
        t = twin or dict(vgprs=0, sgprs=0, loop_vector=0, loop_scalar=0, spill_reads=0)
        args = f"{flags}, {lsteps}" + (f", {split}" if split else "")
        if markdown:
            print(f"| `{kernel}` | `<{args}>` | {k['vgprs']} ({vgpr_waves(k['vgprs'])}) | {t['vgprs']} ({vgpr_waves(t['vgprs']) if twin else 0}) | {k['sgprs']} | "
                  f"{t['sgprs']} | {k['loop_vector']} | {t['loop_vector']} | {k['spill_reads']} | {t['spill_reads']} | {k['scratch']} |")
        else:
            print(f"{kernel}<{args}>: {k['vgprs']} VGPRs ({vgpr_waves(k['vgprs'])} waves; twin {t['vgprs']}), {k['sgprs']} SGPRs (twin {t['sgprs']}), "
                  f"in loops {k['loop_vector']} vector loads (twin {t['loop_vector']}), {k['spill_reads']} SGPR spill reads (twin {t['spill_reads']}), ScratchSize {k['scratch']}: " + ("ok" if not bad else "; ".join(bad).upper()))
        ok = ok and not bad
    if not rows:
        print("no depth-source kernel found")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
