#!/usr/bin/env python3
"""Static check of the multi-view kernels into packed colour targets (atmo_render_views_target_kernel<FLAGS | KF_VIEWS | KF_TARGET, LSTEPS>,
include/atmo_views_target.h) against their float-batch twins (atmo_render_views_kernel<FLAGS | KF_VIEWS, LSTEPS>), in the ISA hipcc emits -- no GPU
needed.  The eight TargetConsts of these kernels sit by value in the kernel-argument segment and are indexed by the wave-uniform view number; what must
hold for that to cost nothing is what tools/views_resources.py asks of the float batch (whose parsing this tool imports):

  - no stack frame (ScratchSize 0) -- a per-lane copy of a constants struct would be one;
  - inside loops, exactly as many vector memory loads as the twin has (its texture fetches): the target's fields arrive through scalar loads, and the
    composite's destination load sits behind the march, outside every loop;
  - the VGPR count on the occupancy step of the twin, or a better one.

    python tools/views_target_resources.py [--markdown] [-DFLAG ...]      exit code 0 = every kernel passes; one line (or table row) per kernel
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from views_resources import HIPCC_FLAGS, KF_VIEWS, SRC, kernels, vgpr_waves  # noqa: E402

KF_TARGET = 1024


def table(asm_text: str):
    """[(flags without KF_VIEWS | KF_TARGET, lsteps, the kernel's numbers, the float-batch twin's numbers, [what fails])], sorted."""
    ks = kernels(asm_text)
    rows = []
    for name, k in ks.items():
        m = re.match(r"_ZN4atmo31atmo_render_views_target_kernelILi(\d+)ELi(\d+)EE", name)
        if not m:
            continue
        flags, lsteps = int(m.group(1)) - KF_VIEWS - KF_TARGET, int(m.group(2))
        twin = next((v for n, v in ks.items() if n.startswith(f"_ZN4atmo24atmo_render_views_kernelILi{flags + KF_VIEWS}ELi{lsteps}EE")), None)
        bad = []
        if twin is None:
            bad.append("no float-batch twin")
        else:
            if vgpr_waves(k["vgprs"]) < vgpr_waves(twin["vgprs"]):
                bad.append(f"VGPRs {k['vgprs']} = {vgpr_waves(k['vgprs'])} waves, the twin's {twin['vgprs']} = {vgpr_waves(twin['vgprs'])}")
            if k["loop_vector"] != twin["loop_vector"]:
                bad.append(f"{k['loop_vector']} vector loads inside loops, the twin has {twin['loop_vector']}")
        if k["scratch"]:
            bad.append(f"ScratchSize {k['scratch']}")
        rows.append((flags, lsteps, k, twin, bad))
    return sorted(rows, key=lambda r: (r[0], r[1]))


def main(argv):
    markdown = "--markdown" in argv
    argv = [a for a in argv if a != "--markdown"]
    out = os.path.join(tempfile.mkdtemp(prefix="viewstres_"), "k.s")
    subprocess.run(["hipcc"] + HIPCC_FLAGS + [SRC, "-o", out] + argv, check=True, stderr=subprocess.DEVNULL)
    rows = table(open(out).read())
    if markdown:
        print("| kernel `<FLAGS, LSTEPS>` | VGPRs (waves) | twin VGPRs (waves) | SGPRs | twin SGPRs | vector loads in loops | twin | scalar loads in loops | twin | scratch |")
        print("|---|---|---|---|---|---|---|---|---|---|")
    ok = bool(rows)
    for flags, lsteps, k, twin, bad in rows:
        t = twin or dict(vgprs=0, sgprs=0, loop_vector=0, loop_scalar=0)
        if markdown:
            print(f"| `<{flags} + 3072, {lsteps}>` | {k['vgprs']} ({vgpr_waves(k['vgprs'])}) | {t['vgprs']} ({vgpr_waves(t['vgprs']) if twin else 0}) | {k['sgprs']} | {t['sgprs']} | "
                  f"{k['loop_vector']} | {t['loop_vector']} | {k['loop_scalar']} | {t['loop_scalar']} | {k['scratch']} |")
        else:
            print(f"atmo_render_views_target_kernel<{flags + KF_VIEWS + KF_TARGET}, {lsteps}>: {k['vgprs']} VGPRs ({vgpr_waves(k['vgprs'])} waves; twin {t['vgprs']}), "
                  f"{k['sgprs']} SGPRs (twin {t['sgprs']}), in loops {k['loop_vector']} vector loads (twin {t['loop_vector']}) and {k['loop_scalar']} scalar loads "
                  f"(twin {t['loop_scalar']}), ScratchSize {k['scratch']}: " + ("ok" if not bad else "; ".join(bad).upper()))
        ok = ok and not bad
    if not rows:
        print("no multi-view target kernel found")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
