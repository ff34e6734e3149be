#!/usr/bin/env python3
"""Static check of the multi-view kernels (atmo_render_views_kernel<FLAGS | KF_VIEWS, LSTEPS>, include/atmo_views.h) against their atmo_render twins
(atmo_render_kernel<FLAGS, LSTEPS, 1>), in the ISA hipcc emits -- no GPU needed.  The per-view constants of these kernels live in a device table instead
of the kernel-argument segment; what must hold for that to cost nothing:

  - no stack frame (ScratchSize 0) -- a per-lane copy of RenderConsts would be one;
  - inside loops, exactly as many vector memory loads as the twin has (its texture fetches): a constant arriving through a vector load would be one more.
    Constants arrive through scalar loads (s_load), which the table prints as well: where the allocator re-loads them inside a loop, it says so;
  - the VGPR count on the occupancy step of the twin, or a better one (waves per SIMD by VGPRs: 512 / the count rounded up to 8, at most 8).

    python tools/views_resources.py [--markdown] [-DFLAG ...]      exit code 0 = every kernel passes; one line (or table row) per kernel
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "godot_atmosphere_shader_amd", "csrc", "atmo_kernels.hip")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-S", "--cuda-device-only"]
KF_VIEWS = 2048
_BB = re.compile(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)")


def vgpr_waves(vgprs: int) -> int:
    return min(8, 512 // (((vgprs + 7) // 8) * 8))


def loop_loads(body: str):
    """(vector memory loads, scalar loads) inside basic blocks the compiler annotates as part of a loop."""
    lines = body.split("\n")
    in_loop, vector, scalar = False, 0, 0
    for i, raw in enumerate(lines):
        ln = raw.strip()
        if _BB.match(ln):
            txt, j = raw, i + 1
            while j < len(lines) and lines[j].strip().startswith(";") and not _BB.match(lines[j].strip()):
                txt += lines[j]
                j += 1
            in_loop = "Loop" in txt
        elif in_loop and ln.startswith(("global_load", "flat_load", "buffer_load", "scratch_load")):
            vector += 1
        elif in_loop and ln.startswith(("s_load", "s_buffer_load")):
            scalar += 1
    return vector, scalar


def kernels(asm_text: str):
    """{mangled name: dict(vgprs, sgprs, scratch, loop_vector, loop_scalar)} for every kernel of the file."""
    out = {}
    for m in re.finditer(r"^(_ZN4atmo\w+):[^\n]*\n(.*?)\.Lfunc_end", asm_text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        rest = asm_text[m.end():m.end() + 8000]
        get = lambda key: int(re.search(rf"; {key}: (\d+)", rest).group(1))   # noqa: E731
        vector, scalar = loop_loads(body)
        out[name] = dict(vgprs=get("NumVgprs"), sgprs=get("TotalNumSgprs"), scratch=get("ScratchSize"), loop_vector=vector, loop_scalar=scalar)
    return out


def table(asm_text: str):
    """[(flags without KF_VIEWS, lsteps, views kernel's numbers, twin's numbers, [what fails])], sorted."""
    ks = kernels(asm_text)
    rows = []
    for name, k in ks.items():
        m = re.match(r"_ZN4atmo24atmo_render_views_kernelILi(\d+)ELi(\d+)EE", name)
        if not m:
            continue
        flags, lsteps = int(m.group(1)) - KF_VIEWS, int(m.group(2))
        twin = next((v for n, v in ks.items() if n.startswith(f"_ZN4atmo18atmo_render_kernelILi{flags}ELi{lsteps}ELi1EE")), None)
        bad = []
        if twin is None:
            bad.append("no atmo_render twin")
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
    out = os.path.join(tempfile.mkdtemp(prefix="viewsres_"), "k.s")
    subprocess.run(["hipcc"] + HIPCC_FLAGS + [SRC, "-o", out] + argv, check=True, stderr=subprocess.DEVNULL)
    rows = table(open(out).read())
    if markdown:
        print("| kernel `<FLAGS, LSTEPS>` | VGPRs (waves) | twin VGPRs (waves) | SGPRs | twin SGPRs | vector loads in loops | twin | scalar loads in loops | twin | scratch |")
        print("|---|---|---|---|---|---|---|---|---|---|")
    ok = bool(rows)
    for flags, lsteps, k, twin, bad in rows:
        t = twin or dict(vgprs=0, sgprs=0, loop_vector=0, loop_scalar=0)
        if markdown:
            print(f"| `<{flags} + 2048, {lsteps}>` | {k['vgprs']} ({vgpr_waves(k['vgprs'])}) | {t['vgprs']} ({vgpr_waves(t['vgprs']) if twin else 0}) | {k['sgprs']} | {t['sgprs']} | "
                  f"{k['loop_vector']} | {t['loop_vector']} | {k['loop_scalar']} | {t['loop_scalar']} | {k['scratch']} |")
        else:
            print(f"atmo_render_views_kernel<{flags + KF_VIEWS}, {lsteps}>: {k['vgprs']} VGPRs ({vgpr_waves(k['vgprs'])} waves; twin {t['vgprs']}), {k['sgprs']} SGPRs (twin {t['sgprs']}), "
                  f"in loops {k['loop_vector']} vector loads (twin {t['loop_vector']}) and {k['loop_scalar']} scalar loads (twin {t['loop_scalar']}), ScratchSize {k['scratch']}: "
                  + ("ok" if not bad else "; ".join(bad).upper()))
        ok = ok and not bad
    if not rows:
        print("no multi-view kernel found")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
