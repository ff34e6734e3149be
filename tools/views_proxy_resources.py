#!/usr/bin/env python3
"""Static check of the multi-view proxy kernels (atmo_render_views_proxy_kernel<FLAGS | KF_VIEWS | KF_PROXY, LSTEPS> and
atmo_render_views_proxy_target_kernel<FLAGS | KF_VIEWS | KF_PROXY | KF_TARGET, LSTEPS>, include/atmo_views_proxy.h) against their two twins each, in the
ISA hipcc emits -- no GPU needed:

  - the single proxy draw's kernel, atmo_render_proxy_kernel<FLAGS | KF_PROXY, LSTEPS> (atmo_render_proxy_target_kernel for the target form);
  - the fullscreen batch's kernel, atmo_render_views_kernel<FLAGS | KF_VIEWS, LSTEPS> (atmo_render_views_target_kernel).

The eight ProxyConsts (and the eight TargetConsts) of these kernels sit by value in the kernel-argument segment and are indexed by the wave-uniform view
number, the RenderConsts in a device table; what must hold for that to cost nothing is what tools/views_resources.py asks of the float batch (whose
parsing this tool imports):

  - no stack frame (ScratchSize 0) -- a per-lane copy of a constants struct would be one;
  - inside loops, exactly as many vector memory loads as the single-proxy twin has (its texture fetches): no constant arrives through a vector load;
  - the VGPR count on the occupancy step of the LOWER of the two twins, or a better one.

    python tools/views_proxy_resources.py [--markdown] [-DFLAG ...]      exit code 0 = every kernel passes; one line (or table row) per kernel
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from views_resources import HIPCC_FLAGS, KF_VIEWS, SRC, kernels, vgpr_waves  # noqa: E402

KF_PROXY, KF_TARGET = 512, 1024
FORMS = (   # (kernel, its extra flags, the single-proxy twin and its flags, the fullscreen-batch twin and its flags)
    ("atmo_render_views_proxy_kernel", KF_VIEWS | KF_PROXY, "atmo_render_proxy_kernel", KF_PROXY, "atmo_render_views_kernel", KF_VIEWS),
    ("atmo_render_views_proxy_target_kernel", KF_VIEWS | KF_PROXY | KF_TARGET, "atmo_render_proxy_target_kernel", KF_PROXY | KF_TARGET,
     "atmo_render_views_target_kernel", KF_VIEWS | KF_TARGET),
)


def _find(ks, kernel, flags, lsteps):
    prefix = f"_ZN4atmo{len(kernel)}{kernel}ILi{flags}ELi{lsteps}EE"
    return next((v for n, v in ks.items() if n.startswith(prefix)), None)


def table(asm_text: str):
    """[(kernel, family flags, extra flags, lsteps, its numbers, the proxy twin's, the batch twin's, [what fails])], the float form first, sorted."""
    ks = kernels(asm_text)
    rows = []
    for kernel, extra, ptwin_name, pextra, vtwin_name, vextra in FORMS:
        part = []
        for name, k in ks.items():
            m = re.match(rf"_ZN4atmo{len(kernel)}{kernel}ILi(\d+)ELi(\d+)EE", name)
            if not m:
                continue
            flags, lsteps = int(m.group(1)) - extra, int(m.group(2))
            ptwin, vtwin = _find(ks, ptwin_name, flags + pextra, lsteps), _find(ks, vtwin_name, flags + vextra, lsteps)
            bad = []
            if ptwin is None or vtwin is None:
                bad.append("a twin is missing")
            else:
                floor = min(vgpr_waves(ptwin["vgprs"]), vgpr_waves(vtwin["vgprs"]))
                if vgpr_waves(k["vgprs"]) < floor:
                    bad.append(f"VGPRs {k['vgprs']} = {vgpr_waves(k['vgprs'])} waves, the lower twin has {floor}")
                if k["loop_vector"] != ptwin["loop_vector"]:
                    bad.append(f"{k['loop_vector']} vector loads inside loops, the proxy twin has {ptwin['loop_vector']}")
            if k["scratch"]:
                bad.append(f"ScratchSize {k['scratch']}")
            part.append((kernel, flags, extra, lsteps, k, ptwin, vtwin, bad))
        rows += sorted(part, key=lambda r: (r[1], r[3]))
    return rows


def main(argv):
    markdown = "--markdown" in argv
    argv = [a for a in argv if a != "--markdown"]
    out = os.path.join(tempfile.mkdtemp(prefix="viewspres_"), "k.s")
    subprocess.run(["hipcc"] + HIPCC_FLAGS + [SRC, "-o", out] + argv, check=True, stderr=subprocess.DEVNULL)
    rows = table(open(out).read())
    if markdown:
        print("| kernel `<FLAGS, LSTEPS>` | VGPRs (waves) | proxy twin | batch twin | SGPRs | proxy twin | batch twin | vector loads in loops | proxy twin | "
              "scalar loads in loops | proxy twin | scratch |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    ok = bool(rows)
    none = dict(vgprs=0, sgprs=0, loop_vector=0, loop_scalar=0)
    for kernel, flags, extra, lsteps, k, ptwin, vtwin, bad in rows:
        p, v = ptwin or none, vtwin or none
        if markdown:
            short = "views_proxy_target" if extra & KF_TARGET else "views_proxy"
            print(f"| {short} `<{flags} + {extra}, {lsteps}>` | {k['vgprs']} ({vgpr_waves(k['vgprs'])}) | {p['vgprs']} ({vgpr_waves(p['vgprs']) if ptwin else 0}) | "
                  f"{v['vgprs']} ({vgpr_waves(v['vgprs']) if vtwin else 0}) | {k['sgprs']} | {p['sgprs']} | {v['sgprs']} | {k['loop_vector']} | {p['loop_vector']} | "
                  f"{k['loop_scalar']} | {p['loop_scalar']} | {k['scratch']} |")
        else:
            print(f"{kernel}<{flags + extra}, {lsteps}>: {k['vgprs']} VGPRs ({vgpr_waves(k['vgprs'])} waves; proxy twin {p['vgprs']}, batch twin {v['vgprs']}), "
                  f"{k['sgprs']} SGPRs (proxy twin {p['sgprs']}, batch twin {v['sgprs']}), in loops {k['loop_vector']} vector loads (proxy twin {p['loop_vector']}) "
                  f"and {k['loop_scalar']} scalar loads (proxy twin {p['loop_scalar']}), ScratchSize {k['scratch']}: " + ("ok" if not bad else "; ".join(bad).upper()))
        ok = ok and not bad
    if not rows:
        print("no multi-view proxy kernel found")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
