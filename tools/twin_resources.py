#!/usr/bin/env python3
"""Static check of every render-kernel family that was added beside an older "twin" (the view batches, the proxy batches, the depth-source kernels, the
cloud-detail target kernels), in the ISA hipcc emits -- no GPU needed.  These kernels take their per-view or per-target constants from somewhere else than their twins do (a device
table, arrays by value in the kernel-argument segment indexed by the wave-uniform view number, a DepthConsts argument of its own); what must hold for
that to cost nothing:

  - no stack frame (ScratchSize 0) -- a per-lane copy of a constants struct would be one;
  - inside loops, exactly as many vector memory loads as the twin has (its texture fetches): a constant arriving through a vector load would be one
    more.  Constants arrive through scalar loads (s_load), which are printed as well: where the allocator re-loads them inside a loop, it says so;
  - the VGPR count on the occupancy step of the twin, or a better one (waves per SIMD by VGPRs: 512 / the count rounded up to 8, at most 8); with two
    twins, of the LOWER of them;
  - the depth-source kernels only: KF_DEPTH in their flags, and no more SGPR spilling than the twin -- v_readlane_b32 (how hipcc reads a spilled scalar
    back) at most SPILL_SLACK more than the twin's.  The first form of the depth load -- the division inside a three-way branch -- cost the single-draw
    cloud kernels 200-300 of them and clouds_high a factor 1.85 (profiles/depth/README.md, 3).

FAMILIES is the table: a new entry point adds its rows there and nothing else.

    python tools/twin_resources.py [--markdown] [--family NAME] [-DFLAG ...]      exit code 0 = every kernel passes; one line (or table row) per kernel
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "godot_atmosphere_shader_amd", "csrc", "atmo_kernels.hip")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-S", "--cuda-device-only"]
KF_PROXY, KF_TARGET, KF_VIEWS, KF_DEPTH, KF_DETAIL = 512, 1024, 2048, 4096, 8192   # the family bits of KernelFlags (csrc/atmo_device.h)
# Lane reads a kernel may have beyond its twin's.  Chosen, not derived: the shipped build's largest difference is 21 (<5139, 0, 1>: 62 against 41; the next
# is 14), the failure this check exists for was 150-300 beyond the twin in sixteen kernels.  24 passes the former and catches the latter with a factor of
# six to spare; a build that fails here by a few reads has to be measured (tools/depth_probe.py), not waved through by raising the number.
SPILL_SLACK = 24


class Family(NamedTuple):
    kernel: str          # its kernels: <FLAGS | bits, LSTEPS[, SPLIT]> of this template
    bits: int            # the family bits its FLAGS carry
    split: bool          # has a SPLIT parameter (a twin that has one is taken at the same SPLIT, or at 1)
    twins: tuple         # ((kernel, bits), ...): the same (FLAGS, LSTEPS) under these bits; the loop-load rule compares against the FIRST
    spill: bool          # the depth rules apply: KF_DEPTH in the flags, spill reads within SPILL_SLACK of the twin's
    count: int           # kernels of the family in the shipped build


FAMILIES = (
    Family("atmo_render_views_kernel", KF_VIEWS, False, (("atmo_render_kernel", 0),), False, 18),
    Family("atmo_render_views_target_kernel", KF_VIEWS | KF_TARGET, False, (("atmo_render_views_kernel", KF_VIEWS),), False, 18),
    Family("atmo_render_views_proxy_kernel", KF_VIEWS | KF_PROXY, False,
           (("atmo_render_proxy_kernel", KF_PROXY), ("atmo_render_views_kernel", KF_VIEWS)), False, 18),
    Family("atmo_render_views_proxy_target_kernel", KF_VIEWS | KF_PROXY | KF_TARGET, False,
           (("atmo_render_proxy_target_kernel", KF_PROXY | KF_TARGET), ("atmo_render_views_target_kernel", KF_VIEWS | KF_TARGET)), False, 18),
    Family("atmo_render_depth_target_kernel", KF_DEPTH | KF_TARGET, True, (("atmo_render_target_kernel", KF_TARGET),), True, 22),
    Family("atmo_render_proxy_depth_target_kernel", KF_DEPTH | KF_PROXY | KF_TARGET, False, (("atmo_render_proxy_target_kernel", KF_PROXY | KF_TARGET),), True, 18),
    Family("atmo_render_views_depth_target_kernel", KF_DEPTH | KF_VIEWS | KF_TARGET, False, (("atmo_render_views_target_kernel", KF_VIEWS | KF_TARGET),), True, 18),
    Family("atmo_render_views_proxy_depth_target_kernel", KF_DEPTH | KF_VIEWS | KF_PROXY | KF_TARGET, False,
           (("atmo_render_views_proxy_target_kernel", KF_VIEWS | KF_PROXY | KF_TARGET),), True, 18),
    # cloud detail into targets through a depth source (include/atmo_detail_target.h): the shading -- and with it the loop loads and the occupancy step to
    # keep -- is the detail draw's, the depth load and the stores are the depth-target kernels'
    Family("atmo_detail_target_kernel", KF_DETAIL | KF_DEPTH | KF_TARGET, False,
           (("atmo_render_detail_kernel", KF_DETAIL), ("atmo_render_depth_target_kernel", KF_DEPTH | KF_TARGET)), True, 6),
    Family("atmo_detail_views_target_kernel", KF_DETAIL | KF_DEPTH | KF_VIEWS | KF_TARGET, False,
           (("atmo_render_detail_kernel", KF_DETAIL), ("atmo_render_views_depth_target_kernel", KF_DEPTH | KF_VIEWS | KF_TARGET)), True, 6),
)
NUMBERS = ("vgprs", "sgprs", "loop_vector", "loop_scalar", "spill_reads", "scratch")
_BB = re.compile(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)")
_NAME = re.compile(r"_ZN4atmo\d+(atmo_(?:render|detail)_(?:[a-z_]+_)?kernel)ILi(\d+)ELi(\d+)E(?:Li(\d+)E)?E")


def short_name(kernel: str) -> str:
    """views_proxy of atmo_render_views_proxy_kernel, detail_target of atmo_detail_target_kernel: what --family takes."""
    return kernel[len("atmo_render_" if kernel.startswith("atmo_render_") else "atmo_"):-len("_kernel")]


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
    """{mangled name: dict of NUMBERS} for every kernel of the file."""
    out = {}
    for m in re.finditer(r"^(_ZN4atmo\w+):[^\n]*\n(.*?)\.Lfunc_end", asm_text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        rest = asm_text[m.end():m.end() + 8000]
        get = lambda key: int(re.search(rf"; {key}: (\d+)", rest).group(1))   # noqa: E731
        vector, scalar = loop_loads(body)
        out[name] = dict(vgprs=get("NumVgprs"), sgprs=get("TotalNumSgprs"), scratch=get("ScratchSize"), loop_vector=vector, loop_scalar=scalar,
                         spill_reads=len(re.findall(r"^\s*v_readlane_b32", body, re.M)))
    return out


class Row(NamedTuple):
    family: Family
    flags: int           # as in the kernel's name, family bits included
    lsteps: int
    split: int | None
    k: dict              # the kernel's NUMBERS
    twins: tuple         # each twin's NUMBERS, or None where it is missing
    bad: list            # what fails; empty = the kernel passes

    @property
    def name(self) -> str:
        return f"{self.family.kernel}<{self.flags}, {self.lsteps}" + (f", {self.split}>" if self.family.split else ">")


def check(asm_text: str, families=FAMILIES):
    """One Row per kernel of every family in `families`, in the table's order and sorted by (FLAGS, LSTEPS, SPLIT) inside a family.  A pure function of the
    assembly text."""
    by_key = {}
    for name, k in kernels(asm_text).items():
        m = _NAME.match(name)
        if m:
            by_key[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)) if m.group(4) else None)] = k
    rows = []
    for fam in families:
        for (_, flags, lsteps, split), k in sorted((key, k) for key, k in by_key.items() if key[0] == fam.kernel):
            base = flags - fam.bits
            twins = tuple(next((t for (s, f, l, sp), t in by_key.items() if s == ts and f == base + tbits and l == lsteps and sp in (None, split or 1)), None)
                          for ts, tbits in fam.twins)
            bad = []
            if fam.spill and not flags & KF_DEPTH:
                bad.append("no KF_DEPTH in its flags")
            if None in twins:
                bad.append("twin missing")
            else:
                floor = min(vgpr_waves(t["vgprs"]) for t in twins)
                if vgpr_waves(k["vgprs"]) < floor:
                    bad.append(f"VGPRs {k['vgprs']} = {vgpr_waves(k['vgprs'])} waves, the " + ("twin has" if len(twins) == 1 else "lower twin has") + f" {floor}")
                if k["loop_vector"] != twins[0]["loop_vector"]:
                    bad.append(f"{k['loop_vector']} vector loads inside loops, the twin has {twins[0]['loop_vector']}")
                if fam.spill and k["spill_reads"] > twins[0]["spill_reads"] + SPILL_SLACK:
                    bad.append(f"{k['spill_reads']} SGPR spill reads, the twin has {twins[0]['spill_reads']}")
            if k["scratch"]:
                bad.append(f"ScratchSize {k['scratch']}")
            rows.append(Row(fam, flags, lsteps, split, k, twins, bad))
    return rows


def compile_asm(extra=()):
    """hipcc -S of atmo_kernels.hip (about two minutes): the assembly text."""
    with tempfile.TemporaryDirectory(prefix="twinres_") as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run(["hipcc"] + HIPCC_FLAGS + [SRC, "-o", out] + list(extra), check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def _cells(row: Row):
    """The columns behind the kernel's name: each number with the twins' in brackets."""
    def with_twins(key, show=str, twins=row.twins):
        return f"{show(row.k[key])} (" + ", ".join("-" if t is None else show(t[key]) for t in twins) + ")"
    return [with_twins("vgprs", lambda v: f"{v} = {vgpr_waves(v)} waves"), with_twins("sgprs"), with_twins("loop_vector", twins=row.twins[:1]),
            with_twins("loop_scalar", twins=row.twins[:1]), with_twins("spill_reads", twins=row.twins[:1]), str(row.k["scratch"])]


def main(argv):
    markdown = "--markdown" in argv
    argv = [a for a in argv if a != "--markdown"]
    families = FAMILIES
    if "--family" in argv:
        i = argv.index("--family")
        families = tuple(f for f in FAMILIES if argv[i + 1] in (f.kernel, short_name(f.kernel)))
        if not families:
            sys.exit(f"--family: one of {', '.join(short_name(f.kernel) for f in FAMILIES)}")
        del argv[i:i + 2]
    rows = check(compile_asm(argv), families)
    heads = ["VGPRs (twins')", "SGPRs (twins')", "vector loads in loops (twin's)", "scalar loads in loops (twin's)", "SGPR spill reads (twin's)", "scratch"]
    if markdown:
        print("| kernel `<FLAGS, LSTEPS[, SPLIT]>` | " + " | ".join(heads) + " | |")
        print("|---" * (len(heads) + 2) + "|")
    for row in rows:
        verdict = "ok" if not row.bad else "; ".join(row.bad).upper()
        if markdown:
            print(f"| `{row.name}` | " + " | ".join(_cells(row)) + f" | {verdict} |")
        else:
            print(f"{row.name}: " + ", ".join(f"{h} {c}" for h, c in zip(heads, _cells(row))) + f": {verdict}")
    ok = True
    for fam in families:
        n = sum(r.family is fam for r in rows)
        if n != fam.count:
            print(f"{fam.kernel}: {n} kernels, the shipped build has {fam.count}")
        ok = ok and n > 0
    return 0 if ok and not any(r.bad for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
