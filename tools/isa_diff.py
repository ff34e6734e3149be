#!/usr/bin/env python3
"""Per-symbol diff of the render kernels of two builds of libatmo_hip.so (no GPU needed): every kernel whose name matches the pattern is disassembled from
both libraries with llvm-objdump, branch targets and addresses stripped to offsets from the kernel's own start, and compared instruction for instruction.

    python tools/isa_diff.py OLD.so NEW.so [symbol regex, default "atmo_render_kernel|atmo_render_proxy_kernel"]

Prints one line per symbol that differs or exists in one build only, and a summary; exit status 1 when an OLD symbol is missing from or differs in NEW.
The literal of an `s_add_u32` / `s_addc_u32` that follows an `s_getpc_b64` is a PC-relative address (of a constant table elsewhere in the code object): it
moves whenever a kernel is added in front of the table, and is not compared -- such kernels are counted as identical, and how many there were is said."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loop_phase import LLVM, device_code_object


def kernels(lib, pattern, tmp, tag):
    co = device_code_object(lib, os.path.join(tmp, tag + ".co"))
    syms = subprocess.run([f"{LLVM}/llvm-readelf", "-sW", co], check=True, capture_output=True, text=True).stdout
    names = sorted({l.split()[-1] for l in syms.splitlines() if " FUNC " in l and re.search(pattern, l.split()[-1])})
    # st_value and st_size of every kernel: what lies behind a symbol's size is not the kernel's (alignment and end-of-section s_nop padding, which
    # llvm-objdump prints up to the next symbol -- 240 of them behind atmo_lut_footprint_kernel until another kernel was placed behind it)
    extent = {l.split()[-1]: (int(l.split()[1], 16), int(l.split()[2])) for l in syms.splitlines() if " FUNC " in l}
    out = {}
    for name in names:
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f"--disassemble-symbols={name}", co], check=True, capture_output=True, text=True).stdout
        # "  <instruction>   // <address>: <raw words>": keep the text and the raw encoding (relative branches encode offsets, so they compare as they are)
        start, size = extent[name]
        ins = [(m.group(1).strip(), m.group(3).strip(), int(m.group(2), 16)) for m in re.finditer(r"^\s+(\S[^\n]*?)\s+// ([0-9A-F]{12}):([^\n]*)", dis, re.M)]
        out[name] = [(text, raw) for text, raw, addr in ins if addr < start + size]
    return out


if __name__ == "__main__":
    old_lib, new_lib = sys.argv[1], sys.argv[2]
    pattern = sys.argv[3] if len(sys.argv) > 3 else r"atmo_render_kernel|atmo_render_proxy_kernel"
    with tempfile.TemporaryDirectory(prefix="isadiff_") as tmp:
        old, new = kernels(old_lib, pattern, tmp, "old"), kernels(new_lib, pattern, tmp, "new")
    def strip_pcrel(ins):
        """The instruction list with the literals of the address arithmetic behind s_getpc_b64 (text and encoding) blanked."""
        out, window = [], 0
        for text, raw in ins:
            if text.startswith("s_getpc_b64"):
                window = 4
            elif window > 0 and re.match(r"s_addc?_u32 s\d+, s\d+, (0x[0-9a-f]+|-?\d+)$", text):
                text, raw = text.rsplit(",", 1)[0] + ", <pc-relative>", raw.split()[0] if raw.split() else raw
            window -= 1
            out.append((text, raw))
        return out

    bad = moved = 0
    for name in sorted(old):
        if name not in new:
            print(f"MISSING in new: {name}")
            bad += 1
        elif old[name] != new[name] and strip_pcrel(old[name]) == strip_pcrel(new[name]):
            moved += 1
        elif old[name] != new[name]:
            first = next((i for i, (a, b) in enumerate(zip(old[name], new[name])) if a != b), min(len(old[name]), len(new[name])))
            print(f"DIFFERS: {name}: {len(old[name])} -> {len(new[name])} instructions, first difference at instruction {first}")
            bad += 1
    added = sorted(set(new) - set(old))
    print(f"{len(old)} kernels in the old build, {len(old) - bad} identical in the new one (text and encoding; {moved} of them up to a PC-relative constant), "
          f"{bad} differ or are missing; "
          f"{len(added)} matching kernels only in the new build")
    sys.exit(1 if bad else 0)
