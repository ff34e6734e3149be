"""Host-only evidence that the render kernels added beside an older "twin" cost what the twin costs: their registers, stack and loads in the ISA hipcc
emits (tools/twin_resources.py: one table of families, one compile per test session) and the position of the headline direct-light view loop in
every kernel that carries it (tools/loop_phase.py: one list of twins)."""
import functools
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import loop_phase
    import twin_resources
finally:
    sys.path.pop(0)


@functools.lru_cache(maxsize=None)
def _asm():
    """atmo_kernels.hip as assembly: compiled once, by the first test that asks."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not found")
    return twin_resources.compile_asm()


@functools.lru_cache(maxsize=None)
def _rows():
    return twin_resources.check(_asm())


@pytest.mark.parametrize("family", twin_resources.FAMILIES, ids=lambda f: twin_resources.short_name(f.kernel))
def test_kernels_keep_their_constants_in_sgprs(family):
    """Every kernel of the family has no stack frame, as many vector loads inside its loops as its twin (the texture fetches: no constant -- no field of
    a RenderConsts, ProxyConsts, TargetConsts or DepthConsts -- arrives through a vector load; the depth load sits in the prologue), a VGPR count on the
    occupancy step of its twin (the proxy batches: of the lower of their two twins) or a better one, and passes the tool's other rules."""
    rows = [r for r in _rows() if r.family is family]
    for r in rows:
        print(r.name, r.k, r.twins, r.bad)
    assert len(rows) == family.count
    waves = twin_resources.vgpr_waves
    for r in rows:
        assert not r.bad, (r.name, r.bad)
        assert r.k["scratch"] == 0, r.name
        assert len(r.twins) == len(family.twins) and None not in r.twins, r.name
        assert r.k["loop_vector"] == r.twins[0]["loop_vector"], r.name
        assert waves(r.k["vgprs"]) >= min(waves(t["vgprs"]) for t in r.twins), r.name
        if family.spill:
            assert r.flags & twin_resources.KF_DEPTH and r.k["spill_reads"] <= r.twins[0]["spill_reads"] + twin_resources.SPILL_SLACK, r.name


def test_the_tool_exits_zero_on_the_library_s_kernels(monkeypatch, capsys):
    """Its command line on the same text: status 0, one line per kernel, every one of them ok."""
    text = _asm()
    monkeypatch.setattr(twin_resources, "compile_asm", lambda extra=(): text)
    assert twin_resources.main([]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == sum(f.count for f in twin_resources.FAMILIES) and all(ln.endswith("scratch 0: ok") for ln in lines)
    assert twin_resources.main(["--family", "views_proxy"]) == 0
    assert len(capsys.readouterr().out.splitlines()) == 18


def _label(kernel, flags, lsteps, split=None):
    """The regular expression of a kernel's label line in the assembly text."""
    return rf"^_ZN4atmo{len(kernel)}{kernel}ILi{flags}ELi{lsteps}E" + (f"Li{split}E" if split else "") + r"E\w*:"


def test_a_stack_frame_fails_its_kernel_and_no_other():
    """The real text with ONE kernel's `; ScratchSize: 0` edited to 16."""
    text = _asm()
    victim = next(r for r in _rows() if r.family.kernel == "atmo_render_views_target_kernel")
    label = re.search(_label(victim.family.kernel, victim.flags, victim.lsteps), text, re.M)
    at = text.index("; ScratchSize: 0", label.end())
    assert "\n_ZN4atmo" not in text[label.end():at]                      # the kernel's own line, not a later kernel's
    rows = twin_resources.check(text[:at] + "; ScratchSize: 16" + text[at + len("; ScratchSize: 0"):])
    assert [(r.name, r.bad) for r in rows if r.bad] == [(victim.name, ["ScratchSize 16"])]


def test_a_missing_twin_fails_its_kernel_and_no_other():
    """The real text without the atmo_render_kernel that is the twin of one view-batch kernel (and of no other kernel)."""
    text = _asm()
    victim = next(r for r in _rows() if r.family.kernel == "atmo_render_views_kernel")
    cut, n = re.subn(_label(victim.family.twins[0][0], victim.flags - victim.family.bits, victim.lsteps, 1) + r".*?\.Lfunc_end", "", text, flags=re.S | re.M)
    assert n == 1
    rows = twin_resources.check(cut)
    assert [(r.name, r.bad) for r in rows if r.bad] == [(victim.name, ["twin missing"])]
    assert len(rows) == len(_rows())


# ---- the headline view loop, read back from the library as built ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _view_loops(pattern):
    from godot_atmosphere_shader_amd.build import build_native

    if not os.path.exists(f"{loop_phase.LLVM}/llvm-objdump"):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    return loop_phase.view_loops(build_native(), pattern)


@pytest.mark.parametrize("pattern,knob", loop_phase.HEADLINE_TWINS, ids=[knob for _, knob in loop_phase.HEADLINE_TWINS])
def test_headline_twin_sits_at_the_fast_loop_position(pattern, knob):
    """Round 6 (profiles/round6/ab_loop_phase.txt): the 32 x 8 direct-light kernel <4, 8, 1> -- the BASELINE configs[1] headline -- is 8.5-11 % slower unless
    the first instruction of its view loop lies FAST_PHASE bytes into a 32-byte block of the instruction stream.  A change anywhere in front of that
    loop can move it by four bytes (that is what made earlier rounds' preamble and SGPR-cap experiments lose 8-10 %).  Every kernel that carries the loop
    -- the geometric-order twin, the view batch's, the packed-target and depth-source forms of all three -- is padded onto the same position by a knob of
    its own; this test reads the position from the library as built and fails until that knob (atmo_kernels.hip) puts it back."""
    rows = _view_loops(pattern)
    assert len(rows) == 1, (pattern, rows)            # one kernel matches, with one loop holding the seven-root cluster of the light march
    name, offset, phase, size = rows[0]
    assert phase == loop_phase.FAST_PHASE, (f"{name}: the view loop starts {phase} bytes into its 32-byte block (at +0x{offset:x}, {size} bytes); the measured-fast "
                                            f"position is {loop_phase.FAST_PHASE}: move {knob} by {((loop_phase.FAST_PHASE - phase) % 32) // 4}")
    assert size == _view_loops(loop_phase.HEADLINE_TWINS[0][0])[0][3], (name, knob)   # the float headline kernel's loop
