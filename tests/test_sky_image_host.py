"""Sky images on the CPU (include/atmo_sky_image.h; godot_atmosphere_shader_amd/sky_image.py): the header's symbol set and the binding, every refusal of
the two device entry points on a host-only context in the header's order (nothing touches a device), the level count, known answers of the numpy
statement -- constant images, a 2 x 2 block, linear light under sRGB, quad order against row-major order, bands against one call -- and the two kernel
families in the compiled assembly.  (tests/test_sky_image_gpu.py holds the kernels to the statement.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import test_kernel_twins_host as T
from godot_atmosphere_shader_amd import lens as L
from godot_atmosphere_shader_amd import sky_image as SI
from godot_atmosphere_shader_amd import targets as TG
from godot_atmosphere_shader_amd.lens import Lens
from godot_atmosphere_shader_amd.ray_quads import quad_order
from test_rays_host import _mode_ctx, _said
from test_views_proxy_host import ROOT, _functions

RGBA, PIXELS = 0x100000, 0x200000   # addresses no refusal dereferences
FORMATS = ("rgba32f", "rgba16f", "rgba8", "rgba8_srgb", "bgra8", "bgra8_srgb", "a2b10g10r10")


def _lib():
    from godot_atmosphere_shader_amd import _native as N

    return N, SI.bind()


def _ctx(N, lib):
    return _mode_ctx(N, lib, N.VARIANT_NO_CLOUDS, light_mode=N.LIGHT_DIRECT, light_steps=8)   # direct light without clouds needs no texture


# ---- the header and the binding ----------------------------------------------------------------------------------------------------------------------
def test_binding_exposes_the_sky_image_header():
    """Fails on a library without the feature: the header does not exist and the symbols are not exported."""
    N, lib = _lib()
    assert _functions("atmo_sky_image.h") == set(SI.SKY_IMAGE_ENTRY_POINTS) and len(SI.SKY_IMAGE_ENTRY_POINTS) == 3
    assert tuple(SI.signatures()) == SI.SKY_IMAGE_ENTRY_POINTS
    tuples = {name: value for name, value in vars(N).items() if name.endswith("_SYMBOLS") and isinstance(value, tuple)}
    assert len(tuples) > 10
    for sym in SI.SKY_IMAGE_ENTRY_POINTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int
        assert not any(sym in symbols for symbols in tuples.values()), sym
        assert not any(sym in symbols for symbols, _, _, _ in N.HEADERS.values())      # declared by sky_image.py, not by a block of _native.HEADERS
    assert lib is N.load() and lib.atmo_abi_version() == N.ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "atmo_sky_image.h")).read()
    assert '#include "atmo_sky_sh.h"' in text and '#include "atmo_target.h"' in text and "THE MIP CHAIN" in text and "Not here" in text
    for name in ("atmo.h", "atmo_target.h", "atmo_lens.h", "atmo_reduced.h"):   # the older headers do not know the new one
        assert "atmo_sky_image" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert "atmo_sky_image.h" in open(os.path.join(ROOT, "include", "atmo_sky_sh.h")).read().split("Not here")[1]
    # the flags and the level's layout are the header's
    defines = dict(re.findall(r"^#define ATMO_SKY_IMAGE_([A-Z]+) (\d+)u", text, flags=re.M))
    assert defines == {"PREMULTIPLIED": str(SI.PREMULTIPLIED), "COMPOSITE": str(SI.COMPOSITE)} and SI.QUADS == L.LENS_QUADS == 1
    assert C.sizeof(SI.AtmoSkyLevel) == 24
    assert [(n, getattr(SI.AtmoSkyLevel, n).offset) for n, _ in SI.AtmoSkyLevel._fields_] == [
        ("pixels", 0), ("row_pitch_bytes", 8), ("reserved", 12), ("layer_pitch_bytes", 16)]


def test_a_library_without_the_symbols_is_refused_by_name():
    class Fn:
        restype = argtypes = None

    class Old:
        atmo_sky_image_resolve = Fn()   # some, not all

    with pytest.raises(RuntimeError, match=r"atmo_sky_image_level_count \(include/atmo_sky_image\.h\)"):
        SI.bind(Old())
    assert Old.atmo_sky_image_resolve.argtypes is not None


@pytest.mark.parametrize("w, h, want", [(1, 1, 1), (2, 1, 2), (5, 3, 3), (512, 512, 10), (2048, 1024, 12), (65536, 1, 17)])
def test_the_level_count(w, h, want):
    N, lib = _lib()
    got = C.c_int(-7)
    assert lib.atmo_sky_image_level_count(w, h, C.byref(got)) == N.ATMO_OK and got.value == want == SI.level_count(w, h) == 1 + int(math.floor(math.log2(max(w, h))))
    assert SI.level_size(w, h, want - 1) == (1, 1) and (want == 1 or max(SI.level_size(w, h, want - 2)) > 1)
    for bad in ((0, h), (w, 0), (65537, h), (w, 65537)):
        got = C.c_int(-7)
        assert lib.atmo_sky_image_level_count(*bad, C.byref(got)) == N.ATMO_E_ARG and got.value == -7
        with pytest.raises(ValueError):
            SI.level_count(*bad)
    assert lib.atmo_sky_image_level_count(w, h, None) == N.ATMO_E_ARG


# ---- the refusals, in the header's order ------------------------------------------------------------------------------------------------------------
def _resolve(lib, ctx, lens=True, kind=L.OCTAHEDRAL, width=8, height=8, rows=(0, 8), face=0, fov=1.0, flags=0, rgba=RGBA, target=True, fmt=1,
             pixels=PIXELS, pitch=0):
    N, _ = _lib()
    nl = N.AtmoLens()
    nl.kind, nl.width, nl.height, nl.y0, nl.y1, nl.face, nl.fov = kind, width, height, rows[0], rows[1], face, fov
    tgt = N.AtmoTarget(pixels, fmt, pitch)
    return _said(lib, ctx, lib.atmo_sky_image_resolve(ctx, C.byref(nl) if lens else None, flags, rgba, C.byref(tgt) if target else None, None))


def _mips(lib, ctx, levels=True, n_levels=3, fmt=1, width=8, height=4, layers=2, pixels=(PIXELS, PIXELS + 0x1000, PIXELS + 0x2000), row=(0, 0, 0),
          layer=(0, 0, 0), reserved=(0, 0, 0)):
    arr = (SI.AtmoSkyLevel * 3)(*[SI.AtmoSkyLevel(pixels[i], row[i], reserved[i], layer[i]) for i in range(3)])
    return _said(lib, ctx, lib.atmo_sky_image_mips(ctx, arr if levels else None, n_levels, fmt, width, height, layers, None))


# (what the message must hold, the one thing wrong), in the order of the checks
RESOLVE_CHECKS = [("null lens", dict(lens=False)), ("unknown lens kind", dict(kind=4)), ("width and height", dict(width=0)),
                  ("2^28", dict(width=1 << 15, height=(1 << 13) + 1, rows=(0, 2))), ("band", dict(rows=(0, 9))),
                  ("fov", dict(kind=L.FISHEYE, fov=7.0)), ("square", dict(kind=L.CUBE_FACE, width=9)), ("face", dict(kind=L.CUBE_FACE, face=6)),
                  ("unknown flag bits", dict(flags=8)), ("PREMULTIPLIED together with", dict(flags=6)), ("even y0", dict(flags=1, rows=(1, 8))),
                  ("null rgba_dev", dict(rgba=0)), ("rgba_dev must be 16-byte aligned", dict(rgba=RGBA + 8)), ("null target", dict(target=False)),
                  ("unknown target format", dict(fmt=3)), ("null target pixels", dict(pixels=0)), ("aligned to the pixel size", dict(pixels=PIXELS + 4)),
                  ("row_pitch_bytes", dict(pitch=56))]
MIPS_CHECKS = [("unknown target format", dict(fmt=20)), ("width and height", dict(width=65537)), ("layers", dict(layers=4097)),
               ("2^30", dict(width=65536, height=65536, layers=1, n_levels=1)), ("n_levels", dict(n_levels=5)), ("null levels", dict(levels=False)),
               ("level 0: null pixels", dict(pixels=(0, PIXELS, PIXELS))), ("level 0: pixels must be aligned", dict(pixels=(PIXELS + 4, PIXELS, PIXELS))),
               ("level 0: row_pitch_bytes", dict(row=(60, 0, 0))), ("level 0: layer_pitch_bytes", dict(layer=(248, 0, 0))),
               ("level 0: reserved", dict(reserved=(1, 0, 0))), ("level 1: null pixels", dict(pixels=(PIXELS, 0, PIXELS))),
               ("level 1: row_pitch_bytes", dict(row=(0, 36, 0))), ("level 2: layer_pitch_bytes", dict(layer=(0, 0, 12))),
               ("level 2: reserved", dict(reserved=(0, 0, -1)))]


@pytest.mark.parametrize("entry", ["atmo_sky_image_resolve", "atmo_sky_image_mips"])
def test_every_refusal_in_the_header_s_order(entry):
    """Each wrong argument alone is ATMO_E_ARG under the entry point's name; of two wrong arguments the one the header lists first is named; a well-formed
    call on a host-only context gets as far as ATMO_E_NO_DEVICE."""
    N, lib = _lib()
    ctx = _ctx(N, lib)
    call, checks = (_resolve, RESOLVE_CHECKS) if entry == "atmo_sky_image_resolve" else (_mips, MIPS_CHECKS)
    try:
        for needle, wrong in checks:
            rc, msg = call(lib, ctx, **wrong)
            assert rc == N.ATMO_E_ARG and msg.startswith(entry + ": ") and needle in msg, (wrong, rc, msg)
        for (needle, first), (_, second) in zip(checks, checks[1:]):
            if set(first) & set(second):
                continue    # two values of one argument
            rc, msg = call(lib, ctx, **first, **second)
            assert rc == N.ATMO_E_ARG and needle in msg, (first, second, rc, msg)
        rc, msg = call(lib, ctx)
        assert rc == N.ATMO_E_NO_DEVICE and msg.startswith(entry + ": ") and "host-only" in msg, (rc, msg)
        if entry == "atmo_sky_image_resolve":
            for flags in (1, 2, 3, 4, 5):
                assert _resolve(lib, ctx, flags=flags)[0] == N.ATMO_E_NO_DEVICE, flags
            for fmt, pitch in ((0, 128), (0, 144), (1, 64), (1, 72), (2, 32), (16, 36), (19, 4096)):
                assert _resolve(lib, ctx, fmt=fmt, pitch=pitch)[0] == N.ATMO_E_NO_DEVICE, (fmt, pitch)
            assert _resolve(lib, ctx, fmt=1, pitch=68)[0] == N.ATMO_E_ARG                                   # no multiple of the pixel size
            assert _resolve(lib, ctx, flags=1, rows=(2, 7))[0] == N.ATMO_E_ARG and _resolve(lib, ctx, flags=1, width=7, height=7, rows=(2, 7))[0] == N.ATMO_E_NO_DEVICE
            assert _resolve(lib, ctx, rows=(3, 3), kind=9, flags=64, rgba=0, target=False)[0] == N.ATMO_OK  # an empty band: nothing else is looked at
            # the flag checks stand behind the lens's own and in front of QUADS' rows
            assert "unknown flag bits" in _resolve(lib, ctx, flags=9, rows=(1, 8))[1] and "face" in _resolve(lib, ctx, flags=8, kind=L.CUBE_FACE, face=6)[1]
            assert lib.atmo_sky_image_resolve(None, None, 0, None, None, None) == N.ATMO_E_ARG              # a null ctx: no message to hold
        else:
            assert _mips(lib, ctx, row=(64, 32, 16), layer=(256, 64, 16))[0] == N.ATMO_E_NO_DEVICE          # the tight pitches, said aloud
            assert _mips(lib, ctx, row=(72, 40, 16), layer=(72 * 4 + 8, 4096, 0))[0] == N.ATMO_E_NO_DEVICE  # and wider ones
            for fmt in (0, 1, 2, 16, 17, 18, 19):
                assert _mips(lib, ctx, fmt=fmt, n_levels=2)[0] == N.ATMO_E_NO_DEVICE, fmt
            # n_levels == 1: level 0 is checked, then nothing is enqueued -- ATMO_OK on a host-only context too
            assert _mips(lib, ctx, n_levels=1, pixels=(PIXELS, 0, 0))[0] == N.ATMO_OK
            assert "level 0: null pixels" in _mips(lib, ctx, n_levels=1, pixels=(0, 0, 0))[1]
            assert _mips(lib, ctx, n_levels=0)[0] == N.ATMO_E_ARG
            assert lib.atmo_sky_image_mips(None, None, 2, 1, 8, 4, 1, None) == N.ATMO_E_ARG
    finally:
        lib.atmo_destroy(ctx)


# ---- the numpy statement: known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_constant_image_has_constant_mips(fmt):
    """The average of four equal values is the value (x + x and 2 x + 2 x are exact, and so is the quarter), and every format's decode is encode's
    fixed point."""
    rng = np.random.default_rng(5)
    texel = TG.encode(rng.uniform(0.0, 1.0, 4).astype(np.float32), fmt)
    level0 = np.broadcast_to(texel, (2, 5, 12, 4)).copy()
    chain = SI.mip_chain(level0, fmt, SI.level_count(12, 5))
    assert [c.shape for c in chain] == [(2, 5, 12, 4), (2, 2, 6, 4), (2, 1, 3, 4), (2, 1, 1, 4)]
    for level in chain:
        assert level.dtype == TG.DTYPES[TG.format_id(fmt)] and np.all(level.reshape(-1, 4).view(np.uint8) == texel.reshape(4).view(np.uint8)[None, :])


def test_a_two_by_two_block_is_its_average():
    block = np.array([[[1, 1, 1, 1], [2, 2, 2, 2]], [[3, 3, 3, 3], [4, 4, 4, 4]]], dtype=np.float32)
    assert SI.mip_level(block, "rgba32f").tolist() == [[[2.5, 2.5, 2.5, 2.5]]]
    # where a side has reached 1 the texel counts twice: a 2 x 1 image averages its two texels, a 1 x 2 likewise
    assert SI.mip_level(block[:1], "rgba32f").tolist() == [[[1.5] * 4]] and SI.mip_level(block[:, :1], "rgba32f").tolist() == [[[2.0] * 4]]
    # floor sizes: the third column and row of a 3 x 3 level are dropped
    odd = np.arange(36, dtype=np.float32).reshape(3, 3, 4)
    assert SI.mip_level(odd, "rgba32f").tobytes() == SI.mip_level(odd[:2, :2], "rgba32f").tobytes()
    with pytest.raises(ValueError):
        SI.mip_chain(block, "rgba32f", 3)


@pytest.mark.parametrize("fmt", ["rgba8_srgb", "bgra8_srgb"])
def test_the_srgb_chain_averages_in_linear_light(fmt):
    level0 = np.zeros((2, 2, 4), dtype=np.uint8)
    level0[0, 0] = level0[1, 1] = 255                        # two texels white and opaque, two black and clear: 0.5 in linear light
    (texel,) = SI.mip_level(level0, fmt).reshape(1, 4)
    half = int(TG.srgb_encode(np.float32(0.5)))
    assert half == 188 and texel.tolist() == [half, half, half, 128]            # not the byte average 128 (alpha is linear: rint(127.5) to even)
    assert SI.mip_level(level0, fmt[:5]).reshape(4).tolist() == [128, 128, 128, 128]


def _random_rows(n, seed):
    rng = np.random.default_rng(seed)
    rgba = rng.uniform(-0.5, 1.5, (n, 4)).astype(np.float32)
    rgba[rng.random(n) < 0.1, 3] = 0.0
    return rgba


LENSES = [Lens.octahedral(7, 5), Lens.cube_face(9, 2), Lens.equirect(33, 6), Lens.fisheye(17, 13, fov=math.radians(220.0)), Lens.fisheye(16, 12, fov=3.0)]


@pytest.mark.parametrize("lens", LENSES, ids=repr)
@pytest.mark.parametrize("fmt", ["rgba16f", "rgba8_srgb"])
def test_quad_order_and_bands_resolve_to_the_one_image(lens, fmt):
    """The same rows in quad order and in row-major order resolve to the same image; an image resolved in bands is the one-call image; the rows of absent
    pixels and of the slots outside the image are never read."""
    w, h = lens.width, lens.height
    rows = _random_rows(w * h, w * h)
    _, present = SI.slots(lens)
    assert present.all() or lens.kind == L.FISHEYE
    poisoned = np.where(present[:, None], rows, np.float32(np.nan))
    order = quad_order(w, h)
    quad_rows = np.where((order >= 0)[:, None], poisoned[np.clip(order, 0, None)], np.float32(np.nan))
    dst = TG.encode(_random_rows(w * h, 3).reshape(h, w, 4), fmt)
    for kw in (dict(), dict(premultiplied=True), dict(dst=dst)):
        whole = SI.resolve(lens, poisoned, fmt, **kw)
        assert whole.shape == (h, w, 4) and whole.dtype == TG.DTYPES[TG.format_id(fmt)]
        assert whole.tobytes() == SI.resolve(lens, rows, fmt, **kw).tobytes()                     # what the absent rows hold does not matter
        assert SI.resolve(lens, quad_rows, fmt, quads=True, **kw).tobytes() == whole.tobytes()
        flat, before = whole.reshape(-1, 4), dst.reshape(-1, 4)
        if "dst" in kw:
            keep = ~present | ~(rows[:, 3] > 0)
            assert keep.any() and flat[keep].tobytes() == before[keep].tobytes()
            assert flat[~keep].tobytes() == TG.blend(rows[~keep], before[~keep], fmt).tobytes()
        else:
            assert not flat[~present].view(np.uint8).any()
            src = np.concatenate([rows[:, :3] * rows[:, 3:4], rows[:, 3:4]], axis=1) if kw else rows
            assert flat[present].tobytes() == TG.encode(src[present], fmt).tobytes()
        y0 = 2
        y1 = h - 1 if h % 2 == 0 else 4
        for quads, cuts in ((False, (0, 1, y0, y1, h)), (True, (0, y0, 4, h))):
            parts = []
            for a, b in zip(cuts, cuts[1:]):
                band = lens.band((a, b))
                slot, _ = SI.slots(band, quads)
                band_rows = np.full((band.counts(quads)[0], 4), np.nan, dtype=np.float32)
                band_rows[slot] = poisoned[a * w:b * w]
                band_kw = dict(kw, dst=dst[a:b]) if "dst" in kw else kw
                parts.append(SI.resolve(band, band_rows, fmt, quads=quads, **band_kw))
            assert np.concatenate(parts).tobytes() == whole.tobytes(), (quads, cuts)
    with pytest.raises(ValueError):
        SI.resolve(lens, rows, fmt, premultiplied=True, dst=dst)


# ---- the kernels in the compiled assembly ----------------------------------------------------------------------------------------------------------------
def test_the_two_kernel_families_have_no_stack_frame():
    """Present under their mangled names (tools/twin_resources.py reads the compiler's own numbers), no private-memory stack, no spill, names of their
    own, and the VGPR and LDS figures the header states."""
    asm = T._asm()
    numbers = T.twin_resources.kernels(asm)
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(_ZN4atmo\w+):[^\n]*\n.*?\.Lfunc_end.*?; LDSByteSize: (\d+)", asm, re.S | re.M)}
    (resolve,) = [n for n in numbers if n.startswith("_ZN4atmo29atmo_sky_image_resolve_kernelE")]
    mips = {n: k for n, k in numbers.items() if n.startswith("_ZN4atmo25atmo_sky_image_mip_kernelILi")}
    assert {n[len("_ZN4atmo25atmo_sky_image_mip_kernel"):].split("EE")[0] + "EE" for n in mips} == {f"ILi{f}EE" for f in (0, 1, 2, 16, 17, 18, 19)}
    for name, k in [(resolve, numbers[resolve])] + list(mips.items()):
        print(name, k, "LDS", lds[name])
        assert k["scratch"] == 0 and k["spill_reads"] == 0, name
    text = open(os.path.join(ROOT, "include", "atmo_sky_image.h")).read()
    assert lds[resolve] == 0 and f"{numbers[resolve]['vgprs']} VGPRs, no LDS, no private-memory stack" in text
    assert {lds[n] for n in mips} == {5120} and f"at most {max(k['vgprs'] for k in mips.values())} VGPRs, 5120 bytes of LDS, no stack" in text

    def base(mangled):     # _ZN4atmo<length><name>...
        m = re.match(r"_ZN4atmo(\d+)", mangled)
        return mangled[m.end():m.end() + int(m.group(1))] if m else mangled

    names = {base(n) for n in numbers}
    new_names = {"atmo_sky_image_resolve_kernel", "atmo_sky_image_mip_kernel"}
    assert new_names <= names
    for a in new_names:
        for b in names - {a}:
            assert a not in b and b not in a, (a, b)
