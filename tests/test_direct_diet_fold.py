"""The power-of-two folding in sun_od_direct<8> (csrc/atmo_kernels.hip), emulated in float32 on the CPU: the old and the new order of the expressions give
the same bits -- the squared distances q[1..7] that feed the seven roots and the final acc * step * density^2 -- on the chosen inputs of
tests/golden/direct_diet and on 10^6 random ones.

fp32 products are formed exactly in float64 (24 + 24 <= 53 bits) and rounded once; an fp32 FMA is the exact float64 product plus the addend by TwoSum,
rounded to odd at 53 bits and then to nearest at 24 (53 >= 2 * 24 + 2: the double rounding is innocuous), so float64 is used only where it is exact."""
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_diet")
sys.path.insert(0, GOLDEN)
import direct_diet_cases as DC  # noqa: E402

f32, f64 = np.float32, np.float64


def mul(a, b):
    return (a.astype(f64) * b.astype(f64)).astype(f32)


def add(a, b):
    return (a.astype(f64) + b.astype(f64)).astype(f32)   # rounded at 53 bits, then at 24: innocuous for a sum of two fp32 numbers (53 >= 2 * 24 + 2)


def fma(a, b, c):
    p = a.astype(f64) * b.astype(f64)   # exact
    c = c.astype(f64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)       # TwoSum: p + c = s + e exactly
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where((e != 0) & even, np.nextafter(s, toward), s)   # round to odd
    return s.astype(f32)


def fmax0(x):
    """v_max_f32(x, 0): a NaN gives 0, -0 gives +0"""
    return np.where(x > 0, x, f32(0.0)).astype(f32)


def chord(r2, bdot, ratm2, clamp_hh):
    """ray_len of sun_od_direct from hh = R_atm^2 - (r2 - bdot^2); clamp_hh=False: the root of a negative hh is NaN (and of -0.0 is -0.0)."""
    hh = add(ratm2, -fma(-bdot, bdot, r2))
    return chord_of_hh(hh, bdot, clamp_hh)


def chord_of_hh(hh, bdot, clamp_hh):
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(fmax0(hh) if clamp_hh else hh).astype(f32)
        return fmax0(np.fmin(add(sq, sq), add(sq, -bdot)))


def old_form(ray_len, r2, bdot, acc, dens2):
    lstep = mul(ray_len, np.full_like(ray_len, 0.125))
    lb, l2 = mul(lstep, add(bdot, bdot)), mul(lstep, lstep)
    q = [fma(np.full_like(l2, j * j), l2, fma(np.full_like(lb, j), lb, r2)) for j in range(1, 8)]
    return q, mul(mul(acc, lstep), dens2)


def new_form(ray_len, r2, bdot, acc, dens2):
    m, l2 = mul(ray_len, bdot), mul(ray_len, ray_len)
    q = [fma(np.full_like(l2, j * j / 64.0), l2, fma(np.full_like(m, j / 4.0), m, r2)) for j in range(1, 8)]
    return q, mul(mul(acc, ray_len), mul(dens2, np.full_like(dens2, 0.125)))


def bits(x):
    return x.view(np.uint32)


def check(r2, bdot, acc, ratm2, dens2, what):
    ratm2, dens2 = np.full_like(r2, ratm2), np.full_like(r2, dens2)
    old_len, new_len = chord(r2, bdot, ratm2, True), chord(r2, bdot, ratm2, False)
    assert np.array_equal(bits(old_len), bits(new_len)), f"{what}: the chord without the clamp in front of the root"
    qo, fo = old_form(old_len, r2, bdot, acc, dens2)
    qn, fn = new_form(new_len, r2, bdot, acc, dens2)
    for j in range(7):
        bad = bits(qo[j]) != bits(qn[j])
        assert not bad.any(), f"{what}: q[{j + 1}] differs at {int(np.argmax(bad))}: r2 {r2[bad][0]!r} bdot {bdot[bad][0]!r} chord {old_len[bad][0]!r}"
    bad = bits(fo) != bits(fn)
    assert not bad.any(), f"{what}: acc * step * density^2 differs at {int(np.argmax(bad))}: acc {acc[bad][0]!r} chord {old_len[bad][0]!r}"
    return old_len


def probe_inputs(radius, height):
    """r2, bdot as the probe kernel forms them from light_inputs (fused sums, left to right), and R_atm^2"""
    pos, sun = DC.light_inputs(radius, height)
    x, y, z = (np.ascontiguousarray(pos[:, i]) for i in range(3))
    sx, sy, sz = (np.ascontiguousarray(sun[:, i]) for i in range(3))
    r2 = fma(z, z, fma(y, y, mul(x, x)))
    bdot = fma(z, sz, fma(y, sy, mul(x, sx)))
    ratm = f32(radius) + f32(height)
    return r2, bdot, f32(ratm * ratm)


def test_fma_emulation_rounds_once():
    """cases where a float64 sum rounded again would be wrong: a product a hair above / below the midpoint of two fp32 neighbours of the addend"""
    one, eps = f32(1.0), f32(2.0 ** -24)
    a = np.array([eps, eps, -eps, 2.0 ** -60], dtype=f32)
    b = np.array([1.0 + 2.0 ** -23, 1.0, 1.0 + 2.0 ** -23, 2.0 ** -60], dtype=f32)
    c = np.array([one, one, one + f32(2.0 ** -23), one + f32(2.0 ** -23) + 0], dtype=f32)
    got = fma(a, b, c)
    want = np.array([1.0 + 2.0 ** -23, 1.0, 1.0, 1.0 + 2.0 ** -23], dtype=f32)   # above the tie: up; the tie: to even; below the tie from above: down; tiny: unchanged
    assert np.array_equal(bits(got), bits(want)), (got, want)


def test_folding_keeps_the_bits_on_the_chosen_inputs():
    rng = np.random.default_rng(7)
    for radius, height in ((100.0, 8.0), (DC.SMALL_PLANET["u_planet_radius"], DC.SMALL_PLANET["u_atmosphere_height"])):
        r2, bdot, ratm2 = probe_inputs(radius, height)
        acc = rng.uniform(0.0, 8.0, size=r2.shape).astype(f32)
        acc[::5] = rng.uniform(0.0, 1.0, size=acc[::5].shape).astype(f32) ** 12   # a sample at the top of the shell: y^3 of a tiny y
        lens = check(r2, bdot, acc, ratm2, f32(1e-3) ** 2, f"radius {radius}")
        assert (lens == 0).any() and (lens > 0).any()
    # the planet of radius 2^-45 is there for this: squared chords in the subnormal range, every one far below half an ulp of r2 >= R^2
    sub = (lens > 0) & (mul(lens, lens) < f32(2.0 ** -126))
    assert sub.sum() >= 16, int(sub.sum())


def test_chord_without_the_clamp_for_signed_zero_and_negative_hh():
    """hh = -0.0 cannot come out of R_atm^2 - (...) under round-to-nearest; fed in directly it must still give the clamped form's chord, like every hh < 0"""
    hh = np.array([-0.0, -0.0, 0.0, 0.0, -1e-3, -1e-3, -np.inf, np.nan, 2.0 ** -149, 1e-3], dtype=f32)
    bd = np.array([3.0, -3.0, 3.0, -3.0, 3.0, -3.0, -1.0, -1.0, -1.0, 1e-30], dtype=f32)
    a, b = chord_of_hh(hh, bd, True), chord_of_hh(hh, bd, False)
    assert np.array_equal(bits(a), bits(b)), (a, b)


def test_folding_keeps_the_bits_on_a_million_random_inputs():
    rng = np.random.default_rng(11)
    n = 1_000_000
    R, top = 100.0, 108.0
    r = rng.uniform(R * 0.995, top * 1.002, size=n)
    k = n // 4
    r[:k] = rng.uniform(top, top * 1.002, size=k)   # hh = R_atm^2 - r2 + bdot^2 reaches 0 only from outside the shell
    cosang = rng.uniform(-1.0, 1.0, size=n)
    r2 = (r * r).astype(f32)
    bdot = (r * cosang).astype(f32)
    # a quarter of them near the tangent: hh around 0 with either sign, chords down to their smallest values
    bdot[:k] = (np.sqrt(np.maximum(r2[:k].astype(f64) - top * top, 0.0)) * rng.choice([-1.0, 1.0], size=k) * (1.0 + rng.normal(size=k) * 1e-6)).astype(f32)
    acc = rng.uniform(0.0, 8.0, size=n).astype(f32)
    check(r2, bdot, acc, f32(top * top), f32(1e-3) ** 2, "random")
