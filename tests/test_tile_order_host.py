"""CPU tests of the tile-order sort's host side: the class rule of the numpy reference (tests/tile_order_ref.py) against a table worked by hand, the
library's heavy_tile_count (atmo_debug_heavy_tile_count) against its float64 restatement, and the three statements of one rule -- tile_cost_class's
classes, the class midpoints inside heavy_tile_count, sharding.heavy_tiles on exact costs -- against each other."""
import ctypes as C

import numpy as np
import pytest

import tile_order_ref as R
from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import sharding

NC = 64   # the library's class count (csrc/atmo_device.h, TILE_ORDER_CLASSES); test_library_states_its_class_count holds the library to it,
          # and the reference states the heavy-tile rule for this count only
WAVES, TRIGGERS, RATIOS = (64, 512, 6144), (0.0, 1.0, 2.0), (0.1, 0.3, 0.5)


def _heavy(totals, n_tiles, ratio, trigger, waves, n_classes=None):
    t = np.ascontiguousarray(totals, dtype=np.uint32)
    return N.load().atmo_debug_heavy_tile_count(t.ctypes.data_as(C.c_void_p), t.size if n_classes is None else n_classes, int(n_tiles),
                                                float(ratio), float(trigger), int(waves))


def test_symbols_are_diagnostics():
    assert "atmo_debug_tile_order" in N.DEBUG_SYMBOLS and "atmo_debug_heavy_tile_count" in N.DEBUG_SYMBOLS
    assert not {"atmo_debug_tile_order", "atmo_debug_heavy_tile_count"} & set(N.CORE_SYMBOLS)


def test_cost_class_table_for_64_classes():
    """The kernel's stated rule, worked by hand."""
    table = {0: 63, 1: 63, 2: 63, 3: 63, 255: 63, 256: 63, 319: 63, 320: 62, 14_680_063: 1, 14_680_064: 0, 2 ** 24: 0, 2 ** 32 - 1: 0}
    costs = np.array(list(table), dtype=np.uint32)
    assert R.cost_class(costs, 64).tolist() == list(table.values())
    for c, k in table.items():   # one at a time as well: scalars take the same path
        assert int(R.cost_class(np.uint32(c), 64)) == k, c


@pytest.mark.parametrize("n_classes", [32, 64])
def test_cost_class_is_monotone_and_its_boundaries_are_where_the_helpers_say(n_classes):
    """Class k starts at class_floor(k); one below lies in class k + 1; the midpoint lies in the class; a heavier tile is never in a lighter class."""
    for k in range(n_classes - 1):
        lo = R.class_floor(k, n_classes)
        assert int(R.cost_class(np.uint32(lo), n_classes)) == k
        assert int(R.cost_class(np.uint32(lo - 1), n_classes)) == k + 1
        assert int(R.cost_class(np.uint32(R.class_midpoint(k, n_classes)), n_classes)) == k
    first, last = {64: (320, 14_680_064), 32: (384, 12_582_912)}[n_classes]   # 256 x 1.25, 2^23 x 1.75; 256 x 1.5, 2^23 x 1.5
    assert R.class_floor(n_classes - 2, n_classes) == first and R.class_floor(0, n_classes) == last
    rng = np.random.default_rng(11)
    c = np.sort((2.0 ** rng.uniform(0, 32, 4000)).astype(np.uint64).astype(np.uint32))
    assert np.all(np.diff(R.cost_class(c, n_classes)) <= 0)
    # the top-bit index: every power of two and its neighbours, exactly
    for b in range(32):
        assert int(R.top_bit(np.uint32(1 << b))) == b and int(R.top_bit(np.uint32((1 << (b + 1)) - 1))) == b


def test_dilate_is_the_box_maximum():
    """The reference's separable running maximum against the definition, evaluated tile by tile."""
    rng = np.random.default_rng(3)
    for ty, tx in ((1, 7), (5, 9), (13, 4)):
        a = rng.integers(0, 2 ** 32, (ty, tx), dtype=np.uint32)
        for rx, ry in ((0, 0), (1, 0), (0, 1), (2, 3), (64, 64)):
            want = np.array([[a[max(y - ry, 0):y + ry + 1, max(x - rx, 0):x + rx + 1].max() for x in range(tx)] for y in range(ty)], dtype=np.uint32)
            assert np.array_equal(R.dilate(a, rx, ry), want), (ty, tx, rx, ry)


def test_reference_order_on_a_case_worked_by_hand():
    # 3 x 2 tiles: classes (64) of 0, 330, 2^24, 330, 300, 2^24 are 63, 62, 0, 62, 63, 0
    cost = np.array([[0, 330, 2 ** 24], [330, 300, 2 ** 24]], dtype=np.uint32)
    order, order2, totals, after = R.tile_order(cost, 0, 0, 64)
    assert order.tolist() == [2, 5, 1, 3, 0, 4]
    assert order2.tolist() == [2, 5, 8, 11, 1, 4, 6, 9, 0, 3, 7, 10]
    assert totals[0] == 2 and totals[62] == 2 and totals[63] == 2 and totals.sum() == 6 and not after.any()
    # one tile of reach along x: the heavy column reaches the middle one; the totals stay those of the measured costs
    order, _, totals_d, _ = R.tile_order(cost, 1, 0, 64)
    assert order.tolist() == [1, 2, 4, 5, 0, 3] and np.array_equal(totals_d, totals)


def test_library_states_its_class_count():
    assert _heavy(np.zeros(NC, np.uint32), 0, 0.3, 2.0, 6144) == 0
    for wrong in (NC // 2, NC * 2, 0, -1):
        assert _heavy(np.zeros(max(wrong, 1), np.uint32), 0, 0.3, 2.0, 6144, n_classes=wrong) == -N.ATMO_E_ARG
        assert b"atmo_debug_heavy_tile_count" in N.load().atmo_last_error_string(None)
    assert N.load().atmo_debug_heavy_tile_count(None, NC, 0, 0.3, 2.0, 6144) == -N.ATMO_E_ARG
    assert _heavy(np.zeros(NC, np.uint32), 0, 0.3, 2.0, 0) == -N.ATMO_E_ARG


def test_heavy_tile_count_equals_its_restatement_on_random_histograms():
    rng = np.random.default_rng(20240)
    nonzero = 0
    for i in range(2000):
        totals = np.zeros(NC, dtype=np.uint32)
        kind = i % 4
        if kind == 0:      # a few heavy tiles over a light bulk, the shape the rule was made for
            totals[rng.integers(NC // 2, NC)] = rng.integers(100, 20000)
            totals[rng.integers(0, NC // 2, 3)] += rng.integers(1, 40, 3).astype(np.uint32)
        elif kind == 1:    # anything anywhere
            totals[:] = rng.integers(0, 300, NC) * (rng.random(NC) < 0.3)
        elif kind == 2:    # neighbouring classes around the thresholds
            k = int(rng.integers(0, NC - 6))
            totals[k:k + 6] = rng.integers(0, 50, 6)
            totals[NC - 1] = rng.integers(0, 20000)
        else:              # two classes
            totals[rng.integers(0, NC, 2)] = rng.integers(1, 5000, 2)
        n_tiles = int(totals.sum())
        waves, trigger, ratio = int(rng.choice(WAVES)), float(rng.choice(TRIGGERS)), float(rng.choice(RATIOS))
        got, want = _heavy(totals, n_tiles, ratio, trigger, waves), R.heavy_tile_count(totals, n_tiles, ratio, trigger, waves)
        assert got == want, (i, totals.tolist(), waves, trigger, ratio)
        nonzero += got > 0
    assert nonzero >= 500, nonzero   # not a comparison of zeros


def test_heavy_tile_count_edges():
    totals = np.zeros(NC, dtype=np.uint32)
    totals[5], totals[50] = 4, 8000
    n = 8004
    full = _heavy(totals, n, 0.3, 2.0, 6144)
    assert full == 4 == R.heavy_tile_count(totals, n, 0.3, 2.0, 6144)
    # totals that are not this grid's histogram
    for wrong in (n - 1, n + 1, 0, 2 * n):
        assert _heavy(totals, wrong, 0.3, 2.0, 6144) == 0 == R.heavy_tile_count(totals, wrong, 0.3, 2.0, 6144)
    # everything in the last class: no measurement, no draw estimate
    last = np.zeros(NC, dtype=np.uint32)
    last[NC - 1] = 16200
    for trigger in TRIGGERS:
        assert _heavy(last, 16200, 0.3, trigger, 6144) == 0 == R.heavy_tile_count(last, 16200, 0.3, trigger, 6144)
    # the cap: one class only, every tile outlives ratio x the draw on 6144 waves, a third is split
    one = np.zeros(NC, dtype=np.uint32)
    one[10] = 1000
    assert _heavy(one, 1000, 0.3, 2.0, 6144) == 1000 // 3 == R.heavy_tile_count(one, 1000, 0.3, 2.0, 6144)
    one[10] = 1001
    assert _heavy(one, 1001, 0.3, 2.0, 6144) == 333
    one[10] = 2
    assert _heavy(one, 2, 0.3, 2.0, 6144) == 0   # a third of two tiles
    # trigger = 0, the forced mode: a flat frame that trigger = 2 leaves alone is split wherever a class outlives ratio x the draw
    flat = np.zeros(NC, dtype=np.uint32)
    flat[20], flat[21] = 30000, 30000
    assert _heavy(flat, 60000, 0.1, 2.0, 64) == 0 == R.heavy_tile_count(flat, 60000, 0.1, 2.0, 64)
    flat[:] = 0
    flat[20], flat[40] = 30, 3000
    # (class 20 lives 491 520 cycles, class 40 15 360: the draw on 128 waves is 950 400, so class 20 outlives 0.3 x but not 2 x the draw)
    assert _heavy(flat, 3030, 0.3, 2.0, 128) == 0 == R.heavy_tile_count(flat, 3030, 0.3, 2.0, 128)
    assert _heavy(flat, 3030, 0.3, 0.0, 128) == 30 == R.heavy_tile_count(flat, 3030, 0.3, 0.0, 128)


def test_three_statements_of_the_heavy_rule_agree():
    """Costs that sit exactly on the class midpoints of classes 1 .. NC - 2 (integers: 352 for class NC - 2, the middle of 320 .. 383, upwards): the histogram of their classes through the
    library's rule == sharding.heavy_tiles on the costs themselves.  Every sum here is an integer below 2^53, so both are exact and no tolerance applies."""
    mids = np.array([R.class_midpoint(k, NC) for k in range(NC)], dtype=np.int64)
    assert mids[NC - 2] == 352 and np.array_equal(R.cost_class(mids[1:NC - 1].astype(np.uint32), NC), np.arange(1, NC - 1))
    rng = np.random.default_rng(77)
    nonzero = 0
    cases = 2000
    for i in range(cases):
        n = int(rng.integers(3, 4000))
        light = int(rng.integers(20, NC - 1))                      # the bulk: classes light .. NC - 2
        classes = rng.integers(light, NC - 1, n)
        n_heavy = int(rng.integers(0, 12))
        if n_heavy:
            classes[rng.integers(0, n, n_heavy)] = rng.integers(1, light + 1, n_heavy)
        costs = mids[classes]
        assert costs.min() >= 352
        waves, trigger, ratio = int(rng.choice(WAVES)), float(np.float32(rng.choice(TRIGGERS))), float(np.float32(rng.choice(RATIOS)))
        totals = np.bincount(R.cost_class(costs.astype(np.uint32), NC), minlength=NC)
        got = _heavy(totals, n, ratio, trigger, waves)
        want = sharding.heavy_tiles(np.sort(costs)[::-1], resident_waves=waves, trigger=trigger, ratio=ratio)
        assert got == want, (i, n, waves, trigger, ratio, totals.tolist())
        assert got == R.heavy_tile_count(totals, n, ratio, trigger, waves)
        nonzero += got > 0
    assert 4 * nonzero >= cases, nonzero
