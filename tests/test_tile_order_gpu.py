"""The tile-order sort (csrc/atmo_kernels.hip: launch_tile_order -- dilation, class totals, histogram, scan, scatter) on known costs, through
atmo_debug_tile_order, against the numpy statement in tests/tile_order_ref.py.  A stable sort by class has one result: every comparison is for equality.
The library fills every buffer the sort sees with 0xFFFFFFFF first, so an entry no kernel wrote shows as that value.

The grids are chosen for the kernels' edges: 256 single-wave workgroups own chunks of ceil(n / 256) tiles and walk them 64 at a time, so up to 16 384 tiles
every workgroup's loop runs once, and the class offsets carried from one trip to the next matter only beyond."""
import ctypes as C

import numpy as np
import pytest

import tile_order_ref as R
from godot_atmosphere_shader_amd import _native as N

pytestmark = pytest.mark.gpu

# The sort's workgroup count: a copy of ORDER_BLOCKS in csrc/atmo_kernels.hip, which the library does not export.  It places the heavy tiles at a chunk boundary
# and decides which grids lie either side of the scatter loop's second trip (64 * ORDER_BLOCKS tiles): if the kernels' constant changes, change this one and
# the grids (128, 128) / (145, 113) with it -- the tests would still pass, but no longer at those edges.
ORDER_BLOCKS = 256
FILL = 0xA5A5A5A5   # what the caller's output arrays hold before a call
GRIDS = [(1, 1), (1, 7), (7, 1),                                   # one tile per workgroup, most workgroups empty
         (63, 1), (64, 1), (65, 1), (16, 16), (257, 1),            # around one wave; 256 tiles: chunk 1 in every workgroup; the first chunk of 2
         (120, 135),                                               # 1920 x 1080: chunk 64, exactly one trip
         (128, 128), (145, 113),                                   # 16 384: the last one-trip size; 16 385: the second trip holds one tile
         (240, 270),                                               # 3840 x 2160: chunk 254, four trips, the last partial
         (240, 540),                                               # the two-lane grid at that size
         (129600, 1)]                                              # a view batch's single row: sorted without order2 and without class totals
DILATE_GRIDS = [(7, 1), (65, 1), (120, 135), (145, 113), (240, 270)]
RADII = [(1, 0), (0, 1), (1, 1), (4, 4), (5, 4), (10, 10), (3, 6), (64, 64)]   # (4, 4): the last one-pass window; (5, 4): the first separable one


def _is_batch_row(grid):
    return grid == (129600, 1)


@pytest.fixture(scope="module")
def ctx():
    lib = N.load()
    c = C.c_void_p()
    assert lib.atmo_create(0, N.VARIANT_NO_CLOUDS, 8, 0, N.LIGHT_LUT, 0, C.byref(c)) == N.ATMO_OK, lib.atmo_last_error_string(None)   # "no_clouds_8"
    yield c
    lib.atmo_destroy(c)


@pytest.fixture(scope="module")
def n_classes(ctx):
    nc = C.c_int(0)
    cost, order = np.zeros(1, dtype=np.uint32), np.full(1, FILL, dtype=np.uint32)
    assert N.load().atmo_debug_tile_order(ctx, cost.ctypes.data_as(C.c_void_p), 1, 1, 0, 0, order.ctypes.data_as(C.c_void_p), None, None, None, C.byref(nc)) == N.ATMO_OK
    assert nc.value in (32, 64)
    return nc.value


def _sort(ctx, cost2d, rx=0, ry=0, with_order2=True, with_totals=True):
    """The library's sort of a (tiles_y, tiles_x) cost map: (order, order2 or None, class_totals or None, cost_after, n_classes)."""
    lib = N.load()
    ty, tx = cost2d.shape
    cost = np.ascontiguousarray(cost2d, dtype=np.uint32).ravel()
    n = cost.size
    order, order2 = np.full(n, FILL, dtype=np.uint32), np.full(2 * n, FILL, dtype=np.uint32)
    totals, after = np.full(64, FILL, dtype=np.uint32), np.full(n, FILL, dtype=np.uint32)
    nc = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.atmo_debug_tile_order(ctx, p(cost), tx, ty, rx, ry, p(order), p(order2) if with_order2 else None, p(totals) if with_totals else None, p(after), C.byref(nc))
    assert rc == N.ATMO_OK, lib.atmo_last_error_string(ctx)
    assert np.all(totals[nc.value:] == FILL)
    if not with_order2:
        assert np.all(order2 == FILL)
    if not with_totals:
        assert np.all(totals == FILL)
    return order, (order2 if with_order2 else None), (totals[:nc.value].copy() if with_totals else None), after, nc.value


def _check(ctx, cost2d, rx=0, ry=0, batch_row=False, what=""):
    """One sort against the reference: order, order2, class totals, the cleared cost map."""
    order, order2, totals, after, nc = _sort(ctx, cost2d, rx, ry, with_order2=not batch_row, with_totals=not batch_row)
    want_order, want_order2, want_totals, want_after = R.tile_order(cost2d, rx, ry, nc)
    n = cost2d.size
    where = (what, cost2d.shape[::-1], rx, ry)
    assert not np.any(order == R.POISON), ("entries of the order that no kernel wrote", np.flatnonzero(order == R.POISON)[:8], where)
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), ("the order is not a permutation of the tiles", where)
    if not np.array_equal(order, want_order):
        bad = np.flatnonzero(order != want_order)
        raise AssertionError(("the order differs from the stable sort by class", where, f"{bad.size} positions, first {bad[:4]}",
                              "got", order[bad[:4]], "want", want_order[bad[:4]]))
    if order2 is not None:
        assert np.array_equal(order2, want_order2), ("order2", where, np.flatnonzero(order2 != want_order2)[:8])
    if totals is not None:
        assert int(totals.astype(np.int64).sum()) == n and np.array_equal(totals, want_totals), ("class totals", where, totals, want_totals)
    assert np.array_equal(after, want_after), ("the cost map is not cleared", where, np.flatnonzero(after)[:8])
    return want_totals


def _shape(cost, grid):
    tx, ty = grid
    return np.ascontiguousarray(np.asarray(cost, dtype=np.uint32).reshape(ty, tx))


def _random_costs(n, seed):
    """2 ** uniform(0, 32): every class, the clipped ends included; a tenth of the tiles without a measurement."""
    rng = np.random.default_rng(seed)
    c = np.minimum(np.floor(2.0 ** rng.uniform(0.0, 32.0, n)), 2.0 ** 32 - 1).astype(np.uint64).astype(np.uint32)
    c[rng.random(n) < 0.1] = 0
    return c


def _class_cost(k, nc):
    """A cost of class k: its middle; the last class's own tiles have no measurement."""
    return 0 if k == nc - 1 else R.class_midpoint(k, nc)


def _chunk(n):
    return (n + ORDER_BLOCKS - 1) // ORDER_BLOCKS


def _one_heavy(n, at):
    c = np.full(n, 300, dtype=np.uint32)   # light: the last class
    c[at] = 1 << 20
    return c


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
class TestPatterns:
    def test_random_costs_over_all_classes(self, ctx, n_classes, grid):
        n = grid[0] * grid[1]
        cost = _random_costs(n, seed=1000 + n)
        if n >= 16200:   # the pattern does reach every class
            assert np.all(np.bincount(R.cost_class(cost, n_classes), minlength=n_classes) > 0)
        _check(ctx, _shape(cost, grid), batch_row=_is_batch_row(grid), what="random")

    def test_equal_costs_keep_the_row_major_order(self, ctx, n_classes, grid):
        """Stability: one class, the order is the identity, and the totals sit in that class."""
        n = grid[0] * grid[1]
        for value in (5000, 0, 0xFFFFFFFF):
            cost2d = _shape(np.full(n, value, dtype=np.uint32), grid)
            order, _, totals, _, _ = _sort(ctx, cost2d, with_order2=not _is_batch_row(grid), with_totals=not _is_batch_row(grid))
            assert np.array_equal(order, np.arange(n, dtype=np.uint32)), value
            if totals is not None:
                k = int(R.cost_class(np.uint32(value), n_classes))
                assert totals[k] == n and int(totals.astype(np.int64).sum()) == n, value
            _check(ctx, cost2d, batch_row=_is_batch_row(grid), what=f"all {value}")

    def test_every_class_boundary(self, ctx, n_classes, grid):
        """For every leading bit and every sub-step of the octave: the boundary value and the value one below it, tiled over the grid."""
        p = n_classes // 16
        bits = p.bit_length() - 1
        values = []
        for msb in range(32):
            for sub in range(p if msb >= bits else 1):
                b = (1 << msb) + (sub << (msb - bits) if msb >= bits else 0)
                values += [b, b - 1]
        values = np.array(values, dtype=np.uint32)
        assert len(np.unique(R.cost_class(values, n_classes))) == n_classes
        n = grid[0] * grid[1]
        _check(ctx, _shape(np.resize(values, n), grid), batch_row=_is_batch_row(grid), what="boundaries")

    def test_all_classes_in_one_wave(self, ctx, n_classes, grid):
        """n_classes consecutive tiles of n_classes different classes, repeated; and the same backwards."""
        n = grid[0] * grid[1]
        run = np.array([_class_cost(k, n_classes) for k in range(n_classes)], dtype=np.uint32)
        assert np.array_equal(R.cost_class(run, n_classes), np.arange(n_classes))
        _check(ctx, _shape(np.resize(run, n), grid), batch_row=_is_batch_row(grid), what="classes ascending")
        _check(ctx, _shape(np.resize(run[::-1], n), grid), batch_row=_is_batch_row(grid), what="classes descending")

    def test_classes_that_differ_in_one_key_bit(self, ctx, n_classes, grid):
        """Two classes k and k ^ (1 << b) alternating tile by tile, for every bit b of the class index: a wrong ballot for one bit merges exactly these."""
        n = grid[0] * grid[1]
        for b in range(n_classes.bit_length() - 1):
            for k in (0, 0x15 & (n_classes - 1)):
                pair = np.array([_class_cost(k, n_classes), _class_cost(k ^ (1 << b), n_classes)], dtype=np.uint32)
                assert R.cost_class(pair, n_classes).tolist() == [k, k ^ (1 << b)]
                _check(ctx, _shape(np.resize(pair, n), grid), batch_row=_is_batch_row(grid), what=f"classes {k} and {k ^ (1 << b)}")

    def test_one_heavy_tile(self, ctx, n_classes, grid):
        """A single heavy tile among light ones: the first tile, the last, and either side of the first chunk boundary."""
        n = grid[0] * grid[1]
        for at in sorted({0, n - 1, min(_chunk(n) - 1, n - 1), min(_chunk(n), n - 1)}):
            cost2d = _shape(_one_heavy(n, at), grid)
            order, _, _, _, _ = _sort(ctx, cost2d, with_order2=not _is_batch_row(grid), with_totals=not _is_batch_row(grid))
            assert order[0] == at
            _check(ctx, cost2d, batch_row=_is_batch_row(grid), what=f"heavy tile at {at}")

    def test_sorted_costs(self, ctx, n_classes, grid):
        n = grid[0] * grid[1]
        cost = np.sort(_random_costs(n, seed=2000 + n))
        _check(ctx, _shape(cost, grid), batch_row=_is_batch_row(grid), what="ascending")
        _check(ctx, _shape(cost[::-1], grid), batch_row=_is_batch_row(grid), what="descending")


@pytest.mark.parametrize("radii", RADII, ids=lambda r: f"r{r[0]}x{r[1]}")
@pytest.mark.parametrize("grid", DILATE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_dilated_key(ctx, n_classes, grid, radii):
    """The order follows the box maximum of the costs, the class totals the costs themselves."""
    rx, ry = radii
    n = grid[0] * grid[1]
    _check(ctx, _shape(_random_costs(n, seed=3000 + n), grid), rx, ry, what="random")
    for at in sorted({0, n - 1, min(_chunk(n) - 1, n - 1), min(_chunk(n), n - 1)}):
        _check(ctx, _shape(_one_heavy(n, at), grid), rx, ry, what=f"heavy tile at {at}")


@pytest.mark.parametrize("radii", [(4, 4), (5, 4)], ids=lambda r: f"r{r[0]}x{r[1]}")
def test_class_totals_are_of_the_undilated_costs(ctx, n_classes, radii):
    """One heavy tile in the middle of light ones: the dilated key holds a whole window of heavy tiles, the measured costs one.  The two histograms differ
    (asserted on the reference), so class totals taken from the key fail here -- on either side of the switch between the one-pass and the separable window."""
    rx, ry = radii
    grid = (120, 135)
    n = grid[0] * grid[1]
    cost2d = _shape(_one_heavy(n, 67 * 120 + 60), grid)
    heavy, light = int(R.cost_class(np.uint32(1 << 20), n_classes)), n_classes - 1
    of_costs = np.bincount(R.cost_class(cost2d.ravel(), n_classes), minlength=n_classes)
    of_key = np.bincount(R.cost_class(R.dilate(cost2d, rx, ry).ravel(), n_classes), minlength=n_classes)
    window = (2 * rx + 1) * (2 * ry + 1)
    assert of_costs[heavy] == 1 and of_costs[light] == n - 1 and of_key[heavy] == window and of_key[light] == n - window
    order, _, totals, _, _ = _sort(ctx, cost2d, rx, ry)
    assert np.array_equal(totals, of_costs) and not np.array_equal(totals, of_key)
    assert np.array_equal(np.sort(order[:window]), np.sort(np.flatnonzero(R.dilate(cost2d, rx, ry).ravel() == 1 << 20)))   # the window leads the order
    _check(ctx, cost2d, rx, ry, what="heavy tile in the middle")


def test_bad_arguments_are_refused_and_write_nothing(ctx, n_classes):
    lib = N.load()
    big_x, big_y = 4096, 1025   # 2^22 + 4096 tiles: the arrays are that large, so that the refusal is not what keeps the call in bounds
    cost = np.full(big_x * big_y, 300, dtype=np.uint32)
    order, order2 = np.full(big_x * big_y, FILL, dtype=np.uint32), np.full(64, FILL, dtype=np.uint32)
    totals, after = np.full(64, FILL, dtype=np.uint32), np.full(64, FILL, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cases = {
        "NULL cost": (None, 4, 4, 0, 0, p(order)),
        "NULL order_out": (p(cost), 4, 4, 0, 0, None),
        "tiles_x = 0": (p(cost), 0, 4, 0, 0, p(order)),
        "tiles_y = 0": (p(cost), 4, 0, 0, 0, p(order)),
        "tiles_x < 0": (p(cost), -4, 4, 0, 0, p(order)),
        "tiles_y < 0": (p(cost), 4, -4, 0, 0, p(order)),
        "both negative": (p(cost), -4, -4, 0, 0, p(order)),
        "more than 2^22 tiles": (p(cost), big_x, big_y, 0, 0, p(order)),
        "a product beyond int": (p(cost), 1 << 16, 1 << 16, 0, 0, p(order)),
        "rx < 0": (p(cost), 4, 4, -1, 0, p(order)),
        "ry < 0": (p(cost), 4, 4, 0, -1, p(order)),
        "rx > 64": (p(cost), 4, 4, 65, 0, p(order)),
        "ry > 64": (p(cost), 4, 4, 0, 65, p(order)),
    }
    for what, (c, tx, ty, rx, ry, o) in cases.items():
        nc = C.c_int(-7)
        # order2 / totals / cost_after of 64 entries suffice for the 4 x 4 grids; the oversized grid is called without them
        small = tx * ty <= 16
        rc = lib.atmo_debug_tile_order(ctx, c, tx, ty, rx, ry, o, p(order2) if small else None, p(totals) if small else None, p(after) if small else None, C.byref(nc))
        assert rc == N.ATMO_E_ARG, what
        assert b"atmo_debug_tile_order" in lib.atmo_last_error_string(ctx), what
        assert np.all(order == FILL) and np.all(order2 == FILL) and np.all(totals == FILL) and np.all(after == FILL) and nc.value == -7, what
        assert np.all(cost[:64] == 300), what
    assert lib.atmo_debug_tile_order(None, p(cost), 4, 4, 0, 0, p(order), None, None, None, None) == N.ATMO_E_ARG
    # 2^22 tiles exactly is the largest grid the call accepts: the limit is inclusive
    nc = C.c_int(0)
    assert lib.atmo_debug_tile_order(ctx, p(cost), 4096, 1024, 0, 0, p(order), None, None, None, C.byref(nc)) == N.ATMO_OK, lib.atmo_last_error_string(ctx)
    assert nc.value == n_classes and np.array_equal(order[:1 << 22], np.arange(1 << 22, dtype=np.uint32)) and np.all(order[1 << 22:] == FILL)
