"""The tile-order sort and the heavy-tile rule restated in numpy, from the comments in front of the kernels (csrc/atmo_kernels.hip: tile_cost_class,
the histogram / scan / scatter kernels, the dilation, the class totals) and of heavy_tile_count (csrc/atmo_api.hip) -- not from their code.  Integer
arithmetic throughout the sort; float64 in the heavy-tile rule, as the C function.

A stable sort by class has exactly one result, so tests compare with these functions for equality."""
import numpy as np

POISON = 0xFFFFFFFF


def _log2_exact(n):
    k = int(n).bit_length() - 1
    if n < 1 or (1 << k) != n:
        raise ValueError(f"{n} is not a power of two")
    return k


def top_bit(cost):
    """Index of the leading one of every non-zero uint32 (0 for 0).  float64 holds a uint32 exactly, so frexp's exponent is exact."""
    c = np.asarray(cost, dtype=np.uint64)
    if c.size and int(c.max()) > 0xFFFFFFFF:
        raise ValueError("costs are uint32")
    _, e = np.frexp(c.astype(np.float64))
    return np.where(c == 0, 0, e.astype(np.int64) - 1)


def cost_class(cost, n_classes):
    """Class 0 is the heaviest.  16 octaves of the cost, 2^8 .. 2^24, in P = n_classes / 16 equal parts each: q = msb * P + sub - 8 * P with sub the
    log2(P) bits below the leading one (0 where the value has not that many), clipped to the classes; zero (no measurement) goes to the last class."""
    p = n_classes // 16
    if p * 16 != n_classes:
        raise ValueError("n_classes must be a multiple of 16")
    bits = _log2_exact(p)
    c = np.asarray(cost, dtype=np.uint64).astype(np.int64)
    msb = top_bit(cost)
    shift = np.maximum(msb - bits, 0)
    sub = np.where(msb >= bits, (c >> shift) & (p - 1), 0)
    q = np.clip(msb * p + sub - 8 * p, 0, n_classes - 1)
    return np.where(c == 0, n_classes - 1, n_classes - 1 - q).astype(np.int64)


def class_floor(k, n_classes):
    """The smallest cost of class k (k < n_classes - 1; the last class starts at 0)."""
    p = n_classes // 16
    bits = _log2_exact(p)
    q = n_classes - 1 - k + 8 * p
    return ((p + q % p) << (q // p)) >> bits


def class_midpoint(k, n_classes):
    """The middle of class k's range, 2^(q div P) (1 + (q mod P + 1/2) / P), where it is an integer (every class but the last, whose range starts at 0)."""
    p = n_classes // 16
    bits = _log2_exact(p)
    q = n_classes - 1 - k + 8 * p
    return ((2 * p + 2 * (q % p) + 1) << (q // p)) >> (bits + 1)


def _max_along(a, r, axis):
    out = a.copy()
    n = a.shape[axis]
    for d in range(1, min(r, n - 1) + 1):
        lo = [slice(None)] * 2
        hi = [slice(None)] * 2
        lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
        lo, hi = tuple(lo), tuple(hi)
        out[lo] = np.maximum(out[lo], a[hi])   # the neighbour d further on
        out[hi] = np.maximum(out[hi], a[lo])   # the neighbour d further back
    return out


def dilate(cost2d, rx, ry):
    """Box maximum over [-ry, ry] x [-rx, rx], clipped at the grid's edges.  (The maximum over a box is the maximum over rows of the maxima along the rows:
    the one-pass and the separable form are one function.)"""
    a = np.asarray(cost2d, dtype=np.uint32)
    assert a.ndim == 2 and rx >= 0 and ry >= 0
    return _max_along(_max_along(a, rx, 1), ry, 0)


def tile_order(cost2d, rx, ry, n_classes):
    """(order, order2, class_totals, cost_after) of a (tiles_y, tiles_x) cost map.
    order: the tiles by the class of their DILATED cost, heaviest class first, row-major inside a class.  order2[2 p], order2[2 p + 1]: the upper and the lower
    half of the tile at position p in the grid of half-height tiles.  class_totals: tiles per class of the UNDILATED costs.  The cost map is cleared."""
    a = np.asarray(cost2d, dtype=np.uint32)
    ty, tx = a.shape
    key = cost_class(dilate(a, rx, ry).ravel(), n_classes)
    order = np.argsort(key, kind="stable").astype(np.uint32)
    y, x = order.astype(np.int64) // tx, order.astype(np.int64) % tx
    order2 = np.empty(2 * order.size, dtype=np.uint32)
    order2[0::2] = (2 * y) * tx + x
    order2[1::2] = (2 * y + 1) * tx + x
    totals = np.bincount(cost_class(a.ravel(), n_classes), minlength=n_classes).astype(np.uint32)
    return order, order2, totals, np.zeros(a.size, dtype=np.uint32)


def heavy_tile_count(class_totals, n_tiles, ratio, trigger, resident_waves):
    """How many tiles at the head of a sorted order are heavy.  Every class counts with the middle of its range, the last (which also holds the tiles
    without a measurement) with 0.  The draw's duration is estimated as the sum of the wave lifetimes, two waves per tile, over the resident waves.
    Nothing is heavy when the totals are not the histogram of n_tiles tiles or the heaviest occupied class does not outlive trigger x the draw;
    otherwise the tiles of the leading classes that outlive ratio x the draw are, at most a third of the grid.  ratio and trigger are C floats.

    How far this is a second opinion: the rule is a dozen lines either way, so this restatement has the C function's shape, down to the order of the
    sum, and a comparison with it mostly guards the C function against an accidental edit.  What is independent of it are sharding.heavy_tiles, which works
    on the costs themselves and knows no classes (test_three_statements_of_the_heavy_rule_agree), and the edges worked by hand in the host tests.
    Only the shipped 64-class rule is stated: a 32-class build uses tuned constants instead of the midpoints, which the comment above the C function
    does not give, so there is nothing to restate them from and such a histogram is refused here."""
    if np.asarray(class_totals).size != 64:
        raise NotImplementedError("the heavy-tile rule is stated for the 64-class build only")
    totals = np.asarray(class_totals, dtype=np.uint32).astype(np.int64)
    nc = totals.size
    p = nc // 16
    ratio, trigger = np.float64(np.float32(ratio)), np.float64(np.float32(trigger))
    life = np.zeros(nc, dtype=np.float64)
    for k in range(nc - 1):
        q = nc - 1 - k + 8 * p
        life[k] = np.ldexp(1.0, q // p) * (1.0 + (q % p + 0.5) / p)
    total = 0.0
    for k in range(nc):   # in class order, as the C loop: the rounding of the sum is part of the rule
        total += life[k] * float(totals[k])
    if int(totals.sum()) != n_tiles or total <= 0.0:
        return 0
    draw = total * 2.0 / float(resident_waves)
    occupied = np.flatnonzero(totals[:-1])
    first = int(occupied[0]) if occupied.size else nc - 1
    if not life[first] > trigger * draw:
        return 0
    heavy = 0
    for k in range(nc):
        if not life[k] > ratio * draw:
            break
        heavy += int(totals[k])
    return min(heavy, n_tiles // 3)
