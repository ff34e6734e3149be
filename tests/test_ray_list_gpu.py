"""Ray lists on the device (include/atmo_ray_list.h).  Needs an MI355X.

(a) the list, its tail, *listed and the culled rows' zeros ARE godot_atmosphere_shader_amd/ray_list.py's, as integers, at the kernels' edges -- the wave, the
    chunk, the scan's second trip; counts below, at and beyond the capacity and no count word; all four flag combinations; guard words intact; a second run
    over the same scratch gives the same bytes; (b) flags == ORDER with every ray live is atmo_ray_order's output; (c) rays at and behind the count change
    nothing, whatever they hold; (d) SOUNDNESS: every ray cull_mask removes has four zero words in the plain atmo_shade_rays result, for all seven ray
    kernels; (e) the list + atmo_shade_rays_indexed over the CAPACITY is atmo_shade_rays over the live rays, bit for bit, and rows behind them are
    untouched; (f) one captured graph serves two lengths, the second written on the device.
The contexts are the ones tests/test_rays_gpu.py builds, the queue the one tests/test_ray_order_gpu.py shuffles."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import ray_list as RL
from godot_atmosphere_shader_amd import ray_order as R
from godot_atmosphere_shader_amd.planet_atmosphere import _to_native_frame
from test_ray_list_host import hand_rays
from test_ray_order_gpu import FIRST, SENTINEL, _dev_u32, _queue, _sentinel_out, _u32
from test_rays_gpu import FAMILIES, H, W, _bits, _camera_and_depth, _dev, _node

pytestmark = pytest.mark.gpu

ORDER, CULL, END = RL.ORDER, RL.CULL, RL.END
ALL_FLAGS = (0, ORDER, CULL, ORDER | CULL)
BIG = 1024 * 1024 + 1024 + 7          # more chunks than the scan takes in one trip
CAPACITIES = [1, 1025, W * H, BIG]
GUARD = 0xFFFFFFFF


def _counts(capacity):
    """Below, at and beyond a wave and a chunk, the capacity, beyond it, and None: no count word."""
    return [0, 1, 63, 64, 65, 1023, 1024, 1025, capacity, capacity + 5, None]


@pytest.fixture(scope="module")
def node():
    n = _node("lut")      # any context with a device serves the list; the cull reads its planet
    yield n
    n.close()


def _consts(n, cam):
    """THE CULL's five constants for the frame the binding hands the library for `cam`."""
    nf = _to_native_frame(n.make_frame(cam, 0.0))
    out, count = (C.c_float * 5)(), C.c_int(0)
    N.check(n._ctx, n._lib.atmo_debug_ray_cull_constants(n._ctx, C.byref(nf), out, 5, C.byref(count)))
    assert count.value == 5
    return np.array(out, dtype=np.float32), nf


def _scratch_words(n, capacity):
    b = C.c_size_t()
    N.check(n._ctx, n._lib.atmo_ray_list_scratch_bytes(capacity, C.byref(b)))
    assert b.value % 16 == 0
    return b.value // 4


def _raw_list(n, nf, rays, count, flags, rgba, scratch):
    """atmo_ray_list itself.  count: an int (a device word is made of it) or None (no word).  index and listed carry a guard word on either side.
    Returns (index with its guards, listed with its guards) as device tensors."""
    capacity = rays.shape[0]
    index = torch.full((capacity + 2,), -1, dtype=torch.int32, device="cuda")
    listed = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    word = None if count is None else _dev_u32(np.array([count], dtype=np.uint32))
    N.check(n._ctx, n._lib.atmo_ray_list(n._ctx, C.byref(nf), rays.data_ptr(), None if word is None else word.data_ptr(), capacity, flags,
                                         rgba.data_ptr(), index[1:].data_ptr(), listed[1:].data_ptr(), scratch.data_ptr(), 4 * scratch.shape[0], None))
    torch.cuda.synchronize()
    if word is not None:
        assert int(_u32(word)[0]) == count           # the count word is read, not written
    return index, listed


@functools.lru_cache(maxsize=None)
def _seeded_rows(capacity):
    """Rows whose cull is mixed: origins within a few radii of the view-space origin, directions uniform and of lengths inside and outside THE CULL's band,
    the host test's hand rays in front, a NaN here and there.  Read only."""
    rng = np.random.default_rng(capacity)
    rows = np.zeros((capacity, 8), dtype=np.float32)
    rows[:, 0:3] = rng.uniform(-60.0, 60.0, (capacity, 3))
    rows[:, 3] = 3.0e38
    d = rng.standard_normal((capacity, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rows[:, 4:7] = d * rng.choice([1.0, 1.0, 1.0, 0.45, 0.6, 1.3, 1.35], (capacity, 1))
    rows[rng.integers(0, capacity, capacity // 97), rng.integers(0, 7, capacity // 97)] = np.nan
    rows.setflags(write=False)
    return rows


def _rows_for(n, capacity):
    """(rows, camera): the shuffled P_space queue for 113 x 67; the culled hand ray alone for capacity 1; else seeded rows behind the hand rays."""
    cam, _ = _camera_and_depth("P_space")
    if capacity == W * H:
        return _queue(n, "P_space")[1].cpu().numpy(), cam
    consts, _ = _consts(n, cam)
    hand, _, _ = hand_rays(consts[:3])
    if capacity == 1:
        return hand[:1].copy(), cam
    rows = _seeded_rows(capacity).copy()
    rows[:hand.shape[0]] = hand
    return rows, cam


# ---- (a) the list is the numpy statement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", CAPACITIES)
def test_the_list_is_the_numpy_statement(node, capacity):
    rows, cam = _rows_for(node, capacity)
    consts, nf = _consts(node, cam)
    keys, mask = R.ray_keys(rows), RL.cull_mask(rows, consts)        # worked out once; ray_list.list_from is ray_list on them
    print(f"capacity {capacity}: the cull removes {mask.mean():.3f} of the rows, {np.unique(keys).size} keys")
    if capacity > 1:
        assert 0.05 < mask.mean() < 0.95 and np.unique(keys).size > capacity // 20
        probe = RL.ray_list(rows[:3000], 2000, ORDER | CULL, consts), RL.list_from(keys[:3000], mask[:3000], 2000, ORDER | CULL)
        assert all(np.array_equal(a, b) for a, b in zip(probe[0], probe[1]))
    else:
        assert mask.all()
    rays = _dev(rows)
    words = _scratch_words(node, capacity)
    for flags in ALL_FLAGS:
        for count in _counts(capacity):
            want_index, want_listed, want_zeros = RL.list_from(keys, mask, count, flags)
            scratch = torch.full((words,), -1, dtype=torch.int32, device="cuda")
            rgba = _sentinel_out(capacity + 2)
            index, listed = _raw_list(node, nf, rays, count, flags, rgba[1:-1], scratch)
            where = (capacity, flags, count)
            got_listed = _u32(listed)
            assert got_listed[0] == got_listed[2] == GUARD and int(got_listed[1]) == want_listed, (where, got_listed.tolist(), want_listed)
            # list, tail and guard words (compared on the device; brought over only to say where they differ)
            want_words = _dev_u32(np.concatenate([[GUARD], want_index, [GUARD]]))
            if not torch.equal(index, want_words):
                got = _u32(index)
                assert got[0] == got[-1] == GUARD, where
                bad = np.nonzero(got[1:-1] != want_index)[0]
                assert bad.size == 0, (where, bad.size, bad[:4].tolist(), got[1:-1][bad[:4]].tolist(), want_index[bad[:4]].tolist())
            assert (want_index[want_listed:] == END).all() and (want_index[:want_listed] != END).all()
            # exactly the culled rows are four zero words; every other row, and the rows on either side, still hold the sentinel
            want_rgba = torch.full((capacity + 2, 4), SENTINEL, dtype=torch.int32, device="cuda")
            want_rgba[1:-1][_dev(want_zeros)] = 0
            if not torch.equal(rgba.view(torch.int32), want_rgba):
                got_rgba = _bits(rgba)
                assert (got_rgba[0] == SENTINEL).all() and (got_rgba[-1] == SENTINEL).all(), where
                bad = np.nonzero((got_rgba[1:-1] != np.where(want_zeros, 0, SENTINEL)[:, None]).any(axis=-1))[0]
                assert bad.size == 0, (where, bad.size, bad[:4].tolist(), got_rgba[1:-1][bad[:4]].tolist(), want_zeros[bad[:4]].tolist())
            if flags & CULL and (count is None or count >= min(capacity, 64)):
                assert want_zeros.any(), where
            # a second run over the same scratch: the same bytes, in the outputs and in the scratch
            if capacity < BIG or count in (capacity, 1025, None):
                before = scratch.clone()
                rgba2 = _sentinel_out(capacity + 2)
                index2, listed2 = _raw_list(node, nf, rays, count, flags, rgba2[1:-1], scratch)
                assert torch.equal(index2, index) and torch.equal(listed2, listed) and torch.equal(rgba2.view(torch.int32), rgba.view(torch.int32)), where
                assert torch.equal(scratch, before), where
    if capacity == BIG:
        assert (capacity + 1023) // 1024 > 1024            # the scan's second trip was taken


def test_no_flags_needs_neither_frame_nor_rgba_nor_listed(node):
    rows, _ = _rows_for(node, 1025)
    rays = _dev(rows)
    scratch = torch.full((_scratch_words(node, 1025),), -1, dtype=torch.int32, device="cuda")
    for flags in (0, ORDER):
        index = torch.full((1025 + 2,), -1, dtype=torch.int32, device="cuda")
        N.check(node._ctx, node._lib.atmo_ray_list(node._ctx, None, rays.data_ptr(), None, 1025, flags, None, index[1:].data_ptr(), None, scratch.data_ptr(),
                                                   4 * scratch.shape[0], None))
        torch.cuda.synchronize()
        want = RL.ray_list(rows, None, flags)[0]
        assert np.array_equal(_u32(index)[1:-1], want) and _u32(index)[0] == _u32(index)[-1] == GUARD


# ---- (b) equivalence -------------------------------------------------------------------------------------------------------------------------------------------
def test_order_alone_over_a_full_queue_is_atmo_ray_order(node):
    _, rays = _queue(node, "P_space")
    want = node.ray_order(rays)
    for count in (None, torch.tensor([W * H], dtype=torch.int32, device="cuda"), torch.tensor([W * H + 9], dtype=torch.int32, device="cuda")):
        index, listed = node.ray_list(rays, count, order=True, cull=False)
        torch.cuda.synchronize()
        assert index.dtype == torch.int32 and tuple(index.shape) == (W * H,) and tuple(listed.shape) == (1,)
        assert torch.equal(index, want) and int(listed.item()) == W * H
    assert np.array_equal(want.cpu().numpy().astype(np.int64), R.ray_order(rays.cpu().numpy()))


# ---- (c) dead rays ---------------------------------------------------------------------------------------------------------------------------------------------
def test_rays_behind_the_count_change_nothing(node):
    cam, rays = _queue(node, "P_space")
    _, nf = _consts(node, cam)
    live = 4001
    rng = np.random.default_rng(4)
    fills = {"NaN": np.full((W * H - live, 8), np.nan, dtype=np.float32),
             "all bits set": np.full((W * H - live, 8), 0xFFFFFFFF, dtype=np.uint32).view(np.float32),
             "infinities and garbage": rng.integers(0, 2 ** 32, (W * H - live, 8), dtype=np.uint64).astype(np.uint32).view(np.float32)}
    words = _scratch_words(node, W * H)
    for flags in ALL_FLAGS:
        pictures = []
        for label in (None,) + tuple(fills):
            dirty = rays.clone()
            if label is not None:
                dirty[live:] = _dev(fills[label])
            rgba = _sentinel_out(W * H)
            scratch = torch.full((words,), -1, dtype=torch.int32, device="cuda")
            index, listed = _raw_list(node, nf, dirty, live, flags, rgba, scratch)
            pictures.append((_u32(index), _u32(listed), _bits(rgba)))
            assert (_bits(rgba)[live:] == SENTINEL).all(), (flags, label)
        for p in pictures[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(p, pictures[0])), flags
        assert int(pictures[0][1][1]) <= live and (pictures[0][0][1:-1][:int(pictures[0][1][1])] < live).all()


# ---- the queue (d), (e) and (f) shade: the shuffled P_space frame with the hand rays dealt into it ----------------------------------------------------------------
def _mixed_queue(n):
    """(camera, rays, consts, native frame): tests/test_ray_order_gpu.py's shuffled 113 x 67 P_space queue with the host test's hand rays -- built around
    this frame's centre -- written over every 500th row."""
    cam, rays = _queue(n, "P_space")
    consts, nf = _consts(n, cam)
    hand, _, _ = hand_rays(consts[:3])
    rays = rays.clone()
    rays[torch.arange(hand.shape[0], device="cuda") * 500 + 3] = _dev(hand)
    return cam, rays, consts, nf


# ---- (d) soundness -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(FAMILIES))
def test_a_culled_ray_is_a_ray_the_kernels_give_zeros(label):
    n = _node(label)
    try:
        cam, rays, consts, _ = _mixed_queue(n)
        rows = rays.cpu().numpy()
        mask = RL.cull_mask(rows, consts)
        hand, hand_culled, _ = hand_rays(consts[:3])
        at = np.arange(hand.shape[0]) * 500 + 3
        assert np.array_equal(mask[at], hand_culled) and np.array_equal(_bits(rays)[at], hand.view(np.uint32))
        plain = _bits(n.shade_rays(rays, cam, width=W, first=FIRST))
        torch.cuda.synchronize()
        zero = ~plain.any(axis=-1)
        print(f"{label}: {zero.mean():.4f} of the rays get zeros, the cull removes {mask.mean():.4f} ({(mask & zero).sum() / zero.sum():.4f} of them)")
        assert 0.1 < mask.mean() < 0.9 and (mask & zero).sum() >= 0.98 * zero.sum() - hand.shape[0]      # the cull's reach, on the device's own zeros
        bad = np.nonzero(mask & ~zero)[0]
        assert bad.size == 0, (label, bad.size, bad[:4].tolist(), rows[bad[:4]].tolist())
    finally:
        n.close()


# ---- (e) end to end ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(FAMILIES))
def test_list_and_indexed_shading_is_the_plain_call_on_the_live_rays(label):
    n = _node(label)
    try:
        cam, rays, _, _ = _mixed_queue(n)
        capacity = W * H
        for live in (capacity, 4001):
            want = _bits(n.shade_rays(rays[:live], cam, width=W, first=FIRST))
            torch.cuda.synchronize()
            assert want.any()
            count = torch.tensor([live], dtype=torch.int32, device="cuda")
            for flags in (CULL, ORDER | CULL, 0, ORDER):
                out = _sentinel_out(capacity)
                index, listed = n.ray_list(rays, count, order=bool(flags & ORDER), cull=bool(flags & CULL), camera=cam, out=out)
                assert tuple(index.shape) == (capacity,)
                assert n.shade_rays(rays, cam, width=W, first=FIRST, out=out, index=index) is out          # n_rays = n_index = capacity
                torch.cuda.synchronize()
                got = _bits(out)
                bad = (got[:live] != want).any(axis=-1)
                assert not bad.any(), (label, live, flags, int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
                assert (got[live:] == SENTINEL).all(), (label, live, flags)
                assert 0 < int(listed.item()) <= live and (int(listed.item()) < live) == bool(flags & CULL), (label, live, flags, int(listed.item()))
    finally:
        n.close()


# ---- (f) one captured graph, two lengths ---------------------------------------------------------------------------------------------------------------------
def test_a_captured_graph_serves_a_count_rewritten_on_the_device():
    n = _node("clouds_high")
    try:
        cam, rays, _, _ = _mixed_queue(n)
        capacity = W * H
        want = {}
        for live in (capacity, 1300):
            want[live] = _bits(n.shade_rays(rays[:live], cam, width=W, first=FIRST))
        torch.cuda.synchronize()
        count = torch.tensor([capacity], dtype=torch.int32, device="cuda")
        out = _sentinel_out(capacity)
        fresh = _sentinel_out(capacity)
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):     # one stream, no parallel branches
                index, listed = n.ray_list(rays, count, order=True, cull=True, camera=cam, out=out)
                n.shade_rays(rays, cam, width=W, first=FIRST, out=out, index=index)
        torch.cuda.synchronize()
        for live in (capacity, 1300):
            count.fill_(live)                           # written on the device; the host never reads it
            out.copy_(fresh)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = _bits(out)
            assert np.array_equal(got[:live], want[live]), live
            assert (got[live:] == SENTINEL).all(), live
            assert 0 < int(listed.item()) < live
    finally:
        n.close()
