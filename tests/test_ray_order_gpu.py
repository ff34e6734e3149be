"""Coherent ray queues on the device (include/atmo_ray_order.h).  Needs an MI355X.

(a) the key kernel equals godot_atmosphere_shader_amd/ray_order.py as integers; (b) the sort on known keys EQUALS numpy's stable argsort, at the kernels'
    edges (the wave, the chunk, the scan's trip); (c) atmo_ray_order end to end; (d) shading through an index list is atmo_shade_rays bit for bit, for all
    seven ray kernels and whatever the list's order; (e) lists that are no permutations; (f) the kernel's name and the Python binding.
The contexts are the ones tests/test_rays_gpu.py builds."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from godot_atmosphere_shader_amd import _native as N
from godot_atmosphere_shader_amd import ray_order as R
from test_ray_order_host import hand_directions, seeded_directions
from test_rays_gpu import FAMILIES, IN_CLOUDS, H, W, _bits, _camera_and_depth, _dev, _node

pytestmark = pytest.mark.gpu

KF_RAYS, KF_INDEX = 16384, 32768
MASK = 2 ** 18 - 1
CHUNK = 1024             # keys a wave of the sort walks (RAY_SORT_CHUNK)
SCAN_TRIP = 1024         # chunks the scan takes in one trip (RAY_SCAN_TRIP)
FIRST = 37               # the queue's place in its image: the jitter texel follows the ray, not the thread
SENTINEL = 0x7FC12345    # a NaN no kernel produces


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


@pytest.fixture(scope="module")
def node():
    n = _node("lut")      # any context with a device serves the order
    yield n
    n.close()


def _scratch_words(node, n):
    b = C.c_size_t()
    N.check(node._ctx, node._lib.atmo_ray_order_scratch_bytes(n, C.byref(b)))
    assert b.value % 4 == 0
    return b.value // 4


# ---- (a) keys ---------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _key_rows():
    d = np.concatenate([hand_directions(), seeded_directions(50_000, seed=7)])
    rows = np.random.default_rng(11).standard_normal((d.shape[0], 8)).astype(np.float32)     # origin, tmax, reserved: anything
    rows[:, 4:7] = d
    rows.setflags(write=False)
    return rows, R.ray_keys(rows)


@pytest.mark.parametrize("n", [1, 63, 64, 65, None])
def test_the_key_kernel_is_the_numpy_statement(node, n):
    rows, want = _key_rows()
    n = rows.shape[0] if n is None else n
    rays = _dev(rows[:n])
    keys = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda")
    N.check(node._ctx, node._lib.atmo_debug_ray_keys(node._ctx, rays.data_ptr(), n, keys[1:].data_ptr(), None))
    torch.cuda.synchronize()
    got = _u32(keys)
    assert got[0] == got[-1] == 0xFFFFFFFF                    # nothing written beside the n keys
    bad = np.nonzero(got[1:-1] != want[:n])[0]
    assert bad.size == 0, (n, bad[:4].tolist(), got[1:-1][bad[:4]].tolist(), want[:n][bad[:4]].tolist(), rows[bad[:4], 4:7].tolist())
    assert int(got[1:-1].max()) <= MASK


# ---- (b) the sort on known keys ---------------------------------------------------------------------------------------------------------------------------------
def _sort(node, keys, scratch=None):
    """atmo_debug_sort_ray_keys on numpy keys: (index as uint32, the scratch tensor).  Index and a fresh scratch are pre-filled with 0xFFFFFFFF."""
    n = keys.shape[0]
    words = _scratch_words(node, n)
    if scratch is None:
        scratch = torch.full((words,), -1, dtype=torch.int32, device="cuda")
    index = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda")
    dkeys = _dev_u32(keys)
    N.check(node._ctx, node._lib.atmo_debug_sort_ray_keys(node._ctx, dkeys.data_ptr(), n, index[1:].data_ptr(), scratch.data_ptr(), 4 * words, None))
    torch.cuda.synchronize()
    got = _u32(index)
    assert got[0] == got[-1] == 0xFFFFFFFF
    assert np.array_equal(_u32(dkeys), keys.astype(np.uint32))          # the keys are not written
    return got[1:-1], scratch


def _key_patterns(n):
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.uint32)
    ties = rng.integers(0, max(2, n // 8), n).astype(np.uint32) * np.uint32(2_654_435_761 & MASK) & np.uint32(MASK)
    return {
        "all equal": np.full(n, 0x2A5A5, dtype=np.uint32),
        "descending": (np.uint32(n - 1) - i),                                    # strictly descending in the low 18 bits while n <= 2^18
        "top digit only": np.where(rng.integers(0, 2, n) == 1, 0x3F000 | 0x123, 0x1F000 | 0x123).astype(np.uint32),
        "bottom digit only": np.where(rng.integers(0, 2, n) == 1, 0x15540 | 0x2A, 0x15540 | 0x2B).astype(np.uint32),
        "random with ties": ties,
        "high bits set": (rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)),
    }


SORT_SIZES = [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK - 72, CHUNK * SCAN_TRIP + CHUNK + 7]


@pytest.mark.parametrize("n", SORT_SIZES)
def test_the_sort_equals_the_stable_argsort(node, n):
    """n = 1, 2, a wave less one / exactly / plus one, a chunk less one / exactly / plus one, a short last chunk, and more chunks than the scan takes in one
    trip.  EQUAL to np.argsort(keys & (2^18 - 1), kind="stable"), not merely a valid permutation; a second run over the same scratch gives the same bytes."""
    for label, keys in _key_patterns(n).items():
        want = np.argsort(keys & np.uint32(MASK), kind="stable").astype(np.uint32)
        got, scratch = _sort(node, keys)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (n, label, bad.size, bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        if label == "all equal":
            assert np.array_equal(got, np.arange(n, dtype=np.uint32))          # the identity comes back
        if label in ("random with ties", "high bits set"):
            before = _u32(scratch).copy()
            again, _ = _sort(node, keys, scratch)
            assert np.array_equal(again, got) and np.array_equal(_u32(scratch), before), (n, label)
    if n > CHUNK * SCAN_TRIP:
        assert (n + CHUNK - 1) // CHUNK > SCAN_TRIP           # the scan's second trip was taken


# ---- the shuffled queue every test below shades --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shuffle():
    p = np.random.default_rng(2026).permutation(W * H)
    p.setflags(write=False)
    return p


def _queue(n, pose):
    """(camera, the pose's 113 x 67 camera rays in the seeded shuffle, as a device tensor)."""
    cam, depth_np = _camera_and_depth(pose)
    rays = n.camera_rays(cam, _dev(depth_np))
    return cam, rays[_dev(_shuffle())].contiguous()


def _sentinel_out(n_rows):
    return torch.full((n_rows, 4), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _indexed_name(label):
    return f"atmo_shade_rays_indexed_kernel<{FAMILIES[label][2] | KF_RAYS | KF_INDEX}, {FAMILIES[label][3]}>"


# ---- (c) the order, end to end -----------------------------------------------------------------------------------------------------------------------------------
def test_the_device_s_order_is_the_numpy_order(node):
    _, rays = _queue(node, "P_space")
    want = R.ray_order(rays.cpu().numpy())
    got = node.ray_order(rays)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and tuple(got.shape) == (W * H,) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    assert np.array_equal(node.ray_order(rays).cpu().numpy(), got.cpu().numpy())            # equal on every run
    assert np.unique(R.ray_keys(rays.cpu().numpy())).size > 500                          # an order that sorts something
    assert tuple(node.ray_order(rays[:0]).shape) == (0,)


# ---- (d) indexed shading is the plain call, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(FAMILIES))
def test_indexed_shading_is_the_plain_call_bit_for_bit(label):
    """The 7 571 rays of the 113 x 67 P_space frame in a seeded shuffle, shaded through the identity, the reverse, a second random permutation and the device's
    own order: each equals atmo_shade_rays of the same queue with the same width and first, as uint32 words.  clouds_high also from inside the cloud layer."""
    n = _node(label)
    try:
        for pose in ("P_space", IN_CLOUDS) if label == "clouds_high" else ("P_space",):
            cam, rays = _queue(n, pose)
            plain = n.shade_rays(rays, cam, width=W, first=FIRST)
            torch.cuda.synchronize()
            assert n.kernel_name == f"atmo_shade_rays_kernel<{FAMILIES[label][2] | KF_RAYS}, {FAMILIES[label][3]}>", n.kernel_name
            want = _bits(plain)
            shaded = np.any(plain.cpu().numpy() != 0.0, axis=-1)
            print(f"{label} {pose}: {shaded.mean():.3f} shaded, {int((~shaded).sum())} discarded")
            assert shaded.mean() >= 0.30, (label, pose, float(shaded.mean()))        # the shares tests/test_rays_gpu.py holds its frames to
            assert (~shaded).any() if pose == "P_space" else shaded.all(), (label, pose)
            count = W * H
            lists = {"identity": np.arange(count), "reverse": np.arange(count)[::-1], "random": np.random.default_rng(5).permutation(count),
                     "device order": None}
            for name, idx in lists.items():
                index = n.ray_order(rays) if idx is None else _dev(idx.astype(np.int32))
                out = _sentinel_out(count)
                assert n.shade_rays(rays, cam, width=W, first=FIRST, out=out, index=index) is out
                torch.cuda.synchronize()
                assert n.kernel_name == _indexed_name(label), n.kernel_name
                bad = (_bits(out) != want).any(axis=-1)
                assert not bad.any(), (label, pose, name, int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
    finally:
        n.close()


# ---- (e) lists that are no permutations ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clouds():
    n = _node("clouds_high")
    cam, rays = _queue(n, "P_space")
    plain = n.shade_rays(rays, cam, width=W, first=FIRST)
    torch.cuda.synchronize()
    yield n, cam, rays, _bits(plain)
    n.close()


@pytest.mark.parametrize("n_index", [1, 63, 64, 65, 257])
def test_a_subset_leaves_the_other_rows_untouched(clouds, n_index):
    n, cam, rays, want = clouds
    every_third = np.arange(0, W * H, 3)[::-1].copy()          # (in descending order: the list's order is not the rows')
    index = _dev(every_third.astype(np.int32))
    out = _sentinel_out(W * H)
    n.shade_rays(rays, cam, width=W, first=FIRST, out=out, index=index[:n_index])
    torch.cuda.synchronize()
    got = _bits(out)
    listed = np.zeros(W * H, dtype=bool)
    listed[every_third[:n_index]] = True
    assert np.array_equal(got[listed], want[listed])
    assert (got[~listed] == SENTINEL).all()
    assert want[listed].any() or n_index == 1


def test_entries_beyond_the_batch_and_duplicates_change_nothing(clouds):
    n, cam, rays, want = clouds
    count = W * H
    rng = np.random.default_rng(9)
    base = rng.permutation(count)[:5000].astype(np.uint32)
    noisy = np.concatenate([base[:1700], np.array([count, count + 5, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32), base[100:300], base[1700:],
                            np.array([count], dtype=np.uint32), base[:64]])
    pictures = []
    for index in (base, noisy):
        out = _sentinel_out(count + 8)                          # eight rows behind the batch: an entry >= n_rays stores nothing there either
        n.shade_rays(rays, cam, width=W, first=FIRST, out=out[:count], index=_dev_u32(index))
        torch.cuda.synchronize()
        pictures.append(_bits(out))
    assert np.array_equal(pictures[0], pictures[1])
    listed = np.zeros(count + 8, dtype=bool)
    listed[base] = True
    assert np.array_equal(pictures[0][:count][listed[:count]], want[listed[:count]]) and (pictures[0][~listed] == SENTINEL).all()


# ---- (f) the binding ---------------------------------------------------------------------------------------------------------------------------------------------
def test_shade_rays_through_the_device_s_order_is_shade_rays(clouds):
    n, cam, rays, _ = clouds
    plain = n.shade_rays(rays, cam, width=W)
    ordered = n.shade_rays(rays, cam, width=W, index=n.ray_order(rays))       # `out` is created, with zeros
    torch.cuda.synchronize()
    assert n.kernel_name == _indexed_name("clouds_high")
    assert np.array_equal(_bits(ordered), _bits(plain)) and _bits(plain).any()
    part = n.shade_rays(rays, cam, width=W, index=n.ray_order(rays)[:1000])
    assert int((_bits(part).any(axis=-1)).sum()) <= 1000                       # rows the list does not name are zeros
    with pytest.raises(TypeError, match="index must be a contiguous CUDA int32 tensor"):
        n.shade_rays(rays, cam, width=W, index=n.ray_order(rays).to(torch.int64))
    with pytest.raises(ValueError, match=r"index must have shape \(m,\)"):
        n.shade_rays(rays, cam, width=W, index=n.ray_order(rays).reshape(-1, 1))
