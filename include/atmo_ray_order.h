/*
 * atmo_ray_order.h -- coherent ray queues: a coherence order computed on the device, and ray kernels that shade THROUGH an index list (libatmo_hip.so, ABI
 * version 5).  Included after atmo_rays.h; same conventions.
 *
 * atmo_shade_rays gives 64 consecutive rays a wavefront.  A queue whose neighbours are unrelated -- a path tracer's miss queue -- gets the same values,
 * slower: every wave marches the longest of 64 unrelated rays and its gathers touch 64 unrelated places (profiles/rays/README.md, sections 2 and 7).  The
 * rays are on the device already, physically permuting 32-byte rays and un-permuting 16-byte results costs two more passes, and only the library knows that
 * ray i's jitter texel belongs to image index first + i and must follow the ray.  So: atmo_ray_order writes an order, atmo_shade_rays_indexed shades through
 * it, and rays and results stay where the caller has them.  The list need not be a permutation: the same call shades a compacted subset of a queue.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up.
 *
 * THE KEY.  Per ray, from dir = (dx, dy, dz) AS GIVEN (not normalised; the origin and tmax take no part); every operation fp32, rounded on its own (RN), none
 * contracted.  tests/test_ray_order_gpu.py holds the kernel to godot_atmosphere_shader_amd/ray_order.py, the same statement in numpy, as integers.
 *  - SUM.  s = RN(RN(|dx| + |dy|) + |dz|).  If s is zero, NaN or infinite the key is 2^18 - 1: an all-zero direction, any NaN component, an overflow.
 *  - PLANE.  u = dx / s, v = dy / s, the IEEE quotients: the direction's point on the octahedron |x| + |y| + |z| = 1, seen from +z.
 *  - FOLD.  Where the SIGN BIT of dz is set (so dz = -0 folds): u' = copysign(RN(1 - |v|), u), v' = copysign(RN(1 - |u|), v), both formed from the unfolded u
 *    and v.  Elsewhere u' = u, v' = v.
 *  - CELL.  qu = clamp((int)floor(RN(RN(u' * 256) + 256)), 0, 511); the product is exact.  qv likewise from v'.
 *  - INTERLEAVE.  key = sum over b = 0 .. 8 of (bit b of qu) << 2 b | (bit b of qv) << (2 b + 1).
 * Two directions of one key lie in one cell of a 512 x 512 octahedral map: at most 2 sqrt(2) / 512 apart in the map, which stretches angles by at most 3 --
 * below 0.95 degrees (0.91 over 4e6 uniform directions).  The key looks at DIRECTIONS only: a queue whose origins differ by a sizeable part of the planet's
 * radius should be ordered by its owner, or shaded per group of origins.
 *
 * THE ORDER.  index[0 .. n) = the stable ascending sort of 0 .. n-1 by key: rays of one key keep their queue order.  One well-defined permutation, a pure
 * function of the rays, equal on every run (np.argsort(keys, kind="stable")).  On the device: the key kernel, then a least-significant-digit radix sort of
 * (key, index) pairs in three 6-bit passes, each a histogram, a scan and a scatter.  No position is decided by an atomic's arrival order, nothing is handed
 * from one workgroup to another inside a launch, and the kernel boundaries on `stream` are the only ordering; every buffer lives in the caller's scratch.
 *
 * WHAT IT BUYS (profiles/rays/README.md section 7 holds the table: 2 073 600 rays of a 1920 x 1080 frame in a fixed random permutation, one MI355X, medians
 * of five interleaved rounds).  atmo_ray_order costs 0.083 ms there, whatever the variant.  atmo_ray_order + atmo_shade_rays_indexed against the plain
 * atmo_shade_rays of the same shuffled queue: clouds_high 0.276 against 0.441 ms, clouds_high_rm 0.602 against 0.965 ms (0.62 x, below the plain call's whole
 * min-max range in both), v1_clouds 0.217 against 0.266 ms (0.82 x).  The variants WITHOUT clouds do not gain: the order alone costs more than their whole
 * shuffled call (0.07 - 0.14 ms), the sum is 1.3 - 2.3 x it, and the two cheapest (the LUT and the v1 march) are slower through a list even with the order
 * for free -- shade those plainly.  Through the identity list a coherent queue costs what the plain call costs (1.00 - 1.04 x).
 */
#ifndef ATMO_RAY_ORDER_H
#define ATMO_RAY_ORDER_H

#include "atmo_rays.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATMO_RAY_KEY_BITS 18     /* 9 + 9 bits of an octahedral cell, Morton-interleaved */

/*
 * The scratch atmo_ray_order and atmo_debug_sort_ray_keys need for n_rays elements, in bytes: 16 per element (two buffers of (key, index) pairs) plus the
 * histograms.  Monotone in n_rays; n_rays == 0 is fine.  Needs no context.  ATMO_E_ARG for a null `bytes` or n_rays > 2^28.
 */
int atmo_ray_order_scratch_bytes(uint32_t n_rays, size_t *bytes);

/*
 * Writes THE ORDER of rays_dev[0 .. n_rays) to index_dev[0 .. n_rays).  It only enqueues kernels on `stream`: it allocates nothing, waits for nothing and
 * uses no side stream, so a graph capture takes it as it is.  It reads no context state but the device: any context that has one serves.  The scratch's
 * contents before and after mean nothing.
 *
 * Checked in this order, before the device is touched (a context of atmo_debug_create_host_only answers the same, then ATMO_E_NO_DEVICE):
 *   ATMO_OK       n_rays == 0: nothing is enqueued, nothing else is looked at
 *   ATMO_E_ARG    n_rays > 2^28; a null rays_dev, index_dev or scratch_dev; rays_dev or scratch_dev not 16-byte aligned, index_dev not 4-byte aligned;
 *                 scratch_bytes below atmo_ray_order_scratch_bytes(n_rays)
 */
int atmo_ray_order(AtmoContext *ctx, const AtmoRay *rays_dev, uint32_t n_rays, uint32_t *index_dev, void *scratch_dev, size_t scratch_bytes, void *stream);

/*
 * atmo_shade_rays through an index list: thread k < n_index shades ray i = index_dev[k].  It reads rays_dev[i], takes the jitter texel of image index
 * first + i and stores to rgba_dev[4 i .. 4 i + 3] -- every listed ray receives what atmo_shade_rays gives it with the same n_rays, width and first, BIT FOR
 * BIT, whatever the list's order.  Unlisted rays are not shaded and their output is left untouched; an entry >= n_rays is skipped and nothing is stored; a
 * duplicate entry is shaded twice and gives the same value.  64 consecutive ENTRIES share a wavefront.
 *
 * Checked in atmo_shade_rays' order with its messages under this name, before the device is touched:
 *   ATMO_OK       n_rays == 0 or n_index == 0: nothing is enqueued, nothing else is looked at
 *   ATMO_E_ARG    a null frame, rays_dev or rgba_dev; rays_dev or rgba_dev not 16-byte aligned; a null index_dev; index_dev not 4-byte aligned; width == 0;
 *                 first + n_rays beyond 2^32
 *   ATMO_E_STATE  atmo_shade_rays' modes and textures, as there
 * atmo_kernel_name reports atmo_shade_rays_indexed_kernel<FLAGS | 16384 | 32768, LSTEPS>.  Ray quads (atmo_ray_quads.h) have no indexed form.
 */
int atmo_shade_rays_indexed(AtmoContext *ctx, const AtmoFrame *frame, const AtmoRay *rays_dev, float *rgba_dev, uint32_t n_rays, uint32_t width, uint32_t first,
                            const uint32_t *index_dev, uint32_t n_index, void *stream);

/*
 * THE KEY of every ray, the key kernel alone: keys_dev[i] = key of rays_dev[i].  Enqueues on `stream`.  n_rays == 0 is ATMO_OK; ATMO_E_ARG for n_rays > 2^28,
 * a null pointer, rays_dev not 16-byte aligned or keys_dev not 4-byte aligned; then ATMO_E_NO_DEVICE on a host-only context.
 */
int atmo_debug_ray_keys(AtmoContext *ctx, const AtmoRay *rays_dev, uint32_t n_rays, uint32_t *keys_dev, void *stream);

/*
 * atmo_ray_order's sort on the caller's keys (the same launches, not a copy): index_dev[0 .. n) = the stable ascending sort of 0 .. n-1 by keys_dev[i] &
 * (2^18 - 1) -- only the low 18 bits of a key take part.  keys_dev is not written.  n == 0 is ATMO_OK; ATMO_E_ARG for n > 2^28, a null pointer, keys_dev or
 * index_dev not 4-byte aligned, scratch_dev not 16-byte aligned, or scratch_bytes below atmo_ray_order_scratch_bytes(n); then ATMO_E_NO_DEVICE on a
 * host-only context.
 */
int atmo_debug_sort_ray_keys(AtmoContext *ctx, const uint32_t *keys_dev, uint32_t n, uint32_t *index_dev, void *scratch_dev, size_t scratch_bytes,
                             void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_RAY_ORDER_H */
