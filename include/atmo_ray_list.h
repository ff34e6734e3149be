/*
 * atmo_ray_list.h -- ray lists built on the device: a queue whose LENGTH is a device word, and a list that leaves the rays out that surely miss the shell
 * (libatmo_hip.so, ABI version 5).  Included after atmo_ray_order.h; same conventions.
 *
 * A path tracer's miss queue has its length in an atomic counter the bounce kernel incremented, and seen from space most of it misses the planet.  Every
 * other ray entry point takes n_rays as a host integer: the tracer copies the counter back and waits, once per bounce, and a captured graph holds one
 * length.  atmo_ray_list reads the length ON THE DEVICE and writes an index list for the existing atmo_shade_rays_indexed, whose n_rays and n_index are
 * then the queue's CAPACITY, a host constant: no read-back, and one capture serves every length (INTEGRATION.md has the per-bounce loop).
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up.
 *
 * SEMANTICS of atmo_ray_list, item by item.  tests/test_ray_list_gpu.py holds the kernels to godot_atmosphere_shader_amd/ray_list.py, the same statement
 * in numpy, as integers.
 *  - LIVE LENGTH.  n = min(*count_dev, capacity), read on the device by the kernels; count_dev == NULL means n = capacity.
 *  - STREAM.  The call only enqueues kernels on `stream`: it allocates nothing, waits for nothing, uses no side stream and never reads *count_dev on the
 *    host.  A graph capture takes it as it is, and a replay uses whatever the word holds at that moment.
 *  - LISTED RAYS.  L = the rays i < n that ATMO_RAY_LIST_CULL does not remove (without the flag: all of them).  index_dev[0 .. |L|) holds L: without
 *    ATMO_RAY_LIST_ORDER ascending by i; with it in the stable ascending sort by atmo_ray_order.h's KEY -- for flags == ATMO_RAY_LIST_ORDER and
 *    n == capacity that is atmo_ray_order's output word for word.
 *  - TAIL.  index_dev[|L| .. capacity) = ATMO_RAY_LIST_END.
 *  - COUNT OUT.  *listed_dev = |L| where the pointer is non-null.
 *  - LEFT ALONE.  Nothing is written beyond `capacity` entries.  Rays i >= n are neither keyed, culled nor stored to: they may hold anything.
 *  - CULL needs `frame` and `rgba_dev`.  Of the frame it reads the view-space centre as every draw forms it (the atmo_set_host_double_precision negation
 *    included).  A culled ray gets rgba_dev[4 i .. 4 i + 3] = +0, stored by the list builder; no other element of rgba_dev is written.
 *  - CONSUMING THE LIST.  atmo_shade_rays_indexed(ctx, frame, rays_dev, rgba_dev, n_rays = capacity, width, first, index_dev, n_index = capacity, stream):
 *    END entries are >= n_rays and are skipped.  After the pair, rgba_dev[0 .. 4 n) is what atmo_shade_rays with n_rays = n writes, BIT FOR BIT, for every
 *    family and both flags; rgba_dev[4 n ..) is untouched.
 *  - DETERMINISM, as atmo_ray_order: no position is decided by an atomic's arrival order, nothing passes between workgroups inside a launch, the kernel
 *    boundaries on `stream` are the only ordering, every buffer is in the caller's scratch, and a second run over the same scratch gives the same bytes.
 *
 * THE CULL.  Per ray, from origin and dir AS GIVEN, c = the frame's view-space centre and R2 = the squared atmosphere radius the context's draws use
 * (RN(R * R), R = planet radius + atmosphere height as the draws round it); every operation fp32, rounded on its own (RN), none contracted.
 * atmo_debug_ray_cull_constants returns c.x, c.y, c.z, R2, RN(R2 * 1.02f).
 *  - c' = RN(c - origin), per component.
 *  - cc = dot(c', c'), b = dot(c', dir), dd = dot(dir, dir): each three rounded products summed left to right.
 *  - g = RN(RN(b * b) * RN(2 - dd)).
 *  - e = RN(cc - R2).
 *  - The ray is culled iff ALL of: cc >= RN(R2 * 1.02f); 0.25f <= dd <= 1.75f; g < RN(e * 0.998f).  A NaN makes a comparison false: such a ray is kept.
 * Why a culled ray surely receives zeros from the ray kernels: they store zeros iff ray_sphere misses, h = R2 - |oc - b d|^2 < 0, and in exact arithmetic
 * |oc - b d|^2 = cc - b^2 (2 - dd).  The first condition (the origin at least 1 % outside the shell) bounds the cancellation in e to a relative error of
 * about 1e-5; the 0.2 % shrink is two orders of magnitude above that and above the kernels' own rounding of h.  Rays that start inside the shell or within
 * 1 % of it, and rays whose direction is far from unit length, are simply kept and shaded.  Of the rays of the project's 113 x 67 camera queues that miss,
 * the cull removes 0.9925 (P_space), 0.9996 (P_limb) and 0.9946 (P_night), and none that hits (tests/test_ray_list_host.py).
 *
 * WHAT IT BUYS (profiles/rays/README.md section 8 holds the table: 2 073 600 rays of a 1920 x 1080 frame in a fixed random permutation, from P_space -- 37 % of
 * the rays miss -- and from P_limb -- 64 % --, one MI355X, medians of five interleaved rounds).  First of all no read-back: the host never learns n.  The list
 * alone costs 0.033 ms without flags, 0.044 ms with CULL, 0.090 ms with ORDER (atmo_ray_order: 0.084 ms; the list is one launch dearer, the tail fill).
 * list + atmo_shade_rays_indexed against the plain atmo_shade_rays of the same queue with n known: CULL alone wins for direct8 (0.92 x from P_space, 0.71 x
 * from P_limb) and from P_limb for direct5 (0.83 x); ORDER | CULL wins for the cloud variants -- clouds_high 0.59 x, clouds_high_rm 0.60 x, v1_clouds 0.78 x
 * from P_space, 0.54, 0.58 and 0.67 x from P_limb, each a little below atmo_ray_order + indexed (0.61, 0.61, 0.78; 0.61, 0.62, 0.75).  Where the list LOSES:
 * lut and v1_no_clouds from both poses under every flag (CULL 1.1 - 1.35 x, ORDER | CULL 1.7 - 2.0 x: their whole call is 0.07 ms), direct5 from P_space
 * (CULL 1.04 x), and ORDER for all four variants without clouds, as atmo_ray_order does (1.0 - 2.0 x).  A queue far below its capacity pays for the capacity:
 * at an eighth, list + indexed is 0.07 ms against 0.025 ms for the plain call on the live rays (cloudless), 0.13 against 0.08 ms (clouds_high) -- the
 * list's grids and the END tail (0.0235 ms per 2 M entries) are the capacity's; size the capacity to the queue.
 */
#ifndef ATMO_RAY_LIST_H
#define ATMO_RAY_LIST_H

#include "atmo_ray_order.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATMO_RAY_LIST_ORDER 1            /* listed rays in atmo_ray_order's order (THE KEY, stable); else in queue order */
#define ATMO_RAY_LIST_CULL  2            /* rays that SURELY miss the shell are not listed and receive zeros */
#define ATMO_RAY_LIST_END   0xFFFFFFFFu  /* what fills the list behind its last entry */

/*
 * The scratch atmo_ray_list needs for a queue of `capacity` rays, in bytes: atmo_ray_order's for as many rays, and the word that carries the live total
 * from one kernel to the next.  Monotone in capacity; capacity == 0 is fine.  Needs no context.  ATMO_E_ARG for a null `bytes` or capacity > 2^28.
 */
int atmo_ray_list_scratch_bytes(uint32_t capacity, size_t *bytes);

/*
 * Builds the list (SEMANTICS above).  The scratch's contents before and after mean nothing.
 *
 * Checked in this order, before the device is touched (a context of atmo_debug_create_host_only answers the same, then ATMO_E_NO_DEVICE):
 *   ATMO_OK       capacity == 0: nothing is enqueued, nothing else is looked at
 *   ATMO_E_ARG    capacity > 2^28; flag bits other than ATMO_RAY_LIST_ORDER | ATMO_RAY_LIST_CULL; a null rays_dev, index_dev or scratch_dev; CULL with a
 *                 null frame or rgba_dev; rays_dev, rgba_dev or scratch_dev not 16-byte aligned; index_dev, a non-null count_dev or a non-null listed_dev
 *                 not 4-byte aligned; scratch_bytes below atmo_ray_list_scratch_bytes(capacity)
 * Without CULL, frame is not looked at and rgba_dev may be null; a non-null rgba_dev is held to its alignment all the same and is not written.
 */
int atmo_ray_list(AtmoContext *ctx, const AtmoFrame *frame, const AtmoRay *rays_dev, const uint32_t *count_dev, uint32_t capacity,
                  int flags, float *rgba_dev, uint32_t *index_dev, uint32_t *listed_dev,
                  void *scratch_dev, size_t scratch_bytes, void *stream);

/*
 * THE CULL's constants for `frame`, without a device: out[0 .. 5) = c.x, c.y, c.z, R2, RN(R2 * 1.02f), *count = 5.  ATMO_E_ARG for a null frame, out or
 * count, or capacity < 5.
 */
int atmo_debug_ray_cull_constants(AtmoContext *ctx, const AtmoFrame *frame, float *out, int capacity, int *count);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_RAY_LIST_H */
