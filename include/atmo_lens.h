/*
 * atmo_lens.h -- lens rays formed on the device: a panorama, a fisheye, an octahedral map, a cube face (libatmo_hip.so, ABI version 5).  Included after
 * atmo_ray_quads.h and atmo_ray_list.h; same conventions.
 *
 * The ray entry points take rays; until now the one ray the library could form itself was a pinhole camera's (atmo_debug_frame_rays).  The callers the ray
 * headers name -- an environment map, a lens-matched projection, a probe that is no 90-degree face -- had to write a kernel of their own, put its rays in
 * the quad layout of atmo_ray_quads.h with absent slots, and hand an image over row by row, which costs the cloud kernels against 2-D blocks
 * (profiles/rays/README.md sections 2 and 12).  atmo_lens_rays writes the AtmoRay array of a lens image, row-major or in quad order, and beside the
 * row-major one the TILE INDEX, the 2-D block order atmo_shade_rays_indexed shades through.  No ray ever exists on the host.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up.
 *
 * LENS SPACE is a camera's view space: -Z forward, +Y up, +X right.  Image row 0 is the top row; pixel (x, y) has its centre at (x + 0.5, y + 0.5).
 * W = width, H = height.  `basis` takes a lens-space direction to ray space (BASIS below), `origin` is every ray's origin in ray space.
 *
 * THE ARITHMETIC CONTRACT, operation by operation.  RN(.) is one fp32 operation rounded to nearest; nothing is fused.
 * godot_atmosphere_shader_amd/lens.py is the same statement in numpy, and tests/test_lens_gpu.py holds the kernels to it.
 *  - OCTAHEDRAL (fp32), the inverse of atmo_ray_order.h's PLANE and FOLD:
 *      u = RN(RN((2 x + 1) / W) - 1), v = RN(RN((2 y + 1) / H) - 1)     2 x + 1 and W are exact in fp32 and the quotient is the IEEE one
 *      z = RN(RN(1 - |u|) - |v|)
 *      where z < 0:  a = copysign(RN(1 - |v|), u), b = copysign(RN(1 - |u|), v);  elsewhere a = u, b = v
 *      n = sqrt(RN(RN(RN(a a) + RN(b b)) + RN(z z))), the IEEE root
 *      d = (a / n, b / n, z / n), IEEE quotients
 *    The map's centre looks along +Z of lens space, as the key's does, and row y ascends with v: at 512 x 512 the key of pixel (x, y) de-interleaves to (x, y).
 *  - CUBE_FACE (fp32): texel (x, y) of face `face` of an N x N face, N = width, by the coverage cubemap's own texel-to-direction table (the reference's
 *    noise_cubemap.gd:110-128, the Vulkan faces) in its operation order:
 *      h = RN(0.5 N);  p = RN(RN(RN(x + 0.5) / h) - 1);  q = RN(RN(RN((N - y - 1) + 0.5) / h) - 1)
 *      (vx, vy, vz) = (1, q, -p);  len = sqrt(RN(RN(RN(vx vx) + RN(vy vy)) + RN(vz vz)));  v = v / len, IEEE root and quotients
 *      +X: (vx, vy, vz)   -X: (-vx, vy, -vz)   +Y: (-vz, vx, -vy)   -Y: (-vz, -vx, vy)   +Z: (-vz, vy, vx)   -Z: (vz, vy, -vx)
 *    A sky face drawn through this lens is addressed by the same table as the coverage cubemap (atmo_generate_noise_cubemap).
 *  - EQUIRECT, a statement in fp64, each component rounded to fp32 once:
 *      phi = ((x + 0.5) / W - 0.5) * (2 pi),  theta = (0.5 - (y + 0.5) / H) * pi          the doubles nearest pi and 2 pi, IEEE double operations in this order
 *      d = (cos theta * sin phi, sin theta, -(cos theta * cos phi))
 *  - FISHEYE (equidistant), a statement in fp64, rounded once:
 *      px = (x + 0.5) - W / 2,  py = H / 2 - (y + 0.5),  rho = sqrt(px px + py py),  R = min(W, H) / 2,  r = rho / R
 *      r > 1: the pixel is ABSENT.  theta = r * (fov / 2), fov widened to double
 *      d = (sin theta * (px / rho), sin theta * (py / rho), -cos theta);  rho == 0 gives (0, 0, -1)
 *    (px, py, their squares' sum and the comparison are exact: r > 1 is the integer test (2x+1-W)^2 + (H-2y-1)^2 > min(W, H)^2.)
 *  - THE TWO TRIGONOMETRIC LENSES.  The device value of each component is the fp32 nearest the fp64 statement, or that value's neighbour: at most 1 fp32
 *    ulp.  (The fp64 sine and cosine of any sound library differ by a few double ulps, which can only move a value across one fp32 rounding boundary.)  The
 *    arguments never leave [-pi, pi]; the kernels evaluate them with a reduction to [-pi/4, pi/4] by quarter turns and polynomials, no table and no stack.
 *  - BASIS.  Component r of dir is RN(RN(RN(B[r] dx) + RN(B[3 + r] dy)) + RN(B[6 + r] dz)), unfused, no normalisation: the basis is used AS GIVEN.  The
 *    identity and every signed permutation are exact.  An absent ray stays all-zero.
 *  - THE REST OF THE ROW.  origin is copied; tmax = distance_dev[y * distance_pitch + x] where a buffer is given, else lens->tmax; reserved = 0.  An absent
 *    ray is eight +0 floats.
 *
 * ORDERS.
 *  - ROW-MAJOR (flags == 0).  Ray i = (y - y0) * W + x.  Shade it with atmo_shade_rays(..., width = W, first = y0 * W).
 *  - QUADS (ATMO_LENS_QUADS).  Slot 4 q + j follows atmo_ray_quads.h LAYOUT with q counted inside the band: Q = (y0 / 2) * qpr + q.  Shade it with
 *    first_quad = (y0 / 2) * qpr.  Slots outside the image, and fisheye pixels outside the circle, are absent rays.
 *
 * THE TILE INDEX (index_dev; row-major only): the 2-D block order for image-shaped batches.  16 x 4 tiles, the draw kernels' block: tiles in row-major
 * order, lanes row-major inside a tile.  Entry k has tile t = k / 64 and lane l = k % 64; with tpr = ceil(W / 16):
 *     x = 16 (t % tpr) + (l & 15),   y = y0 + 4 (t / tpr) + (l >> 4)
 * The entry is (y - y0) * W + x for a pixel inside the band that is not absent, else ATMO_RAY_LIST_END.  n_index = 64 * tpr * ceil((y1 - y0) / 4).
 * atmo_shade_rays_indexed and atmo_shade_rays_detail consume it as it is (n_rays = n_rays, n_index = n_index): every listed ray gets the plain call's
 * bits, absent pixels are never shaded, and their rows are left untouched.
 *
 * WHAT IT COSTS (profiles/rays/README.md section 12 holds the table).  The kernels write 32 bytes a ray and do nothing else of note: no atomics, nothing
 * handed from one workgroup to another.  Each lane writes whole rays as two 16-byte stores; under QUADS four consecutive lanes write one quad's 128
 * contiguous bytes.
 */
#ifndef ATMO_LENS_H
#define ATMO_LENS_H

#include "atmo_ray_quads.h"
#include "atmo_ray_list.h"

#ifdef __cplusplus
extern "C" {
#endif

enum AtmoLensKind { ATMO_LENS_EQUIRECT = 0, ATMO_LENS_FISHEYE = 1, ATMO_LENS_OCTAHEDRAL = 2, ATMO_LENS_CUBE_FACE = 3 };
#define ATMO_LENS_QUADS 1u            /* flags: quad order (atmo_ray_quads.h LAYOUT) instead of row-major */

typedef struct AtmoLens {
    int32_t kind;                     /* AtmoLensKind */
    int32_t width, height;            /* the image; CUBE_FACE: width == height */
    int32_t y0, y1;                   /* the band of rows [y0, y1) this call writes; the whole image: 0, height */
    int32_t face;                     /* CUBE_FACE: 0..5 = +X -X +Y -Y +Z -Z; else ignored */
    float   fov;                      /* FISHEYE: the full angle across the image circle, radians, in (0, 6.2831855f]; else ignored */
    float   tmax;                     /* every ray's tmax when no distance buffer is given (FLT_MAX: none) */
    float   origin[3];                /* every ray's origin, in ray space */
    float   basis[9];                 /* lens space -> ray space, column-major 3 x 3, used AS GIVEN */
} AtmoLens;

/*
 * The lengths of a call's two arrays: *n_rays = W * rows (row-major) or 4 * qpr * ceil(rows / 2) (QUADS), rows = y1 - y0, qpr = (W + 1) / 2; *n_index =
 * 64 * ceil(W / 16) * ceil(rows / 4), the tile index's.  Needs no context; either output may be null.  The lens is held to the checks of the call below
 * that concern the lens and the flags alone, in its order (a null lens; an empty band gives 0 and 0 and ATMO_OK; kind, flag bits, the image's size, the
 * band, fov, face, QUADS' even rows), as ATMO_E_ARG.
 */
int atmo_lens_ray_counts(const AtmoLens *lens, uint32_t flags, uint32_t *n_rays, uint32_t *n_index);

/*
 * Writes the rays of the band (ORDERS above) to rays_dev[0 .. n_rays) and, where index_dev is given, THE TILE INDEX to index_dev[0 .. n_index), in the
 * same launch.  It only enqueues kernels on `stream`: it allocates nothing and waits for nothing, so a graph capture takes it as it is.  It reads no
 * context state but the device: any context that has one serves.  distance_dev: H rows of distance_pitch floats (the whole image's, whatever the band), or
 * null with distance_pitch 0.
 *
 * Checked in this order, before the device is touched (a context of atmo_debug_create_host_only answers the same, then ATMO_E_NO_DEVICE); every message names
 * this entry point:
 *   ATMO_E_ARG    a null lens
 *   ATMO_OK       y0 == y1, an empty band: nothing is enqueued, nothing else is looked at
 *   ATMO_E_ARG    an unknown kind; flag bits other than ATMO_LENS_QUADS
 *   ATMO_E_ARG    width < 1 or height < 1; width * height > 2^28
 *   ATMO_E_ARG    y0 < 0, y1 > height or y1 < y0
 *   ATMO_E_ARG    FISHEYE: fov NaN or outside (0, 6.2831855f];  CUBE_FACE: width != height, face outside 0 .. 5
 *   ATMO_E_ARG    QUADS: an odd y0, or an odd y1 other than height
 *   ATMO_E_ARG    a null rays_dev; rays_dev not 16-byte aligned; index_dev not 4-byte aligned
 *   ATMO_E_ARG    QUADS together with an index_dev
 *   ATMO_E_ARG    a distance buffer with distance_pitch < width; a distance_pitch != 0 without a buffer
 */
int atmo_lens_rays(AtmoContext *ctx, const AtmoLens *lens, uint32_t flags,
                   const float *distance_dev, uint32_t distance_pitch /* floats per row; 0 with a null buffer */,
                   AtmoRay *rays_dev, uint32_t *index_dev /* nullable; row-major only */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_LENS_H */
