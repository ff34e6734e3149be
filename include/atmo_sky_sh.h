/*
 * atmo_sky_sh.h -- the sky as light: the solid angle of every lens pixel, and shaded rays projected onto the nine real spherical harmonics of bands 0 to 2
 * (libatmo_hip.so, ABI version 5).  Included after atmo_lens.h (it includes it); same conventions.
 *
 * atmo_lens_rays forms the rays of a panorama, a fisheye, an octahedral map or a cube face, and the ray entry points shade them.  A renderer that wants
 * the sky's light on a surface -- an ambient term, a probe near the planet, the diffuse light under the clouds -- had to copy the float image back or
 * reduce it with a kernel of its own, rederive each lens's pixel solid angle from atmo_lens.h's arithmetic, and pick a summation order that repeats.
 * Both are here: atmo_lens_solid_angles writes the weights beside the rays, atmo_sky_sh9 sums weight x basis x radiance in ONE STATED ORDER, so that the
 * 37 sums have the same bits on every run, whatever else the device does.  Nothing is read back and nothing waits.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up.
 *
 * THE ARITHMETIC CONTRACT, in atmo_lens.h's style: RN(.) is one fp32 operation rounded to nearest, nothing is fused, roots and quotients are the IEEE
 * ones.  godot_atmosphere_shader_amd/sky_sh.py is the same statement in numpy, and tests/test_sky_sh_gpu.py holds the kernels to it.
 *
 * SOLID ANGLES, in steradians, with every quantity named as in atmo_lens.h (W, H, n, h, len, theta, rho, R, fov):
 *  - OCTAHEDRAL (fp32):  w = RN(RN(RN(4 / W) / H) / RN(RN(n n) n)),  n the lens's own root.  A pixel is du dv = (2 / W)(2 / H) of the L1 octahedron
 *    |a| + |b| + |z| = 1, whose area element seen from the centre is du dv / |p|^3, |p| = n.
 *  - CUBE_FACE (fp32):   w = RN(RN(RN(1 / h) / h) / RN(RN(len len) len)),  h and len the lens's own.  A texel is (1 / h)^2 of the plane vx = 1.
 *  - EQUIRECT, a statement in fp64, rounded to fp32 once:  w = ((2 pi / W) * (pi / H)) * cos theta, the doubles nearest 2 pi and pi, in this order.
 *  - FISHEYE, a statement in fp64, rounded once: with k = (fov / 2) / R, fov widened to double,
 *      w = (k * sin theta) / rho,   and   w = k * k   where rho == 0;   a pixel outside the circle is ABSENT.
 *    (theta = k rho, so d omega = sin theta d theta d phi = (k sin theta / rho) rho d rho d phi.)
 *  - No weight is negative: a value of the two fp64 statements that is not above 0 is +0.  (fov may exceed 2 pi by one fp32 rounding, so theta may pass
 *    pi and sin theta turn negative in the outermost pixels.)
 *  - THE TWO TRIGONOMETRIC LENSES get the rule their directions have: the device value is the fp32 nearest the fp64 statement, or that value's neighbour --
 *    at most 1 fp32 ulp.  The kernels take cos theta and sin theta from the evaluation atmo_lens_rays uses (a reduction by quarter turns with pi / 2 held
 *    in two doubles, then polynomials on [-pi / 4, pi / 4]).  Its reduced argument r = theta - k pi / 2 carries a relative error of at most
 *    2^-53 + 2^-106 / |r|, and the weight's three further double operations add 2^-53 each.  Wherever sin theta >= 2^-10 (cos theta for the panorama)
 *    that is a few double ulps, which can only move the weight across one fp32 rounding boundary.  BELOW 2^-10 THE SAME RULE HOLDS: theta is a double,
 *    no double other than 0 lies closer to a multiple of pi / 2 than 6e-17 (pi's own distance from its nearest double is 1.2e-16), so |r| >= 6e-17 and the
 *    second term stays below 2e-16 -- still a few double ulps, nine decimal orders inside an fp32 ulp.  theta == 0 is the fisheye's centre pixel alone,
 *    which has its own statement.  A weight that small may be an fp32 denormal (a fisheye more than 2^26 pixels across); it is rounded once all the same.
 *  - ORDER AND ABSENT SLOTS.  One float per slot of the ray array atmo_lens_rays(lens, flags) writes, in the same order: row-major or ATMO_LENS_QUADS, the
 *    same band, the counts of atmo_lens_ray_counts.  An absent slot (outside the image, outside the fisheye's circle) gets +0.  The basis, the origin and
 *    tmax do not enter.
 *
 * THE PROJECTION.  Per ray i with weight w = weight_dev[i] (1 where weight_dev is null), direction (x, y, z) = rays_dev[i].dir AS GIVEN -- the
 * coefficients live in the space the rays live in -- and (r, g, b, a) = rgba_dev[i]:
 *  - RADIANCE  c = (RN(r a), RN(g a), RN(b a), a): what blend_mix puts over a black background, and the alpha row for a host's own background.
 *  - BASIS, the constants the floats nearest these decimals:
 *      Y0 = 0.28209479                       Y1 = RN(0.48860251 y)             Y2 = RN(0.48860251 z)         Y3 = RN(0.48860251 x)
 *      Y4 = RN(1.0925484 RN(x y))            Y5 = RN(1.0925484 RN(y z))        Y6 = RN(0.31539157 RN(RN(3 RN(z z)) - 1))
 *      Y7 = RN(1.0925484 RN(x z))            Y8 = RN(0.54627422 RN(RN(x x) - RN(y y)))
 *  - TERM  t[k][ch] = RN(RN(w Y_k) c_ch), k = 0 .. 8, ch = r g b a; the 37th term is w itself.
 *  - A ray with w == 0 (either sign) contributes NOTHING: neither its direction nor its rgba row is read, whatever they hold (the indexed shading calls
 *    leave the rows of absent pixels untouched, NaN included).  A NaN weight is not 0.
 *
 * THE ORDER OF THE 37 SUMS is part of the contract.  It does not depend on the device, on the number of compute units or on what else runs: there are no
 * float atomics and nothing is handed from one workgroup to another inside a launch.  With the constants below (sky_sh.py reads them from this text):
 *  - A SEGMENT is ATMO_SKY_SH_SEGMENT = LANES * RAYS_PER_LANE = 4096 consecutive rays, handled by one workgroup of ATMO_SKY_SH_LANES = 256 lanes.
 *  - Lane t adds the terms of the rays 4096 seg + 256 j + t, j = 0 .. 15, in that order, starting from +0: v = RN(v + t).  Rays at or beyond n_rays are
 *    not read.
 *  - THE TREE reduces the 256 lane values: v[t] = RN(v[t] + v[t + s]) for s = 128, 64, ..., 1.  v[0] is the segment's partial, written to the scratch.
 *  - A second launch of one workgroup gives lane t the partials t, t + 256, ... in that order, from +0, then runs THE TREE.
 *  - out[j] = total[j], or RN(out[j] + total[j]) under ATMO_SKY_SH_ACCUMULATE.  Six cube faces are six calls; the five behind the first carry the flag.
 *
 * `out_dev` is ATMO_SKY_SH_FLOATS = 40 floats, 16-byte aligned: out[4 k + ch] the coefficient of Y_k in channel ch; out[36] the sum of the weights, the
 * solid angle covered; out[37 .. 39] are +0.  SCRATCH: the caller's, 16-byte aligned, 40 floats per segment (atmo_sky_sh9_scratch_bytes); its contents
 * before the call do not matter.  The library allocates nothing and both calls only enqueue on `stream`: a graph capture takes them as they are.
 *
 * WHAT IT COSTS.  atmo_lens_solid_angle_kernel<KIND, QUADS>: one lane per slot, one 4-byte store, at most 24 VGPRs, no LDS.  atmo_sky_sh9_segment_kernel:
 * 4 + 16 + 16 bytes read per ray with a weight (the second 16 bytes of the AtmoRay and the rgba row as 16-byte loads, skipped where the weight is 0),
 * 37 running sums per lane in registers, 86 VGPRs, 37888 bytes of LDS (37 x 256 floats for the tree's two steps across waves), no private-memory
 * stack.  atmo_sky_sh9_total_kernel: one workgroup, 91 VGPRs, the same LDS, no stack.  profiles/sky_sh/README.md holds the timings.
 *
 * Not here: prefiltered radiance, bands above 2.  (The resolve of ray results into packed image formats and the mip chain: atmo_sky_image.h.)
 */
#ifndef ATMO_SKY_SH_H
#define ATMO_SKY_SH_H

#include "atmo_lens.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATMO_SKY_SH_ACCUMULATE 1u     /* flags: out[j] = RN(out[j] + total[j]) instead of out[j] = total[j] */
#define ATMO_SKY_SH_LANES 256         /* THE ORDER OF THE SUMS: lanes of a workgroup */
#define ATMO_SKY_SH_RAYS_PER_LANE 16  /* THE ORDER OF THE SUMS: rays a lane adds; a segment is LANES * RAYS_PER_LANE rays */
#define ATMO_SKY_SH_FLOATS 40         /* floats of `out_dev` and of one segment's partial in the scratch: 36 coefficients, the weights' sum, three +0 */

/*
 * One float per slot of the ray array atmo_lens_rays(lens, flags) writes, to weight_dev[0 .. n_rays): SOLID ANGLES above.  It only enqueues a kernel on
 * `stream`: it allocates nothing and waits for nothing.  It reads no context state but the device.
 *
 * Checked in this order, before the device is touched (a context of atmo_debug_create_host_only answers the same, then ATMO_E_NO_DEVICE); every message
 * names this entry point:
 *   ATMO_E_ARG    a null ctx (no message)
 *   the checks of atmo_lens_rays on the lens and the flags, in its order: a null lens; ATMO_OK for an empty band (nothing is enqueued, nothing else is
 *                 looked at); kind and flag bits; the image's size; the band; fov and face; ATMO_LENS_QUADS' even rows
 *   ATMO_E_ARG    a null weight_dev; weight_dev not 4-byte aligned
 */
int atmo_lens_solid_angles(AtmoContext *ctx, const AtmoLens *lens, uint32_t flags, float *weight_dev, void *stream);

/*
 * The bytes of scratch atmo_sky_sh9 needs for n_rays rays: 160 * ceil(n_rays / 4096).  Needs no context.
 * ATMO_E_ARG: null bytes; n_rays > 2^28.
 */
int atmo_sky_sh9_scratch_bytes(uint32_t n_rays, size_t *bytes);

/*
 * THE PROJECTION of rays_dev[0 .. n_rays) with the results rgba_dev[0 .. n_rays) (atmo_shade_rays' rows) and the weights weight_dev[0 .. n_rays) into
 * out_dev.  Two kernels on `stream`, nothing else.  It reads no context state but the device.
 *
 * Checked in this order, before the device is touched (a host-only context answers the same, then ATMO_E_NO_DEVICE); every message names this entry point:
 *   ATMO_E_ARG    a null ctx (no message)
 *   ATMO_E_ARG    a null out_dev; out_dev not 16-byte aligned
 *   ATMO_E_ARG    flag bits other than ATMO_SKY_SH_ACCUMULATE
 *   ATMO_OK       n_rays == 0, nothing else is looked at: with ACCUMULATE nothing is enqueued; without it out_dev receives 40 +0 (one asynchronous
 *                 memset -- the one thing a host-only context cannot do here: ATMO_E_NO_DEVICE)
 *   ATMO_E_ARG    a null rays_dev or rgba_dev; either not 16-byte aligned
 *   ATMO_E_ARG    weight_dev not 4-byte aligned
 *   ATMO_E_ARG    n_rays > 2^28
 *   ATMO_E_ARG    a null scratch_dev; scratch_dev not 16-byte aligned; scratch_bytes below atmo_sky_sh9_scratch_bytes(n_rays)
 */
int atmo_sky_sh9(AtmoContext *ctx, const AtmoRay *rays_dev, const float *rgba_dev, const float *weight_dev /* nullable: every ray weighs 1 */,
                 uint32_t n_rays, uint32_t flags, void *scratch_dev, size_t scratch_bytes, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_SKY_SH_H */
