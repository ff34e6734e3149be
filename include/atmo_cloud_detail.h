/*
 * atmo_cloud_detail.h -- full-quality clouds: the detail fetch and live TIME (libatmo_hip.so, ABI version 5).  Included after atmo.h; same conventions.
 *
 * Every cloud shader of the reference evaluates get_density_full (cloud_funcs.gdshaderinc:31-68), whose last term is a second fetch of the shape volume,
 * texture(u_cloud_shape_texture, pos_world * 15.0 + vec3(time * 0.01)).r.  One line of the reference's main include switches it off for every shader,
 * `#define CLOUDS_ALWAYS_LOW_QUALITY` (planet_atmosphere_main.gdshaderinc:49: the author's GPU), and everything else of this library follows that line:
 * detail = 0.5, AtmoFrame::time dead.  The switch below is that line commented out, at run time: the clouds of a context are drawn with the detail fetch,
 * and they move with AtmoFrame::time.  Off (the default) nothing changes: the same kernels, the same bits.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up.
 *
 * THE ARITHMETIC CONTRACT.  Each item is a scalar fp32 evaluation of the text, every operation rounded on its own (RN = round to nearest even); the
 * functions that carry it are compiled without contraction.  tests/test_cloud_detail_gpu.py holds the kernels to the executed reference text
 * (tests/golden/reference_exec_detail.npz) at the project's 1e-4 rule.
 *  - c = RN(time * 0.01f), computed by the host once per draw from AtmoFrame::time (atmo_debug_cloud_detail_constants shows it).
 *  - q = RN(RN(p * 15.0f) + c) per component of the sample position p (model space), NOT fused: at a planet radius of 100 the texel coordinate is about
 *    1e5, where an fp32 ulp is 2^-7 of a texel -- the reference's own quantisation of the filter weights is part of the picture.
 *  - detail = the exact trilinear filter of the bound u_cloud_shape_texture at q -- the filter `shape` itself goes through: repeat wrap, exact byte / 255
 *    texels (the float copy when present), every product and sum of the three mixes rounded; a volume whose size n is no power of two through the
 *    unfused RN(RN(q * n) - 0.5).  detail lies in [0, 1 + 2^-20].
 *  - density = clamp(RN(RN(RN(RN(RN(shape - RN(0.2f * detail)) + m) * hc) * 50) - 20), 0, 1), m = mix(-1.2, 1.5, coverage), hc the height curve.
 *  - get_density_low (detail = 0.5, RN(0.2f * 0.5f) = 0.1f) is the function every other kernel evaluates, bit for bit.
 *  - EARLY OUTS.  The expression is monotone non-decreasing in shape and non-increasing in detail, so it is <= its value at (the largest shape, detail = 0)
 *    and >= its value at (the smallest shape, detail = 1 + 2^-20): where the first is <= 0 the result is 0, where the second is >= 1 it is 1, exactly, and
 *    neither volume fetch is made (atmo_kernels.hip, cloud_density_precise, states the argument beside each test).  The height-curve test hc > 0 and
 *    the layer skip do not depend on detail.
 *  - RANGE.  The wrapped texel index is exact while |floor(q * n - 0.5)| < 2^24 for a volume whose size is no power of two (the wrap divides in fp32),
 *    and while it fits an int32 for a power of two (masks): |p * 15 + c| * n below 1.6e7, e.g. time up to 2.6e7 s with n = 64.  Beyond it the fetch is
 *    still in bounds (the index is wrapped, then used) but no longer the reference's texel.
 *  - RAYMARCHED LIGHT.  get_light_raymarched (clouds:132-136) chooses get_density for all six taps where alpha0 < 0.3 and get_density_low where not;
 *    alpha0 is the march's alpha before the current sample, which the kernels carry as 1 - the running product of the transmittances.  That is the
 *    text's alpha up to a few ulp (the two recurrences, the hardware exp2): a pixel whose alpha0 comes within ~4e-6 of 0.3 at a lit sample may take the
 *    other branch than an fp32 evaluation of the text would -- a discontinuity of the text itself.
 *
 * WHAT DRAWS.  The six LUT-light cloud forms of the default mode: the v2 cloud variants with and without raymarched cloud light and the v1 cloud variant,
 * each under the level-0 and the declared cubemap sampler; precise cloud mode (atmo_set_precision 1, their default), up to 32 view steps, one lane per
 * ray.  atmo_render and atmo_render_composite draw them, on a row-major launch (no tile-order feedback; the picture does not depend on the launch
 * order).  atmo_kernel_name reports atmo_render_detail_kernel<FLAGS | 8192, 0>.  profiles/cloud_detail/README.md holds what the fetch costs.
 */
#ifndef ATMO_CLOUD_DETAIL_H
#define ATMO_CLOUD_DETAIL_H

#include "atmo.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * enable != 0: the context's cloud draws evaluate get_density_full with CLOUDS_ALWAYS_LOW_QUALITY off.  Accepted on any context; a variant without clouds
 * has no density to evaluate and draws as before, through every entry point.  With it on and a cloud variant:
 *   ATMO_OK       atmo_render, atmo_render_composite
 *   ATMO_E_STATE  every other draw entry point -- atmo_render_tiles[_split], atmo_measure_tile_costs, atmo_render_target and atmo_render_depth_target
 *                 (every format), the proxy draws, the view batches, atmo_render_planets and atmo_plan_planets (the message names the draw) -- where its
 *                 mode check stands; and atmo_render[_composite] themselves with atmo_set_precision 0 or 2, atmo_set_lane_split 2, the direct light
 *                 mode or more than 32 view steps.  The message names cloud detail.  Nothing is enqueued.  (Ray batches, ray lists and ray quads of
 *                 such a context: atmo_ray_detail.h.  Packed and pitched colour targets and depth sources, single draws and view batches:
 *                 atmo_detail_target.h.)
 */
int atmo_set_cloud_detail(AtmoContext *ctx, int enable);
int atmo_get_cloud_detail(AtmoContext *ctx, int *enabled);

/*
 * The constants a cloud-detail draw of `frame` hands its kernel, without a device (a context of atmo_debug_create_host_only answers the same):
 *   out[0] = c = RN(frame->time * 0.01f)
 *   out[1], out[2] = the bounds of RN(shape - RN(0.2f * detail)) the early outs test against: the smallest shape with detail = 1 + 2^-20, the largest
 *                    shape with detail = 0 (shape: the mix / invert of a filtered texel in [0, 1 + 2^-20] by u_cloud_shape_factor / _invert)
 *   out[3] = RN(0.2f * (1 + 2^-20)), the largest detail term
 * *count = 4; ATMO_E_ARG for a null argument or a capacity below 4.  Whether the switch is on does not matter.
 */
int atmo_debug_cloud_detail_constants(AtmoContext *ctx, const AtmoFrame *frame, float *out, int capacity, int *count);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_CLOUD_DETAIL_H */
