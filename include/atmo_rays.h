/*
 * atmo_rays.h -- shade caller-supplied rays: origins, directions and distances per ray (libatmo_hip.so, ABI version 5).  Included after atmo.h; same
 * conventions.
 *
 * Every draw entry point of atmo.h and its siblings forms its rays itself, from AtmoFrame::inv_projection_matrix and a depth buffer (main:128-169).  A
 * compute renderer has rays before it has matrices -- a path tracer's secondary rays that leave the scene and need the sky with its clouds, a fisheye or
 * lens-matched projection, a panorama for an environment map, a probe that is no 90-degree face.  atmo_shade_rays takes a device array of rays and
 * returns, per ray, what atmosphere_fragment returns for a fragment with that ray: ALBEDO.rgb and ALPHA.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up.
 *
 * THE ARITHMETIC CONTRACT.  Per ray, with c = AtmoFrame::planet_center_viewspace; every operation fp32, rounded on its own (RN) unless the item says
 * otherwise.  tests/test_rays_gpu.py holds the kernels to atmo_render bit for bit where the rays are a camera's (atmo_debug_frame_rays) and to the oracle at
 * the project's 1e-4 rule where the origins differ per ray.
 *  - CENTRE.  c' = RN(c - origin) per component.  Everything the reference does with in_v_planet_center_viewspace and ray_origin = 0 (main:141-162,
 *    v2:57-82, v1:15-63) is done with c' and origin 0: the three sphere tests, the atmosphere march's positions relative to the centre.  Moving the
 *    origin into the centre costs one rounding of c - origin (exact whenever the two are close in magnitude or share their low bits).
 *  - SUN DIRECTION.  The frame's, uniform: normalize(sun_center_viewspace - planet_center_viewspace), computed by the host as for every draw.
 *  - DISTANCE.  linear_depth = tmax, then linear_depth = RN(RN(tmax * RN(1 - f)) + RN(gd * f)) with f = u_sphere_depth_factor and gd the ground sphere's
 *    first hit or 1e7 (main:150-160; the expression every kernel evaluates), then t_end = min(t_end, linear_depth).  NaN and infinity follow the
 *    arithmetic: tmax = FLT_MAX with f = 0 limits nothing; tmax = +inf with f = 0 meets gd * 0 = 0 and stays +inf.
 *  - JITTER.  Ray i has image index k = first + i, x = k % width, y = k / width; its jitter is the u_blue_noise_texture texel (x & 255, y & 255), byte /
 *    255 exactly -- the texel atmo_render reads for pixel (x, y) of a viewport `width` wide.
 *  - CLOUDS, MODEL-SPACE ORIGIN.  (M * (origin, 1)).xyz with M = u_world_to_model_matrix * inv_view_matrix (the host's product, as for every draw):
 *    component r is RN(RN(RN(RN(M[0+r] * o.x) + RN(M[4+r] * o.y)) + RN(M[8+r] * o.z)) + RN(M[12+r] * 1)), column-major M, the four products summed left
 *    to right, nothing fused.  For origin = (+0, +0, +0) these are the bits of the origin every other draw of the frame marches from.
 *  - CLOUDS, MARCH-DISTANCE CAP.  raymarch_cloud's max_d (clouds:186-202) is a function of length(ray_origin) in model space and therefore the ray's own:
 *    mix(ground, space, smoothstep(bottom, RN(top * 1.05), RN(sqrt(|origin_model|^2)))) with the IEEE root and quotient, the sum of squares left to
 *    right, smoothstep as RN(t * t) * RN(3 - RN(2 t)); `ground` and `space` are the host's values.  For origin = 0: the frame's own cap, bit for bit.
 *  - CLOUDS, MODEL-SPACE DIRECTION.  (M * (dir, 0)).xyz, three products summed left to right, as in every draw.
 *  - CLOUDS, SAMPLER.  The coverage cubemap is sampled at level 0, whatever atmo_set_sampler_lod says and whether or not a mip chain is bound: rays carry
 *    no 2 x 2 quad to difference.  A context that DEMANDS the declared sampler (mode 1) with a chain bound is refused.
 *  - dir is used AS GIVEN.  ray_sphere assumes a unit direction (util:20-40); the library does not normalise it.
 *
 * WHAT DRAWS.  The default forms: the v2 variants under the baked LUT (with and without clouds, with raymarched cloud light) and, without clouds, under the
 * direct light march; the v1 variants with and without clouds; precise cloud and v1 arithmetic (atmo_set_precision 1, their default), up to 32 view
 * steps, one lane per ray, cloud detail off.  atmo_kernel_name reports atmo_shade_rays_kernel<FLAGS | 16384, LSTEPS>.  64 consecutive rays share a
 * wavefront: a batch whose neighbouring rays are neighbours in space marches in step; a shuffled queue gives the same values, slower
 * (profiles/rays/README.md has both) -- atmo_ray_order.h orders such a queue on the device and shades it through the order, in place.
 */
#ifndef ATMO_RAYS_H
#define ATMO_RAYS_H

#include "atmo.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AtmoRay {      /* 32 bytes, the array 16-byte aligned */
    float origin[3];          /* in the frame's view space ("ray space": what inv_view_matrix maps to world) */
    float tmax;               /* the ray's linear_depth: distance to the first opaque hit; FLT_MAX for none */
    float dir[3];             /* unit length, used AS GIVEN (ray_sphere assumes it, util:20-40); not normalised by the library */
    float reserved;           /* not read */
} AtmoRay;

/*
 * Shades rays_dev[0 .. n_rays): rgba_dev[4 i .. 4 i + 3] receives ALBEDO.rgb and ALPHA of ray i; a ray that misses the atmosphere's shell always receives
 * (0, 0, 0, 0) (atmo_set_target_cleared does not apply).  The call only enqueues on `stream`, and it allocates nothing.
 *
 * Of `frame` it reads inv_view_matrix, planet_center_viewspace, sun_center_viewspace and time (dead, as in every low-quality draw); the
 * atmo_set_host_double_precision negation applies as in every draw.  It neither reads nor checks inv_projection_matrix, the viewport or the rect.
 * width and first place ray i at image index first + i of an image `width` wide (JITTER above): a frame's rays handed over in several calls, or in one,
 * get the same jitter.
 *
 * Checked in this order, before the device is touched (a context of atmo_debug_create_host_only answers the same up to ATMO_E_NO_DEVICE):
 *   ATMO_OK       n_rays == 0: nothing is enqueued, nothing else is looked at
 *   ATMO_E_ARG    a null frame, rays_dev or rgba_dev; a pointer that is not 16-byte aligned; width == 0; first + n_rays beyond 2^32
 *   ATMO_E_STATE  (the message names the mode) atmo_set_precision 0 or 2; more than 32 view steps; atmo_set_lane_split 2; a cloud variant in the direct light
 *                 mode; a cloud variant with cloud detail on (atmo_ray_detail.h has the entry point that shades it); atmo_set_sampler_lod 1 with a mip
 *                 chain bound
 *   ATMO_E_STATE  u_optical_depth_texture / u_cloud_shape_texture not set, as every draw
 */
int atmo_shade_rays(AtmoContext *ctx, const AtmoFrame *frame, const AtmoRay *rays_dev, float *rgba_dev, uint32_t n_rays, uint32_t width, uint32_t first,
                    void *stream);

/*
 * Writes, for every pixel of the frame's rect in the rect's row-major order, the ray the float kernels form for it (main:128-148): origin 0, dir = the
 * prologue's normalised direction, tmax = the prologue's linear_depth BEFORE the sphere-depth mix.  Camera rays from the library's own arithmetic: shaded by
 * atmo_shade_rays with width = the rect's width (a full-width rect: the viewport's) they give atmo_render's frame under the level-0 sampler, bit for bit.
 * depth_dev: the viewport's depth, h rows of w floats, as atmo_render's; rays_dev: (x1 - x0) (y1 - y0) AtmoRay, 16-byte aligned.  Enqueues on `stream`.
 * ATMO_E_ARG for a bad frame (atmo_render's checks), a null or misaligned pointer; an empty rect is ATMO_OK.  Needs no texture and no particular mode.
 */
int atmo_debug_frame_rays(AtmoContext *ctx, const AtmoFrame *frame, const float *depth_dev, AtmoRay *rays_dev, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_RAYS_H */
