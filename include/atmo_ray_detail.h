/*
 * atmo_ray_detail.h -- full-quality clouds for ray batches, ray lists and ray quads (libatmo_hip.so, ABI version 5).  Included after atmo_ray_list.h,
 * atmo_ray_quads.h and atmo_cloud_detail.h (it includes them); same conventions.
 *
 * atmo_set_cloud_detail (atmo_cloud_detail.h) is the reference's `#define CLOUDS_ALWAYS_LOW_QUALITY` commented out at run time: the detail fetch of
 * get_density_full, live TIME, the alpha0 < 0.3 branch of the raymarched cloud light.  atmo_render draws it.  atmo_shade_rays, atmo_shade_rays_indexed and
 * atmo_shade_ray_quads refuse a cloud context that has it on -- so a host that draws its main view with detail on got a second, visibly different cloud
 * field from its miss queue, its environment panorama or its lens-matched projection, one that does not move with AtmoFrame::time.  The two entry points
 * below are those three calls with the refusal gone: the same rays, the same lists, the same quads, shaded with get_density_full.  The three older entry
 * points refuse as before.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the two symbols below up, binds them in place of the three older
 * ones, and toggles atmo_set_cloud_detail.
 *
 * atmo_shade_rays_detail, index_dev == NULL.  The whole batch, as atmo_shade_rays: ray i of rays_dev is shaded into rgba_dev[4 i .. 4 i + 3], image
 * index first + i of an image `width` wide.  n_index is not looked at.
 *
 * atmo_shade_rays_detail, index_dev != NULL.  atmo_shade_rays_indexed's rules (atmo_ray_order.h): entry k of the list names ray index_dev[k] of the batch;
 * ATMO_RAY_LIST_END entries and entries >= n_rays are skipped; a list may be a subset, and rows of rgba_dev that no entry names are untouched;
 * n_index == 0 is ATMO_OK with nothing looked at.  A ray receives the bits the index_dev == NULL call gives it, whatever the list's order.  What
 * atmo_ray_order and atmo_ray_list write is consumed as it is, a count word on the device included.  A ray that atmo_ray_list culled keeps the zeros the
 * list builder stored for it: the cull is the sure-miss test of the atmosphere's shell, and a miss is a miss with or without detail.
 *
 * atmo_shade_ray_quads_detail.  atmo_shade_ray_quads' LAYOUT and ABSENT RAYS (atmo_ray_quads.h), as they stand there.
 *
 * CLOUD DETAIL IN EFFECT (the switch on and a cloud variant).  The three cloud families are shaded with get_density_full, under the union of the two
 * existing contracts:
 *  - every item of atmo_rays.h (and, for quads, the two items atmo_ray_quads.h reads differently) holds per ray: CENTRE, SUN DIRECTION, DISTANCE, JITTER,
 *    CLOUDS: MODEL-SPACE ORIGIN, MARCH-DISTANCE CAP and MODEL-SPACE DIRECTION, dir used AS GIVEN, and the sampler -- level 0 for atmo_shade_rays_detail,
 *    the declared sampler differenced against the quad's partner slots for atmo_shade_ray_quads_detail;
 *  - every item of atmo_cloud_detail.h holds per sample: c = RN(time * 0.01f), q = RN(RN(p * 15.0f) + c), the exact trilinear filter, the density
 *    expression, the EARLY OUTS, the RANGE, and RAYMARCHED LIGHT with its alpha0 < 0.3 and the discontinuity stated there.  With raymarched light the light
 *    is evaluated in place at each lit sample under both samplers, as in the detail draws;
 *  - p is the lane's sample position in model space, marched from the ray's OWN model-space origin (atmo_rays.h, CLOUDS: MODEL-SPACE ORIGIN) with the
 *    ray's own march-distance cap: the detail fetch reads whatever position the ray holds;
 *  - AtmoFrame::time is live.
 * Where the rays are a camera's (atmo_debug_frame_rays) the picture is the detail draw's -- atmo_render with the switch on, under the level-0 sampler for
 * atmo_shade_rays_detail and under the declared sampler for a frame's quads -- bit for bit; where the origins differ per ray it is the detail draw of the
 * moved camera at the project's 1e-4 rule (tests/test_ray_detail_gpu.py).  atmo_kernel_name reports atmo_detail_rays_kernel<FLAGS | 8192 | 16384, 0>
 * (24593, 24595, 24601; in quads 24625, 24627, 24633) and, through a list, atmo_detail_rays_indexed_kernel<FLAGS | 8192 | 16384 | 32768, 0> (57361,
 * 57363, 57369).  Measured once on an MI355X at 1920 x 1080 (profiles/rays/README.md, section 9, which also names what was not measured): 1.07 - 1.30 x
 * the like-for-like detail draw for a camera's rays, 1.03 - 1.23 x for its quads; detail on costs a ray call 1.12 - 1.49 x the same call with it off.
 *
 * CLOUD DETAIL NOT IN EFFECT (the switch off, or a variant without clouds).  The call IS atmo_shade_rays, atmo_shade_rays_indexed or atmo_shade_ray_quads:
 * the same kernels, the same bits, the same atmo_kernel_name, and the same answers with this header's entry point named in front.
 */
#ifndef ATMO_RAY_DETAIL_H
#define ATMO_RAY_DETAIL_H

#include "atmo_cloud_detail.h"
#include "atmo_ray_list.h"
#include "atmo_ray_quads.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Shades the batch (index_dev == NULL) or the rays a list names.  The call only enqueues on `stream`, and it allocates nothing.
 *
 * Checked in this order, before the device is touched (a context of atmo_debug_create_host_only answers the same up to ATMO_E_NO_DEVICE); every message
 * names this entry point:
 *   ATMO_E_ARG    a null ctx (no message)
 *   ATMO_OK       n_rays == 0, or a non-null index_dev with n_index == 0: nothing is enqueued, nothing else is looked at
 *   ATMO_E_ARG    a null frame, rays_dev or rgba_dev; rays_dev or rgba_dev not 16-byte aligned; index_dev not 4-byte aligned; width == 0;
 *                 first + n_rays beyond 2^32
 *   ATMO_E_STATE  atmo_shade_rays' mode refusals in its order: atmo_set_precision 2 or 0; more than 32 view steps; atmo_set_lane_split 2; a cloud variant
 *                 in the direct light mode.  Its cloud-detail item is gone
 *   ATMO_E_STATE  atmo_set_sampler_lod 1 on a cloud variant with a mip chain bound: rays sample the cubemap at level 0
 *   ATMO_E_STATE  u_optical_depth_texture / u_cloud_shape_texture not set, as every draw
 *   ATMO_E_NO_DEVICE  a host-only context
 */
int atmo_shade_rays_detail(AtmoContext *ctx, const AtmoFrame *frame, const AtmoRay *rays_dev, float *rgba_dev, uint32_t n_rays, uint32_t width,
                           uint32_t first, const uint32_t *index_dev, uint32_t n_index, void *stream);

/*
 * Shades the 4 n_quads rays of rays_dev.  The call only enqueues on `stream`, and it allocates nothing.  atmo_shade_ray_quads' checks in its order under
 * this entry point's name, the cloud-detail item of its mode refusals gone: n_quads == 0 is ATMO_OK; the argument block; the mode refusals; a variant
 * without clouds; atmo_set_sampler_lod 0; the textures; no mip chain of u_cloud_coverage_cubemap; ATMO_E_NO_DEVICE.
 */
int atmo_shade_ray_quads_detail(AtmoContext *ctx, const AtmoFrame *frame, const AtmoRay *rays_dev, float *rgba_dev, uint32_t n_quads, uint32_t width,
                                uint32_t first_quad, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_RAY_DETAIL_H */
