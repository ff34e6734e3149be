/*
 * atmo_ray_quads.h -- shade caller-supplied rays in 2 x 2 quads: the declared cubemap sampler for rays (libatmo_hip.so, ABI version 5).  Included after
 * atmo.h; it includes atmo_rays.h for AtmoRay; same conventions.
 *
 * atmo_shade_rays (atmo_rays.h) samples the coverage cubemap at level 0: a single ray carries no 2 x 2 quad to difference.  The sampler the reference
 * DECLARES is linear-mipmap with implicit LOD (cloud_funcs.gdshaderinc:15,45) -- the library's default for atmo_render -- and it matters exactly where the
 * cubemap is minified: small frames, wide lenses, a 256 x 128 environment map.  A ray does have a quad if the caller hands one over: any renderer whose rays
 * come from an image has the 2 x 2 neighbours at hand.  atmo_shade_ray_quads takes the rays four at a time and samples the cubemap as the declared-sampler
 * pixel kernels do, each ray differencing against the two partner rays of its quad.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbol below up.
 *
 * LAYOUT.  rays_dev holds 4 n_quads AtmoRay, rgba_dev 16 n_quads floats.  Slot 4 q + j (j = 0 .. 3) of quad q is the ray of image pixel
 *     x = 2 (Q % qpr) + (j & 1),   y = 2 (Q / qpr) + (j >> 1),   Q = first_quad + q,   qpr = (width + 1) / 2
 * -- the quads of an image `width` wide in row-major order, the four pixels of a quad in row-major order.  Slots j ^ 1 and j ^ 2 hold that ray's
 * horizontal and vertical partner.  rgba_dev[4 (4 q + j) .. + 3] receives ALBEDO.rgb and ALPHA of slot 4 q + j.
 *
 * ABSENT RAYS.  A ray whose dir is exactly (+-0, +-0, +-0) is absent: it receives (0, 0, 0, 0), reaches no texture call, and contributes a zero
 * derivative to its partners -- exactly what a pixel outside the viewport is to the pixel kernels (the odd last column or row of an image).  Every other
 * ray is shaded and stored; a caller that needs a ray only as a partner ignores its output.
 *
 * THE ARITHMETIC CONTRACT.  Every item of atmo_rays.h holds as it stands there, per ray: CENTRE, SUN DIRECTION, DISTANCE, CLOUDS: MODEL-SPACE ORIGIN,
 * MARCH-DISTANCE CAP and MODEL-SPACE DIRECTION, and dir used AS GIVEN.  Two items read differently:
 *  - JITTER.  Slot 4 q + j reads the u_blue_noise_texture texel (x & 255, y & 255) of ITS pixel (x, y) above, byte / 255 exactly -- the texel atmo_render
 *    reads for pixel (x, y) of a viewport `width` wide.  A frame's quads handed over in several calls (first_quad), or in one, get the same jitter.
 *  - CLOUDS, SAMPLER.  The coverage cubemap is sampled as the declared-sampler pixel kernels sample it (atmo_render_kernel<49 / 51 / 57, 0, 1>), with
 *    the derivatives taken from the partner slots' sample positions AT THE SAME CALL:
 *      . a march sample: lambda from the two partners' cube coordinates at the same march step, in the oracle's operations (cube_sample_lod_quad: the
 *        cancellation-free face differences, rho^2 with the IEEE quotient, a correctly rounded log2), the two nearest levels mixed;
 *      . a light tap of the raymarched cloud light: the partners' sample positions at that step moved by the same tap offset, in the fused arithmetic of
 *        the pixel kernels' light taps (cube_sample_lod_fast);
 *      . the level-0 certificate as it stands: a sample whose partners are provably within a texel is level 0's tap, bit for bit what the full path
 *        returns.  Its bound is taken from the four rays' own positions at the first and the last march sample; rays with origins, directions and caps
 *        of their own are still affine in the step index, so the bound needs no change (atmo_kernels.hip, march_clouds).
 *    A partner that is absent, misses the atmosphere's shell, is gated out of the cloud march (render_clouds' tests, clouds:249-324), or has left the
 *    evaluation at that sample through an early-out contributes nothing: lambda is taken from the partners that do reach the call, 0 with none.
 * Where the quads are a camera's (atmo_debug_frame_rays put in quad order, absent rays beyond the image) the picture is atmo_render's under the declared
 * sampler, bit for bit; where the origins differ per quad the oracle's at the project's 1e-4 rule (tests/test_ray_quads_gpu.py).
 *
 * WHAT DRAWS.  The three cloud families of atmo_shade_rays: the v2 clouds under the baked LUT with and without raymarched cloud light, and the v1
 * clouds; precise arithmetic (atmo_set_precision 1, their default), up to 32 view steps, one lane per ray, cloud detail off.  atmo_kernel_name reports
 * atmo_shade_rays_kernel<16433, 0>, <16435, 0> and <16441, 0>.  Four consecutive lanes hold a quad, a wavefront 16 quads: quads that are neighbours in the
 * image march in step.
 */
#ifndef ATMO_RAY_QUADS_H
#define ATMO_RAY_QUADS_H

#include "atmo_rays.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Shades the 4 n_quads rays of rays_dev (LAYOUT above).  The call only enqueues on `stream`, and it allocates nothing.  Of `frame` it reads what
 * atmo_shade_rays reads.  There is no fallback to the level-0 ray kernels: their jitter order is row-major and this call's is quad order.
 *
 * Checked in this order, before the device is touched (a context of atmo_debug_create_host_only answers the same up to ATMO_E_NO_DEVICE); every message
 * names this entry point and the mode:
 *   ATMO_OK       n_quads == 0: nothing is enqueued, nothing else is looked at
 *   ATMO_E_ARG    a null frame, rays_dev or rgba_dev; a pointer that is not 16-byte aligned; width == 0; first_quad + n_quads beyond 2^30
 *   ATMO_E_STATE  atmo_shade_rays' refusals in its order: atmo_set_precision 0 or 2; more than 32 view steps; atmo_set_lane_split 2; a cloud variant in the
 *                 direct light mode; a cloud variant with cloud detail on (atmo_ray_detail.h has the entry point that shades it)
 *   ATMO_E_STATE  a variant without clouds: it has no texture call to difference (use atmo_shade_rays)
 *   ATMO_E_STATE  atmo_set_sampler_lod 0: level 0 is atmo_shade_rays' sampler
 *   ATMO_E_STATE  u_optical_depth_texture / u_cloud_shape_texture not set, as every draw; then, under atmo_set_sampler_lod -1 or 1: no mip chain of
 *                 u_cloud_coverage_cubemap bound -- level 0 is all there is (use atmo_shade_rays)
 * (Every variant this call accepts needs u_cloud_shape_texture, which only a device context can hold: a host-only context's last answer is that texture's
 * refusal, and ATMO_E_NO_DEVICE stands behind it.)
 */
int atmo_shade_ray_quads(AtmoContext *ctx, const AtmoFrame *frame, const AtmoRay *rays_dev, float *rgba_dev, uint32_t n_quads, uint32_t width,
                         uint32_t first_quad, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_RAY_QUADS_H */
