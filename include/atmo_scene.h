/*
 * atmo_scene.h -- drawing several atmospheres into one frame (libatmo_hip.so, ABI version 5).  Included after atmo.h; same conventions.
 *
 * PlanetAtmosphere has two draw modes (planet_atmosphere.gd:1-3, 285-321).  Near the planet it draws a fullscreen quad in clip mode: that is
 * atmo_render / atmo_render_composite.  Beyond atmo_clip_distance = 1.75 (R + H + camera near) 1.1 it draws a BoxMesh of edge atmo_clip_distance
 * centred on the node -- "so multiple atmospheres can be drawn at lower cost" (README.md) -- rasterised like any unshaded blend_mix spatial material:
 * back faces culled, clipped by the near and far planes, depth-tested against the opaque scene, no depth write.  The calls below are that draw.
 *
 * Fragment test (stated exactly; csrc/atmo_device.h ProxyConsts, csrc/atmo_kernels.hip proxy_fragment_passes): the pixel's segment runs from the near
 * plane to the far plane, inv_projection_matrix (ndc_x, ndc_y, z, 1) for z from 1 down to 0 (reverse-Z), ndc at the pixel centre as in atmo_render, mapped
 * into the proxy's model space through inv_view_matrix and the inverse of model_matrix.  The pixel is COVERED when the segment's near end lies outside the
 * closed box |x|, |y|, |z| <= box_size / 2 and the segment enters the box (the front face of a convex mesh under back-face culling with near / far
 * clipping); the fragment's depth z_in is the reverse-Z depth of the entry point; it PASSES when z_in >= depth_dev[p]: GREATER_OR_EQUAL, the depth test
 * of Godot 4.3's reverse-Z forward renderers (engine behaviour, not in the reference tree).  Passing pixels are shaded exactly as atmo_render /
 * atmo_render_composite shade them -- the same bits --, every other pixel stores nothing.  A covered pixel whose ray then misses the shell is a
 * discarded fragment (stored as (0,0,0,0) by atmo_render_proxy unless atmo_set_target_cleared; never by the composite).  A reference quirk kept:
 * the box's half-edge 0.9625 (R + H + near) is smaller than R + H unless near > 0.039 (R + H), so seen face-on from far away the box cuts the rim
 * of the halo.  The proxy draws assume a reverse-Z projection (depth 1 on the near plane, 0 on the far plane; the far plane may lie at infinity, and
 * the projection may be off-axis or orthographic); a forward-Z matrix, which atmo_render accepts, is not supported by the proxy draws.
 *
 * Launch: only the box's screen rectangle (its part between the planes that the rect sees, projected, grown by one pixel, cut to frame->x0..y1), row-major, no tile
 * order or feedback state; no launch at all when nothing of the box is left (behind the camera, beyond the far plane, off the rect) -- ATMO_OK.
 * Nothing is allocated: a draw can be captured into a HIP graph like atmo_render.  Stream rules are atmo_render's.  The frame, the textures, the
 * uniforms and DOUBLE_PRECISION (atmo_set_host_double_precision) are used as by atmo_render.
 * Modes: the kernels exist for the forms a default context draws with -- atmo_set_precision 1, up to 32 view steps, one lane per ray, either cubemap
 * sampler; a context in precision 0 or 2, with more than 32 view steps or with atmo_set_lane_split 2 fails with ATMO_E_STATE.
 */
#ifndef ATMO_SCENE_H
#define ATMO_SCENE_H

#include "atmo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces: the far-mode draw of PlanetAtmosphere (planet_atmosphere.gd:1-3,56-58,98-101,300-321): the BoxMesh of edge box_size around model_matrix
   (16 floats, column-major, the node's global transform), rasterised with back-face culling, near/far clipping and the depth test against depth_dev;
   fragments outside it are not shaded and not written.  rgba_dev addressed as in atmo_render: (y1 - y0) rows of (x1 - x0) float4. */
int atmo_render_proxy(AtmoContext *ctx, const AtmoFrame *frame, const float *model_matrix, float box_size, const float *depth_dev, float *rgba_dev,
                      void *stream);
/* The same draw blended over the scene colour buffer as atmo_render_composite does (viewport_h rows of viewport_w float4, in place). */
int atmo_render_proxy_composite(AtmoContext *ctx, const AtmoFrame *frame, const float *model_matrix, float box_size, const float *depth_dev,
                                float *scene_rgba_dev, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_SCENE_H */
