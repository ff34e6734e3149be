/*
 * atmo_views_proxy.h -- several FAR-MODE views of one planet in ONE launch (libatmo_hip.so, ABI version 5).  Includes atmo_views_target.h and atmo_scene.h;
 * same conventions.
 *
 * PlanetAtmosphere has two draw modes: the fullscreen quad near the planet (atmo_render*) and, beyond atmo_clip_distance, the BoxMesh proxy
 * (atmo_render_proxy*, atmo_scene.h).  The batches of atmo_views.h and atmo_views_target.h draw up to eight views of the planet in one launch -- stereo eyes,
 * split screen, probe faces -- in the fullscreen mode only.  In a solar-system scene most planets are far: an XR host would be back to one
 * atmo_render_proxy_target call per eye, a six-face probe to six calls, each with its own host call and its own end-of-draw drain.  The two functions here
 * are the far-mode form of the two batches: atmo_render_proxy[_composite] / atmo_render_proxy_target per view, in one launch.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (atmo.h, atmo_scene.h, atmo_target.h, atmo_views.h and atmo_views_target.h keep their function sets).  A host
 * looks atmo_render_views_proxy / atmo_render_views_proxy_target up by symbol.
 *
 * ONE BOX PER BATCH.  model_matrix (column-major 4 x 4, the node's global transform) and box_size are atmo_render_proxy's and hold for every view: the planet
 * is the context's, and the node has one mesh.  The cameras differ per view (views[i].frame).
 *
 * THE CONTRACT
 *  - Pixels.  View i's bytes are bit for bit what atmo_render_proxy (atmo_render_views_proxy, composite == 0), atmo_render_proxy_composite (composite != 0) or
 *    atmo_render_proxy_target (atmo_render_views_proxy_target) writes for (views[i].frame, model_matrix, box_size, views[i].depth_dev, views[i]'s output) --
 *    which pixels are written at all included -- whatever the other views are.  Everything those draws inherit is inherited: the fragment test of
 *    atmo_scene.h (front faces of the box between the near and the far plane, GREATER_OR_EQUAL against the reverse-Z depth buffer), covered-discard
 *    handling, atmo_set_target_cleared, atmo_set_host_double_precision, the encode / decode / blend contract of atmo_target.h, and, under the declared cubemap
 *    sampler, the even grid origin of EACH view's launch rectangle with failing pixels shaded as helper lanes.  Pixels outside the box's fragments, and bytes
 *    between a row's last pixel and the next row, are never touched.  A batch of tight RGBA32F targets through atmo_render_views_proxy_target IS
 *    atmo_render_views_proxy, byte for byte.  tests/test_views_proxy_gpu.py holds every kernel to it with no tolerance.
 *  - Launch.  Per view the launch covers the box's screen rectangle exactly as a single proxy draw computes it -- the box's part between the near and the far
 *    plane, projected, grown by one pixel -- cut to that view's rect.  The grid is the concatenation of those rectangles' tile grids, view-major and row-major
 *    inside a view.  There is no tile order, no cost recording and no feedback state: the rectangles change every frame, as the single proxy draw's.
 *    atmo_get_feedback_stats and the feedback state of atmo_render_views are not touched; the draws are not counted by atmo_set_timing, as the single proxy
 *    draw's are not.
 *  - Addressing.  As the single draws: composite == 0 -- the output is the view's RECT's first pixel ((y1 - y0) rows of (x1 - x0) pixels), not the cut
 *    rectangle's; composite != 0 -- the viewport's first pixel.  Target rows are row_pitch_bytes apart (0 = tight).
 *  - Views that draw nothing.  A view whose rect is empty is skipped: its pointers (and its target) are not looked at.  A view whose box leaves no tile --
 *    behind the camera, beyond the far plane, off the rect -- gets all its argument checks and contributes no tile.  When no view has a tile the call returns
 *    ATMO_OK with no launch and no staging slot taken.  n_views == 0 is ATMO_OK and does nothing.
 *  - Checks.  ATMO_E_ARG, and a per-view message names the view ("view i"): n_views outside 0 .. ATMO_MAX_VIEWS; null views with n_views > 0; null
 *    model_matrix; box_size not positive or not finite; a singular model, view or projection matrix; and every per-view check of the corresponding batch
 *    entry point -- atmo_render_views': viewport size, rect inside the viewport, non-null depth_dev, non-null 16-byte aligned rgba_dev;
 *    atmo_render_views_target's: null target pixels, unknown format, pixels aligned to the pixel size, row_pitch_bytes, one format per batch.  The overlap
 *    rule is that entry point's (atmo_views.h: disjoint byte ranges; atmo_views_target.h: rules (a) and (b), so the side-by-side halves of one double-wide
 *    image are accepted), applied to the bytes of the frame's RECT, not of the cut rectangle: a batch that is accepted stays accepted wherever the planet
 *    moves.  Argument errors that need no matrix arithmetic come in front of the mode check; a singular matrix may be reported behind it, as
 *    atmo_render_proxy does.  Nothing is enqueued when any view is refused.
 *  - Modes.  The one list the proxy draws, the batches and the packed targets share: atmo_set_precision 1, at most 32 view steps, one lane per ray
 *    (atmo_set_lane_split 0 / 1), either cubemap sampler, baked-LUT or direct light, v2 and v1, with and without clouds or raymarched cloud light.  Anything
 *    else is ATMO_E_STATE, for every target format.
 *  - Call behaviour and streams.  As atmo_render_views: the call only enqueues and performs no host wait in the steady state (the per-view constants travel
 *    through the same ring of 16 staging slots, shared with the other batches; the proxies and the targets travel as kernel arguments); texture updates on
 *    other streams are ordered on the device; a call on a capturing stream fails with ATMO_E_STATE, because the per-view constants are context-owned.
 *
 * WHERE A BATCH IS SLOWER than N atmo_render_proxy_composite / atmo_render_proxy_target calls (measured on an MI355X, composites into float and RGBA16F
 * images, a still camera, profiles/views/README.md "Proxy batches"; everywhere else measured it is faster: 0.85-0.94 of the sequential time for two
 * 1920 x 1080 views of the direct-light atmosphere, 0.60-0.65 for the cloud families, 0.39 for the six 512 x 512 faces of a probe, three of which see the
 * planet): two 1920 x 1080 views of the 8-step baked-LUT atmosphere without clouds, whose two proxy draws take 15.5 us together: +19.6 % into float images
 * (18.5 against 15.5 us per stereo frame), +20.1 % into RGBA16F images (18.7 against 15.6 us).  The sequential arm's own spread there is 15 %, the batch's
 * 2-3 %; the batch's copy of the per-view constants and its event are not amortised by two draws of 8 us.
 *
 * WHAT COMES NEXT (not part of this header): a launch policy for proxy draws (tile order, heavy-tile lane split), motion-aware orders per view.
 */
#ifndef ATMO_VIEWS_PROXY_H
#define ATMO_VIEWS_PROXY_H

#include "atmo_views_target.h"
#include "atmo_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Draws views[0 .. n_views) through the box proxy in one launch on `stream`: atmo_render_proxy per view (composite == 0), or atmo_render_proxy_composite
 * (composite != 0). */
int atmo_render_views_proxy(AtmoContext *ctx, const AtmoView *views, int n_views, const float *model_matrix, float box_size, int composite, void *stream);

/* The same into each view's colour target: atmo_render_proxy_target per view, plain or blended in place. */
int atmo_render_views_proxy_target(AtmoContext *ctx, const AtmoViewTarget *views, int n_views, const float *model_matrix, float box_size, int composite,
                                   void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_VIEWS_PROXY_H */
