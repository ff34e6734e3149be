/*
 * atmo_views.h -- several views of one planet in ONE launch (libatmo_hip.so, ABI version 5).  Included after atmo.h; same conventions.
 *
 * A context draws one view per atmo_render call.  A host that needs several views of the same planet in a frame -- the two eyes of an XR multiview
 * pass (VIEW_INDEX in Godot), a split screen, the six faces of a sky or reflection probe, the viewports of several windows on one GPU -- would issue
 * N draws back to back, and pay N times what a draw pays once: the host call, and the drain at the end of every cloud draw (26-42 us that only the
 * NEXT draw's waves can fill).  Two views alternating on one (grid, stream) key also look like a fast camera to the tile feedback of atmo_render and
 * get no order at all (atmo.h, atmo_set_tile_feedback).  atmo_render_views shades all views in one launch: one context with its uniforms and
 * textures, one set of per-view frame constants, ONE tile order over all views -- the heavy tiles of every view first, the cheap tiles of all of
 * them filling one common drain.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (atmo.h is unchanged).  A host looks atmo_render_views up by symbol.
 *
 * THE CONTRACT
 *  - Pixels.  View i's pixels are bit for bit what atmo_render(ctx, &views[i].frame, views[i].depth_dev, views[i].rgba_dev, stream) writes -- or
 *    atmo_render_composite when `composite` is set --, whatever the other views are and whatever order the tiles run in: discard handling,
 *    atmo_set_target_cleared, atmo_set_host_double_precision, and, under the declared cubemap sampler, the even grid origin of EACH view's rect
 *    (the 2 x 2 quads are those of that view's viewport).  tests/test_views_gpu.py holds every family to it with no tolerance.
 *  - What is shared.  Uniforms and textures are the context's: all views see the same planet.  Per view: the matrices, the viewport size, the
 *    varyings, the time, the rect, the depth buffer and the output -- sizes and rects may differ between views.
 *  - Empty views.  A view whose rect is empty (x0 == x1 or y0 == y1) is skipped; its pointers are not looked at.
 *  - View count.  n_views == 0 is ATMO_OK and does nothing.  n_views < 0 or > ATMO_MAX_VIEWS is ATMO_E_ARG.
 *  - Per-view checks.  Every view gets atmo_render's: viewport size, rect inside the viewport, non-null device pointers, rgba_dev 16-byte aligned
 *    (ATMO_E_ARG, the message names the view).
 *  - Overlap.  The byte ranges the views WRITE -- composite == 0: the (y1 - y0) x (x1 - x0) float4 pixels at rgba_dev; composite != 0: the rows
 *    y0 .. y1 of the viewport_h x viewport_w scene buffer, from pixel x0 of the first to pixel x1 of the last -- must be pairwise disjoint: the
 *    views run concurrently, in no order.  Checked on the host; an overlap is ATMO_E_ARG.  (Split-screen halves of ONE scene buffer that sit side by
 *    side interleave row by row: pass them as views of their own viewports, or draw such a pair with two calls.)  Depth buffers may be shared.
 *  - Atomicity.  Nothing is enqueued when any view is refused.
 *  - Call behaviour.  The call only enqueues; in the steady state it performs no host wait, and a host may enqueue many batches ahead without
 *    synchronising.  The per-view constants travel through a ring of 16 context-owned staging slots, each guarded by an event
 *    behind the launch that read it: the call blocks only when all 16 batches before it are still in flight -- a swap-chain-like host, two or three
 *    frames ahead, never does.
 *  - Streams.  As atmo_render: everything is enqueued on `stream`; a texture update on another stream is ordered in front of the launch on the
 *    device, and a later texture update waits for this launch.
 *  - Modes.  The kernels exist for the forms a default context draws with -- exactly the proxy draw's list (atmo_scene.h): atmo_set_precision 1, up
 *    to 32 view steps, one lane per ray (atmo_set_lane_split 0 / 1), either cubemap sampler, baked-LUT or direct light, v2 and v1, with and without
 *    clouds or raymarched cloud light.  A context in precision 0 or 2, with more than 32 view steps or with atmo_set_lane_split 2 fails with
 *    ATMO_E_STATE.
 *  - Graph capture.  The per-view constants live in context-owned device memory that the next batch overwrites, so a replayed graph would read
 *    another batch's constants: a call on a capturing stream fails with ATMO_E_STATE, as the tile-list draws do.  Capture atmo_render per view.
 *
 * TILE ORDER.  Batches have one feedback state per context, separate from the four (grid, stream) states of atmo_render (it never recycles those),
 * keyed by the batch's signature: stream, kernel family, n_views and each view's tile grid.  A new signature restarts it.  It works as for single
 * draws: the first two batches of a signature are not measured, the next four record per-tile wave durations, then every 8th does; a sort on the
 * context's side stream turns them into one heaviest-first order over the concatenation of all views' tiles (64 cost classes, view-major and
 * row-major inside a class), which later batches pick up once it is complete; nothing under 512 tiles in total.  atmo_set_tile_feedback,
 * ATMO_TILE_FEEDBACK and atmo_get_feedback_stats apply as for single draws.  The picture never depends on the order.
 *    Motion: each view's previous frame is kept and its screen-space motion estimated as for single draws.  While ANY view moves by more than half a
 *    pixel per frame the learnt order is neither used nor recorded, and the batch runs view-major, row-major.  Motion-aware dilation of the cost map
 *    per view, the in-stream sort and the geometric order of the cloudless direct-light kernel are deliberately not part of batches, nor is the
 *    heavy-tile lane split.
 *
 * WHERE A BATCH IS SLOWER than N atmo_render calls (measured on an MI355X, DESIGN.md 5.10 / profiles/views/README.md; everywhere else measured it is
 * faster, 0.46-0.97 of the sequential time on a still camera): (1) a moving camera -- panning 1 degree per frame, two 1920 x 1080 views: +4.8 % for the
 * cloudless direct-light kernel, +1.6 % for clouds_high_rm, because the batch runs unordered while single draws keep their motion-aware orders; (2) two
 * views of the 8-step baked-LUT atmosphere without clouds (15-25 us draws): +9 % at 1920 x 1080, +11 % at 1280 x 720 -- the batch's copy of the per-view
 * constants and its event are not amortised by two such draws (eight are: 0.82).
 *
 * PACKED AND PITCHED COLOUR TARGETS per view (RGBA16F / RGBA8 / a row pitch, and with the pitch the side-by-side halves of one image): atmo_views_target.h.
 *
 * WHAT COMES NEXT (not part of this header): motion-aware orders per view.  Far-mode (proxy) views are atmo_views_proxy.h.
 */
#ifndef ATMO_VIEWS_H
#define ATMO_VIEWS_H

#include "atmo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATMO_MAX_VIEWS 8

typedef struct AtmoView {
    AtmoFrame frame;        /* per view: matrices, viewport size, varyings, time, rect -- sizes and rects may differ between views */
    const float *depth_dev; /* as atmo_render: viewport_h rows of viewport_w floats */
    float *rgba_dev;        /* composite == 0: (y1 - y0) x (x1 - x0) float4; composite != 0: the view's viewport_h x viewport_w scene buffer */
} AtmoView;

/* Draws views[0 .. n_views) in one launch on `stream`: atmo_render per view (composite == 0) or atmo_render_composite (composite != 0). */
int atmo_render_views(AtmoContext *ctx, const AtmoView *views, int n_views, int composite, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_VIEWS_H */
