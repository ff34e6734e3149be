/*
 * atmo_views_target.h -- several views of one planet in ONE launch, into the colour buffers a renderer owns (libatmo_hip.so, ABI version 5).  Includes
 * atmo_views.h and atmo_target.h; same conventions.
 *
 * atmo_render_views (atmo_views.h) shades up to eight views in one launch, with one tile order over all views and one common drain -- into tightly packed
 * float4 buffers.  The hosts it was built for do not own float4 buffers: an XR swapchain image is RGBA16F or RGBA8, and the two eyes are often the two halves
 * of one double-wide image, so each eye has a row pitch.  atmo_render_target (atmo_target.h) stores and blends in those formats, exactly, one view per call.
 * atmo_render_views_target is both: the batch of atmo_views.h with every view stored, or blended in place, as atmo_render_target does it.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (atmo.h, atmo_views.h and atmo_target.h keep their function sets).  A host looks atmo_render_views_target up
 * by symbol.
 *
 * THE CONTRACT
 *  - Pixels.  View i's bytes are bit for bit what atmo_render_target(ctx, &views[i].frame, views[i].depth_dev, &views[i].target, composite, stream) writes,
 *    whatever the other views are and whatever order the tiles run in.  It therefore inherits the encode / decode / blend contract of atmo_target.h (the
 *    quiet NaN 0x7e00, UNORM8 ties to even, decode -- blend in fp32 -- encode once), discard handling, atmo_set_target_cleared,
 *    atmo_set_host_double_precision, and, under the declared cubemap sampler, the even grid origin of EACH view's rect.  Bytes between a row's last pixel and
 *    the next row are never touched.  tests/test_views_target_gpu.py holds every kernel to it with no tolerance.
 *  - Addressing.  As atmo_render_target: composite == 0 -- target.pixels is the rect's first pixel, (y1 - y0) rows of (x1 - x0) pixels; composite != 0 --
 *    target.pixels is the viewport's first pixel, viewport_h rows of viewport_w pixels, blended in place inside the rect.  Rows are row_pitch_bytes apart
 *    (0 = tight).
 *  - Format.  One format per batch: all non-empty views carry the same target.format, otherwise ATMO_E_ARG.  Pitches and sizes may differ per view.
 *    RGBA16F and RGBA8_UNORM are drawn by kernels of their own; RGBA32F by the kernels of atmo_render_views with each view's pitch in pixels -- a batch of
 *    tight RGBA32F targets IS atmo_render_views, byte for byte.
 *  - Per-view checks.  Every view gets atmo_render_views' checks (viewport size, rect inside the viewport, non-null depth_dev) and atmo_render_target's:
 *    null target pixels, unknown format, pixels aligned to the pixel size (16 / 8 / 4 bytes), row_pitch_bytes 0 or at least the row's bytes and a multiple of
 *    the pixel size.  ATMO_E_ARG; the message names the view.  All argument checks come in front of the mode check below.
 *  - Empty views, view count, atomicity, call behaviour, streams: as atmo_render_views.  A view whose rect is empty is skipped, its pointers and its target
 *    are not looked at; n_views == 0 is ATMO_OK and does nothing, n_views < 0 or > ATMO_MAX_VIEWS is ATMO_E_ARG; nothing is enqueued when any view is
 *    refused; the call only enqueues and performs no host wait in the steady state (the per-view constants travel through the same ring of 16 staging slots;
 *    the targets travel as kernel arguments); a call on a capturing stream fails with ATMO_E_STATE.
 *  - Modes.  What both the batch and the packed targets exist for, which is one list: atmo_set_precision 1, at most 32 view steps, one lane per ray
 *    (atmo_set_lane_split 0 / 1), either cubemap sampler, baked-LUT or direct light, v2 and v1, with and without clouds or raymarched cloud light.  Anything
 *    else is ATMO_E_STATE -- for RGBA32F targets too (they are the batch's kernels).
 *  - Overlap.  The views run concurrently, in no order, so the bytes they write must not overlap.  A view writes rows = y1 - y0 rows of
 *    row_bytes = (x1 - x0) * pixel_bytes, pitch bytes apart (the row pitch in effect: row_pitch_bytes, or the tight pitch for 0), from base, the address of
 *    its first written pixel: target.pixels for composite == 0, target.pixels + y0 * pitch + x0 * pixel_bytes for a composite.  Two views are accepted when
 *    one of these holds:
 *      (a) their byte ranges [base, base + (rows - 1) * pitch + row_bytes) are disjoint;
 *      (b) they have the same pitch P, and with A the view of lower base, d = base_B - base_A, q = d / P, r = d % P (integer division):
 *          either q >= rows_A, or both r >= row_bytes_A and r + row_bytes_B <= P.
 *    Everything else is ATMO_E_ARG ("overlapping"), checked on the host.  The rule never accepts two views that share a byte; it is exact for equal pitches
 *    whose rows do not wrap (r + row_bytes <= P), and conservative otherwise: interleaved rows of different pitches are refused even where no byte is
 *    shared.  Two row bands of one image satisfy (a); the side-by-side halves of one double-wide image -- pixels = image and image + half_width *
 *    pixel_bytes, row_pitch_bytes = the image's row -- satisfy (b), plain or composite: the layout atmo_render_views has to refuse.  Depth buffers may be
 *    shared.
 *
 * TILE ORDER.  As for float batches (atmo_views.h): one feedback state per context, keyed by the batch's signature -- stream, kernel family, n_views and each
 * view's tile grid.  The kernel family is part of it, so a packed batch learns an order of its own and a host alternating between float and packed batches
 * of one shape restarts the learning each time.  atmo_set_tile_feedback, ATMO_TILE_FEEDBACK and atmo_get_feedback_stats apply.  While any view moves by more
 * than half a pixel per frame the batch runs view-major, row-major.  The picture never depends on the order.
 *
 * WHERE A BATCH IS SLOWER than N atmo_render_target calls (measured on an MI355X with RGBA16F composites, profiles/views/README.md "Packed batches";
 * everywhere else measured it is faster, 0.46-0.97 of the sequential time on a still camera): (1) a moving camera -- panning 1 degree per frame, two
 * 1920 x 1080 views of clouds_high_rm: +4.0 %, because the batch runs unordered while single draws keep their motion-aware orders; (2) two 1920 x 1080 views
 * of the 8-step baked-LUT atmosphere without clouds (25 us draws): +6.0 %, which is as much as either arm's own spread there (5-7 %) -- the batch's copy of
 * the per-view constants and its event are not amortised by two such draws (eight 1280 x 720 views are: 0.79).
 *
 * WHAT COMES NEXT (not part of this header): motion-aware orders per view, the heavy-tile lane split for batches.  Far-mode (proxy) views of both batches are
 * atmo_views_proxy.h.
 */
#ifndef ATMO_VIEWS_TARGET_H
#define ATMO_VIEWS_TARGET_H

#include "atmo_views.h"
#include "atmo_target.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AtmoViewTarget {
    AtmoFrame frame;          /* per view: matrices, viewport size, varyings, time, rect -- sizes and rects may differ between views */
    const float *depth_dev;   /* as atmo_render: viewport_h rows of viewport_w floats */
    AtmoTarget target;        /* addressed as atmo_render_target: composite == 0 the rect's first pixel, else the viewport's */
} AtmoViewTarget;

/* Draws views[0 .. n_views) in one launch on `stream`: atmo_render_target per view, plain (composite == 0) or blended in place (composite != 0). */
int atmo_render_views_target(AtmoContext *ctx, const AtmoViewTarget *views, int n_views, int composite, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_VIEWS_TARGET_H */
