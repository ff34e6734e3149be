/*
 * atmo_planets.h -- a frame's FAR planets in as few launches as blending allows (libatmo_hip.so, ABI version 5).  Includes atmo_views_proxy.h; same
 * conventions.
 *
 * The reference draws a planet beyond atmo_clip_distance as a small BoxMesh "so multiple atmospheres can be drawn at lower cost": atmo_render_proxy*
 * (atmo_scene.h, atmo_target.h).  atmo_render_views_proxy[_target] (atmo_views_proxy.h) batches several VIEWS OF ONE PLANET.  What the far mode exists for is
 * several PLANETS IN ONE FRAME: a host that draws six far planets makes six calls and six launches, each bound by the call rather than by its pixels
 * (profiles/proxy/README.md).  The kernels of atmo_views_proxy.h read one table entry per draw -- every uniform, every texture pointer, the box and the
 * target -- and nothing in an entry says that the entries belong to one context.  atmo_render_planets is the host side of that: one entry per (planet, view).
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (the seven older headers keep their function sets).  A host looks atmo_render_planets / atmo_plan_planets up
 * by symbol.
 *
 * The call is COMPOSITE ONLY: a frame's planets share a colour buffer and are blended into it.  Plain per-view outputs remain atmo_render_views_proxy's.
 *
 * THE CONTRACT
 *  - Pixels.  Take the n calls atmo_render_proxy_target(draws[i].ctx, &draws[i].frame, draws[i].model_matrix, draws[i].box_size, draws[i].depth_dev,
 *    &draws[i].target, 1, stream) issued in list order (for a tight RGBA32F target: atmo_render_proxy_composite).  After atmo_render_planets every byte of
 *    every target is what those calls leave, bit for bit -- which pixels are touched at all included.  Everything the single draws inherit is inherited:
 *    the fragment test of atmo_scene.h, atmo_set_host_double_precision per context, the encode / decode / blend contract of atmo_target.h, and, under the
 *    declared cubemap sampler, the even grid origin of each draw's launch rectangle with failing pixels shaded as helper lanes.  The caller sorts the list
 *    back to front; the library keeps that order wherever it can matter.  tests/test_planets_gpu.py holds it to this with no tolerance.
 *  - The plan.  Deterministic, and stated exactly (atmo_plan_planets returns it; csrc/atmo_planets_plan.h is its text):
 *      * Per draw the launch rectangle (cx0, cy0, cx1, cy1) and its tile grid are the single proxy draw's (atmo_debug_proxy_launch_rect reports them).  A
 *        draw without a tile -- an empty rect; the box behind the camera, beyond the far plane, off the rect -- is in no launch.
 *      * The FOOTPRINT of a draw is the bytes of that rectangle in its target: rows cy0 .. cy1, each (cx1 - cx0) * pixel_bytes long and pitch bytes apart
 *        (the row pitch in effect), from target.pixels + cy0 * pitch + cx0 * pixel_bytes.
 *      * Two draws MAY TOUCH unless rule (a) or rule (b) of atmo_views_target.h proves their footprints disjoint.  The test never calls two footprints that
 *        share a byte disjoint; it is conservative (interleaved rows of different pitches may touch), which only costs a launch.
 *      * level(j) = 0 when no earlier draw i < j may touch j, otherwise 1 + the maximum level(i) over those i.
 *      * The FAMILY KEY of a draw: the device; the kernel flags its context resolves for a proxy draw; whether that family's unrolled 8-light-step twin is
 *        the one a single draw would launch; and the kernel that stores its target -- the float kernel (RGBA32F), or the packed kernel WITH the format,
 *        because a packed launch holds one format.  Formats, pitches, viewports and rects may differ freely across the draws of a call.
 *      * Launches are formed level by level; within a level the keys are taken in the order in which they first appear among that level's draws, in list
 *        order; within a key the draws are cut into chunks of ATMO_MAX_VIEWS, in list order.  Launches are enqueued on `stream` in that order.
 *    Why this is the sequential result: two draws that may touch always sit in different levels and keep their order; all other draws write disjoint bytes
 *    and commute.
 *  - Launch.  Each launch is the KF_VIEWS | KF_PROXY [| KF_TARGET] kernel of its key, exactly as atmo_render_views_proxy[_target] issues it: table entry k
 *    holds the constants of the launch's k-th draw made from THAT DRAW'S OWN CONTEXT, with its launch rectangle; its box and its target travel by value.
 *    The staging slot comes from the ring of the launch's first context.  Every distinct context of a launch is ordered behind its texture updates on other
 *    streams in front of the launch, and behind the launch gets the bookkeeping of a draw (atmo_kernel_name reports the views-proxy kernel of its family;
 *    a later texture update on another stream waits for the launch on the device).  Not timed and not counted by atmo_set_timing; no tile order and no
 *    feedback state are touched, as for every proxy draw.
 *  - Checks.  Nothing is enqueued when any check fails; atmo_plan_planets performs the same checks (but for the textures and the stream, which need a
 *    device).  ATMO_E_ARG: n_draws outside 0 .. ATMO_MAX_PLANET_DRAWS; null draws with n_draws > 0; a null ctx; contexts on different devices; and every
 *    per-draw check of atmo_render_proxy_target -- unknown format, null or misaligned pixels, row_pitch_bytes, viewport size, rect, box_size, null depth_dev,
 *    a singular matrix -- with the message naming the draw ("draw i").  ATMO_E_STATE: a context outside the default forms, with the single draw's message
 *    (atmo_set_precision 1, at most 32 view steps, one lane per ray); a context whose textures are not set; a capturing stream (the table is
 *    context-owned, as in the other batches).  Argument errors that need no matrix arithmetic come in front of the mode check, for all draws; a singular
 *    matrix may be reported behind it.  The message is stored on the context of the draw it names; a message that names no draw on draws[0].ctx; where that
 *    is null, or draws is, or n_draws is negative, in the slot atmo_last_error_string(NULL) reads.
 *  - Nothing to draw.  n_draws == 0, or no draw with a tile: ATMO_OK, no launch and no staging slot.
 *  - The same context may appear more than once (stereo: the planet once per eye).
 *  - Call behaviour.  As atmo_render_views_proxy: the call only enqueues.  A launch takes one of the 16 staging slots of its first context's ring; a call
 *    that needs more than 16 launches from one ring may wait on the host for its own earlier launches.
 *
 * WHERE IT IS SLOWER than the n atmo_render_proxy_target calls (measured on an MI355X against the parent commit's library, RGBA16F composites at
 * 1920 x 1080, a still camera, profiles/planets/README.md; six planets apart on screen are faster everywhere measured: 0.43 of the sequential time for the
 * 8-step baked-LUT atmosphere, 0.48 for the direct-light one, 0.22 for clouds_high and clouds_high_rm, 0.40 for three cloud planets beside three cloudless
 * ones): draws that TOUCH.  A planet with a moon in front of it are two levels and two launches -- the single draws' work, plus a copy of the constants and an
 * event per launch: 249.3 against 234.1 us per frame, +6.5 %, with spreads of 0.5 % in both arms.  The call is for frames in which most planets are apart.
 */
#ifndef ATMO_PLANETS_H
#define ATMO_PLANETS_H

#include "atmo_views_proxy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATMO_MAX_PLANET_DRAWS 64

typedef struct AtmoPlanetDraw {
    AtmoContext *ctx;          /* the planet: its uniforms, textures, variant, modes */
    AtmoFrame frame;           /* as atmo_render_proxy_target's (the varyings differ per planet; viewport and rect may too) */
    float model_matrix[16];    /* the node's global transform, column-major */
    float box_size;
    const float *depth_dev;
    AtmoTarget target;         /* composite addressing: the viewport's first pixel; any of the seven formats, a row pitch */
} AtmoPlanetDraw;

/* draws[0 .. n_draws) blended in place in LIST ORDER (the caller sorts back to front), in as few launches as the plan above allows. */
int atmo_render_planets(const AtmoPlanetDraw *draws, int n_draws, void *stream);

/* The plan only; no device is needed and the pointers are not dereferenced: launch_of[i] = the index of the launch that holds draw i, or -1 when it has no
 * tile (n_draws entries); *n_launches = the number of launches.  Either output may be null. */
int atmo_plan_planets(const AtmoPlanetDraw *draws, int n_draws, int *launch_of, int *n_launches);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_PLANETS_H */
