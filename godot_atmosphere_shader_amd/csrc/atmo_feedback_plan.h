// The tile-order feedback's POLICY (host only; no HIP call, no context): which order a draw uses, whether it records tile costs, where the sort runs and
// how far the cost map is dilated, as a pure function of the context's knobs, the kernel family and a snapshot of the state's counters.  The MECHANISM is
// atmo_api.hip's; render_impl and views_enqueue act on what feedback_plan returns, atmo_debug_feedback_plan (include/atmo_debug.h) exposes it to the tests.
#pragma once

#include "../../include/atmo_debug.h"
#include "atmo_device.h"

#include <cmath>

namespace atmo {

constexpr float FB_STILL_PX = 0.5f;   // pixels per frame below which a camera counts as still (tile feedback)
// A moving camera (planet_atmosphere.gd:285-341 writes new matrices every frame; demo/avatar.gd, demo/mouse_look.gd): an order
// is used fb_lag frames after the costs it was sorted from were measured.  The host predicts how far the picture's features
// move in that time; the sort dilates the cost map by that distance, so a tile counts as cheap only if everything within
// reach of it was cheap (atmo_tile_dilate_kernel); costs are recorded every 2nd draw instead of every fb_period-th while
// the camera moves; and an order whose reach the motion has outrun is not used (row-major instead).
// reach beyond which an order says nothing about the frame it would be used on: 160 px for the in-stream sort (a frame of lag),
// 48 px for the side-stream sort (four to six frames of lag: measured, recording every 2nd frame without a usable order costs 1-2 %)
constexpr float FB_MAX_REACH_PX = 160.0f, FB_MAX_REACH_SIDE_PX = 48.0f, FB_INSTREAM_PX = 3.0f, FB_INSTREAM_LONG_PX = 8.0f;

enum : int32_t { FB_ORDER_NONE = 0, FB_ORDER_SIDE = 1, FB_ORDER_INSTREAM = 2 };   // AtmoFeedbackPlanOut::order

// Every fb_period-th draw records the wave durations per tile; a sort on the side stream turns them into the next
// order, which later draws pick up once a host-side event query says it is complete: no draw ever waits for a sort.
// `in` holds the state's counters as they stand after the motion update and the poll of the pending sort.
static inline AtmoFeedbackPlanOut feedback_plan(const AtmoFeedbackPlanIn &in) {
    AtmoFeedbackPlanOut out = {FB_ORDER_NONE, 0, 0, 0, 0, 0, 0.0f, 0};
    float motion_px = in.motion_px;
    if (in.batch) {
        // One order over all views of a batch, learnt as a single draw's on a still camera.  While any view moves (motion_px: the fastest view's), the
        // batch is neither ordered nor recorded (no dilation per view: atmo_views.h); a still batch follows the single draw's rule for a camera at rest.
        if (motion_px > FB_STILL_PX) {
            out.invalidate_active = 1;
            return out;
        }
        motion_px = 0.0f;
    }
    const bool moving = motion_px > FB_STILL_PX;
    const unsigned period = moving ? (in.fb_period < in.moving_period ? in.fb_period : in.moving_period) : in.fb_period;
    // what an order sorted now would have to cover: it is in use from ~2 frames after its recording draw until the next takes over
    const float want_reach = moving ? motion_px * (float)(period + 4u) * in.reach_scale : 0.0f;
    // nothing measured now says anything about the frame it would order -- or the frames are so short (the baked-LUT atmosphere
    // without clouds: 20-50 us, +3 % from the order at best) that recording and sorting every other frame costs more than it brings
    const bool short_frames = !(in.flags & (KF_CLOUDS | KF_LIGHT_DIRECT));
    const bool too_fast = want_reach > FB_MAX_REACH_SIDE_PX || (moving && short_frames);
    // In-stream mode: while the camera moves by more than a few pixels per frame, the kernels whose cost map is worth it
    // (raymarched cloud light: the heaviest tiles cost 10x the mean, frames of 0.4-1.3 ms, +48 % from the order on a still
    // camera) sort on the DRAW stream, right behind every draw.  The next draw is then ordered by this frame's costs -- one
    // frame of lag instead of four to six, so the dilation stays at a tile or two and the order keeps its meaning -- at the
    // price of ~10 us of sort kernels on the critical path per frame.  Measured (profiles/round3/ab_tile_feedback_motion.txt):
    // clouds_high_rm panning 1 degree per frame +20 % in-stream against +7 % with the side-stream sort, but 35 % against 37 %
    // at 0.1 degree per frame; clouds_high (0.18 ms frames, +7 % at best) loses 7 % in-stream: side stream only.
    // one frame of lag and one of margin -- of the silhouette's motion when the window is taken from it (below)
    const float is_reach = (in.axis_windows ? std::fmax(in.sil_px[0], in.sil_px[1]) : motion_px) * 2.0f * in.reach_scale;
    // Which kernels: raymarched cloud light from 3 px per frame; since round 4 (per-axis windows) also the other 64-step cloud kernels in
    // the precise mode (0.2 ms frames: +10..13 % where the side-stream order had nothing left, measured from 8 px per frame; at 1.4 px per
    // frame the side stream is 2-3 points better).  Shorter frames (`clouds`, the fast cloud mode: 0.12-0.16 ms) are neutral in-stream
    // (-0.4..+3 %) and stay on the side stream; the cloudless direct-light kernel LOSES 9-12 % in-stream under a pan (ATMO_FB_INSTREAM=2).
    const bool is_rm = (in.flags & KF_CLOUD_LIGHT_RM) != 0;
    const bool is_long = (in.flags & KF_CLOUDS) && (in.flags & KF_PRECISE) && in.cloud_steps >= 64;
    const bool is_kernel = in.instream == 2 ? (in.flags & (KF_CLOUDS | KF_LIGHT_DIRECT)) != 0 : (is_rm || (is_long && in.axis_windows));
    const float is_px = is_rm ? FB_INSTREAM_PX : FB_INSTREAM_LONG_PX;
    const bool instream = in.instream && motion_px >= is_px && is_kernel && !in.pending && is_reach <= FB_MAX_REACH_PX;
    const float tile_h = (float)(in.tile_h > 0 ? in.tile_h : 8);   // pixel rows per tile of this launch (8, or 4 with two lanes per ray)
    if (instream) {
        if (in.is_last_n + 1u == in.n) out.order = FB_ORDER_INSTREAM;  // the sort behind the previous draw of this key wrote the in-stream order
        out.record = 1;
        out.sort_instream = 1;
        out.reach_px = is_reach;
        out.dil_rx = (int)std::ceil(out.reach_px / 16.0f);
        out.dil_ry = (int)std::ceil(out.reach_px / tile_h);
        if (in.axis_windows) {
            // Round 4: the window per screen axis, from the motion of the planet's SILHOUETTE alone (two frames of it, one tile at least).  The
            // expensive tiles of these kernels sit on the limb, which an orbit leaves where it is while the surface points behind motion_px sweep
            // across the disc: the isotropic window (7 x 13 tiles at 1 degree of orbit per frame) buried the ranking of exactly those tiles, and
            // a pan needs nothing vertically (profiles/round4/ab_tile_feedback_motion.txt).
            out.dil_rx = (int)std::ceil(2.0f * in.sil_px[0] * in.reach_scale / 16.0f);
            out.dil_ry = (int)std::ceil(2.0f * in.sil_px[1] * in.reach_scale / tile_h);
            out.dil_rx = out.dil_rx < 1 ? 1 : (out.dil_rx > 10 ? 10 : out.dil_rx);
            out.dil_ry = out.dil_ry < 1 ? 1 : (out.dil_ry > 10 ? 10 : out.dil_ry);
        }
        out.invalidate_active = 1;  // whatever the side stream sorted last belongs to an older picture
        return out;
    }
    if (in.active >= 0) {
        // still conservative?  features have moved about motion_px * (frames since the costs were measured)
        const float moved = motion_px * (float)(in.n - in.order_born);
        if (moved <= in.order_reach_px + 8.0f) out.order = FB_ORDER_SIDE;
    }
    // the first two draws of a key are not measured (cold clocks and caches rank the tiles poorly); the next four
    // record back to back (the order settles in a few frames), then every period-th
    if (!too_fast && !in.pending && in.n >= 2 && (in.n < 6 || in.n - in.last_record >= period)) {
        out.record = 1;
        out.sort_side = 1;
        out.reach_px = want_reach;
        out.dil_rx = out.reach_px > 0.0f ? (int)std::ceil(out.reach_px / 16.0f) : 0;
        out.dil_ry = out.reach_px > 0.0f ? (int)std::ceil(out.reach_px / tile_h) : 0;
    }
    return out;
}

}  // namespace atmo
