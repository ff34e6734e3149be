/*
 * atmo_detail_target.h -- full-quality clouds into a renderer's colour and depth buffers (libatmo_hip.so, ABI version 5).  Included after atmo_depth.h,
 * atmo_views_target.h and atmo_cloud_detail.h (it includes them); same conventions.
 *
 * atmo_set_cloud_detail (atmo_cloud_detail.h) is the reference's `#define CLOUDS_ALWAYS_LOW_QUALITY` commented out at run time: the detail fetch of
 * get_density_full, live AtmoFrame::time, the alpha0 < 0.3 branch of the raymarched cloud light.  atmo_render and atmo_render_composite draw it, into tight
 * float4 pixels from a tight float depth buffer; atmo_render_target, atmo_render_depth_target, atmo_render_views_target and
 * atmo_render_views_depth_target refuse a cloud context that has it on -- so the library's best picture was the one a renderer could not take without a
 * float4 copy of its colour buffer and a float copy of its depth buffer, the two conversion passes atmo_target.h and atmo_depth.h were written to remove.
 * The two entry points below are atmo_render_depth_target and atmo_render_views_depth_target with the refusal gone.  The older entry points refuse as
 * before.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the two symbols below up, binds them in place of the older target
 * calls, and toggles atmo_set_cloud_detail.  A plain float depth buffer is an AtmoDepth of ATMO_DEPTH_D32_SFLOAT with row_pitch_bytes 0, so there is one
 * single-draw entry point, not two.
 *
 * THE CONTRACT is the union of the three existing ones; this header adds no arithmetic of its own.
 *
 * CLOUD DETAIL IN EFFECT (the switch on and a cloud variant).
 *  - The shaded fp32 ALBEDO.rgb / ALPHA of a pixel are the bits atmo_render with the switch on produces for it, handed a tight float buffer that holds the
 *    decoded depth values (atmo_depth.h, THE NUMERICAL CONTRACT and PIXELS): every item of atmo_cloud_detail.h holds per sample.
 *  - The store, and the composite's decode / blend / encode, are atmo_target.h's contract in all seven formats, RGBA32F included, with or without a pitch.
 *  - Discarded fragments are stored as zero unless atmo_set_target_cleared, and never by a composite, which leaves their bytes alone.
 *  - A rect is the crop of the full frame, under the declared sampler too (pixels in front of an odd origin are shaded as helpers and store nothing).
 *  - AtmoFrame::time is live; in a batch each view's c = RN(time * 0.01f) is its own frame's.
 *  - In a batch, each view is bit for bit its own atmo_render_detail_target draw.  One target format per batch, and the overlap rule of
 *    atmo_views_target.h, as they stand there.
 * atmo_kernel_name reports atmo_detail_target_kernel<FLAGS | 8192 | 4096 | 1024, 0> (13329, 13331, 13337; under the declared sampler 13361, 13363,
 * 13369) and atmo_detail_views_target_kernel<FLAGS | 8192 | 4096 | 2048 | 1024, 0> (15377 ... 15417).
 *
 * CLOUD DETAIL NOT IN EFFECT (the switch off, or a variant without clouds).  The calls ARE atmo_render_depth_target and atmo_render_views_depth_target: the
 * same kernels, the same bits, the same atmo_kernel_name, tile order and feedback, and the same answers with this header's entry point named in front.
 *
 * LAUNCH.  With detail in effect: row-major, and view-major for the batch; no learnt tile order, no cost recording, nothing beside the draw stream, as
 * atmo_render's detail draw.  The single draw allocates nothing and can be captured into a HIP graph.  The batch follows
 * atmo_render_views_depth_target's rule on capture (refused: context-owned per-view constants) and uses its staging ring.
 *
 * UNCHANGED.  Every entry point atmo_cloud_detail.h lists as refusing keeps refusing: the proxy draws, atmo_render_planets, tile lists, cost measurements
 * and the older target calls.  The proxy (far-mode) draws have no detail form: the detail fetch's frequency, 15 x the shape's, is below a pixel at the
 * distances a proxy is drawn from.
 */
#ifndef ATMO_DETAIL_TARGET_H
#define ATMO_DETAIL_TARGET_H

#include "atmo_cloud_detail.h"
#include "atmo_depth.h"
#include "atmo_views_target.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * atmo_render_depth_target for a context of any atmo_set_cloud_detail state.  The call only enqueues on `stream`.
 *
 * Checked in this order, before the device is touched (a context of atmo_debug_create_host_only answers the same up to ATMO_E_NO_DEVICE); every message
 * names this entry point:
 *   ATMO_E_ARG    a null ctx (no message)
 *   ATMO_E_ARG    atmo_render_depth_target's argument checks in its order: the frame, the target (null, unknown format, null or misaligned pixels), the
 *                 viewport and the rect, the target's pitch
 *   ATMO_E_STATE  the mode.  Detail in effect: no cloud-detail kernel for atmo_set_precision 0 or 2, atmo_set_lane_split 2, the direct light mode or more
 *                 than 32 view steps (the message names cloud detail).  Not in effect: atmo_render_depth_target's "no depth-source kernel" refusal
 *   ATMO_OK       an empty rect: nothing is enqueued, the depth is not looked at
 *   ATMO_E_ARG    the depth source (null, unknown format, null or misaligned texels, bad pitch)
 *   ATMO_E_STATE  u_optical_depth_texture / u_cloud_shape_texture not set, as every draw
 *   ATMO_E_NO_DEVICE  a host-only context
 */
int atmo_render_detail_target(AtmoContext *ctx, const AtmoFrame *frame, const AtmoDepth *depth, const AtmoTarget *target, int composite, void *stream);

/*
 * atmo_render_views_depth_target for a context of any atmo_set_cloud_detail state: its checks in its order under this entry point's name -- the count
 * (n_views == 0 is ATMO_OK), null views, every view's frame, then per non-empty view the target, the depth source, one format per batch and the overlap
 * rule (a refusal that concerns one view names it) -- then the mode as above (ATMO_E_STATE), the textures, ATMO_E_NO_DEVICE.  A batch whose rects are all
 * empty is ATMO_OK behind the mode check, as there.
 */
int atmo_render_views_detail_target(AtmoContext *ctx, const AtmoViewDepthTarget *views, int n_views, int composite, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_DETAIL_TARGET_H */
