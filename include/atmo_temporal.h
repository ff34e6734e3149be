/*
 * atmo_temporal.h -- a draw that marches ONE pixel of every scale x scale block a frame and takes the others from the last frame's result, reprojected
 * (libatmo_hip.so, ABI version 5).  Included after atmo_reduced.h (it includes it); same conventions.
 *
 * The reference's author describes the technique (Horizon Zero Dawn's clouds) and what it needs that a Godot shader cannot have: two extra render targets
 * and the current and previous depth.  A library with caller-owned buffers can: atmo_render_temporal_target gathers the depth of this frame's texel of
 * every block, draws that low frame with the kernels atmo_render draws with, and resolves every full-resolution pixel: the pixels marched this frame
 * from the low frame, the others from the previous history where it is still the same surface, and from atmo_reduced.h's depth-aware spatial filter where
 * it is not.  Under a still camera scale^2 calls leave every pixel of the history holding a ray marched at its own centre: full-resolution sampling at
 * the reduced draw's cost per frame.  Under motion a pixel is at most scale^2 - 1 frames old.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up.
 *
 * THE CONTRACT is exact: godot_atmosphere_shader_amd/temporal.py states every step in numpy, fp32, unfused, in a fixed order, every quotient IEEE, and
 * tests/test_temporal_gpu.py holds the kernels to it bit for bit.  With W x H the viewport, s the scale, low_w = ceil(W / s), low_h = ceil(H / s):
 *
 *  1. PHASE.  A phase p in 0 .. s^2 - 1 names the texel of every block that this frame marches: (ox, oy) = (p mod s, p div s).  The caller may pass any
 *     phase.  atmo_temporal_phase(s, f) is the Bayer order, in which consecutive frames are far apart in the block, at f mod s^2 (the non-negative
 *     remainder):   s = 2:  0 3 1 2      s = 4:  0 10 2 8 5 15 7 13 1 11 3 9 4 14 6 12.   Its period is s^2 and it visits every phase once.
 *
 *  2. THE PHASE FRAME is low_frame of atmo_reduced.h, item 2, with one more term in the translation: the centre of low pixel i lies on the centre of full
 *     pixel i s + ox (and j s + oy).  Column 0 = kx M0, column 1 = ky M1, column 3 = (M0 tx + M1 ty) + M3 with
 *         tx = (kx - 1) + (2 ox + 1 - s) / W,   ty = (ky - 1) + (2 oy + 1 - s) / H,
 *     everything in double, rounded once per element (always: the translation is never 0).  Low pixels whose full pixel does not exist (i s + ox >= W or
 *     j s + oy >= H) are drawn and never read.
 *
 *  3. THE PHASE DEPTH.  Low texel (i, j) is the DECODED depth (atmo_depth.h), bits untouched, of texel (min(i s + ox, W - 1), min(j s + oy, H - 1)).
 *
 *  4. HISTORY.  Two caller-owned buffers of one layout, one read (previous) and one written (current); the caller swaps them each frame; they may not
 *     overlap.  The layout: W H float4, (rgb, alpha) straight as atmo_render writes them; then W H float, the reciprocal eye depth q (atmo_reduced.h, item
 *     3) of the pixel's own depth in its own frame; then W H uint8, the age.  Each part is padded to a multiple of 16 bytes, rows are tight, and
 *     atmo_temporal_size gives the byte count.  Age 255 means "not history": such a texel is never reused.
 *
 *  5. RESOLVE of full pixel (x, y).  nx, ny = the draws' NDC of the pixel (atmo_reduced.h, item 3), d0 its own decoded depth, m = inv_projection_matrix,
 *         V[r] = ((m[r] nx + m[4 + r] ny) + m[8 + r] d0) + m[12 + r],  r = 0 .. 3,      q0 = V[3] / V[2]   (item 3's q, the same operations).
 *
 *   5a. FRESH.  x mod s == ox and y mod s == oy: the pixel is low texel (x div s, y div s), bits untouched; age 0.
 *
 *   5b. REPROJECTION (every other pixel, unless `reset`).  With P = prev_clip_from_view (column-major; previous projection x previous view x current inverse
 *       view, formed by the caller and used as given) and R = prev_inv_projection:
 *         C[r] = ((P[r] V[0] + P[4 + r] V[1]) + P[8 + r] V[2]) + P[12 + r] V[3],  r = 0 .. 3  (V undivided: a reverse-Z sky texel under an infinite far
 *         plane has V[3] = 0 and reprojects as a direction);
 *         C[3] > 0 false: no history texel is valid.   u = C[0] / C[3],  v = C[1] / C[3],  dp = C[2] / C[3];
 *         fpx = ((u + 1) 0.5) W - 0.5,  fpy = ((v + 1) 0.5) H - 0.5   (the previous frame's pixel position; W, H as floats);
 *         qe = (((R[3] u + R[7] v) + R[11] dp) + R[15]) / (((R[2] u + R[6] v) + R[10] dp) + R[14])   (0 for that sky texel).
 *
 *   5c. VALIDITY of history texel (i, j), i and j floats that hold integers: 0 <= i < W and 0 <= j < H (no clamping; false for a NaN); its age < max_age;
 *       its stored q, qk:  |qe - qk| <= history_tolerance max(|qe|, |qk|)   (max = fmaxf; false where the difference is a NaN); and C[3] > 0.
 *
 *   5d. SNAP.  jx = floor(fpx + 0.5), jy = floor(fpy + 0.5).  If |fpx - jx| <= 1/64 and |fpy - jy| <= 1/64: where texel (jx, jy) is valid the pixel is
 *       that texel, bits untouched, its age the texel's + 1, saturating at 254; where it is not, the pixel goes to 5f with no bilinear attempt.
 *
 *   5e. BILINEAR (otherwise).  i0 = floor(fpx), fx = fpx - i0, gx = 1 - fx; the same along y.  Taps in the order 00, 10, 01, 11: (i0, j0), (i0 + 1, j0),
 *       (i0, j0 + 1), (i0 + 1, j0 + 1), with the weights gx gy, fx gy, gx fy, fx fy.  A tap counts when it is valid (5c) and its weight > 0.  Over the taps
 *       that count, in order, from zero: Wsum += w; A += w a; C += w (a rgb); where Wsum != 1, A and C are divided by it; the pixel is (C / A, A), its rgb 0
 *       where A > 0 is false (atmo_reduced.h, item 5).  Age: the largest of the counted taps' + 1, saturating at 254.  No tap counts: 5f.
 *
 *   5f. SPATIAL FALLBACK: atmo_reduced.h, item 5, over the phase-positioned low samples.  Along x: i0 = floor((x - ox) / s), fx = ((x - ox) - s i0) / s;
 *       neighbours i0 and i0 + 1, clamped to 0 .. max(ceil((W - ox) / s), 1) - 1, the low texels whose full pixel exists; the same along y.  The same
 *       weights in the same order (exact dyadics that sum to 1; here fx may be 0).  Neighbour k agrees when |q0 - qk| <= depth_tolerance max(|q0|, |qk|),
 *       qk the q of its low depth at the pixel's own (x, y), and counts when it agrees and its weight > 0.  None counts: the one with the smallest
 *       |q0 - qk| of the four (strict comparison, the first wins) counts alone, with weight 1.  The sums, the division and the pixel as in 5e.  Age 255.
 *
 *   5g. RESET.  reset != 0: every pixel that is not fresh takes 5f; the previous history is never read and may be null.
 *
 *   5h. OUTPUT.  The pixel, q0 and the age go into the current history (every pixel of the viewport, always).  The pixel goes into the target by item 6 of
 *       atmo_reduced.h: all seven formats, row pitch, plain or composite; a composite leaves a pixel whose A > 0 is false untouched in the target.
 *
 * WHAT LAGS.  The history is reprojected at the SCENE's depth.  A cloud in front of a distant surface moves across the screen, under a translating
 * camera, as its own distance says, not the surface's: it lags by at most s^2 - 1 frames, until its block's texel is marched again.  Rotation and a still
 * camera reproject exactly.
 *
 * SCRATCH as atmo_reduced.h's: low_w low_h floats padded to 16 bytes, then low_w low_h float4; 16-byte aligned.  The library allocates nothing and all
 * work is enqueued on the caller's stream in order.
 *
 * Not here: rects (the frame's rect must be the whole viewport), view batches, the proxy draws, tile lists and atmo_render_planets; reprojection through a
 * cloud shell (above); colour-neighbourhood clamping; jitter that changes per frame; scales other than 2 and 4.
 */
#ifndef ATMO_TEMPORAL_H
#define ATMO_TEMPORAL_H

#include "atmo_reduced.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AtmoTemporal {
    int32_t scale;                  /* 2 or 4 */
    int32_t phase;                  /* 0 .. scale^2 - 1: the texel of every block marched this frame */
    float depth_tolerance;          /* 5f: as AtmoReduced's; finite, >= 0 */
    float history_tolerance;        /* 5c: the relative difference of reciprocal eye depth up to which a history texel is the same surface; finite, >= 0 */
    int32_t max_age;                /* 1 .. 255: a history texel is reused while its age is below this */
    int32_t reset;                  /* != 0: the previous history is not read */
    float prev_clip_from_view[16];  /* column-major: previous projection x previous view x current inverse view */
    float prev_inv_projection[16];  /* column-major: the previous frame's inv_projection_matrix */
} AtmoTemporal;

/*
 * The low frame's size, the scratch's bytes (atmo_reduced_size's) and one history buffer's bytes; any of the four outputs may be null.  Needs no context.
 * ATMO_E_ARG: a viewport outside 1 .. 65536, a scale other than 2 and 4.
 */
int atmo_temporal_size(int viewport_w, int viewport_h, int scale, int *low_w, int *low_h, size_t *scratch_bytes, size_t *history_bytes);

/* Item 1's sequence at frame_index (any int); -1 for a scale other than 2 and 4. */
int atmo_temporal_phase(int scale, int frame_index);

/*
 * Item 3: low_depth_dev (low_w low_h floats, tight) from the depth buffer `depth`.  Only enqueues on `stream`.
 * Checked in atmo_reduced_depth's order under this entry point's name, with "phase must be 0 .. scale^2 - 1" behind the scale.
 */
int atmo_temporal_depth(AtmoContext *ctx, const AtmoFrame *frame, const AtmoDepth *depth, int scale, int phase, float *low_depth_dev, void *stream);

/*
 * Item 5: the low frame low_rgba_dev (low_w low_h float4, tight) of phase opt->phase with its depth low_depth_dev, the previous history and the depth
 * buffer into the current history and `target` (addressed as atmo_reduced_upsample's).  Only enqueues on `stream`.
 * Checked in atmo_reduced_upsample's order and wording under this entry point's name -- the frame, the target, null opt, the scale, depth_tolerance, the
 * rect --, then: a phase outside 0 .. scale^2 - 1; a history_tolerance that is negative or not finite; max_age outside 1 .. 255; the two low buffers as
 * atmo_reduced_upsample; null history_cur_dev, a history not aligned to 16 bytes; histories that overlap; a null history_prev_dev without reset; the depth
 * source; ATMO_E_NO_DEVICE a host-only context.
 */
int atmo_temporal_resolve(AtmoContext *ctx, const AtmoFrame *frame, const AtmoDepth *depth, const AtmoTemporal *opt, const float *low_depth_dev,
                          const float *low_rgba_dev, const void *history_prev_dev, void *history_cur_dev, const AtmoTarget *target, int composite,
                          void *stream);

/*
 * The whole path on `stream`: atmo_temporal_depth into the scratch; the launch atmo_render makes for the phase frame (item 2) with that depth, into the
 * scratch's float4 frame -- cloud detail, lane split, precision, tile order and its feedback as atmo_render_reduced_target has them --;
 * atmo_temporal_resolve.  atmo_kernel_name reports the low draw's kernel.
 * Checked in atmo_temporal_resolve's order under this entry point's name, with "null or misaligned (16 bytes) scratch_dev" in the place of the two low
 * buffers; then, behind the depth source, ATMO_E_STATE where atmo_render would refuse the low frame, and ATMO_E_NO_DEVICE.  Nothing is enqueued by a
 * refused call.
 */
int atmo_render_temporal_target(AtmoContext *ctx, const AtmoFrame *frame, const AtmoDepth *depth, const AtmoTemporal *opt, void *scratch_dev,
                                const void *history_prev_dev, void *history_cur_dev, const AtmoTarget *target, int composite, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_TEMPORAL_H */
