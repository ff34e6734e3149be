/*
 * atmo_reduced.h -- a draw at half or quarter resolution, put into the renderer's full-resolution colour buffer by a filter that respects depth edges
 * (libatmo_hip.so, ABI version 5).  Included after atmo_depth.h (it includes it); same conventions.
 *
 * A cloud draw is what a frame pays for, and its cost is per pixel.  atmo_render_reduced_target marches 1 / scale^2 of the pixels: it reduces the depth
 * buffer to one texel per scale x scale block, draws the low frame with the kernels atmo_render draws with, and upsamples the result into the target --
 * bilinear, each of the four low neighbours weighed only where its depth agrees with the full-resolution pixel's own, in any of the seven target formats,
 * plain or blended.  Spatial only: no history buffer, no reprojection, no interleaving.  The host writes neither the depth reduction nor the upsample.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up.
 *
 * THE CONTRACT is exact: godot_atmosphere_shader_amd/reduced.py states every step in numpy, fp32, unfused, in a fixed order, and tests/test_reduced_gpu.py
 * holds the kernels to it bit for bit.  With W x H the viewport and s the scale:
 *
 *  1. SIZES.  low_w = ceil(W / s), low_h = ceil(H / s).
 *
 *  2. THE LOW FRAME is the caller's frame with viewport (low_w, low_h), the whole of it as its rect, and inv_projection_low = inv_projection * A, where A is
 *     the identity with A[0][0] = kx, A[1][1] = ky and the translation column (kx - 1, ky - 1, 0, 1); kx = low_w s / W, ky = low_h s / H (quotients in
 *     double).  The centre of low pixel i lies where the centre of its block lies in the full frame.  The product is formed in double -- column 0 = kx M0,
 *     column 1 = ky M1, column 3 = (M0 (kx - 1) + M1 (ky - 1)) + M3 -- and rounded once per element; with kx = ky = 1 (s divides W and H) the matrix is the
 *     caller's, bits untouched.
 *
 *  3. RECIPROCAL EYE DEPTH of depth d seen through pixel (px, py):  n = 2 ((p + 0.5) / size) - 1 (the draws' own NDC: one IEEE quotient), and with
 *     m = inv_projection_matrix (column-major)
 *         z = m[2] nx + m[6] ny + m[10] d + m[14],   w = m[3] nx + m[7] ny + m[11] d + m[15],   q = w / z
 *     summed left to right.  0 for a reverse-Z sky texel under an infinite far plane; defined for forward-Z, orthographic and off-axis matrices alike.
 *
 *  4. DEPTH REDUCTION.  Low texel (i, j) covers the texels of its block that exist and is written with the DECODED depth (atmo_depth.h), bits untouched, of
 *     ONE of them: where i + j is even the one with the smallest |q| (the farthest), where odd the one with the largest (the nearest) -- a checkerboard,
 *     so that both sides of a depth edge are present among any pixel's neighbours.  The block is scanned row-major from its first texel with a strict
 *     comparison: ties keep the earlier texel, and a NaN never replaces the current choice.
 *
 *  5. UPSAMPLE of full pixel (x, y).  Along x: t = 2 x + 1 - s, i0 = floor(t / 2 s), fx = (t - 2 s i0) / 2 s; neighbours i0 and i0 + 1, clamped to the low
 *     image; the same along y.  Weights in the order 00, 10, 01, 11: (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy -- exact dyadics that sum to 1.
 *     q0 = q of the pixel's own depth; qk = q of neighbour k's low depth AT THE PIXEL'S OWN (x, y).  Neighbour k is valid when
 *         |q0 - qk| <= depth_tolerance * max(|q0|, |qk|).
 *     No neighbour valid: the one with the smallest |q0 - qk| (strict comparison, the first wins) counts as the only valid one, with weight 1.
 *     Over the valid neighbours in order, from zero:  Wsum += w;  A += w a;  C += w (a rgb)  -- premultiplied, so that the (0, 0, 0, 0) of a discarded
 *     low pixel does not darken the limb.  Where Wsum != 1, A and C are divided by it.  The pixel is (C / A, A), its rgb 0 where A > 0 is false.
 *
 *  6. STORE.  The pixel goes where a draw's pixel goes: atmo_target.h's contract.  A plain call encodes it (every pixel of the viewport is written).  A
 *     composite decodes the destination, blends (blend_mix) and encodes once, and leaves a pixel whose A > 0 is false untouched.  Bytes between rows are
 *     never written.
 *
 * SCRATCH.  The caller owns it: low_w low_h floats (the low depth), padded to a multiple of 16 bytes, then low_w low_h float4 (the low frame);
 * atmo_reduced_size gives the byte count; 16-byte aligned.  The library allocates nothing, and all work is enqueued on the caller's stream in order, so
 * atmo_render_reduced_target can be captured into a HIP graph wherever atmo_render can.
 *
 * A stereo pair is two calls on the halves of a double-wide image, through the pitch and pointer rules of AtmoDepth and AtmoTarget.
 *
 * Not here: rects (the frame's rect must be the whole viewport), view batches, the proxy draws, tile lists and atmo_render_planets; scales other than
 * 2 and 4; any temporal accumulation.
 */
#ifndef ATMO_REDUCED_H
#define ATMO_REDUCED_H

#include "atmo_depth.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AtmoReduced {
    int32_t scale;          /* 2 or 4 */
    float depth_tolerance;  /* the relative difference of reciprocal eye depth up to which a low neighbour counts; finite, >= 0 */
} AtmoReduced;

/*
 * The low frame's size and the scratch's bytes for a viewport and a scale; any of the three outputs may be null.  Needs no context.
 * ATMO_E_ARG: a viewport outside 1 .. 65536, a scale other than 2 and 4.
 */
int atmo_reduced_size(int viewport_w, int viewport_h, int scale, int *low_w, int *low_h, size_t *scratch_bytes);

/*
 * Step 4: low_depth_dev (low_w low_h floats, tight) from the depth buffer `depth` of the frame's viewport.  Only enqueues on `stream`.
 * Checked in this order, every message naming the entry point: ATMO_E_ARG a null ctx (no message); the frame, its viewport and rect; a scale other than
 * 2 and 4; a rect that is not the whole viewport; null or misaligned (4 bytes) low_depth_dev; the depth source (null, unknown format, null or misaligned
 * texels, bad pitch); ATMO_E_NO_DEVICE a host-only context.
 */
int atmo_reduced_depth(AtmoContext *ctx, const AtmoFrame *frame, const AtmoDepth *depth, int scale, float *low_depth_dev, void *stream);

/*
 * Steps 5 and 6: the low frame low_rgba_dev (low_w low_h float4, tight: ALBEDO.rgb, ALPHA as atmo_render writes them) with its depth low_depth_dev, into
 * `target`.  `target` is addressed as atmo_render_target's with composite != 0, whatever `composite` is here: pixels = the viewport's first pixel,
 * viewport_h rows of viewport_w pixels, row_pitch_bytes apart.  Only enqueues on `stream`.
 * Checked in this order: ATMO_E_ARG a null ctx (no message); the frame, then the target (null, unknown format, null or misaligned pixels), the viewport and
 * the rect, the target's pitch, as atmo_render_depth_target; null opt, a scale other than 2 and 4, a depth_tolerance that is negative or not finite; a rect
 * that is not the whole viewport; null low_depth_dev or low_rgba_dev, low_depth_dev not aligned to 4 bytes, low_rgba_dev not to 16; the depth source;
 * ATMO_E_NO_DEVICE a host-only context.
 */
int atmo_reduced_upsample(AtmoContext *ctx, const AtmoFrame *frame, const AtmoDepth *depth, const AtmoReduced *opt, const float *low_depth_dev,
                          const float *low_rgba_dev, const AtmoTarget *target, int composite, void *stream);

/*
 * The whole path on `stream`: atmo_reduced_depth into the scratch; the launch atmo_render makes for the low frame (step 2) with that depth, into the
 * scratch's float4 frame -- the same kernels in every mode atmo_render draws in, with cloud detail, lane split and precision as the context has them,
 * tile order and its feedback as atmo_render's --; atmo_reduced_upsample.  atmo_kernel_name reports the low draw's kernel.
 * Checked in atmo_reduced_upsample's order under this entry point's name, with "null or misaligned (16 bytes) scratch_dev" in the place of the two low
 * buffers; then, behind the depth source, ATMO_E_STATE where atmo_render would refuse the low frame (the mode of a cloud-detail draw, a demanded sampler
 * that cannot be had, textures not set), and ATMO_E_NO_DEVICE for a host-only context.  Nothing is enqueued by a refused call.
 */
int atmo_render_reduced_target(AtmoContext *ctx, const AtmoFrame *frame, const AtmoDepth *depth, const AtmoReduced *opt, void *scratch_dev,
                               const AtmoTarget *target, int composite, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_REDUCED_H */
