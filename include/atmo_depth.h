/*
 * atmo_depth.h -- reading the depth buffer a renderer owns, in its own format and row pitch (libatmo_hip.so, ABI version 5).  Included after atmo.h;
 * same conventions.  It is atmo_target.h mirrored onto the input side.
 *
 * Every other entry point takes `const float *depth_dev`: viewport_h rows of exactly viewport_w floats (D32_SFLOAT, tight).  A renderer's depth buffer
 * is often not that: Godot 4.3 allocates its 3-D depth buffer as D24_UNORM_S8 where the device offers it, mobile and XR depth swapchains are often
 * D16_UNORM, the two eyes of a stereo frame share one double-wide image, and an imported linear image has a row pitch that need not be width * 4.
 * The calls below are the packed-target draws of atmo_target.h, atmo_views_target.h and atmo_views_proxy.h with the depth sample read in the buffer's
 * own format, so a host neither runs a conversion pass nor keeps a float copy of its depth buffer.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbols below up, and asks atmo_depth_texel_bytes(format) != 0
 * for each format it wants.
 *
 * THE NUMERICAL CONTRACT (exact: no tolerance; godot_atmosphere_shader_amd/depth_formats.py states the same in numpy, tests/test_depth_gpu.py holds the
 * kernels to it on every D16 code and every 24-bit code):
 *  - D32_SFLOAT: the float, its bits passed through (NaN, infinities, -0 and subnormals as atmo_render reads them).
 *  - D16_UNORM: d = (float)code / 65535.0f, ONE IEEE fp32 division (Vulkan's UNORM rule).
 *  - X8_D24_UNORM: d = (float)(word & 0xFFFFFF) / 16777215.0f, ONE IEEE fp32 division.  Bits 24-31 are IGNORED: a stencil byte up there does no harm.
 *    Anchors (fp32 bits): D16 1 -> 0x37800080, 32768 -> 0x3f000080, 65534 -> 0x3f7fff00, 65535 -> 0x3f800000; X8_D24 1 -> 0x33800001,
 *    8388608 -> 0x3f000001, 16777214 -> 0x3f7fffff, 16777215 -> 0x3f800000.  Only the top code decodes to 1.0 and only 0 to 0.0, so both far planes --
 *    reverse-Z 0 and forward-Z 1 -- are exact.
 *  - PIXELS: every draw below writes, byte for byte, what the entry point of the same name without `depth_` writes when it is handed a tight float
 *    buffer holding the decoded values.  Everything else is that draw's: discards, atmo_set_target_cleared, the composite rules, proxy coverage; tile
 *    order and feedback, the heavy-tile lane split; stream rules; nothing is allocated, so a single draw can be captured into a HIP graph.
 *
 * Targets: all seven formats of atmo_target.h, RGBA32F included, with or without a pitch.
 *
 * Modes: the kernels exist for the forms a default context draws with (atmo_target.h "Modes": atmo_set_precision 1, up to 32 view steps,
 * atmo_set_lane_split 0 / 1); otherwise ATMO_E_STATE -- for an RGBA32F target too, which these calls draw with kernels of their own.
 *
 * Not here: depth sources for the float4-only entry points (use RGBA32F through these calls), the tile-list draws and atmo_measure_tile_costs,
 * atmo_render_planets; 8-byte D32_SFLOAT_S8 texels, multisampled depth and tiled (non-linear) images.
 */
#ifndef ATMO_DEPTH_H
#define ATMO_DEPTH_H

#include "atmo.h"
#include "atmo_scene.h"
#include "atmo_target.h"
#include "atmo_views.h"

#ifdef __cplusplus
extern "C" {
#endif

enum AtmoDepthFormat {
    ATMO_DEPTH_D32_SFLOAT = 0,   /* 4-byte texel: the float, bits passed through */
    ATMO_DEPTH_D16_UNORM = 1,    /* 2-byte texel (VK_FORMAT_D16_UNORM) */
    ATMO_DEPTH_X8_D24_UNORM = 2  /* 4-byte little-endian word, depth in bits 0-23, bits 24-31 ignored: what a buffer copy of the depth aspect of
                                    VK_FORMAT_D24_UNORM_S8_UINT / VK_FORMAT_X8_D24_UNORM_PACK32 produces */
};

typedef struct AtmoDepth {
    const void *texels;       /* device pointer to the VIEWPORT's first texel (whatever the rect); aligned to the texel size */
    int32_t format;           /* AtmoDepthFormat */
    int32_t row_pitch_bytes;  /* bytes from one row to the next of the viewport_h rows; 0 = tight (viewport_w * texel size); otherwise >= that and a
                                 multiple of the texel size */
} AtmoDepth;

/* Bytes per texel of a format: 4 / 2 / 4; 0 for a format this library does not know -- the capability query. */
int atmo_depth_texel_bytes(int format);

/*
 * atmo_render_target with the depth buffer `depth`.  ATMO_E_ARG, where atmo_render_target refuses a null depth_dev: null depth or texels, unknown
 * format, misaligned texels, bad pitch.  The order of refusals is otherwise atmo_render_target's.
 */
int atmo_render_depth_target(AtmoContext *ctx, const AtmoFrame *frame, const AtmoDepth *depth, const AtmoTarget *target, int composite, void *stream);

/* atmo_render_proxy_target with the depth buffer `depth`. */
int atmo_render_proxy_depth_target(AtmoContext *ctx, const AtmoFrame *frame, const float *model_matrix, float box_size, const AtmoDepth *depth,
                                   const AtmoTarget *target, int composite, void *stream);

typedef struct AtmoViewDepthTarget {
    AtmoFrame frame;    /* as AtmoViewTarget's */
    AtmoDepth depth;    /* this view's depth buffer: formats and pitches may differ between the views of a batch */
    AtmoTarget target;  /* as AtmoViewTarget's: one format per batch, and the overlap rule of atmo_views_target.h */
} AtmoViewDepthTarget;

/*
 * atmo_render_views_target / atmo_render_views_proxy_target (atmo_views_target.h, atmo_views_proxy.h) with a depth buffer per view.  The side-by-side
 * halves of one double-wide depth image are texels = image and image + half_width * texel size, row_pitch_bytes = the image's row.  A refusal that
 * concerns one view's depth names the view.
 */
int atmo_render_views_depth_target(AtmoContext *ctx, const AtmoViewDepthTarget *views, int n_views, int composite, void *stream);
int atmo_render_views_proxy_depth_target(AtmoContext *ctx, const AtmoViewDepthTarget *views, int n_views, const float *model_matrix, float box_size,
                                         int composite, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_DEPTH_H */
