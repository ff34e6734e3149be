// atmo_device.h -- structures shared by the host API (atmo_api.hip) and the gfx950 kernels
// (atmo_kernels.hip).  Not part of the public C ABI (that is include/atmo.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace atmo {

// Everything a render launch needs that is constant over the draw.  Passed BY VALUE as the kernel
// argument, so every field lands in SGPRs through scalar loads of the kernarg segment.
// Values marked [host] are per-frame expressions of the reference shader that do not depend on the
// pixel; the API evaluates them once in fp32, in the reference's operation order.
constexpr int GEO_MAX_ROWS = 272;   // tile rows the geometric order covers: 3840 x 2160 in 8-pixel rows (taller grids: the learnt order)
constexpr int GEO_MAX_HINTS = 256;  // ... and 65 536 tiles, one hint per 256 blocks
struct RenderConsts {
    // --- atmosphere_fragment prologue (shaders/include/planet_atmosphere_main.gdshaderinc:128-169)
    float inv_p[16];
    float inv_v[16];
    float cam_pos_world[3];  // [host] inv_v * (0,0,0,1)                      main:136
    float vw, vh;            // VIEWPORT_SIZE as floats
    int32_t w, h;            // VIEWPORT_SIZE
    int32_t x0, y0, x1, y1;  // rect shaded by this launch
    float center[3];         // v_planet_center_viewspace
    float sun_dir[3];        // [host] normalize(sun_center_vs - planet_center_vs)   main:164
    float planet_radius, atmosphere_height;
    float atmosphere_radius; // [host] R + H                                   main:144
    float density;           // u_density
    float sphere_depth_factor;
    // --- compute_atmosphere_v2 (shaders/include/atmosphere_funcs_v2.gdshaderinc:32-101)
    float coeff[3];          // [host] pow4(400/lambda) * strength             v2:47-51
    float ambient[3], modulate[3];
    int32_t view_steps;
    int32_t light_steps;     // direct light mode only
    // --- compute_atmosphere, v1 "lite" (shaders/include/atmosphere_funcs_v1.gdshaderinc:8-12,48-63)
    float day0[3], day1[3], night0[3], night1[3];
    float day_night_transition_scale;
    // --- render_clouds / raymarch_cloud (shaders/include/cloud_funcs.gdshaderinc:175-324)
    float clouds_bottom, clouds_top;  // [host] R + u_cloud_{bottom,top} * H   clouds:260-261
    float cloud_thickness;            // [host] top - bottom
    float inv_cloud_thickness;        // [host] RN(1 / thickness), for exact_div_uniform
    float layer_r2_lo, layer_r2_hi;   // [host] (bottom (1 - 1e-6))^2, (top (1 + 1e-6))^2: |p|^2 outside [lo, hi] => surely outside the cloud layer
    float cloud_density_scale, cloud_blend, coverage_bias, shape_factor, shape_scale;
    int32_t shape_invert;             // u_cloud_shape_invert == 1.0           clouds:57
    float shape_lo01, shape_hi01;     // [host] bounds of (shape - 0.1) over every filtered texel value: coverage-first early outs
    float cov_rot[4];                 // mat2 column-major
    float view_to_model[16];          // [host] u_world_to_model_matrix * inv_view   clouds:285
    float origin_model[3];            // [host] (view_to_model * (0,0,0,1)).xyz      clouds:286
    float sun_dir_model[3];           // [host] (view_to_model * (sun_dir,0)).xyz    clouds:288
    float max_d;                      // [host] march-distance cap             clouds:186-202
    float inv_cloud_steps;            // [host] 1/float(steps)                 clouds:206
    int32_t cloud_steps;
    float rm_offset[6];               // [host] float(i) * step_len_i, step_len_i = reach/6 * 1.2^i   clouds:108,114-115,129,143
    float rm_weight[6];               // [host] step_len_i * density_scale     clouds:138
    float rm_tap[6][3];               // [host] rm_offset[i] * sun_dir_model: the uniform product of clouds:129, rounded once on the host
    // --- textures (device memory owned by the context)
    const float *lut;        // u_optical_depth_texture: (lut_h+2) rows of (lut_w+2), clamp-to-edge apron
    int32_t lut_w, lut_h;
    const float *lut4;       // what the kernels sample: (lut_h+1) rows of (lut_w+1) footprints, 4 floats = the 2x2 apron texels at (i,j),(i+1,j),(i,j+1),(i+1,j+1)
    const uint8_t *blue;     // u_blue_noise_texture 256x256
    const uint32_t *shape;   // u_cloud_shape_texture: n^3 xy-footprint words (repeat wrap baked in)
    int32_t shape_n;
    int32_t shape_log2n;     // [host] log2(shape_n) when it is a power of two, else -1 (shape_addr)
    const uint32_t *cube;    // u_cloud_coverage_cubemap: 6 x (n+1)^2 footprint words of the seamless-apron faces; null => 1.0
    int32_t cube_n;
    int32_t cube_levels;             // mip levels bound; level l = (cube_n >> l)-sided faces, footprints at cube + cube_level_off[l]
    const uint32_t *cube_level_off;  // device array of 16 element offsets
    uint32_t cube_bytes;             // bytes of the packed footprint chain (buffer-load bound)
    int32_t cube_lod_fast;           // 1: cube_n is a power of two <= 1024 (closed-form level offsets, fp32 addressing)
    float lod0_inv_c;                // [host] 1 / the level-0 certificate's constant C (cube_lod_level0_certain); +inf: never certain
    float lod0_last, lod0_drift;     // [host] cloud_steps - 1 and (cloud_steps + 1) * sqrt(3) 2^-23 (quad_march_spread2)
    // --- per-pixel streams
    const float *depth;      // h rows of w
    float4 *out;             // plain: (y1-y0) rows of (x1-x0); composite: the h x w scene colour buffer, blended in place
    int32_t out_pitch;       // pixels per output row
    int32_t out_x0, out_y0;  // viewport pixel that maps to out[0]
    int32_t composite;       // 1 => straight-alpha "mix" blend over the existing contents, discarded pixels untouched
    // --- launch order (atmo_set_tile_feedback)
    int32_t tiles_x;                // tiles per row of the launch grid
    const uint32_t *tile_order;     // null => tile = linear block index; else the tile each block shades (heaviest first)
    uint32_t *tile_cost;            // null => no feedback; else per-tile max wave duration in shader cycles (atomicMax)
#ifdef ATMO_WAVE_TRACE  // diagnostic build (tools/wave_timeline.py): 4 x uint64 per wave = start, end (100 MHz), HW_ID, XCC_ID
    unsigned long long *wave_trace;
#endif
    // --- exact short division of the pixel coordinates (pixel_coord in atmo_kernels.hip)
    float rcp_vw, rcp_vh;           // [host] RN(1 / vw), RN(1 / vh)
    // --- sure-miss test in front of the exact prologue (shade_pixel)
    const float *cube_f4;           // level 0 of `cube` with every footprint's four texels as exact byte / 255 floats (16 B), or null
    const float *shape_f4;          // the same for `shape`
    float miss_k;                   // [host] (|c|^2 - R_atm^2) (1 - 1e-3)^2 when the test is usable, else 0
    int32_t gx0, gy0;               // [host] viewport pixel of the launch grid's first tile: (x0, y0), rounded down to even for the declared-sampler kernels
    int32_t store_discards;         // 1: a discarded fragment stores (0,0,0,0); 0: it stores nothing (composite, or atmo_set_target_cleared)
    int32_t cost_rows_halved;       // 1: this launch draws HEAVY tiles of a one-lane grid as pairs of half-height tiles (render_impl's split path): tile_cost is indexed by the one-lane tile
    // --- the GEOMETRIC tile order of the cloudless variants (round 6; geo_tile in atmo_kernels.hip, geo_order_fill in atmo_api.hip).  Seen from outside the
    // atmosphere shell the tiles whose rays can hit it form ONE run of columns per tile row -- the shell's silhouette is a conic --, so "the tiles that shade
    // first, row-major, the all-miss tiles behind them" is a closed-form map from the block index to the tile: no order buffer, no recording draw, no sort,
    // nothing learnt from earlier frames and therefore nothing that lags behind a moving camera.  geo_rows = 0: off (tile = block index, or tile_order).
    int32_t geo_rows;                           // [host] tile rows of the launch grid, or 0
    uint16_t geo_prefix[GEO_MAX_ROWS + 1];      // [host] geo_prefix[r] = tiles that can shade in the rows above r; [geo_rows] = all of them
    uint8_t geo_first[GEO_MAX_ROWS];            // [host] first column of row r's run (its length: geo_prefix[r + 1] - geo_prefix[r])
    // where to start looking: geo_hint[0][v] = the last row r with geo_prefix[r] <= 256 v (blocks of the first part), geo_hint[1][v] = the last row r with
    // r tiles_x - geo_prefix[r] <= 256 v (blocks of the second part) -- the row of block b then lies in [hint[b >> 8], hint[(b >> 8) + 1]]: one or two steps of a
    // binary search instead of nine (every step is a dependent scalar load in every wave's preamble)
    uint16_t geo_hint[2][GEO_MAX_HINTS + 2];
    // --- what the camera and the uniforms make redundant in the prologue of the cloudless direct-light kernels (shade_pixel, march_atmosphere:
    // ATMO_PROLOGUE_CAMERA_FORMS; prologue_camera_fill in atmo_api.hip holds the predicates and their premises).  Behind every older field: no other kernel reads
    // them, and the older fields keep their places in the kernel-argument segment.
    uint32_t prologue_mode;         // [host] PM_* bits: which short forms give this draw the general forms' bits; 0 under the environment's ATMO_PROLOGUE_CAMERA=0
    int32_t cam_skip_px, cam_skip_py;   // [host] PM_CAMERA: the pixel column / row whose lanes must take the general rows (nx or ny = 0 under a -0 constant term), or -1
    float inv_view_steps;           // [host] 1 / view_steps, exact, under PM_POW2_STEPS; else 0
    float view_steps_f;             // [host] (float)view_steps
    float atmosphere_radius2;       // [host] atmosphere_radius^2, planet_radius^2, density^2, density^2 / 8, -coeff * LOG2E: one IEEE operation each, which the
    float planet_radius2;           //        kernels evaluated in vector instructions once per wave (gfx950 has no scalar float ALU)
    float dens2, dens2_8;
    float coeff_log2e[3];
};
// RenderConsts::prologue_mode
enum PrologueMode : uint32_t {
    PM_CAMERA = 1,           // perspective inv_projection (entries 1..4, 6..10 are zeros), rigid inv_view (bottom row 0 0 0 1)
    PM_POW2_STEPS = 2,       // view_steps is a power of two: x / n == x * inv_view_steps
    PM_NO_SPHERE_DEPTH = 4,  // sphere_depth_factor is a zero (and PM_CAMERA): the ground-sphere term of linear_depth is multiplied by zero
};

struct BakeConsts {
    float planet_radius, atmosphere_height, density;
    int32_t w, h, steps;
    float *out;  // (h+2) x (w+2), apron written by the edge texels' lanes
};

struct NoiseCubemapConsts {
    int32_t resolution;
    uint32_t seed;
    float frequency, gain;
    int32_t octaves;
    float scale[3];
    uint8_t *out;  // 6 faces of resolution^2 bytes
};

// the shape-volume generator (include/atmo_noise_volume.h): AtmoNoiseVolume's fields, the base period the host derived from them, where the texels go
struct NoiseVolumeConsts {
    int32_t n;           // the volume is n^3 texels, [z][y][x]
    uint32_t seed;
    float frequency, gain;
    int32_t octaves;
    float offset[3];
    int32_t seamless, invert, normalize;
    int32_t period0;     // seamless: P_0 = max(1, (int)rintf((float)n * frequency)); octave o tiles with P_0 << o lattice cells per side
    uint8_t *out;        // n^3 bytes
    uint32_t *minmax;    // normalize: ~bits(min t) and bits(max t) over the volume, both kept as maxima (t >= +0: unsigned order is float order)
};

// kernel launchers (atmo_kernels.hip)
enum KernelFlags : int { KF_CLOUDS = 1, KF_CLOUD_LIGHT_RM = 2, KF_LIGHT_DIRECT = 4, KF_LITE = 8, KF_PRECISE = 16, KF_CUBE_LOD = 32,
                          KF_ATMO_REF = 64 /* the v2 atmosphere march in the reference's operation order (atmo_set_precision 2) */,
                          KF_VIEW_POS = 128 /* view_steps > 32: the fast v2 march accumulates the view-space position like the reference (march_atmosphere<VIEWPOS>) */,
                          KF_GEO = 256 /* the block -> tile map is the geometric order's closed form (RenderConsts::geo_rows): a twin of the plain direct-light kernel, so that
                                          the draws that do not use it keep their preamble to the byte (the lookup compiled in cost a still camera 0.6 %) */,
                          KF_PROXY = 512 /* the far-mode BoxMesh draw (atmo_render_proxy, include/atmo_scene.h): shade_pixel first evaluates the proxy fragment test
                                            (ProxyConsts); its own kernel (atmo_render_proxy_kernel), so the kernels of atmo_render stay what they were */,
                          KF_TARGET = 1024 /* a packed colour target (atmo_render_target, include/atmo_target.h): shade_pixel's stores and its blend go through
                                              store_target<FMT> on TargetConsts instead of RenderConsts::out; kernels of their own (atmo_render_target_kernel,
                                              atmo_render_proxy_target_kernel), for the same reason */,
                          KF_VIEWS = 2048 /* several views in one launch (atmo_render_views, include/atmo_views.h): the block index runs over the concatenation of all
                                             views' tiles and shade_pixel reads the view's RenderConsts from a device table (ViewsConsts); a kernel of its own
                                             (atmo_render_views_kernel), for the same reason; with KF_TARGET: the same into packed colour targets, one
                                             TargetConsts per view (atmo_render_views_target_kernel, include/atmo_views_target.h) */,
                          KF_DEPTH = 4096 /* the depth buffer in its own format and row pitch (atmo_render_depth_target, include/atmo_depth.h): shade_pixel's depth read
                                             goes through load_depth on DepthConsts instead of RenderConsts::depth, and its stores take all seven target formats;
                                             always with KF_TARGET, kernels of their own (atmo_render[_proxy|_views|_views_proxy]_depth_target_kernel), for the
                                             same reason */,
                          KF_DETAIL = 8192 /* the cloud density with the reference's CLOUDS_ALWAYS_LOW_QUALITY off (atmo_set_cloud_detail, include/atmo_cloud_detail.h):
                                              the detail fetch of get_density_full and the alpha0 branch of get_light_raymarched, through DetailConsts; a kernel of
                                              its own (atmo_render_detail_kernel), for the same reason */,
                          KF_RAYS = 16384 /* caller-supplied rays (atmo_shade_rays, include/atmo_rays.h): no camera prologue -- origin, direction and distance limit come
                                             from an AtmoRay per lane, through RayConsts; the planet centre and the clouds' model-space origin are per-lane operands of
                                             the marches (their LANE forms); kernels of their own (atmo_shade_rays_kernel), for the same reason */,
                          KF_INDEX = 32768 /* the ray kernels through an index list (atmo_shade_rays_indexed, include/atmo_ray_order.h): thread k shades ray index[k] of
                                              the batch, through RayIndexConsts; always with KF_RAYS, kernels of their own (atmo_shade_rays_indexed_kernel), for the
                                              same reason */ };

// The far-mode draw's proxy (planet_atmosphere.gd:300-321: a BoxMesh of edge box_size centred on the node, rasterised with back-face culling, near / far
// clipping and Godot 4.3's reverse-Z GREATER_OR_EQUAL depth test).  Pixel (nx, ny) of the existing prologue's NDC: its segment from the near plane (z = 1) to
// the far plane (z = 0) is inv_p (nx, ny, z, 1), in the proxy's model space  H(z) = K (nx, ny, z, 1) = a + z b,  K = model^-1 inv_view inv_p (affine times
// projective: homogeneous coordinates, w > 0 between the planes).  |H_i| <= h H_w is linear in z for each of the six faces, so the part of the segment inside
// the closed box is an interval [z_lo, z_hi] of depths, solved in closed form: covered = the interval is not empty and excludes z = 1 (the near end lies
// outside); the front-face fragment's depth is its near end, z_in = z_hi.  Built by the host in double and rounded once (proxy_consts in atmo_api.hip).
struct ProxyConsts {
    float k[4][4];   // [host] rows x, y, z, w of K (row-major here: k[row][col])
    float half;      // [host] box_size / 2
};

// A packed colour target (include/atmo_target.h): where and how the kernels of the KF_TARGET family store.  A kernel argument of its own, behind
// RenderConsts (and ProxyConsts), so that the float kernels' argument layout -- and with it their code -- stays what it was.  RenderConsts::out is not read
// by these kernels; out_x0 / out_y0 / composite / store_discards mean what they mean to the float kernels.
enum TargetFormat : int { TF_RGBA32F = 0, TF_RGBA16F = 1, TF_RGBA8_UNORM = 2,
                          TF_RGBA8_SRGB = 16, TF_BGRA8_UNORM = 17, TF_BGRA8_SRGB = 18, TF_A2B10G10R10_UNORM = 19 };   // == AtmoTargetFormat
// the formats the KF_TARGET kernels store: everything but RGBA32F; 8 bytes a pixel for RGBA16F, 4 for every other one
inline bool target_format_packed(int format) { return format == TF_RGBA16F || format == TF_RGBA8_UNORM || (format >= TF_RGBA8_SRGB && format <= TF_A2B10G10R10_UNORM); }
struct TargetConsts {
    void *pixels;          // the pixel (out_x0, out_y0) maps to
    int32_t pitch_bytes;   // bytes from one row to the next
    int32_t format;        // a packed format (RGBA32F targets are drawn by the float kernels: a pitch in whole pixels is all they need);
                           // uniform, read only where a pixel is addressed and stored
};

// A depth source (include/atmo_depth.h): where and how the kernels of the KF_DEPTH family read the depth sample.  A kernel argument of its own, behind every
// older one.  RenderConsts::depth is null in these draws and not read.
enum DepthFormat : int { DF_D32_SFLOAT = 0, DF_D16_UNORM = 1, DF_X8_D24_UNORM = 2 };   // == AtmoDepthFormat
inline int depth_texel_bytes(int format) { return format == DF_D16_UNORM ? 2 : (format == DF_D32_SFLOAT || format == DF_X8_D24_UNORM) ? 4 : 0; }
struct DepthConsts {
    const void *texels;    // the viewport's first texel
    int32_t pitch_bytes;   // bytes from one row to the next
    int32_t format;        // uniform, read only where the sample is loaded and decoded
};

// Cloud detail (include/atmo_cloud_detail.h states the arithmetic): what the KF_DETAIL kernels read beside RenderConsts.  A kernel argument of its own, behind
// RenderConsts, which stays what it was.
struct DetailConsts {
    float c;            // [host] RN(AtmoFrame::time * 0.01f): the detail fetch is the shape volume at RN(RN(p * 15) + c)
    float shape_lo_d;   // [host] bounds of RN(shape - RN(0.2 * detail)) over every filtered texel value of `shape` and detail in [0, 1 + 2^-20]: what the
    float shape_hi_d;   //        coverage-first early outs of a FULL-quality sample test against (RenderConsts::shape_lo01 / shape_hi01 are detail = 0.5's)
};

// Caller-supplied rays (include/atmo_rays.h states the arithmetic): what the KF_RAYS kernels read beside RenderConsts.  A kernel argument of its own, behind
// RenderConsts, which stays what it was (of it these kernels read the uniforms, the textures and the sun direction; no matrix but view_to_model, no rect).
struct RayConsts {
    const float4 *rays;    // n AtmoRay = 2 n float4: (origin, tmax), (dir, reserved); 16-byte aligned
    float4 *out;           // n float4
    uint32_t n;            // rays of this launch (> 0)
    uint32_t width, first; // ray i is image index first + i of an image `width` wide: the blue-noise texel of its jitter
    // [host] the march-distance cap of raymarch_cloud (clouds:186-202) up to the ray's own part, smoothstep(md_e0, md_e1, |origin_model|):
    float md_ground, md_space;   // march_distance_ground, march_distance_space (the two values fill_consts mixes into RenderConsts::max_d)
    float md_e0, md_e1;          // clouds_bottom, clouds_top * 1.05
};
// An index list over a batch of rays (include/atmo_ray_order.h): what the KF_INDEX kernels read beside RenderConsts and RayConsts.  A kernel argument of its
// own, behind RayConsts, which stays what it was: the rays, their outputs and their jitter texels stay addressed by the ray's place in the batch.
struct RayIndexConsts {
    const uint32_t *index; // n_index entries; thread k shades ray index[k]; an entry >= RayConsts::n is skipped
    uint32_t n_index;      // entries of this launch (> 0)
};
// ... and of the kernel that writes a frame's camera rays (atmo_debug_frame_rays): the rect of rc, row-major
struct FrameRaysConsts {
    const float *depth;    // h rows of w
    float4 *rays;          // (y1 - y0) (x1 - x0) AtmoRay
};

// Several views in one launch (include/atmo_views.h).  The per-view RenderConsts live in a device table (the kernel's first argument: a const __restrict__
// pointer, indexed by a wave-uniform view number, so every field still arrives through scalar loads); this is what the launch itself needs.  The grid is
// one-dimensional over the concatenation of the views' tiles: global tile t belongs to the view v with first_block[v] <= t < first_block[v + 1] and is that
// view's tile t - first_block[v], row-major in its own grid (RenderConsts::tiles_x).
constexpr int MAX_VIEWS = 8;   // == ATMO_MAX_VIEWS
struct ViewsConsts {
    uint32_t first_block[MAX_VIEWS + 1];   // prefix of the views' tile counts (an empty view adds nothing); entries behind n_views repeat the total
    const uint32_t *order;                 // null => global tile = block index (view-major, row-major inside a view); else the global tile each block shades
    uint32_t *cost;                        // null => no feedback; else per GLOBAL tile the longest wave's duration in shader cycles (atomicMax)
};
// ... and where every view of a batch into packed colour targets stores (atmo_render_views_target): the eight TargetConsts by value in the kernel-argument
// segment, indexed by the same wave-uniform view number, so they too arrive through scalar loads and the staging ring carries RenderConsts only.
struct ViewsTargetConsts {
    ViewsConsts v;
    TargetConsts target[MAX_VIEWS];        // entries of empty views and behind n_views are zero: no tile maps to them
};
// Several far-mode (proxy) views in one launch (atmo_render_views_proxy, include/atmo_views_proxy.h): the launch of ViewsConsts without a tile order or
// cost recording -- every view's grid is the box's screen rectangle and changes every frame, as the single proxy draw's -- and each view's ProxyConsts
// (one box, eight cameras: K differs per view).  By value in the kernel-argument segment and indexed by the wave-uniform view number, as
// ViewsTargetConsts::target: scalar loads.  table[v] carries the CUT rectangle (x0 .. y1, gx0, gy0, tiles_x); the output stays addressed by the frame's.
struct ViewsProxyConsts {
    uint32_t first_block[MAX_VIEWS + 1];   // prefix of the views' tile counts (a view without a tile adds nothing); entries behind n_views repeat the total
    ProxyConsts proxy[MAX_VIEWS];          // entries of views without a tile and behind n_views are zero: no tile maps to them
};
struct ViewsProxyTargetConsts {
    ViewsProxyConsts p;
    TargetConsts target[MAX_VIEWS];        // as ViewsTargetConsts::target
};

// ... and where every view of a depth-source batch reads its depth (atmo_render_views[_proxy]_depth_target): the eight DepthConsts by value in the
// kernel-argument segment, a kernel argument of its own behind ViewsTargetConsts / ViewsProxyTargetConsts, indexed by the wave-uniform view number
struct ViewsDepthConsts {
    DepthConsts depth[MAX_VIEWS];          // entries of views without a tile and behind n_views are zero: no tile maps to them
};
// ... and every view's cloud-detail constants (atmo_render_views_detail_target, include/atmo_detail_target.h): c = RN(time * 0.01f) is the view's own frame's,
// so there are eight DetailConsts, by value in the kernel-argument segment behind ViewsDepthConsts, indexed by the wave-uniform view number
struct ViewsDetailConsts {
    DetailConsts detail[MAX_VIEWS];        // entries of views without a tile and behind n_views are zero: no tile maps to them
};

hipError_t launch_render(int flags, int split, const RenderConsts &rc, hipStream_t stream, int tile_list_blocks = 0);  // > 0: rc.tile_order lists that many tiles of the rect's grid
// Every launcher below draws the DEFAULT-FORM families (what a default context selects: one lane per ray, the precise cloud and v1 forms, up to 32 view
// steps) and no other.  The list stands once, ATMO_DEFAULT_FAMILIES in atmo_kernels.hip: default_family_supported and launch_default_family are made from it.
//   a new family:       one line at the end of that list; every launcher below then has it.  The ray and cloud-detail launchers draw the SUBSET a constexpr
//                       predicate beside their kernels selects (rays_family, ray_quads_family, detail_family, rays_detail_family): there it is a change
//                       to that predicate and to the count its static_assert holds
//   a new entry point:  its kernel, and one launch_default_family (or launch_family_subset<predicate>) call whose lambda names that kernel and its family bits
// flags = a draw's family WITHOUT the entry point's own bits (KF_PROXY, KF_VIEWS, KF_TARGET, ...), which the launcher adds.
bool default_family_supported(int flags);
// the proxy draws: one lane per ray, row-major grid of the rect in rc
hipError_t launch_render_proxy(int flags, const RenderConsts &rc, const ProxyConsts &pc, hipStream_t stream);
// the multi-view draws: one lane per ray; table_dev holds one RenderConsts per view (light_steps is the context's: the same in all of them);
// total_blocks = vc.first_block[MAX_VIEWS]
hipError_t launch_render_views(int flags, int light_steps, const RenderConsts *table_dev, const ViewsConsts &vc, hipStream_t stream);
// the multi-view draws into packed colour targets (atmo_render_views_target, include/atmo_views_target.h): the same launch with the KF_VIEWS | KF_TARGET
// kernels; vtc.target[v] is view v's target, every non-empty view in the one packed format vtc.target[first non-empty].format (RGBA32F batches are
// launch_render_views with the pitch in RenderConsts::out_pitch)
hipError_t launch_render_views_target(int flags, int light_steps, const RenderConsts *table_dev, const ViewsTargetConsts &vtc, hipStream_t stream);
// the multi-view proxy draws (atmo_render_views_proxy[_target], include/atmo_views_proxy.h): the KF_VIEWS | KF_PROXY [| KF_TARGET] kernels over the
// concatenation of every view's cut rectangle's grid, view-major and row-major
hipError_t launch_render_views_proxy(int flags, int light_steps, const RenderConsts *table_dev, const ViewsProxyConsts &vpc, hipStream_t stream);
hipError_t launch_render_views_proxy_target(int flags, int light_steps, const RenderConsts *table_dev, const ViewsProxyTargetConsts &vptc, hipStream_t stream);
// the packed-target draws: the float draws' launches (grid, tile order, cost feedback, tile lists for the heavy-tile split) with the KF_TARGET kernels.
// target_family_supported says which (flags, split) exist: the default families with split 1 and the two declared-sampler cloud families with split 2;
// launch_render_target also takes KF_LIGHT_DIRECT | KF_GEO (the geometric-order twin; ask target_family_supported without KF_GEO).
bool target_family_supported(int flags, int split);
hipError_t launch_render_target(int flags, int split, const RenderConsts &rc, const TargetConsts &tc, hipStream_t stream, int tile_list_blocks = 0);
hipError_t launch_render_proxy_target(int flags, const RenderConsts &rc, const ProxyConsts &pc, const TargetConsts &tc, hipStream_t stream);
// the depth-source draws (include/atmo_depth.h): the four packed-target launches above with the KF_DEPTH | KF_TARGET kernels, which read the depth through
// DepthConsts and store every target format, RGBA32F included.  (flags, split) as launch_render_target's: target_family_supported says which exist.
hipError_t launch_render_depth_target(int flags, int split, const RenderConsts &rc, const TargetConsts &tc, const DepthConsts &dc, hipStream_t stream,
                                      int tile_list_blocks = 0);
hipError_t launch_render_proxy_depth_target(int flags, const RenderConsts &rc, const ProxyConsts &pc, const TargetConsts &tc, const DepthConsts &dc,
                                            hipStream_t stream);
hipError_t launch_render_views_depth_target(int flags, int light_steps, const RenderConsts *table_dev, const ViewsTargetConsts &vtc,
                                            const ViewsDepthConsts &vdc, hipStream_t stream);
hipError_t launch_render_views_proxy_depth_target(int flags, int light_steps, const RenderConsts *table_dev, const ViewsProxyTargetConsts &vptc,
                                                  const ViewsDepthConsts &vdc, hipStream_t stream);
// the cloud-detail draws (atmo_set_cloud_detail; include/atmo_cloud_detail.h): the six LUT-light cloud families of the default forms (detail_family_supported),
// one lane per ray, row-major over the grid of the rect in rc, no tile order and no cost recording; flags WITHOUT KF_DETAIL, which the launcher adds
bool detail_family_supported(int flags);
hipError_t launch_render_detail(int flags, const RenderConsts &rc, const DetailConsts &xc, hipStream_t stream);
// ... into a colour target of any of the seven formats, reading a depth source (atmo_render_detail_target, atmo_render_views_detail_target;
// include/atmo_detail_target.h): the same six families with the KF_DETAIL | KF_DEPTH | KF_TARGET kernels, the single draw as launch_render_detail, the batch
// view-major as launch_render_views_depth_target without a tile order or a cost map (vtc.v.order and vtc.v.cost must be null); flags WITHOUT these bits
hipError_t launch_render_detail_target(int flags, const RenderConsts &rc, const TargetConsts &tc, const DepthConsts &dc, const DetailConsts &xc, hipStream_t stream);
hipError_t launch_render_views_detail_target(int flags, const RenderConsts *table_dev, const ViewsTargetConsts &vtc, const ViewsDepthConsts &vdc,
                                             const ViewsDetailConsts &vxc, hipStream_t stream);
// the ray draws (include/atmo_rays.h, atmo_ray_quads.h, atmo_ray_order.h, atmo_ray_detail.h), one launcher for all five entry points.  flags WITHOUT
// KF_RAYS | KF_INDEX | KF_DETAIL, which the launcher adds.  64 consecutive rays per wave, 256 per workgroup, row-major over the batch -- or, with ic, over
// the list's ic->n_index entries.  hipErrorInvalidValue for arguments outside the limits and for any other family.
//   RAY_BATCH: the six level-0 families (rays_family_supported; the direct-light one with 8 light steps unrolled or any count); first + n <= 2^32
//   RAY_QUADS: the three cloud families under the declared sampler (ray_quads_family_supported; flags WITH KF_CUBE_LOD); yc.n = 4 n_quads, yc.first =
//              first_quad, yc.width = quads per row of the image, (width + 1) / 2; first_quad + n_quads <= 2^30; no ic
//   xc:        the KF_DETAIL kernels, DetailConsts behind the ray arguments: the three cloud families of the shape
enum RayShape : int { RAY_BATCH, RAY_QUADS };
bool rays_family_supported(int flags);
bool ray_quads_family_supported(int flags);
hipError_t launch_shade_rays(int flags, RayShape shape, const RenderConsts &rc, const RayConsts &yc, const RayIndexConsts *ic, const DetailConsts *xc,
                             hipStream_t stream);
// the coherence order of a ray queue (atmo_ray_order; include/atmo_ray_order.h states the key): the key kernel, then a stable least-significant-digit radix
// sort of (key, index) pairs in three 6-bit passes, every buffer in the caller's scratch (ray_order_scratch_bytes(n) bytes, 16-byte aligned), kernels on
// `stream` only.  launch_ray_sort is the sort alone, on keys that are already there (atmo_debug_sort_ray_keys); n <= RAY_ORDER_MAX_RAYS
constexpr int RAY_KEY_BITS = 18;                       // == ATMO_RAY_KEY_BITS
constexpr uint32_t RAY_ORDER_MAX_RAYS = 1u << 28;
size_t ray_order_scratch_bytes(uint32_t n);
hipError_t launch_ray_keys(const float4 *rays, uint32_t n, uint32_t *keys, hipStream_t stream);
hipError_t launch_ray_sort(const uint32_t *keys, uint32_t n, uint32_t *index, void *scratch, hipStream_t stream);
hipError_t launch_ray_order(const float4 *rays, uint32_t n, uint32_t *index, void *scratch, hipStream_t stream);
// a ray list (atmo_ray_list; include/atmo_ray_list.h): the order's passes in COUNTED form -- the bound of every kernel is a device word, *count clamped to
// capacity, then the live total the first scatter leaves in the scratch -- with the sure-miss cull in the key kernel and a tail fill behind the last pass.
// Kernels of their own beside the order's (which stay what they are); the scan is the order's.  ray_list_scratch_bytes(capacity) bytes, 16-byte aligned
constexpr int RAY_LIST_ORDER = 1, RAY_LIST_CULL = 2;   // == ATMO_RAY_LIST_ORDER, ATMO_RAY_LIST_CULL
constexpr uint32_t RAY_LIST_END = 0xFFFFFFFFu;         // == ATMO_RAY_LIST_END
// THE CULL's constants: a kernel argument of the list's key kernel alone
struct RayCullConsts {
    float cx, cy, cz;   // the view-space centre, RenderConsts::center
    float r2, r2_far;   // RenderConsts::atmosphere_radius2 and RN(r2 * 1.02f)
};
size_t ray_list_scratch_bytes(uint32_t capacity);
hipError_t launch_ray_list(const float4 *rays, const uint32_t *count, uint32_t capacity, int flags, const RayCullConsts &cull, float4 *rgba, uint32_t *index,
                           uint32_t *listed, void *scratch, hipStream_t stream);
// the camera rays of the rect in rc, as the float kernels' prologue forms them (atmo_debug_frame_rays)
hipError_t launch_frame_rays(const RenderConsts &rc, const FrameRaysConsts &fc, hipStream_t stream);
// the rays of a lens image (atmo_lens_rays; include/atmo_lens.h states the arithmetic): atmo_lens_rays_kernel<KIND, QUADS>, one lane per ray, and with
// lc.index the 16 x 4 tile index in the same launch.  lc.n = the launch's threads: 4 per quad of the band (quads), the index's entries (lc.index), else the
// band's rays; at most 2^32.  The band is not empty.  Kernels on `stream` only
constexpr int LENS_EQUIRECT = 0, LENS_FISHEYE = 1, LENS_OCTAHEDRAL = 2, LENS_CUBE_FACE = 3;   // == AtmoLensKind
struct LensConsts {
    float4 *rays;            // the band's AtmoRay array, 16-byte aligned
    uint32_t *index;         // null, or the tile index (row-major only)
    const float *distance;   // null, or h rows of `pitch` floats: every ray's tmax
    uint32_t pitch;
    int w, h, y0, y1, face;  // the image, the band [y0, y1) and CUBE_FACE's face
    uint32_t qpr, tpr;       // quads per row, (w + 1) / 2; tiles per row, (w + 15) / 16
    uint64_t n;              // threads of the launch
    float fov, tmax;
    float origin[3], basis[9];
};
hipError_t launch_lens_rays(int kind, bool quads, const LensConsts &lc, hipStream_t stream);
// load_depth's decode over n texels of a caller's array: out[i] = decode(texels[i]) (atmo_debug_decode_depth)
hipError_t launch_decode_depth(int format, const void *texels, float *out, size_t n, hipStream_t stream);
// store_target<format> over n pixels: dst[i] = encode(src[i]), or encode(blend(src[i], decode(dst[i]))) when composite (atmo_debug_store_target)
hipError_t launch_store_target(int format, int composite, const float *src_rgba, void *dst, size_t n, hipStream_t stream);
hipError_t launch_bake(const BakeConsts &bc, hipStream_t stream);
hipError_t launch_tile_order(uint32_t *cost, uint32_t *order, int tiles_x, int tiles_y, int rx, int ry, uint32_t *tmp1, uint32_t *tmp2,
                             uint32_t *scratch, hipStream_t stream, uint32_t *order2 = nullptr, uint32_t *class_totals = nullptr);
// 64 classes, the sort's per-class state being one lane of a wave (profiles/round6/ab_order_classes.txt: against 32 half octaves clouds_high 1920x1080 -3.7 %)
constexpr int TILE_ORDER_CLASSES = 64;      // cost classes of the sort: 16 octaves of the wave duration (2^8 .. 2^24 cycles) in TILE_ORDER_PER_OCTAVE equal
constexpr int TILE_ORDER_PER_OCTAVE = 4;    // parts each (by the duration's two leading mantissa bits), class 0 the heaviest (tile_cost_class)
size_t tile_order_scratch_bytes();
hipError_t launch_tile_list_bound(const uint32_t *in, uint32_t *out, int n, uint32_t tiles_n, uint32_t sentinel, hipStream_t stream,
                                  uint32_t *out2 = nullptr, int n_heavy = 0, int tiles_x = 1, uint32_t sentinel2 = 0);  // atmo_render_tiles[_split]
hipError_t launch_layout_lut(const float *lut, int w, int h, float *out, hipStream_t stream);
hipError_t launch_lut_footprints(const float *apron, int w, int h, float *out4, hipStream_t stream);
hipError_t launch_layout_shape(const uint8_t *t, int n, uint32_t *out, hipStream_t stream);
hipError_t launch_layout_cube(const uint8_t *faces, int n, uint32_t *out, hipStream_t stream);
hipError_t launch_footprints_f4(const uint32_t *words, size_t n_words, float *out4, hipStream_t stream);
hipError_t launch_cube_mip(const uint8_t *level, int n, uint8_t *next, hipStream_t stream);
void render_grid(const RenderConsts &rc, int split, int *tiles_x, int *tiles_y);
void render_tile_size(int split, int *tile_w, int *tile_h);  // pixels per workgroup tile of a launch with `split` lanes per ray
hipError_t launch_noise_cubemap(const NoiseCubemapConsts &nc, hipStream_t stream);
// the whole generation on `stream`: (normalize) the two words re-initialised and the min/max pass, then the store pass
hipError_t launch_noise_volume(const NoiseVolumeConsts &nv, hipStream_t stream);
const char *render_kernel_name(int flags, int light_steps, int split);
hipError_t launch_log2_cr(const float *x_dev, float *out_dev, int n, hipStream_t stream);
hipError_t launch_light_probe(const float *pos, const float *dir, int n, float planet_radius, float atmosphere_height, float density,
                              int light_steps, float *out, hipStream_t stream);
hipError_t launch_selftest(uint32_t first_bits, uint32_t count, float c, float rc, unsigned int *mismatch_dev, hipStream_t stream);
// Reduced-resolution draws (include/atmo_reduced.h states the arithmetic): what the two passes around the low draw read.  The viewport is w x h, the low
// image low_w x low_h = ceil(w / s) x ceil(h / s), s = 1 << log2s (2 or 4).  pz / pw: rows 2 and 3 of the frame's inv_projection (m[2], m[6], m[10], m[14]
// and m[3], m[7], m[11], m[15]).
struct ReducedConsts {
    float pz[4], pw[4];
    int32_t w, h, low_w, low_h, log2s;
    float tol;                // AtmoReduced::depth_tolerance (the upsample)
    int32_t composite;        // the upsample blends into the target and leaves pixels without alpha alone
    float *low_depth;         // low_w * low_h floats, tight: written by the reduction, read by the upsample
    const float4 *low_rgba;   // low_w * low_h float4, tight (the upsample)
};
// atmo_reduced_pick_kernel: one lane per low texel, the block scanned row-major
hipError_t launch_reduced_pick(const ReducedConsts &dc, const DepthConsts &depth, hipStream_t stream);
// atmo_reduced_upsample_kernel: one lane per pixel of the viewport, 64 consecutive pixels of a row per wave; every target format
hipError_t launch_reduced_upsample(const ReducedConsts &dc, const DepthConsts &depth, const TargetConsts &tc, hipStream_t stream);
// Sky ambient light (include/atmo_sky_sh.h states the arithmetic and THE ORDER OF THE SUMS; sky_sh.py reads these constants out of the header's text).
// atmo_lens_solid_angle_kernel<KIND, QUADS>: one lane per slot of the band's ray array -- lc.rays names nothing here, lc.index is null, lc.n = the band's
// rays --, one float each.  The projection: atmo_sky_sh9_segment_kernel, one workgroup of SKY_SH_LANES per SKY_SH_SEGMENT consecutive rays, its partial
// (SKY_SH_ROW floats) to the scratch; atmo_sky_sh9_total_kernel, one workgroup over the partials, to `out`.  Kernels on `stream` only
constexpr int SKY_SH_LANES = 256, SKY_SH_PER_LANE = 16, SKY_SH_SEGMENT = SKY_SH_LANES * SKY_SH_PER_LANE;
constexpr int SKY_SH_SUMS = 37, SKY_SH_ROW = 40;   // 9 coefficients x rgba and the weights' sum; a partial and `out` are 40 floats, the last three +0
constexpr uint32_t SKY_SH_MAX_RAYS = 1u << 28;
constexpr int SKY_SH_ACCUMULATE = 1;               // == ATMO_SKY_SH_ACCUMULATE
inline uint32_t sky_sh_segments(uint32_t n_rays) { return (n_rays + (uint32_t)(SKY_SH_SEGMENT - 1)) / (uint32_t)SKY_SH_SEGMENT; }
inline size_t sky_sh_scratch_bytes(uint32_t n_rays) { return (size_t)sky_sh_segments(n_rays) * SKY_SH_ROW * sizeof(float); }
struct SkyShConsts {
    const float4 *rays;    // n AtmoRay, 16-byte aligned: the second float4 of each is read
    const float4 *rgba;    // n rows
    const float *weight;   // null: every ray weighs 1
    float4 *partial;       // the scratch: sky_sh_segments(n) rows of SKY_SH_ROW floats
    float4 *out;           // SKY_SH_ROW floats
    uint32_t n, segments;
    int32_t accumulate;
};
hipError_t launch_lens_solid_angles(int kind, bool quads, const LensConsts &lc, float *weight, hipStream_t stream);
hipError_t launch_sky_sh9(const SkyShConsts &c, hipStream_t stream);
// Sky images (include/atmo_sky_image.h states both operations; sky_image.py restates them in numpy).
// atmo_sky_image_resolve_kernel: one lane per pixel of the band, the row of its ray slot as one 16-byte load, the store of the KF_DEPTH kernels (every
// target format, a uniform field).  tc.pixels is pixel (0, 0) of the whole image.  Row-major: a wave is 64 pixels of a row; QUADS: 32 pixels of two rows,
// 16 whole quads.  atmo_sky_image_mip_kernel<FMT>: one workgroup of SKY_MIP_LANES per SKY_MIP_BLOCK x SKY_MIP_BLOCK texels of lv[0] of one layer, up to
// SKY_MIP_STEPS levels below it through LDS.  Kernels on `stream` only
constexpr uint32_t SKY_IMAGE_QUADS = 1u, SKY_IMAGE_PREMULTIPLIED = 2u, SKY_IMAGE_COMPOSITE = 4u;   // == ATMO_LENS_QUADS, ATMO_SKY_IMAGE_*
struct SkyResolveConsts {
    const float4 *rgba;     // the band's rows in ray order, 16-byte aligned
    int32_t w, h, y0, y1;   // the image and the band [y0, y1), not empty
    int32_t fisheye;        // the lens has absent pixels: atmo_lens.h's integer test on (w, h)
    uint32_t qpr;           // quads per row, (w + 1) / 2
    uint32_t flags;         // SKY_IMAGE_*
    uint32_t blocks_x;      // [launcher] workgroups along a row
};
hipError_t launch_sky_image_resolve(SkyResolveConsts c, const TargetConsts &tc, hipStream_t stream);
constexpr int SKY_MIP_STEPS = 5, SKY_MIP_BLOCK = 32, SKY_MIP_LANES = 256;
struct SkyMipLevel {
    void *pixels;
    int64_t layer_pitch;    // bytes, in effect (never 0)
    int32_t row_pitch;      // bytes, in effect
    int32_t w, h;
    int32_t unused;
};
struct SkyMipConsts {
    SkyMipLevel lv[SKY_MIP_STEPS + 1];   // lv[0] is read, lv[1 .. steps] are written; by value in the kernel arguments
    int32_t steps;                       // 1 .. SKY_MIP_STEPS
    int32_t layers;
};
hipError_t launch_sky_image_mips(int format, const SkyMipConsts &c, hipStream_t stream);
// Temporal draws (include/atmo_temporal.h states the arithmetic; temporal.py restates it in numpy): what the two passes read beside ReducedConsts (the
// sizes, rows 2 and 3 of the current inv_projection, depth_tolerance, composite, the low buffers).  By value in the kernel arguments.
struct TemporalConsts {
    float m[16];               // the frame's inv_projection_matrix, column-major (the resolve forms all four rows)
    float pc[16];              // AtmoTemporal::prev_clip_from_view
    float rz[4], rw[4];        // rows 2 and 3 of AtmoTemporal::prev_inv_projection
    int32_t ox, oy;            // the phase's texel of every block
    int32_t max_age, reset;
    float htol;                // AtmoTemporal::history_tolerance
    const float4 *prev_rgba;   // the previous history's three parts (all null under reset: never read)
    const float *prev_q;
    const uint8_t *prev_age;
    float4 *cur_rgba;          // the current history's
    float *cur_q;
    uint8_t *cur_age;
};
// atmo_temporal_depth_kernel: one lane per low texel, a plain gather (reads c's sizes and low_depth, t's ox and oy)
hipError_t launch_temporal_depth(const ReducedConsts &c, const TemporalConsts &t, const DepthConsts &depth, hipStream_t stream);
// atmo_temporal_resolve_kernel: one lane per pixel of the viewport in the upsample kernel's lane map; every target format
hipError_t launch_temporal_resolve(const ReducedConsts &c, const TemporalConsts &t, const DepthConsts &depth, const TargetConsts &tc, hipStream_t stream);

}  // namespace atmo
