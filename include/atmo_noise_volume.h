/*
 * atmo_noise_volume.h -- generating the cloud shape volume on the device (libatmo_hip.so, ABI version 5).  Included after atmo.h; same conventions.
 *
 * Of the four textures the kernels read, u_cloud_shape_texture was the one without a producer in this library: the LUT is baked by
 * atmo_bake_optical_depth, the coverage cubemap comes from atmo_generate_noise_cubemap, the jitter table is fixed data.  In the reference's demo the
 * shape volume is a seamless NoiseTexture3D over a FastNoiseLite (demo/planet_atmosphere_test.tscn:48-57,113) -- engine code.  The call below is that
 * resource's generator over THIS build's seeded value noise (the noise of atmo_generate_noise_cubemap): stream-ordered, with a noise-space offset, so a
 * host can re-run it every frame in front of the draw and get shape volumes that evolve over time, without a host round trip.
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 (no other header changes).  A host looks the symbol below up.
 *
 * THE NUMERICAL CONTRACT (exact: no tolerance; tests/noise_volume_host.py states the same in float32 numpy, tests/test_noise_volume_gpu.py holds the
 * kernels to it byte for byte).  Everything is IEEE binary32, every operation rounded on its own (nothing fused), divisions correctly rounded.
 *  - The volume is n x n x n bytes, indexed [z][y][x], x fastest: texel (x, y, z) is byte (z * n + y) * n + x.
 *  - COORDINATE.  q = ((float)x + offset[0], (float)y + offset[1], (float)z + offset[2]): integer texel coordinates, as Noise.get_image_3d samples them,
 *    one rounded add per axis.
 *  - VALUE NOISE.  value(p, s), for a point p and a 32-bit seed s: per axis f = floor(p), t = p - f, w = t * t * (3 - 2 * t), i0 = (int)f, i1 = i0 + 1.
 *    lattice(ix, iy, iz, s) = (float)(hash(((uint32)ix * 0x9E3779B1) ^ ((uint32)iy * 0x85EBCA77) ^ ((uint32)iz * 0xC2B2AE3D) ^ s) >> 8) * 2^-24, where
 *    hash(h): h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16.  Trilinear: along x first, a * (1 - wx) + b * wx for the four
 *    (y, z) corners, then along y, then along z, each product and sum rounded.
 *  - NOT SEAMLESS.  Octave o evaluates value(q * freq_o, seed + 1013 * o) on the unbounded lattice; freq_0 = frequency, freq_{o+1} = freq_o * 2.
 *  - SEAMLESS.  P_0 = max(1, (int)rintf((float)n * frequency)) (round half to even of the fp32 product), P_o = P_0 << o, freq_o = (float)P_o / (float)n
 *    (one division).  Octave o evaluates value(q * freq_o, seed + 1013 * o) with i0 and i1 = i0 + 1 of every axis each taken modulo P_o, with a
 *    non-negative result, before hashing.  Octave o then repeats every n texels along each axis exactly: the volume tiles by construction, there is no
 *    blend skirt; an offset of a multiple of n texels along an axis reproduces the bytes and an offset of whole texels rotates them along it (while
 *    the adds stay exact).
 *  - FRACTAL SUM.  total = 0, norm = 0, amp = 1; per octave: total += amp * value; norm += amp; amp *= gain.  v = 2 * (total / norm) - 1;
 *    t = 0.5 + 0.5 * v.  t lies in [+0, 1] and is never -0 or NaN.
 *  - NORMALIZE.  mn, mx = the minimum and the maximum of t over the whole volume (independent of the order of reduction).  If mx != mn:
 *    t = (t - mn) / (mx - mn); otherwise t stays.
 *  - QUANTISE.  b = (uint8)clamp(t * 255, 0, 255), truncating (the cubemap generator's L8 store).
 *  - INVERT.  b = 255 - b.
 *
 * WHAT IT COSTS (profiles/noise_volume/README.md: tools/noise_volume_probe.py on one MI355X; device time per call, 4 octaves).  Without normalize one
 * pass: 7.4 / 45 / 347 us for a seamless 64^3 / 128^3 / 256^3 volume (5.6 / 32 / 246 us not seamless).  With normalize the noise is evaluated twice -- a
 * min/max pass (reduced inside each wavefront with cross-lane operations and inside the block through LDS, then at most one atomic per block on each
 * of two context-owned words, re-initialised in front of every pass), then the store pass -- rather than kept: an fp32 scratch of 512^3 texels would be
 * 512 MB.  25 / 93 / 704 us.  bind adds the re-layout (and up to 64^3 the float copy): 10 / 12 / 38 us.  A frame that regenerates and binds the demo's
 * 64^3 volume pays 35 us on the stream and no host wait; the float64 numpy volume of the tests took 0.066 s of that machine's host.
 */
#ifndef ATMO_NOISE_VOLUME_H
#define ATMO_NOISE_VOLUME_H

#include "atmo.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AtmoNoiseVolume {
    int32_t  size;        /* n; the shape texture is cubic: 1 .. 512 (atmo_set_texture's bound) */
    uint32_t seed;
    float    frequency;   /* > 0, finite */
    int32_t  octaves;     /* 1 .. 16 */
    float    gain;        /* finite, > 0 */
    float    offset[3];   /* texels, finite; animate for evolving shapes */
    int32_t  seamless, invert, normalize;
} AtmoNoiseVolume;

/*
 * Generates the volume `v` describes into a context-owned device buffer, on `stream`; nothing in the generation waits on the host.
 *  - bind != 0: the buffer then becomes u_cloud_shape_texture through atmo_set_texture(ctx, "u_cloud_shape_texture", ATMO_TEX_3D_R8, n, n, n, 1, buffer,
 *    ATMO_MEM_DEVICE, stream): the same ordering against draws and updates on other streams, the same re-layout and float-copy kernels, a same-size
 *    update overwriting the bound copy in place.  With texels_host == NULL the call only enqueues.
 *  - texels_host != NULL: n^3 bytes are copied there and the call returns once the stream has reached the copy -- the only host wait.
 *  - with neither, the texels stay in the context's buffer (a measurement); the next generation overwrites them.
 * The buffer changes size only when n does (that re-allocation waits for the device, as a texture's size change does).  A context generates on one
 * stream at a time: a generation on another stream than the previous one's is ordered behind that one's texture update, not behind a generation that
 * was not bound.
 *
 * Refusals: nothing is enqueued or allocated when one fires, and the ATMO_E_ARG ones are checked before the device is touched (a context of
 * atmo_debug_create_host_only answers them the same; a call that passes them gets ATMO_E_NO_DEVICE there).  The message names the field:
 *   ATMO_E_ARG    v == NULL; size outside 1 .. 512; octaves outside 1 .. 16; frequency or gain not finite or not > 0; an offset not finite;
 *                 seamless and P_0 << (octaves - 1) above 2^24 (`frequency`: the periods must stay exact in fp32);
 *                 (n + max |offset|) * freq_last >= 2^30 in either mode, freq_last the last octave's frequency (`offset`: the float-to-int conversion
 *                 of the lattice index must stay defined)
 *   ATMO_E_STATE  texels_host given on a stream that is capturing a HIP graph (the call would have to wait inside the capture)
 */
int atmo_generate_noise_volume(AtmoContext *ctx, const AtmoNoiseVolume *v, int bind, uint8_t *texels_host, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_NOISE_VOLUME_H */
