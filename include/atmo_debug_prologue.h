/*
 * atmo_debug_prologue.h -- what the camera makes redundant in the prologue of the cloudless direct-light kernels (libatmo_hip.so, ABI version 5).
 * Includes atmo.h; same conventions.  Diagnostics for the tests and the tools, like atmo_debug.h; no call here needs a device.
 *
 * The kernels of the family `direct light, no clouds` (the default command of bench.py and its twins) evaluate the reference's prologue exactly.  For the
 * cameras and uniforms a renderer really sends, parts of it multiply by zero or divide by a power of two.  The host classifies every draw and hands the
 * kernels a wave-uniform mask; under a set bit the kernel takes a short form that gives the SAME BITS as the general one, and the general form stays the
 * fall-back for every other draw (csrc/atmo_api.hip: prologue_camera_fill states each predicate with its premises).
 *
 * Feature detection: ATMO_ABI_VERSION stays 5 and the older headers keep their function sets; these calls are looked up by symbol.
 *
 * ATMO_PROLOGUE_CAMERA=0 in the environment of atmo_create makes the mask 0 for every draw of that context (A/B runs and the tests).
 */
#ifndef ATMO_DEBUG_PROLOGUE_H
#define ATMO_DEBUG_PROLOGUE_H

#include "atmo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bits of the mask */
#define ATMO_PROLOGUE_CAMERA 1u          /* perspective inv_projection and rigid inv_view: the two 4 x 4 products without their zero terms */
#define ATMO_PROLOGUE_POW2_STEPS 2u      /* view_steps is a power of two: the view step's length by a product with the exact reciprocal */
#define ATMO_PROLOGUE_NO_SPHERE_DEPTH 4u /* u_sphere_depth_factor is a zero (and bit 1): no ground-sphere hit in front of the march */

/* The mask a draw of `frame` by `ctx` carries (a context of atmo_debug_create_host_only will do).  *skip_px / *skip_py (either may be null): under bit 1
 * the viewport's pixel column / row whose waves take the general form all the same -- the centre of an odd viewport, where the NDC coordinate is 0,
 * under a constant term of inv_projection that is -0 -- or -1. */
int atmo_debug_prologue_mode(AtmoContext *ctx, const AtmoFrame *frame, unsigned int *mode, int *skip_px, int *skip_py);

/* The uniform products handed to the kernels, and the values they are made from: 1 / view_steps (0 unless bit 2), (float)view_steps,
 * atmosphere_radius^2, planet_radius^2, density^2, density^2 / 8, -coeff[0..2] * log2(e); then atmosphere_radius, planet_radius, density, coeff[0..2],
 * sphere_depth_factor.  *count = 16; out may be null. */
int atmo_debug_prologue_constants(AtmoContext *ctx, const AtmoFrame *frame, float *out, int capacity, int *count);

#ifdef __cplusplus
}
#endif

#endif /* ATMO_DEBUG_PROLOGUE_H */
