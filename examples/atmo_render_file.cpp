// atmo_render_file.cpp -- a host that uses ONLY the C ABI (include/atmo.h) and the HIP runtime: no Python, no torch.
// It is what a GDExtension or any other native host does: create a context for a shader variant,
// set uniforms by the reference's names, bake the optical-depth LUT on the device, draw, read the frame back.
//
//   hipcc -O2 -I include examples/atmo_render_file.cpp -L godot_atmosphere_shader_amd -latmo_hip \
//         -Wl,-rpath,$PWD/godot_atmosphere_shader_amd -o atmo_render_file
//   ./atmo_render_file <frame.bin> <depth.bin> <out.bin> <planet_radius> <atmosphere_height> <u_density> <view_steps> [--target rgba16f|rgba8|rgba8_srgb|bgra8|bgra8_srgb|a2b10g10r10]
//                      [--depth-format d32f|d16|x8d24 [--depth-pitch BYTES]] [--detail 0|1] [--time SECONDS]
//
// frame.bin = one AtmoFrame struct; depth.bin = viewport_h*viewport_w floats; out.bin = rect RGBA float4.
// tests/test_gpu_parity.py::test_native_host_matches_python_binding checks the bytes against the Python path.
// --target (include/atmo_target.h): the draw stores RGBA16F (8 bytes per pixel), or RGBA8_UNORM / RGBA8_SRGB / BGRA8_UNORM / BGRA8_SRGB /
// A2B10G10R10_UNORM (4), instead, as into a renderer's own colour buffer;
// out.bin then holds those pixels, tightly packed (tests/test_target_gpu.py::test_native_host_draws_into_a_packed_target).
// --depth-format (include/atmo_depth.h): depth.bin is the renderer's own depth buffer -- viewport_h rows of D32_SFLOAT, D16_UNORM or X8_D24_UNORM texels,
// --depth-pitch bytes apart (default: tight) -- and the draw reads it as it is (atmo_render_depth_target, into any --target, RGBA32F included;
// tests/test_depth_gpu.py::test_native_host_reads_a_d16_depth_buffer).
// --detail (include/atmo_cloud_detail.h): the context is the clouds_high variant instead, its shape volume generated on the device (a seamless 32^3
// atmo_generate_noise_volume, no coverage cubemap: uniform cover); --detail 1 draws it with the reference's CLOUDS_ALWAYS_LOW_QUALITY off -- the
// detail fetch, which moves with TIME -- and --detail 0 as shipped.  --time overrides frame.bin's AtmoFrame::time.  Float depth and RGBA32F only:
// a cloud-detail draw goes through atmo_render.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "atmo.h"
#include "atmo_target.h"
#include "atmo_depth.h"
#include "atmo_noise_volume.h"
#include "atmo_cloud_detail.h"

#define CHECK_ATMO(call)                                                                       \
    do {                                                                                       \
        int rc_ = (call);                                                                      \
        if (rc_ != ATMO_OK) {                                                                  \
            std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, atmo_last_error_string(ctx)); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)
#define CHECK_HIP(call)                                                              \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                      \
            std::fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(e_));        \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static bool read_file(const char *path, void *dst, size_t bytes) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t n = std::fread(dst, 1, bytes, f);
    std::fclose(f);
    return n == bytes;
}

int main(int argc, char **argv) {
    int format = ATMO_TARGET_RGBA32F, depth_format = -1, depth_pitch = 0;   // depth_format -1: depth.bin holds tight floats, drawn by the float-depth calls
    int detail = -1;                                                        // -1: the cloudless variant; 0 / 1: clouds_high, cloud detail off / on
    bool have_time = false;
    float time_s = 0.0f;
    bool usage = argc < 8 || (argc - 8) % 2 != 0;
    for (int i = 8; !usage && i + 1 < argc; i += 2) {
        const char *opt = argv[i], *val = argv[i + 1];
        if (std::strcmp(opt, "--target") == 0) {
            if (std::strcmp(val, "rgba16f") == 0) format = ATMO_TARGET_RGBA16F;
            else if (std::strcmp(val, "rgba8") == 0) format = ATMO_TARGET_RGBA8_UNORM;
            else if (std::strcmp(val, "rgba8_srgb") == 0) format = ATMO_TARGET_RGBA8_SRGB;
            else if (std::strcmp(val, "bgra8") == 0) format = ATMO_TARGET_BGRA8_UNORM;
            else if (std::strcmp(val, "bgra8_srgb") == 0) format = ATMO_TARGET_BGRA8_SRGB;
            else if (std::strcmp(val, "a2b10g10r10") == 0) format = ATMO_TARGET_A2B10G10R10_UNORM;
            else { std::fprintf(stderr, "--target: rgba16f, rgba8, rgba8_srgb, bgra8, bgra8_srgb or a2b10g10r10\n"); return 2; }
        } else if (std::strcmp(opt, "--depth-format") == 0) {
            if (std::strcmp(val, "d32f") == 0) depth_format = ATMO_DEPTH_D32_SFLOAT;
            else if (std::strcmp(val, "d16") == 0) depth_format = ATMO_DEPTH_D16_UNORM;
            else if (std::strcmp(val, "x8d24") == 0) depth_format = ATMO_DEPTH_X8_D24_UNORM;
            else { std::fprintf(stderr, "--depth-format: d32f, d16 or x8d24\n"); return 2; }
        } else if (std::strcmp(opt, "--depth-pitch") == 0) {
            depth_pitch = std::atoi(val);
        } else if (std::strcmp(opt, "--detail") == 0) {
            detail = std::atoi(val) != 0 ? 1 : 0;
        } else if (std::strcmp(opt, "--time") == 0) {
            have_time = true;
            time_s = (float)std::atof(val);
        } else {
            usage = true;
        }
    }
    if (usage || (depth_pitch != 0 && depth_format < 0) || (detail >= 0 && (depth_format >= 0 || format != ATMO_TARGET_RGBA32F))) {
        std::fprintf(stderr, "usage: %s frame.bin depth.bin out.bin planet_radius atmosphere_height u_density view_steps [--target rgba16f|rgba8|rgba8_srgb|bgra8|bgra8_srgb|a2b10g10r10] "
                             "[--depth-format d32f|d16|x8d24 [--depth-pitch BYTES]] [--detail 0|1] [--time SECONDS]\n", argv[0]);
        return 2;
    }
    AtmoContext *ctx = nullptr;
    AtmoFrame frame;
    if (!read_file(argv[1], &frame, sizeof(frame))) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    if (have_time) frame.time = time_s;
    // a host detects depth sources by the query, not by the ABI version (which they did not change)
    const size_t texel_bytes = depth_format < 0 ? sizeof(float) : (size_t)atmo_depth_texel_bytes(depth_format);
    if (texel_bytes == 0) { std::fprintf(stderr, "this libatmo_hip does not read depth format %d\n", depth_format); return 1; }
    const size_t depth_row = depth_pitch > 0 ? (size_t)depth_pitch : (size_t)frame.viewport_w * texel_bytes;
    if (depth_row < (size_t)frame.viewport_w * texel_bytes) { std::fprintf(stderr, "--depth-pitch is below a row of the viewport\n"); return 2; }
    const size_t depth_bytes = depth_row * (size_t)frame.viewport_h;
    std::vector<unsigned char> depth(depth_bytes);
    if (!read_file(argv[2], depth.data(), depth_bytes)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
    const float radius = (float)std::atof(argv[4]), height = (float)std::atof(argv[5]), density = (float)std::atof(argv[6]);
    const int view_steps = std::atoi(argv[7]);

    if (atmo_abi_version() != ATMO_ABI_VERSION) { std::fprintf(stderr, "ABI mismatch\n"); return 1; }
    int rc = atmo_create(0, detail >= 0 ? ATMO_VARIANT_CLOUDS_HIGH : ATMO_VARIANT_NO_CLOUDS, view_steps, 0, ATMO_LIGHT_LUT, 0, &ctx);
    if (rc != ATMO_OK) { std::fprintf(stderr, "atmo_create -> %d: %s\n", rc, atmo_last_error_string(nullptr)); return 1; }
    // planet_atmosphere.gd:114-115 and the demo's shader_params (planet_atmosphere_test.tscn:97-104)
    CHECK_ATMO(atmo_set_param_f32(ctx, "u_planet_radius", &radius, 1));
    CHECK_ATMO(atmo_set_param_f32(ctx, "u_atmosphere_height", &height, 1));
    CHECK_ATMO(atmo_set_param_f32(ctx, "u_density", &density, 1));
    const float strength = 1.0f;
    CHECK_ATMO(atmo_set_param_f32(ctx, "u_scattering_strength", &strength, 1));
    if (atmo_set_param_f32(ctx, "u_not_a_uniform", &strength, 1) != ATMO_E_NAME) { std::fprintf(stderr, "expected ATMO_E_NAME\n"); return 1; }
    CHECK_ATMO(atmo_bake_optical_depth(ctx, nullptr));  // replaces OpticalDepthBaker's SubViewport round trip
    if (detail >= 0) {
        const AtmoNoiseVolume volume = {32, 7u, 0.15f, 3, 0.5f, {0.0f, 0.0f, 0.0f}, /*seamless*/ 1, /*invert*/ 0, /*normalize*/ 1};
        CHECK_ATMO(atmo_generate_noise_volume(ctx, &volume, /*bind*/ 1, nullptr, nullptr));
        CHECK_ATMO(atmo_set_cloud_detail(ctx, detail));   // (a host detects the feature by the symbol: the ABI version did not change)
    }

    const size_t rect_pix = (size_t)(frame.x1 - frame.x0) * (frame.y1 - frame.y0);
    // a host detects packed targets by the query, not by the ABI version (which they did not change)
    const size_t pixel_bytes = (size_t)atmo_target_pixel_bytes(format);
    if (pixel_bytes == 0) { std::fprintf(stderr, "this libatmo_hip does not draw into target format %d\n", format); return 1; }
    void *d_depth = nullptr;
    void *d_rgba = nullptr;
    CHECK_HIP(hipMalloc(&d_depth, depth_bytes));
    CHECK_HIP(hipMalloc(&d_rgba, rect_pix * pixel_bytes));
    CHECK_HIP(hipMemcpy(d_depth, depth.data(), depth_bytes, hipMemcpyHostToDevice));
    const char *drawn_by = "atmo_render";
    if (depth_format >= 0) {
        const AtmoDepth source = {d_depth, depth_format, depth_pitch};
        const AtmoTarget target = {d_rgba, format, /*row_pitch_bytes: tight*/ 0};
        CHECK_ATMO(atmo_render_depth_target(ctx, &frame, &source, &target, /*composite*/ 0, nullptr));
        drawn_by = "atmo_render_depth_target";
    } else if (format == ATMO_TARGET_RGBA32F) {
        CHECK_ATMO(atmo_render(ctx, &frame, (const float *)d_depth, (float *)d_rgba, nullptr));
    } else {
        drawn_by = "atmo_render_target";
        const AtmoTarget target = {d_rgba, format, /*row_pitch_bytes: tight*/ 0};
        CHECK_ATMO(atmo_render_target(ctx, &frame, (const float *)d_depth, &target, /*composite*/ 0, nullptr));
    }
    CHECK_HIP(hipDeviceSynchronize());
    std::vector<unsigned char> rgba(rect_pix * pixel_bytes);
    CHECK_HIP(hipMemcpy(rgba.data(), d_rgba, rgba.size(), hipMemcpyDeviceToHost));
    FILE *f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(rgba.data(), 1, rgba.size(), f) != rgba.size()) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    std::fclose(f);
    std::printf("%s: %zu pixels shaded, %zu bytes each\n", drawn_by, rect_pix, pixel_bytes);
    (void)hipFree(d_depth);
    (void)hipFree(d_rgba);
    CHECK_ATMO(atmo_destroy(ctx));
    return 0;
}
