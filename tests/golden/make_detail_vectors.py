#!/usr/bin/env python3
"""Generates tests/golden/reference_exec_detail.npz: the reference's shader text executed with `#define CLOUDS_ALWAYS_LOW_QUALITY`
(planet_atmosphere_main.gdshaderinc:49) commented out -- the detail fetch of get_density_full and the alpha0 branch of get_light_raymarched live, TIME
read -- for the frames of tests/cloud_detail_cases.py.  What include/atmo_cloud_detail.h's switch is held to.

    python tests/golden/make_detail_vectors.py        # needs the reference tree; about four minutes; the same bytes every time

At generation time the reference's shader directory is copied into a temporary directory, that one line is commented out in the copy, and
make_reference_vectors.SHADERS is pointed at it; the committed interpreter (gdshader_vm.py through make_reference_vectors.run_frame) executes the
copy, unedited otherwise.  Nothing of the text is stored: the file holds the cases' names, the outputs, and what the conditions below measured.
Cameras, depths and the LUT are reference_exec.npz's.

THE CONDITIONS every frame must meet (asserted here; tests/test_cloud_detail_host.py re-asserts them on the committed file, so that no GPU test
passes on nothing).  A frame that misses one gets another pose or time -- 12.25, then 3.0 -- never a lower bar.  One did: clouds_high_rm with the
24^3 shape volume at t = 37.5 held one pixel, under the level-0 sampler, that changed with the threshold (condition 4); it stands at t = 12.25, where
both samplers meet all four (cloud_detail_cases.T_SUBSTITUTE).
  1. It differs from the LOW-QUALITY frame (the shipped text) of the same pose and sampler by more than 1e-3 in at least 1 % of its pixels.
  2. A t = 37.5 frame differs from the t = 0 frame of the same scene likewise.
  3. A raymarched-light frame at t = 37.5 differs by more than 1e-4 in at least 20 pixels from the same text with ALL six taps forced to
     get_density_low, and with all forced to get_density (two more temporary copies): both sides of alpha0 < 0.3 are in the picture.
  4. A raymarched-light frame is bit-identical with the literal 0.3 replaced by 0.2999 and by 0.3001 (two more copies): no pixel's alpha0 comes
     within 1e-4 of the threshold at a lit sample, 25 times the ~4e-6 by which a kernel's alpha0 can differ from the text's -- so the test compares
     every pixel.
"""
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_reference_vectors as M  # noqa: E402
import reference_scenes as RS  # noqa: E402
import vm_textures as T  # noqa: E402
import cloud_detail_cases as CD  # noqa: E402
from godot_atmosphere_shader_amd import scene as S  # noqa: E402

REFERENCE_SHADERS = M.SHADERS
MIN_FRACTION, MIN_PIXELS = 0.01, 20


def edited_copy(tmp, name, edits):
    """A copy of the reference's shader directory with `edits` = [(file under include/, regex, replacement)], each of which must match exactly once."""
    dst = os.path.join(tmp, name)
    shutil.copytree(REFERENCE_SHADERS, dst)
    for rel, pattern, repl in edits:
        path = os.path.join(dst, "include", rel)
        text, n = re.subn(pattern, repl, open(path).read())
        assert n == 1, (rel, pattern, n)
        open(path, "w").write(text)
    return dst


DETAIL_ON = ("planet_atmosphere_main.gdshaderinc", r"(?m)^#define CLOUDS_ALWAYS_LOW_QUALITY", "//#define CLOUDS_ALWAYS_LOW_QUALITY")
COPIES = {
    "detail": [DETAIL_ON],
    # get_light_raymarched's two branches (clouds:132-136) made the same call
    "all_low": [DETAIL_ON, ("cloud_funcs.gdshaderinc", r"(alpha0 < 0\.3\) \{\s*density = )get_density\(", r"\1get_density_low(")],
    "all_full": [DETAIL_ON, ("cloud_funcs.gdshaderinc", r"(\} else \{\s*density = )get_density_low\(pos,", r"\1get_density(pos,")],
    "thr_lo": [DETAIL_ON, ("cloud_funcs.gdshaderinc", r"alpha0 < 0\.3\)", "alpha0 < 0.2999)")],
    "thr_hi": [DETAIL_ON, ("cloud_funcs.gdshaderinc", r"alpha0 < 0\.3\)", "alpha0 < 0.3001)")],
}


def main():
    t_start = time.time()
    z = np.load(os.path.join(HERE, "reference_exec.npz"))
    demo, model_matrix = RS.scenes()["demo"]
    cube = S.make_coverage_cubemap(RS.CUBE_N)
    chain, padded = T.mip_chain(cube), T.pad_cubemap(cube)
    blue = S.make_blue_noise()
    out = {"viewport": np.array([RS.W, RS.H]), "cases": np.array([c["name"] for c in CD.CASES]), "samplers": np.array(CD.SAMPLERS),
           "crc_cubemap": np.uint32(S.checksum(cube)), "crc_blue_noise": np.uint32(S.checksum(blue))}
    shapes = {}

    def run(shaders, case, sampler, t):
        n = case["shape_n"]
        if n not in shapes:
            shapes[n] = S.make_shape_texture(n)
            out[f"crc_shape_{n}"] = np.uint32(S.checksum(shapes[n]))
        params = demo if case["invert"] is None else dict(demo, u_cloud_shape_invert=case["invert"])
        units = dict(u_optical_depth_texture=T.LutTexture(z["lut_demo"]), u_blue_noise_texture=T.ByteTexture2D(blue),
                     u_cloud_shape_texture=T.ShapeTexture(shapes[n]))
        if sampler == "lod0":
            units["u_cloud_coverage_cubemap"] = T.CubeTexture(padded)
        cam = RS.camera_from_fixture(z, RS.W, RS.H, case["pose"])
        M.SHADERS = shaders
        try:
            rgba, disc, _, _ = M.run_frame(case["shader"], None, params, np.eye(4), model_matrix, cam, z[f"depth_demo_{case['pose']}"], units, time_s=t,
                                           cube_chain=chain if sampler == "declared" else None)
        finally:
            M.SHADERS = REFERENCE_SHADERS
        return rgba, disc

    differs = lambda a, b, tol: np.abs(a - b).max(-1) > tol
    with tempfile.TemporaryDirectory(prefix="detail_shaders_") as tmp:
        copies = {name: edited_copy(tmp, name, edits) for name, edits in COPIES.items()}
        for case in CD.CASES:
            for sampler in CD.SAMPLERS:
                k = CD.key(case, sampler)
                rgba, disc = run(copies["detail"], case, sampler, case["time"])
                out[f"rgba_{k}"], out[f"discard_{k}"] = rgba, np.packbits(disc)
                # 1. against the shipped (low-quality) text
                low, low_disc = run(REFERENCE_SHADERS, case, sampler, case["time"])
                assert (low_disc == disc).all(), k
                d_low = differs(rgba, low, 1e-3)
                assert d_low.mean() >= MIN_FRACTION, (k, "condition 1", d_low.mean())
                out[f"differs_from_low_{k}"] = np.packbits(d_low)
                note = f"low {100 * d_low.mean():.1f} %"
                # 2. against t = 0
                if case["time"] != 0.0:
                    still, _ = run(copies["detail"], case, sampler, 0.0)
                    twin = CD.t0_twin(case)
                    if twin is not None and f"rgba_{CD.key(twin, sampler)}" in out:
                        assert (still == out[f"rgba_{CD.key(twin, sampler)}"]).all(), k
                    d_t0 = differs(rgba, still, 1e-3)
                    assert d_t0.mean() >= MIN_FRACTION, (k, "condition 2", d_t0.mean())
                    out[f"differs_from_t0_{k}"] = np.packbits(d_t0)
                    note += f", t0 {100 * d_t0.mean():.1f} %"
                if CD.is_rm(case):
                    # 3. both sides of alpha0 < 0.3 are in the picture
                    if case["time"] != 0.0:
                        for side in ("all_low", "all_full"):
                            forced, _ = run(copies[side], case, sampler, case["time"])
                            d = differs(rgba, forced, 1e-4)
                            assert d.sum() >= MIN_PIXELS, (k, "condition 3", side, int(d.sum()))
                            out[f"differs_from_{side}_{k}"] = np.packbits(d)
                            note += f", {side} {int(d.sum())} px"
                    # 4. no pixel near the threshold
                    changed = 0
                    for side in ("thr_lo", "thr_hi"):
                        moved, _ = run(copies[side], case, sampler, case["time"])
                        changed += int((moved.view(np.uint32) != rgba.view(np.uint32)).any(-1).sum())
                    assert changed == 0, (k, "condition 4", changed)
                    out[f"threshold_sensitive_pixels_{k}"] = np.int64(changed)
                print(f"{time.time() - t_start:6.1f}s {k}: {int((~disc).sum())} of {disc.size} fragments kept, max rgba {rgba.max():.4f}; {note}", flush=True)
    path = os.path.join(HERE, "reference_exec_detail.npz")
    M.save_npz_reproducibly(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
