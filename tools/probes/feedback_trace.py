"""The tile-order feedback's decisions, draw by draw, as the counters of atmo_get_feedback_stats show them: (states, ordered_draws, sorts, recycled) after
every draw of a few fixed sequences, with the device synchronised after each draw, so that every pending sort is seen complete by the next one and the
numbers do not depend on timing.  Two libraries that decide alike print the same text:

  tools/ab_build_commit.sh pre <parent commit>
  ATMO_HIP_LIB=$PWD/godot_atmosphere_shader_amd/libatmo_hip_pre.so python tools/probes/feedback_trace.py > pre.txt
  python tools/probes/feedback_trace.py > new.txt && cmp pre.txt new.txt

Arguments: the sequences to run (still pan1 orbit5 seven_rects batch; default: all) -- a short run for an API trace, say.
ATMO_HEAVY_SPLIT=0: whether a draw's heavy tiles go to the lane-split kernel depends on measured clocks (profiles/feedback_refactor/)."""
import os
import sys

os.environ["ATMO_HEAVY_SPLIT"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from godot_atmosphere_shader_amd import scene as S  # noqa: E402
from godot_atmosphere_shader_amd.demo import demo_params, demo_textures, make_node  # noqa: E402

TEX, PARAMS = demo_textures(), demo_params()
DEV = torch.device("cuda")


def stats(node):
    st = node.feedback_stats()
    return "(%d, %d, %d, %d)" % (st["states"], st["ordered_draws"], st["sorts"], st["recycled"])


def single(label, config, cams, rects=None):
    """One atmo_render per camera (rects[k % len]: its rect)."""
    node = make_node(config, TEX, PARAMS)
    stream = torch.cuda.current_stream().cuda_stream
    for k, cam in enumerate(cams):
        rect = rects[k % len(rects)] if rects else None
        depth = bench.depth_ground_sphere_torch(torch, S, cam, DEV)
        x0, y0, x1, y1 = rect or (0, 0, cam.width, cam.height)
        out = torch.empty((y1 - y0, x1 - x0, 4), dtype=torch.float32, device=DEV)
        node.render_prepared(node.prepare_frame(cam, rect=rect), depth.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        print(f"{label} {config} draw {k}: {stats(node)}")
    node.close()


def batch(label, config, cam_pairs):
    """One atmo_render_views per pair of cameras."""
    node = make_node(config, TEX, PARAMS)
    for k, pair in enumerate(cam_pairs):
        depths = [bench.depth_ground_sphere_torch(torch, S, c, DEV) for c in pair]
        node.render_views(list(pair), depths)
        torch.cuda.synchronize()
        print(f"{label} {config} batch {k}: {stats(node)}")
    node.close()


def main():
    want = set(sys.argv[1:]) or {"still", "pan1", "orbit5", "seven_rects", "batch"}
    w, h = 960, 540
    still = S.Camera.from_pose(w, h, "P_space")
    pan = bench.motion_cameras(S, w, h, ("pan", 1.0), 24)
    for config in ("clouds_high_rm", "clouds_high", "no_clouds_32x8_direct"):
        if "still" in want:
            single("still", config, [still] * 24)
        if "pan1" in want:
            single("pan1", config, pan)
        if "orbit5" in want:
            single("orbit5", config, bench.motion_cameras(S, w, h, ("orbit", 5.0), 24))
    if "seven_rects" in want:
        # tests/test_gpu_parity.py::test_tile_feedback_keeps_one_state_per_rect_and_stream: more keys than slots, the recycling budget runs out
        cam = S.Camera.from_pose(1280, 720, "P_space")
        single("seven_rects", "clouds_high", [cam] * 70, rects=[(0, 0, 1280 - 16 * k, 720) for k in range(7)])
    if "batch" in want:
        other = S.Camera.from_pose(w, h, "P_limb")
        for config in ("clouds_high_rm", "no_clouds_32x8_direct"):
            batch("still", config, [(still, other)] * 24)
            batch("pan1", config, [(c, other) for c in pan])


if __name__ == "__main__":
    main()
