"""GPU test of what tests/test_ray_binding_calls_host.py cannot reach: the ray methods on a real side stream.  The host file proves that the stream's
context is entered around every allocation; only a device proves that the work is ordered on that stream.  Every ray method is called three ways --
stream=None, stream=side (a torch.cuda.Stream) and stream=side.cuda_stream (its raw handle) -- and the three results are the same bits.  No graph capture,
and nothing runs on the side stream before the default stream, which made the inputs, has been waited for.

70 rays are one full wavefront and a ragged one; the 18 x 6 viewport and lens image are two 16 x 4 tile columns and two tile rows, both ragged; the
5 x 3 quads have absent slots on both edges."""
import math

import numpy as np
import pytest
import torch

from common import demo_params, demo_textures, make_node
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.lens import Lens

pytestmark = pytest.mark.gpu

SENTINEL = 0.25
LIVE = 50      # the counted queue's live length: 20 rows of the 70 stay as they were


@pytest.fixture(scope="module")
def nodes():
    lut = make_node("no_clouds_8", demo_textures(), demo_params())
    clouds = make_node("clouds_high", demo_textures(), demo_params())      # the declared sampler: a mip chain is bound
    yield lut, clouds
    lut.close()
    clouds.close()


def _camera(w, h):
    cam = S.Camera.from_pose(w, h, "P_space")
    return cam, torch.from_numpy(S.depth_ground_sphere(cam)).cuda()


def _every_ray_call(lut, clouds, given, s):
    """Every ray method once on stream `s`, in one chain; `given` holds the inputs, made on the default stream.  Returns name -> tensor."""
    cam70, rays, count = given["cam70"], given["rays"], given["count"]
    (cam, depth), (qcam, qdepth), lens = given["view"], given["quad_view"], given["lens"]
    r = {}
    r["plain"] = lut.shade_rays(rays, cam70, stream=s)
    r["clouds_plain"] = clouds.shade_rays(rays, cam70, stream=s)
    r["order"] = lut.ray_order(rays, stream=s)
    r["ordered"] = lut.shade_rays(rays, cam70, index=r["order"], stream=s)
    r["listed_out"] = given["listed_out"]
    r["list_index"], r["list_count"] = lut.ray_list(rays, count, order=True, cull=True, camera=cam70, out=r["listed_out"], stream=s)
    lut.shade_rays(rays, cam70, out=r["listed_out"], index=r["list_index"], stream=s)
    r["camera_rays"] = lut.camera_rays(cam, depth, stream=s)
    r["camera_ray_quads"] = clouds.camera_ray_quads(qcam, qdepth, stream=s)
    r["quads"] = clouds.shade_ray_quads(r["camera_ray_quads"], qcam, width=qcam.width, stream=s)
    r["lens_rays"], r["lens_index"] = lut.lens_rays(lens, tile_index=True, stream=s)
    r["lens_quads"] = lut.lens_rays(lens, quads=True, stream=s)
    r["image_tiles"] = lut.render_lens(lens, cam, quads=False, stream=s)
    r["image_quads"] = clouds.render_lens(lens, cam, quads=True, stream=s)
    return r


def test_every_way_to_name_the_stream_computes_the_same_bits(nodes):
    lut, clouds = nodes
    cam70, depth70 = _camera(10, 7)
    given = dict(cam70=cam70, rays=lut.camera_rays(cam70, depth70), count=torch.tensor([LIVE], dtype=torch.int32, device="cuda"),
                 view=_camera(18, 6), quad_view=_camera(5, 3), lens=Lens.fisheye(18, 6, fov=math.radians(200.0)))
    assert tuple(given["rays"].shape) == (70, 8)
    side = torch.cuda.Stream()
    results = {}
    for way, s in (("none", None), ("side", side), ("side_handle", side.cuda_stream)):
        given["listed_out"] = torch.full((70, 4), SENTINEL, dtype=torch.float32, device="cuda")      # rows behind the live length keep it
        torch.cuda.synchronize()      # the inputs, and the way before: done before anything starts on another stream
        got = _every_ray_call(lut, clouds, given, s)
        side.synchronize()
        torch.cuda.synchronize()
        results[way] = {name: t.cpu().numpy().view(np.uint32) for name, t in got.items()}
    first = results["none"]
    assert first["plain"].shape == (70, 4) and first["order"].shape == (70,) and first["camera_rays"].shape == (108, 8)
    assert first["camera_ray_quads"].shape == (24, 8) and first["quads"].shape == (24, 4) and first["lens_rays"].shape == (108, 8)
    assert first["lens_index"].shape == (256,) and first["lens_quads"].shape == (108, 8) and first["image_tiles"].shape == first["image_quads"].shape == (6, 18, 4)
    for name in ("plain", "clouds_plain", "ordered", "quads", "image_tiles", "image_quads"):
        assert first[name].any(), f"{name}: nothing was shaded"
    assert np.array_equal(first["plain"], first["ordered"]) and sorted(first["order"].tolist()) == list(range(70))
    sentinel = np.float32(SENTINEL).view(np.uint32)
    assert 0 < int(first["list_count"][0]) <= LIVE and (first["listed_out"][LIVE:] == sentinel).all() and (first["listed_out"][:LIVE] != sentinel).any(axis=1).all()
    for way in ("side", "side_handle"):
        for name, want in first.items():
            assert np.array_equal(results[way][name], want), f"{name}: stream given as {way} computed other bits"
