"""GPU test of what tests/test_binding_calls_host.py cannot reach: real CUDA tensors, and stream=None, which is torch's current stream on the tensor's
device.  Every draw method of the binding is called four ways -- stream=None, stream=None under `with torch.cuda.stream(side)`, stream=side and
stream=side.cuda_stream -- into equal buffers, and the four results are the same bits.  64 x 40 is the smallest frame with more than one tile row and
column; the proxy draws go into sentinel-filled buffers and must change them, so a frame the box misses cannot pass."""
import numpy as np
import pytest
import torch

from common import demo_textures, make_node
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd.planet_atmosphere import MODE_FAR, MODE_NEAR

pytestmark = pytest.mark.gpu

W, H = 64, 40
SENTINEL = 7.0


@pytest.fixture(scope="module")
def node():
    n = make_node("no_clouds_32x8_direct", demo_textures(cube_n=64, shape_n=32))
    n.global_transform = np.eye(4)
    yield n
    n.close()


def _near_cams():
    return [S.Camera.from_pose(W, H, "P_space"), S.Camera.from_pose(W, H, "P_limb")]


def _far_cams():   # as tests/test_proxy_gpu.py's _far_cam and tests/test_views_proxy_gpu.py's _B: the box in the middle of the picture
    return [S.Camera(W, H, (31.0, 17.0, 420.0), (0.0, 0.0, 0.0)), S.Camera(W, H, (-140.0, 60.0, 380.0), (0.0, 0.0, 0.0))]


def _depth(cam):
    return torch.from_numpy(S.depth_ground_sphere(cam)).cuda()


def _sentinel():
    return torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")


def _scene(seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand((H, W, 4), generator=g, dtype=torch.float32).cuda()


# method -> (far mode?, the call: (node, cameras, depths, buffers, stream) -> the tensors drawn into)
METHODS = {
    "render": (False, lambda n, c, d, b, s: [n.render(c[0], d[0], b[0], stream=s)]),
    "render_composite": (False, lambda n, c, d, b, s: [n.render_composite(c[0], d[0], b[0], stream=s)]),
    "render_proxy": (True, lambda n, c, d, b, s: [n.render_proxy(c[0], d[0], b[0], stream=s)]),
    "render_proxy_composite": (True, lambda n, c, d, b, s: [n.render_proxy_composite(c[0], d[0], b[0], stream=s)]),
    "render_views": (False, lambda n, c, d, b, s: n.render_views(c, d, b, stream=s)),
    "render_views_proxy": (True, lambda n, c, d, b, s: n.render_views_proxy(c, d, b, stream=s)),
    "draw@near": (False, lambda n, c, d, b, s: [n.draw(c[0], d[0], b[0], stream=s)]),
    "draw@far": (True, lambda n, c, d, b, s: [n.draw(c[0], d[0], b[0], stream=s)]),
    "draw_views@near": (False, lambda n, c, d, b, s: n.draw_views(c, d, b, stream=s)),
    "draw_views@far": (True, lambda n, c, d, b, s: n.draw_views(c, d, b, stream=s)),
}


@pytest.mark.parametrize("method", list(METHODS))
def test_every_way_to_name_the_stream_draws_the_same_bits(node, method):
    far, call = METHODS[method]
    cams = _far_cams() if far else _near_cams()
    depths = [_depth(c) for c in cams]
    node._process(0.0, cams[0], time=0.0)       # the mode switch of planet_atmosphere.gd:285-341: `draw` follows it
    assert node._mode == (MODE_FAR if far else MODE_NEAR)
    composite = "composite" in method or "draw" in method
    fills = [_scene(3 + i) if composite else _sentinel() for i in range(len(cams))]
    side = torch.cuda.Stream()
    results = []
    for way in ("none", "none_under_side", "side", "side_handle"):
        bufs = [f.clone() for f in fills]
        torch.cuda.synchronize()                # the buffers are filled on the default stream: done before a draw on another one starts
        if way == "none":
            outs = call(node, cams, depths, bufs, None)
        elif way == "none_under_side":
            with torch.cuda.stream(side):
                outs = call(node, cams, depths, bufs, None)
        else:
            outs = call(node, cams, depths, bufs, side if way == "side" else side.cuda_stream)
        side.synchronize()
        torch.cuda.synchronize()
        assert all(o is b for o, b in zip(outs, bufs))
        results.append([o.cpu().numpy().view(np.uint32) for o in outs])
    for i, first in enumerate(results[0]):
        assert (first != fills[i].cpu().numpy().view(np.uint32)).any(), f"view {i}: nothing was drawn"
        for way, other in zip(("none_under_side", "side", "side_handle"), results[1:]):
            assert np.array_equal(first, other[i]), f"view {i}: stream given as {way} drew other bits"
