"""GPU tests of the cloud shape volume generator (include/atmo_noise_volume.h): the device bytes against the float32 numpy statement
(tests/noise_volume_host.py) byte for byte on the table's cases, stale extrema, the bound layout and the frames drawn from it against a host-upload
twin, stream order without host waits, the refusal inside a graph capture, and the NoiseVolume resource on a node.  Frames are 96 x 54, clouds_high,
the default sampler."""
import ctypes as C

import numpy as np
import pytest
import torch

import noise_volume_host as H
from godot_atmosphere_shader_amd import scene as S

pytestmark = pytest.mark.gpu

W, HGT = 96, 54
# every case of the table with normalize on and off, and one of each with invert
VARIANTS = [(k, norm, False) for k in H.CASES for norm in (True, False)] + [("n5", True, True), ("n33", False, True)]


def _desc(name, normalize=True, invert=False, offset=None):
    from godot_atmosphere_shader_amd import _native as N

    c = H.CASES[name]
    return N.AtmoNoiseVolume(c["n"], H.SEED, c["frequency"], c["octaves"], H.GAIN, (C.c_float * 3)(*(offset or c["offset"])), int(c["seamless"]),
                             int(invert), int(normalize))


def _generate(lib, ctx, desc, bind=0, stream=None):
    from godot_atmosphere_shader_amd import _native as N

    out = np.empty((desc.size,) * 3, dtype=np.uint8)
    N.check(ctx, lib.atmo_generate_noise_volume(ctx, C.byref(desc), bind, out.ctypes.data_as(C.c_void_p), stream))
    return out


@pytest.fixture(scope="module")
def gen_ctx():
    from godot_atmosphere_shader_amd import _native as N

    lib = N.load()
    ctx = C.c_void_p()
    N.check(None, lib.atmo_create(0, N.VARIANT_NO_CLOUDS, 0, 0, N.LIGHT_LUT, 0, C.byref(ctx)))
    yield lib, ctx
    lib.atmo_destroy(ctx)


@pytest.fixture(scope="module")
def scene():
    from common import demo_params, demo_textures

    cam = S.Camera.from_pose(W, HGT, "P_clouds")
    depth = torch.from_numpy(S.depth_ground_sphere(cam)).cuda()
    return dict(demo_textures(cube_n=64, shape_n=32)), demo_params(), cam, depth


@pytest.mark.parametrize("name,normalize,invert", VARIANTS, ids=[f"{k}-{'norm' if n else 'raw'}{'-inv' if i else ''}" for k, n, i in VARIANTS])
def test_device_bytes_equal_the_statement(gen_ctx, name, normalize, invert):
    lib, ctx = gen_ctx
    got = _generate(lib, ctx, _desc(name, normalize, invert))
    want = H.case_volume(name, normalize, invert)
    bad = int((got != want).sum())
    print(f"{name} normalize={normalize} invert={invert}: {bad} of {want.size} bytes differ")
    assert np.array_equal(got, want)


def test_a_second_generation_does_not_see_the_first_ones_extrema(gen_ctx):
    """n16's t spans [0.0806, 0.8528], n33's [0.1753, 0.8525]: extrema left over from n16 would mis-scale every byte of n33.  Each way round, on one
    context, and once more after a different size."""
    lib, ctx = gen_ctx
    assert H.case_t("n16").min() < H.case_t("n33").min() and H.case_t("n16").max() > H.case_t("n33").max()
    for name in ("n16", "n33", "n16", "n5", "n33"):
        assert np.array_equal(_generate(lib, ctx, _desc(name)), H.case_volume(name)), name


def _read_shape_layout(node):
    from godot_atmosphere_shader_amd import _native as N

    nbytes = C.c_size_t(0)
    N.check(node._ctx, node._lib.atmo_read_texture_layout(node._ctx, b"u_cloud_shape_texture", None, 0, C.byref(nbytes), None))
    out = np.empty(nbytes.value // 4, dtype=np.uint32)
    N.check(node._ctx, node._lib.atmo_read_texture_layout(node._ctx, b"u_cloud_shape_texture", out.ctypes.data_as(C.c_void_p), nbytes.value, None, None))
    return out


def _host_layout(lib, texels):
    from godot_atmosphere_shader_amd import _native as N

    n = texels.shape[0]
    texels = np.ascontiguousarray(texels)
    want = np.empty(n * n * n, dtype=np.uint32)
    assert lib.atmo_host_layout_shape(texels.ctypes.data_as(C.c_void_p), n, want.ctypes.data_as(C.c_void_p)) == N.ATMO_OK
    return want


def test_bind_gives_the_layout_and_the_frame_of_a_host_upload(scene):
    from common import make_node
    from godot_atmosphere_shader_amd import _native as N

    tex, params, cam, depth = scene
    node = make_node("clouds_high", tex, params)
    twin = make_node("clouds_high", dict(tex, shape=H.case_volume("n24")), params)
    before = node.render(cam, depth).cpu().numpy()
    N.check(node._ctx, node._lib.atmo_generate_noise_volume(node._ctx, C.byref(_desc("n24")), 1, None, None))   # bind, no read-back: only enqueues
    n = C.c_int(0)
    N.check(node._ctx, node._lib.atmo_get_texture_size(node._ctx, b"u_cloud_shape_texture", C.byref(n), None, None, None))
    assert n.value == 24
    assert np.array_equal(_read_shape_layout(node), _host_layout(node._lib, H.case_volume("n24")))
    got, want = node.render(cam, depth).cpu().numpy(), twin.render(cam, depth).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, before)                              # the picture shows the shape volume: the comparison discriminates
    # bind and read-back in one call: the same bytes both ways; a size change re-binds
    texels = _generate(node._lib, node._ctx, _desc("n33", normalize=False), bind=1)
    assert np.array_equal(texels, H.case_volume("n33", normalize=False))
    assert np.array_equal(_read_shape_layout(node), _host_layout(node._lib, texels))
    node.close()
    twin.close()


def test_generate_bind_draw_in_stream_order_without_host_waits(scene):
    """Three frames on a non-default stream, offset[2] = 0, 0.5, 1.0 of the n = 24 case: generate, bind and draw enqueued with no host synchronisation in
    between, read back at the end; each equals its host-upload twin, and the updates add no device-wide wait."""
    from common import make_node
    from godot_atmosphere_shader_amd import _native as N

    tex, params, cam, depth = scene
    c = H.CASES["n24"]
    offsets = [(0.0, 0.0, z) for z in (0.0, 0.5, 1.0)]
    volumes = [H.generate_volume_host(24, H.case_noise(c), off, True) for off in offsets]
    twin = make_node("clouds_high", tex, params)
    want = []
    for vol in volumes:
        twin.set_shader_parameter("u_cloud_shape_texture", vol)
        want.append(twin.render(cam, depth).cpu().numpy())
    twin.close()
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])      # the frames tell the offsets apart

    node = make_node("clouds_high", tex, params)
    side = torch.cuda.Stream()
    outs = [torch.zeros((HGT, W, 4), dtype=torch.float32, device="cuda") for _ in offsets]
    node.render(cam, depth, out=outs[0], stream=side)      # the first draw on the stream: the bake and the feedback state are behind it
    torch.cuda.synchronize()
    outs[0].zero_()
    torch.cuda.synchronize()

    def syncs():
        k = C.c_uint()
        N.check(node._ctx, node._lib.atmo_get_host_wait_stats(node._ctx, C.byref(k)))
        return k.value

    s0 = syncs()
    for off, out in zip(offsets, outs):
        N.check(node._ctx, node._lib.atmo_generate_noise_volume(node._ctx, C.byref(_desc("n24", offset=off)), 1, None, C.c_void_p(side.cuda_stream)))
        node.render(cam, depth, out=out, stream=side)
    assert syncs() == s0
    side.synchronize()
    for k, out in enumerate(outs):
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k
    node.close()


def test_read_back_is_refused_inside_a_graph_capture(scene):
    """texels_host waits for the stream: on a capturing stream ATMO_E_STATE, nothing enqueued or allocated, the capture still usable."""
    from common import make_node
    from godot_atmosphere_shader_amd import _native as N

    tex, params, cam, depth = scene
    node = make_node("clouds_high", tex, params)
    ref = node.render(cam, depth).clone()
    torch.cuda.synchronize()
    out = torch.zeros_like(ref)
    frame = node.prepare_frame(cam)
    host = np.zeros((16, 16, 16), dtype=np.uint8)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc = node._lib.atmo_generate_noise_volume(node._ctx, C.byref(_desc("n16")), 0, host.ctypes.data_as(C.c_void_p), C.c_void_p(side.cuda_stream))
            assert rc == N.ATMO_E_STATE and b"texels_host" in node._lib.atmo_last_error_string(node._ctx)
            node.render_prepared(frame, depth.data_ptr(), out.data_ptr(), side.cuda_stream)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and not host.any()
    assert np.array_equal(_generate(node._lib, node._ctx, _desc("n16")), H.case_volume("n16"))      # outside a capture: as before
    node.close()


def test_node_draws_a_noise_volume_resource_like_its_bytes(scene):
    """node.set_shader_parameter("u_cloud_shape_texture", NoiseVolume(...)) draws the frame of the array form; get_data() gives the statement's bytes."""
    from common import make_node
    from godot_atmosphere_shader_amd import NoiseVolume

    tex, params, cam, depth = scene
    c = H.CASES["n24"]
    res = NoiseVolume(noise=H.case_noise(c), size=c["n"], seamless=c["seamless"], offset=c["offset"])
    node = make_node("clouds_high", tex, params)
    node.set_shader_parameter("u_cloud_shape_texture", res)
    got = node.render(cam, depth).cpu().numpy()
    node.set_shader_parameter("u_cloud_shape_texture", H.case_volume("n24"))
    want = node.render(cam, depth).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(res.get_data(), H.case_volume("n24"))
    res.offset = (0.0, 0.0, 4.25)                                       # animate, bind again in front of the next draw
    res.bind_to(node)
    moved = node.render(cam, depth).cpu().numpy()
    node.set_shader_parameter("u_cloud_shape_texture", H.generate_volume_host(24, H.case_noise(c), (0.0, 0.0, 4.25), True))
    assert np.array_equal(moved.view(np.uint32), node.render(cam, depth).cpu().numpy().view(np.uint32)) and not np.array_equal(moved, got)
    node.close()
    res.close()
