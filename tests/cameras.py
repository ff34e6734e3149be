"""Camera kinds no `scene.Camera` makes -- off-axis (stereo eye) frusta, a sub-pixel-jittered frustum, an infinite far plane, an orthographic projection,
a rolled view -- and the depth buffers that go with them, for tests/test_projections_host.py and tests/test_projections_gpu.py.  Needs no GPU.

Each camera is a `scene.Camera` with its matrices replaced: width, height, near, far, reverse_z, projection, inv_projection, inv_view, view,
pixel_view_dirs().  The projections follow `scene.perspective`: Vulkan clip space (y down), reverse-Z in [0, 1] (1 = the near plane).  What they
put into inv_projection that the symmetric perspective leaves zero:

    eye_left / eye_right, jitter    elements 12, 13 (the fourth column's x, y): the frustum's axis is not the view axis
    infinite_far                    element 15 == 0: w = 0 at depth 0
    ortho                           element 10 (the depth column's z) != 0, element 11 == 0: the segment's direction is the same for every pixel, and
                                    the reference's ray (normalize of the undivided view-space xyz, from the camera's position) depends on the depth sample
"""
import math

import numpy as np

from godot_atmosphere_shader_amd import scene as S

KINDS = ("eye_left", "eye_right", "jitter", "infinite_far", "ortho")
ROLLED_UP = tuple((np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])).tolist())
IPD = 0.064                       # interpupillary distance, world units
EYE_X = (1.3, 0.7)                # the left eye's left / right extents, in units of the symmetric frustum's; the right eye's mirrored
EYE_Y = (0.9, 1.1)                # bottom / top, both eyes
JITTER_PX = (0.3, -0.2)           # the picture's shift, pixels (x to the right, y down)

# view space (-z ahead, +y up, OpenGL clip) -> Vulkan clip with reverse-Z in [0, 1]: y flipped, z' = (w - z) / 2
_FIX = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -0.5, 0.5], [0, 0, 0, 1]], dtype=np.float64)


def frustum(left, right, bottom, top, near, far):
    """glFrustum's extents on the near plane (far may be math.inf), as a view -> clip matrix in this module's convention."""
    if math.isinf(far):
        zz, zw = -1.0, -2.0 * near
    else:
        zz, zw = (far + near) / (near - far), 2.0 * far * near / (near - far)
    gl = np.array([[2.0 * near / (right - left), 0, (right + left) / (right - left), 0],
                   [0, 2.0 * near / (top - bottom), (top + bottom) / (top - bottom), 0],
                   [0, 0, zz, zw],
                   [0, 0, -1, 0]], dtype=np.float64)
    return _FIX @ gl


def orthographic(size, aspect, near, far):
    """Camera3D.PROJECTION_ORTHOGONAL with keep_aspect = KEEP_HEIGHT: `size` world units from the bottom to the top of the picture."""
    t = 0.5 * size
    r = t * aspect
    gl = np.array([[1.0 / r, 0, 0, 0], [0, 1.0 / t, 0, 0], [0, 0, -2.0 / (far - near), -(far + near) / (far - near)], [0, 0, 0, 1]], dtype=np.float64)
    return _FIX @ gl


def _inverse(projection, near, infinite):
    if not infinite:
        return np.linalg.inv(projection)
    # [[a, 0, c, 0], [0, b, d, 0], [0, 0, 0, n], [0, 0, -1, 0]]: written out, so that w = 0 at depth 0 exactly (element 15 is a true zero)
    a, b, c, d = projection[0, 0], projection[1, 1], projection[0, 2], projection[1, 2]
    inv = np.array([[1.0 / a, 0, 0, c / a], [0, 1.0 / b, 0, d / b], [0, 0, 0, -1.0], [0, 0, 1.0 / near, 0.0]], dtype=np.float64)
    assert np.allclose(projection @ inv, np.eye(4), atol=1e-12)
    return inv


def make(kind, width, height, eye, target, up=ROLLED_UP, fovy_deg=75.0, near=0.1, far=800.0, ortho_size=None):
    """A camera of `kind` ("plain": the symmetric control, `scene.Camera` untouched) that looks from `eye` at `target`.  Every kind but the control
    is rolled by default (up = ROLLED_UP).  The eyes sit -/+ IPD / 2 along the camera's right vector and look parallel to the centre camera."""
    cam = S.Camera(width, height, eye, target, up, fovy_deg=fovy_deg, near=near, far=far)
    cam.kind = kind
    if kind in ("plain", "rolled"):
        return cam
    aspect = width / height
    t = near * math.tan(math.radians(fovy_deg) * 0.5)
    r = t * aspect
    if kind in ("eye_left", "eye_right"):
        sign = -1.0 if kind == "eye_left" else 1.0
        lo, hi = EYE_X if kind == "eye_left" else EYE_X[::-1]
        cam.projection = frustum(-lo * r, hi * r, -EYE_Y[0] * t, EYE_Y[1] * t, near, far)
        cam.inv_view = cam.inv_view.copy()
        cam.inv_view[:3, 3] += sign * 0.5 * IPD * cam.inv_view[:3, 0]
        cam.view = np.linalg.inv(cam.inv_view)
    elif kind == "jitter":
        shift = np.eye(4)
        shift[0, 3], shift[1, 3] = 2.0 * JITTER_PX[0] / width, 2.0 * JITTER_PX[1] / height     # NDC, after the divide: x_clip += dx w_clip
        cam.projection = shift @ frustum(-r, r, -t, t, near, far)
    elif kind == "infinite_far":
        cam.far = math.inf
        cam.projection = frustum(-r, r, -t, t, near, math.inf)
    elif kind == "ortho":
        assert ortho_size is not None and ortho_size > 0.0
        cam.ortho_size = float(ortho_size)
        cam.projection = orthographic(ortho_size, aspect, near, far)
    else:
        raise ValueError(kind)
    cam.inv_projection = _inverse(cam.projection, near, kind == "infinite_far")
    return cam


def from_pose(kind, width, height, pose, **kw):
    """`make` at one of scene.POSES with the demo camera's fovy / near / far."""
    pose = S.POSES[pose] if isinstance(pose, str) else pose
    args = dict(S.DEMO_CAMERA)
    args.update(kw)
    return make(kind, width, height, pose["eye"], pose["target"], **args)


def from_cam_kw(kind, cam_kw, **kw):
    """`make` from a random scene's camera keywords (random_scenes.random_scene_parts)."""
    args = dict(cam_kw)
    args.update(kw)
    return make(kind, **args)


# ---- depth buffers ----------------------------------------------------------------------------------------------------------------------------------

def _segments(cam):
    """The pixel centres' near ends (view space, (H, W, 3)), the unit directions towards their far ends and the segments' lengths (inf: no far end)."""
    xs = (np.arange(cam.width) + 0.5) / cam.width * 2.0 - 1.0
    ys = (np.arange(cam.height) + 0.5) / cam.height * 2.0 - 1.0
    gx, gy = np.meshgrid(xs, ys)
    one, zero = np.ones_like(gx), np.zeros_like(gx)
    hn = np.stack([gx, gy, one, one], axis=-1) @ cam.inv_projection.T        # depth 1: the near plane
    hf = np.stack([gx, gy, zero, one], axis=-1) @ cam.inv_projection.T       # depth 0: the far plane
    wn, wf = hn[..., 3:4], hf[..., 3:4]
    assert np.all(wn != 0.0)
    pn = hn[..., :3] / wn
    # far - near = (F wn - N wf) / (wn wf); at wf == 0 the far end is the direction F, approached with w of wn's sign
    d = (hf[..., :3] * wn - hn[..., :3] * wf) * np.sign(wn) * np.sign(np.where(wf != 0.0, wf, wn))
    dist = np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        length = np.where(wf[..., 0] != 0.0, dist[..., 0] / np.abs(wn * wf)[..., 0], np.inf)
    return pn, d / dist, length


def depth_ground_sphere(cam, center_world=(0.0, 0.0, 0.0), radius=S.DEMO_PLANET_RADIUS):
    """The depth buffer of an opaque sphere, written from the projection itself: the first hit of each pixel's near-far segment in view space, pushed
    through `cam.projection`; the far plane (0) where the segment misses.  Right for every kind of this module (scene.depth_ground_sphere shoots one
    direction per pixel from the view-space origin, which is not where an orthographic pixel's segment starts)."""
    assert cam.reverse_z
    pn, d, length = _segments(cam)
    c = (cam.view @ np.array([*center_world, 1.0]))[:3]
    oc = pn - c
    b = np.sum(oc * d, axis=-1)
    h = b * b - (np.sum(oc * oc, axis=-1) - radius * radius)
    hit = h >= 0.0
    t = -b - np.sqrt(np.where(hit, h, 0.0))
    hit &= (t > 0.0) & (t < length)
    p = pn + np.where(hit, t, 0.0)[..., None] * d
    clip = np.concatenate([p, np.ones_like(p[..., :1])], axis=-1) @ cam.projection.T
    return np.where(hit, clip[..., 2] / clip[..., 3], 0.0).astype(np.float32)


def depth_pattern(cam):
    """A smooth synthetic depth buffer with texels in [0.05, 0.95]: under `ortho` neighbouring rays then really differ with depth."""
    ys, xs = np.meshgrid(np.arange(cam.height, dtype=np.float64), np.arange(cam.width, dtype=np.float64), indexing="ij")
    d = 0.5 + 0.45 * np.sin(0.37 + 0.11 * xs + 0.05 * ys) * np.cos(0.23 * ys - 0.04 * xs)
    assert d.min() >= 0.05 and d.max() <= 0.95
    return d.astype(np.float32)


def depth_of(cam, **sphere):
    """The depth buffer a test draws a camera with: the synthetic pattern under `ortho`, the ground sphere otherwise."""
    return depth_pattern(cam) if getattr(cam, "kind", "") == "ortho" else depth_ground_sphere(cam, **sphere)


# ---- the cases of tests/test_projections_gpu.py (tests/test_projections_host.py proves on the CPU that each is worth drawing) ---------------------------

SINGLE_KINDS = ("eye_left", "jitter", "infinite_far", "ortho")
SINGLE_CONFIGS = [("no_clouds_8", "declared"), ("no_clouds_32x8_direct", "declared"), ("clouds_high", "declared"), ("clouds_high", "lod0"),
                  ("clouds_high_rm", "declared"), ("clouds_high_rm", "lod0"), ("v1_clouds", "declared"), ("v1_clouds", "lod0")]
POSE_SIZES = {"P_space": (113, 37), "P_limb": (96, 54)}          # partial 16 x 8 tiles both ways
# Orthographic sizes, chosen on the CPU oracle (the camera's position is the rays' origin, the size only spreads their directions): P_space 150 / 300 /
# 600 shade 0.90 / 0.71 / 0.37 of the pattern-depth frame, P_limb 150 / 300 / 600 shade 0.14 / 0.28 / 0.37
ORTHO_SIZE = {"P_space": 300.0, "P_limb": 600.0}
GEO_SIZE = (353, 201)             # 23 x 26 tiles: the tile-order policies leave launches of fewer than 512 tiles alone
GEO_KINDS = ("eye_left", "eye_right", "jitter", "rolled")


def demo_camera(kind, pose, size=None):
    """The demo-scene camera of a single-draw case."""
    w, h = size or POSE_SIZES[pose]
    return from_pose(kind, w, h, pose, **(dict(ortho_size=ORTHO_SIZE[pose]) if kind == "ortho" else {}))


def depth_factors(kind):
    """u_sphere_depth_factor per kind: with an infinite far plane 0 and 0.35 (1 multiplies the far plane's inf by 0 in the reference's own mix)."""
    return (0.0, 0.35) if kind == "infinite_far" else (0.0,)


# The far mode: the demo planet's box (edge 1.75 (R + H + near) 1.1 = 208.1) seen from (31, 17, 420) -- under `ortho` a picture 420 units high --,
# face-on, corner-on, and straddling the near plane off to the side.
PROXY_SIZE = (96, 54)
PROXY_ORTHO_SIZE = 420.0


def _rot(ax_deg_pairs):
    m = np.eye(4)
    for axis, deg in ax_deg_pairs:
        a, r = np.radians(deg), np.eye(4)
        i, j = {"x": (1, 2), "y": (2, 0)}[axis]
        r[i, i], r[i, j], r[j, i], r[j, j] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        m = m @ r
    return m


def _shift(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def proxy_box_size(near, radius=S.DEMO_PLANET_RADIUS, height=S.DEMO_ATMOSPHERE_HEIGHT):
    return 1.75 * (radius + height + near) * 1.1


def proxy_poses(kind):
    """(name, camera, model matrix) of the launch-rectangle cases."""
    w, h = PROXY_SIZE
    kw = dict(ortho_size=PROXY_ORTHO_SIZE) if kind == "ortho" else {}
    yield "face_on", make(kind, w, h, (0.0, 0.0, 600.0), (0.0, 0.0, 0.0), **kw), np.eye(4)
    yield "corner_on", make(kind, w, h, (3.0, -2.0, 450.0), (3.0, -2.0, 0.0), **kw), _rot([("x", 35.26438968), ("y", 45.0)])
    yield "near_straddle", make(kind, w, h, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), near=20.0, **kw), _shift(150.0, 40.0, -60.0) @ _rot([("y", 30.0)])


def proxy_draw_camera(kind):
    """The camera of the GPU proxy draws (the demo planet at the origin, its box unrotated)."""
    w, h = PROXY_SIZE
    return make(kind, w, h, (31.0, 17.0, 420.0), (0.0, 0.0, 0.0), **(dict(ortho_size=PROXY_ORTHO_SIZE) if kind == "ortho" else {}))


# The planets of one frame (tests/test_planets_gpu.py's scene under the left eye's frustum): P and Q apart on screen, M in front of P.
PLANETS_SIZE = (480, 270)
PLANETS = {"P": ((-150.0, 24.0, 0.0), 100.0, 8.0), "Q": ((237.0, -35.0, -100.0), 83.0, 12.0), "M": ((-77.0, 30.0, 250.0), 45.0, 5.0)}


PLANETS_ORTHO_SIZE = 1100.0        # 4.07 units a pixel: P's box is 51 pixels wide


def planets_camera(kind="eye_left"):
    return make(kind, *PLANETS_SIZE, (0.0, 0.0, 700.0), (0.0, 0.0, 0.0), far=5000.0, **(dict(ortho_size=PLANETS_ORTHO_SIZE) if kind == "ortho" else {}))


def planets_depth(cam):
    return np.maximum.reduce([depth_ground_sphere(cam, pos, r) for pos, r, _ in PLANETS.values()])       # reverse-Z: the nearest wins
