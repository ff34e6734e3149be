"""The random scenes of the fuzz (tests/test_gpu_parity.py::test_parity_random_scenes), as a module that needs no GPU: the scene of a seed, its
textures, its shader variant and the node that draws it -- and, for tests/test_draw_paths_random_gpu.py, the same scenes placed somewhere else in the
world and seen from far away, with a list of seeds (SEEDS) whose frames tests/test_random_scenes_host.py proves worth drawing on the CPU oracle.

Every random draw of a seed's scene comes from np.random.default_rng(1000 + seed) in the order `random_scene` makes them; the placement and the far
cameras of a seed come from ONE other generator, np.random.default_rng(5000 + seed), in the order `_placement_draws` makes them: the far camera's
direction, the second far camera's direction, then (used by odd seeds only) the model matrix's angle and its translation."""
import functools
import os

import numpy as np

from common import demo_params
from godot_atmosphere_shader_amd import scene as S

SIZES = [(96, 54), (80, 45), (64, 64), (113, 37)]


def random_scene_parts(rng, k):
    """Random planet / camera / shader parameters: exercises the code paths the demo scene does not.  (params, camera keywords with eye and target, sun)."""
    R = float(rng.choice([1.0, 10.0, 100.0, 637.1]))
    H = R * float(rng.uniform(0.03, 0.25))
    dens_target = float(rng.uniform(0.3, 3.0))  # vertical optical depth rho^2 * H / 4 of order one
    params = demo_params(
        u_planet_radius=R, u_atmosphere_height=H, u_density=float(np.sqrt(4.0 * dens_target / H)),
        u_scattering_strength=float(rng.uniform(0.3, 3.0)),
        u_scattering_wavelengths=(float(rng.uniform(600, 750)), float(rng.uniform(500, 580)), float(rng.uniform(400, 480))),
        u_atmosphere_modulate=tuple(rng.uniform(0.5, 1.0, 3).tolist()),
        u_atmosphere_ambient_color=tuple(rng.uniform(0.0, 0.01, 3).tolist()),
        u_sphere_depth_factor=float(rng.choice([0.0, 0.35, 1.0])),
        u_cloud_density_scale=float(rng.uniform(0.5, 60.0) / H * 8.0),
        u_cloud_bottom=float(rng.uniform(0.05, 0.3)), u_cloud_top=float(rng.uniform(0.4, 0.9)),
        u_cloud_blend=float(rng.uniform(0.0, 1.0)), u_cloud_shape_invert=float(rng.choice([0.0, 1.0])),
        u_cloud_coverage_bias=float(rng.uniform(-0.2, 0.2)), u_cloud_shape_factor=float(rng.uniform(0.0, 1.0)),
        u_cloud_shape_scale=float(rng.uniform(0.05, 0.4) * 100.0 / R),
    )
    a = float(rng.uniform(0, 2 * np.pi))
    params["u_cloud_coverage_rotation"] = (np.cos(a), np.sin(a), -np.sin(a), np.cos(a))
    # camera: somewhere between just above the ground and 3 radii out, looking roughly at the limb or the planet
    alt = float(rng.choice([0.02 * H, 0.4 * H, 0.9 * H, 1.5 * H, 0.6 * R, 2.0 * R]))
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    eye = d * (R + alt)
    tangent = np.cross(d, rng.normal(size=3))
    tangent /= np.linalg.norm(tangent)
    target = eye + tangent * R * 0.5 - d * R * float(rng.uniform(-0.1, 0.6))
    sun = rng.normal(size=3)
    sun = sun / np.linalg.norm(sun) * R * 50.0
    w, h = SIZES[k % 4]
    cam_kw = dict(width=w, height=h, eye=eye, target=target, fovy_deg=float(rng.uniform(40, 90)), near=0.05 * H, far=20.0 * R)
    return params, cam_kw, tuple(sun.tolist())


def random_scene(rng, k):
    """(params, camera, sun) of `random_scene_parts`."""
    params, cam_kw, sun = random_scene_parts(rng, k)
    return params, S.Camera(**cam_kw), sun


# (shader, the oracle's step-count config, PlanetAtmosphere keywords) by seed % 6
VARIANTS = [
    ("planet_atmosphere_no_clouds", dict(view_steps=16), dict(view_steps=16)),
    ("planet_atmosphere_no_clouds", dict(view_steps=64, light_steps=5), dict(view_steps=64, light_mode="direct", light_steps=5)),
    ("planet_atmosphere_clouds", dict(view_steps=8, cloud_steps=8), dict(cloud_steps=8)),
    ("planet_atmosphere_clouds_high_rm", dict(view_steps=8, cloud_steps=24, cloud_light_rm=1), dict(cloud_steps=24)),
    ("planet_atmosphere_clouds_high", dict(view_steps=12, cloud_steps=64, light_steps=8), dict(view_steps=12, light_mode="direct", light_steps=8)),
    ("planet_atmosphere_clouds_high_rm", dict(view_steps=8, cloud_steps=64, cloud_light_rm=1, light_steps=3), dict(light_mode="direct", light_steps=3)),
]
# the same six for the batches, the proxy draws and the depth sources, which refuse more than 32 view steps: the second one with 32 instead of 64
VARIANTS_BATCH = list(VARIANTS)
VARIANTS_BATCH[1] = ("planet_atmosphere_no_clouds", dict(view_steps=32, light_steps=5), dict(view_steps=32, light_mode="direct", light_steps=5))

variants, variants_batch = VARIANTS, VARIANTS_BATCH


def variant_of(seed, table=VARIANTS):
    return table[seed % len(table)]


def is_cloud_variant(seed):
    return "cloud_steps" in variant_of(seed)[1]


@functools.lru_cache(maxsize=64)
def _textures(seed):
    shape_n = [64, 32, 24, 48][seed % 4]
    cube_n = [256, 64, 17, 128][seed % 4]
    return dict(blue_noise=S.make_blue_noise(seed + 1), shape=S.make_shape_texture(shape_n, seed=seed, cells=4),
                cubemap=None if seed % 5 == 4 else S.make_coverage_cubemap(cube_n, seed=seed))


def textures(seed):
    """The seed's textures: 24 and 48 are shape volumes that are no power of two, 17 a cubemap face that is none; every fifth seed has no cubemap.
    (Made once per seed; the arrays are shared and read only.)"""
    return dict(_textures(seed))


def samplers(seed, tex):
    """The `cubemap_lod` settings a seed runs under: a cloud scene with a cubemap under the library's default (as declared: linear-mipmap, implicit
    LOD; the oracle gets the chain and cube_lod=1) and, stated, level 0 only; every other scene once."""
    return (None, False) if is_cloud_variant(seed) and tex["cubemap"] is not None else (None,)


def near_depth(seed, cam, radius, center_world=(0.0, 0.0, 0.0)):
    return S.depth_ground_sphere(cam, center_world=center_world, radius=radius) if seed % 3 else S.depth_far(cam)


def make_node(params, tex, sun, cam, shader, kw, lod, model=None, precise_atmosphere=False):
    """The node of test_parity_random_scenes: the scene's parameters as the inspector holds them, `_process` for `cam`, the textures.  `model`: the
    node's global_transform (default: identity, untouched)."""
    from godot_atmosphere_shader_amd import PlanetAtmosphere, load_shader

    node = PlanetAtmosphere(blue_noise=tex["blue_noise"], precise_atmosphere=precise_atmosphere, cubemap_lod=lod, **kw)
    node.custom_shader = load_shader(shader)
    node.planet_radius, node.atmosphere_height, node.sun_path = params["u_planet_radius"], params["u_atmosphere_height"], sun
    for k, v in params.items():
        if k not in ("u_planet_radius", "u_atmosphere_height", "u_cloud_coverage_rotation", "u_world_to_model_matrix"):
            node.set(f"shader_params/{k}", v)
    if model is not None:
        node.global_transform = np.asarray(model, dtype=np.float64)
    node._process(0.0, cam, time=0.0)
    node.set_shader_parameter("u_cloud_coverage_rotation", np.asarray(params["u_cloud_coverage_rotation"], dtype=np.float32))
    node.set_shader_parameter("u_cloud_shape_texture", tex["shape"])
    if tex["cubemap"] is not None:
        node.set_shader_parameter("u_cloud_coverage_cubemap", tex["cubemap"])
    return node


def oracle_render(oracle, params, tex, ocfg, declared, lut, cam, sun, depth, model=None, nthreads=8):
    """The oracle's frame of a scene: linear colours (the node took them as the inspector holds them, sRGB, and converted them on upload:
    `source_color`), the cubemap's mip chain and cube_lod=1 under the declared sampler, the planet's model matrix in the frame and its inverse in the
    parameters.  (rgba, hits)."""
    from godot_atmosphere_shader_amd.planet_atmosphere import make_frame

    model = np.eye(4) if model is None else np.asarray(model, dtype=np.float64)
    oparams = dict(params, u_atmosphere_modulate=tuple(S.srgb_to_linear(params["u_atmosphere_modulate"]).tolist()),
                   u_atmosphere_ambient_color=tuple(S.srgb_to_linear(params["u_atmosphere_ambient_color"]).tolist()))
    if not np.array_equal(model, np.eye(4)):
        oparams["u_world_to_model_matrix"] = S.col_major(np.linalg.inv(model))
    otex = dict(tex, optical_depth=lut)
    if declared:
        otex["cubemap"] = oracle.cubemap_mip_chain(tex["cubemap"])
    return oracle.render(oparams, otex, dict(ocfg, cube_lod=1) if declared else ocfg, make_frame(cam, model, sun), depth, nthreads=nthreads)


# ---- the fuzz's seeds --------------------------------------------------------------------------------------------------------------------------------

# Seeds 0-11, then (round 6) the four scenes of the 1 212-scene soak that exceeded 1e-4 in rounds 3-5 -- 442 / 658 / 890 carried a 24^3 shape volume whose
# filter coordinates the kernels had fused (fma(p, n, -0.5): the same bits as the reference's rounded product only for power-of-two n), 1040 one ulp of
# the declared sampler's lambda; profiles/round6/fuzz_four.txt -- and 20 more drawn from the 1 212 (np.random.default_rng(6).choice(arange(12, 1212), 20)).
# ATMO_FUZZ_EXTRA=n: seeds 12 .. 12 + n - 1 as well, on demand (the soak: n = 1200); ATMO_FUZZ_FIRST=k: k .. k + n - 1 instead (fresh scenes).
FUZZ_ALWAYS = list(range(12))
FUZZ_SEEDS = FUZZ_ALWAYS + [442, 658, 890, 1040] + [159, 234, 406, 418, 449, 456, 521, 537, 546, 553, 624, 648, 766, 792, 816, 817, 826, 915, 1133, 1187]
# Seeds 1, 2, 4 and 6 look past their planets: their frames shade nothing, and the comparison is black with black.  Each has a replacement here, chosen by
# `fuzz_replacement` (tests/test_random_scenes_host.py runs the rule again and prints every seed's shaded share): same variant, same textures sizes, same
# frame size (s' = s mod 60), a frame that shades at least 10 % of its pixels.
FUZZ_REPLACEMENTS = {1: 61, 2: 62, 4: 64, 6: 66}
FUZZ_SEEDS += list(FUZZ_REPLACEMENTS.values())
_FUZZ_FIRST = int(os.environ.get("ATMO_FUZZ_FIRST", "12"))
FUZZ_SEEDS += [k for k in range(_FUZZ_FIRST, _FUZZ_FIRST + int(os.environ.get("ATMO_FUZZ_EXTRA", "0"))) if k not in FUZZ_SEEDS]


# ---- the draw paths' seeds, placements and far cameras --------------------------------------------------------------------------------------------------

# 0..59 without the frames that shade nothing (1, 2, 4, 6, 14, 21, 29, 32, 33) or under 6 % (20, 25, 51), and without 30, whose far camera leaves 33 of
# 3 031 covered pixels within rounding distance of the proxy box's silhouette (tests/proxy_geometry.py: unstable): 47 seeds
DROPPED = (1, 2, 4, 6, 14, 20, 21, 25, 29, 30, 32, 33, 51)
SEEDS = [s for s in range(60) if s not in DROPPED]
FAR_FOVY_DEG = 40.0
# u_sphere_depth_factor = 1 reads nothing from the depth buffer; the depth-source family draws such a seed a second time with this factor
DEPTH_SOURCE_FACTOR = 0.35


def scene_of(seed):
    """(params, camera keywords, sun, textures) of a seed, as test_parity_random_scenes draws them."""
    params, cam_kw, sun = random_scene_parts(np.random.default_rng(1000 + seed), seed)
    return params, cam_kw, sun, textures(seed)


def _placement_draws(seed):
    rng = np.random.default_rng(5000 + seed)
    dirs = []
    for _ in range(2):
        d = rng.normal(size=3)
        dirs.append(d / np.linalg.norm(d))
    angle = float(rng.uniform(0, 2 * np.pi))
    shift = rng.normal(size=3)
    return dirs, angle, shift


def model_matrix(seed, radius):
    """Even seeds: identity.  Odd seeds: a rotation about y by a uniform angle plus a translation normal(3) * 0.5 R."""
    if seed % 2 == 0:
        return np.eye(4)
    _, a, shift = _placement_draws(seed)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    m[:3, 3] = shift * 0.5 * radius
    return m


def _point(m, p):
    return (m @ np.array([p[0], p[1], p[2], 1.0]))[:3]


def placed(seed):
    """The seed's scene with the planet moved: (params, textures, model matrix M, near camera, sun, near depth).  The near camera's eye and target and
    the sun are transformed by M, the node gets global_transform = M, the ground sphere's depth its centre."""
    params, cam_kw, sun, tex = scene_of(seed)
    R = params["u_planet_radius"]
    M = model_matrix(seed, R)
    cam = S.Camera(**dict(cam_kw, eye=_point(M, cam_kw["eye"]), target=_point(M, cam_kw["target"])))
    centre = tuple(M[:3, 3].tolist())
    return params, tex, M, cam, tuple(_point(M, sun).tolist()), near_depth(seed, cam, R, centre)


def far_camera(seed, which=0):
    """(camera, depth) from 4 (R + H) away, looking at the planet's centre: the near camera's frame size, fovy 40 degrees, the ground sphere in the depth
    buffer.  which=1: the second direction of the seed's generator."""
    params, cam_kw, _, _ = scene_of(seed)
    R, H = params["u_planet_radius"], params["u_atmosphere_height"]
    centre = model_matrix(seed, R)[:3, 3]
    d = _placement_draws(seed)[0][which]
    cam = S.Camera(cam_kw["width"], cam_kw["height"], eye=centre + d * 4.0 * (R + H), target=centre, fovy_deg=FAR_FOVY_DEG, near=0.05 * H, far=20.0 * R)
    return cam, S.depth_ground_sphere(cam, center_world=tuple(centre.tolist()), radius=R)


def proxy_box(params, cam):
    """The far mode's box edge, PlanetAtmosphere.proxy_box_size: 1.75 (R + H + near) 1.1."""
    return 1.75 * (params["u_planet_radius"] + params["u_atmosphere_height"] + cam.near) * 1.1


def partial_rect(cam):
    """Rn: an odd-origin partial rect."""
    return (3, 5, cam.width - 2, cam.height - 1)


def fuzz_replacement(seed, listed, shaded_share):
    """The replacement of an always-run seed whose frame is empty: the smallest s' >= 12 with s' = seed (mod 60) that is not in `listed` and whose
    oracle frame shades at least 10 % (`shaded_share(s')`)."""
    s = seed % 60
    while True:
        if s >= 12 and s not in listed and shaded_share(s) >= 0.10:
            return s
        s += 60
