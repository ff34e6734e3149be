"""The frames and light-march inputs of tests/golden/direct_diet: one definition for the script that recorded them from the parent build
(make_direct_diet_golden.py) and for the tests that draw them again (tests/test_direct_diet_gpu.py, tests/test_direct_diet_fold.py).

Frames: no_clouds_32x8_direct at 67 x 35 -- partial tiles in both directions, the silhouette inside the frame at P_space -- from three demo poses and one
pose inside the shell off the axes; P_ground and P_shell have rc.miss_k <= 0, which switches the sure-miss test off."""
import numpy as np

W, H = 67, 35
POSES = {
    "P_space": "P_space",
    "P_limb": "P_limb",
    "P_ground": "P_ground",
    "P_shell": dict(eye=(20.0, 103.0, 10.0), target=(60.0, 60.0, 130.0)),   # 105.4 from the centre: inside the shell (108), above the ground
}
SENTINEL = 0.25   # what a target_cleared draw finds in the pixels it must leave alone
SMALL_PLANET = dict(u_planet_radius=2.0 ** -45, u_atmosphere_height=2.0 ** -49)   # the light march's squared step is subnormal here (see light_inputs)


def frame_cases():
    """[(file stem, draw)]: draw = dict(pose=..., cleared=bool) plus light_steps=9 | target="rgba8" | views=(pose, pose)."""
    cases = []
    for pose in POSES:
        cases.append((f"frame_{pose}_store", dict(pose=pose, cleared=False)))
        cases.append((f"frame_{pose}_cleared", dict(pose=pose, cleared=True)))
    cases.append(("frame_P_space_9steps", dict(pose="P_space", cleared=False, light_steps=9)))
    cases.append(("frame_P_limb_rgba8", dict(pose="P_limb", cleared=False, target="rgba8")))
    cases.append(("frame_views_space_limb", dict(views=("P_space", "P_limb"), cleared=False)))
    return cases


def _nudge(x, k):
    """x moved by k units in the last place (float32)."""
    return (np.float32(x).view(np.int32) + np.int32(k)).view(np.float32)


def light_inputs(radius=100.0, height=8.0, seed=20240607):
    """(pos, dir), 4096 x 3 float32 each: sample positions relative to the planet centre and sun directions for atmo_debug_marched_optical_depth on a
    planet of that radius and height.  The probe computes r2 = |pos|^2, bdot = pos . dir, y3 from r, and hh = R_atm^2 - (r2 - bdot^2):
      * 1536 chosen: pos = (x, R_atm + k ulp, 0), dir = (+-1, 0, 0), so that bdot = +-x and hh = R_atm^2 - y^2 up to rounding: k = -8 .. 8 walks hh from
        just above through exactly 0 (k = 0 with an exactly squared x) to just below; x of both signs from 0 and 1e-30 (x^2 underflows) up to half the radius;
        the chord -- ray_len = min(2 sq, sq - bdot) -- shrinks to its smallest non-zero values where sq and bdot nearly cancel (hh = -0.0 cannot arise:
        a difference of equal numbers is +0 under round-to-nearest; the CPU test feeds it in directly);
      * 2560 bulk: positions anywhere in the shell (and a little outside either way), sun directions over the whole sphere."""
    rng = np.random.default_rng(seed)
    R, top = np.float32(radius), np.float32(radius) + np.float32(height)
    xs = [0.0, 1e-30, 1e-20, 2.0 ** -12, 1e-3, 0.25, 1.0, 3.0, 17.5, 0.4 * radius]
    xs = [np.float32(x * (radius / 100.0)) for x in xs]
    pos, sun = [], []
    for x in xs:
        for sx in (1.0, -1.0):
            for sd in (1.0, -1.0):
                for k in range(-8, 9):
                    pos.append((np.float32(sx) * x, _nudge(top, k), 0.0))
                    sun.append((sd, 0.0, 0.0))
    # sq and bdot nearly cancelling: pos = (x, y, 0) with x^2 + y^2 = R_atm^2 and the sun along x, so that sq ~ |x| ~ bdot
    while len(pos) < 1536:
        a = rng.uniform(0.05, 1.5)
        x, y = np.float32(top * np.cos(a)), np.float32(top * np.sin(a))
        pos.append((_nudge(x, int(rng.integers(-3, 4))), _nudge(y, int(rng.integers(-3, 4))), 0.0))
        sun.append((1.0, 0.0, 0.0))
    n = 4096 - len(pos)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = rng.uniform(float(R) * 0.995, float(top) * 1.002, size=(n, 1))
    s = rng.normal(size=(n, 3))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    pos = np.concatenate([np.asarray(pos, dtype=np.float32), (v * r).astype(np.float32)])
    sun = np.concatenate([np.asarray(sun, dtype=np.float32), s.astype(np.float32)])
    assert pos.shape == sun.shape == (4096, 3)
    return np.ascontiguousarray(pos), np.ascontiguousarray(sun)
