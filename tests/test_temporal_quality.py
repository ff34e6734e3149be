"""The quality record of temporal draws (include/atmo_temporal.h), on the CPU oracle at 64 x 40: the numpy statement's output along a 1-degree-per-frame
orbit of 2 s^2 frames and under a still camera after s^2 frames, against the oracle's full-resolution frame of the same pose -- beside the same figure for
reduced.upsample and for pixel repetition of the last low frame.  The figures are printed (profiles/temporal/README.md records them).  Two things are
asserted, neither from the figures themselves: a still camera leaves every pixel a ray marched at its own centre -- what remains against the full frame
is the march's jitter, which the shader reads from the blue-noise texture at the DRAWN pixel's coordinate, the low frame's here (main:169) --, so it is
closer in the mean than the spatial filter, which has 1 / s^2 of the rays; and along the orbit the temporal output is closer in the mean than pixel repetition."""
import numpy as np
import pytest

from common import CONFIGS, demo_frame, demo_params, demo_textures, oracle_inputs
from godot_atmosphere_shader_amd import reduced as R
from godot_atmosphere_shader_amd import scene as S
from godot_atmosphere_shader_amd import temporal as TP
from test_temporal import _moved

W, H = 64, 40


def _premultiplied(img):
    img = img.astype(np.float64)
    return np.concatenate([img[..., :3] * img[..., 3:4], img[..., 3:4]], axis=-1)


def _err(a, full):
    d = np.abs(_premultiplied(a) - _premultiplied(full))
    return d.mean(), d.max()


@pytest.fixture(scope="module")
def draw(oracle32):
    lut = oracle32.bake_optical_depth(S.DEMO_PLANET_RADIUS, S.DEMO_ATMOSPHERE_HEIGHT, S.DEMO_SHADER_PARAMS["u_density"])
    cfg, tex = oracle_inputs(oracle32, CONFIGS["clouds_high"][1], demo_textures(), lut, declared=True)
    return lambda frame, depth: oracle32.render(demo_params(), tex, cfg, frame, depth, nthreads=8)[0]


def _sequence(draw, cams, s, tol=0.1, htol=0.1):
    """The statement's histories along `cams`, reset on the first: (the last history's rgba, the last frame, its depth, its low frame and low depth)."""
    hist = None
    for f, cam in enumerate(cams):
        frame, depth = demo_frame(cam), S.depth_ground_sphere(cam)
        p = TP.phase_of_frame(s, f)
        low_depth = TP.phase_depth(depth, s, p)
        low = draw(TP.phase_frame(frame, s, p), low_depth)
        prev = cams[f - 1] if f else None
        hist = TP.resolve(frame, depth, low_depth, low, s, p, tol, htol, None, hist, TP.prev_clip_from_view(frame, prev) if f else None,
                          S.col_major(prev.inv_projection) if f else None, reset=f == 0)
    return hist[0], frame, depth, low


@pytest.mark.parametrize("s", [2, 4])
def test_the_quality_record(draw, s):
    n = s * s
    orbit = [_moved("plain", (W, H), yaw_deg=float(k))[0] for k in range(2 * n)]
    out, frame, depth, last_low = _sequence(draw, orbit, s)
    full = draw(frame, depth)
    assert 0.1 < np.any(full != 0.0, axis=-1).mean() < 0.99
    low_depth = R.reduce_depth(frame, depth, s)
    up = R.upsample(frame, depth, low_depth, draw(R.low_frame(frame, s), low_depth), s, 0.1)
    nearest = np.repeat(np.repeat(last_low, s, axis=0), s, axis=1)[:H, :W]
    still, sframe, sdepth, _ = _sequence(draw, [orbit[0]] * n, s)
    sfull = draw(sframe, sdepth)
    e_t, e_u, e_n, e_s = _err(out, full), _err(up, full), _err(nearest, full), _err(still, sfull)
    print(f"\ntemporal quality clouds_high {W}x{H} s={s}: orbit of {2 * n} frames mean {e_t[0]:.3e} max {e_t[1]:.3e}; reduced.upsample mean {e_u[0]:.3e} "
          f"max {e_u[1]:.3e}; pixel repetition mean {e_n[0]:.3e} max {e_n[1]:.3e}; still camera after {n} frames mean {e_s[0]:.3e} max {e_s[1]:.3e}")
    assert e_s[0] < e_u[0]
    assert e_t[0] < e_n[0]
