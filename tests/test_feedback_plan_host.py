"""The tile-order feedback's policy on known inputs, without a GPU: atmo_debug_feedback_plan is csrc/atmo_feedback_plan.h's feedback_plan, the function
atmo_render and atmo_render_views decide with -- which order a draw uses, whether it records tile costs, where the sort runs, how far the cost map is
dilated.  The answers below were worked out from the rules (the thresholds FB_STILL_PX 0.5, FB_INSTREAM_PX 3, FB_INSTREAM_LONG_PX 8, FB_MAX_REACH_SIDE_PX 48,
FB_MAX_REACH_PX 160), with the default knobs unless a case says otherwise."""
import ctypes as C

import pytest

from godot_atmosphere_shader_amd import _native as N

KF_CLOUDS, KF_CLOUD_LIGHT_RM, KF_LIGHT_DIRECT, KF_PRECISE = 1, 2, 4, 16
RM = KF_CLOUDS | KF_CLOUD_LIGHT_RM
NONE, SIDE, INSTREAM = 0, 1, 2   # AtmoFeedbackPlanOut.order
NEVER = 0xFFFFFFFF               # is_last_n: no in-stream sort yet


def plan(**kw):
    """feedback_plan of the default knobs (fb_period 8, moving_period 2, reach scale 1, instream 1, axis windows on), tile_h 8, a fresh state -- with `kw` over it."""
    sil = kw.pop("sil", (0.0, 0.0))
    a = dict(fb_period=8, moving_period=2, reach_scale=1.0, instream=1, axis_windows=1, cloud_steps=32, flags=KF_CLOUDS, tile_h=8, batch=0, n=0, last_record=0,
             pending=0, active=-1, order_born=0, order_reach_px=0.0, is_last_n=NEVER, motion_px=0.0)
    a.update(kw)
    i, o = N.AtmoFeedbackPlanIn(**a), N.AtmoFeedbackPlanOut()
    i.sil_px[0], i.sil_px[1] = sil
    assert N.load().atmo_debug_feedback_plan(C.byref(i), C.byref(o)) == N.ATMO_OK
    assert o.record == (o.sort_side or o.sort_instream) and not (o.sort_side and o.sort_instream)   # a recording draw is followed by exactly one sort
    return o


def test_the_entry_point_is_a_debug_symbol_and_checks_its_arguments():
    assert "atmo_debug_feedback_plan" in N.DEBUG_SYMBOLS and "atmo_debug_feedback_plan" not in N.CORE_SYMBOLS
    i, o = N.AtmoFeedbackPlanIn(), N.AtmoFeedbackPlanOut()
    assert N.load().atmo_debug_feedback_plan(None, C.byref(o)) == N.ATMO_E_ARG
    assert N.load().atmo_debug_feedback_plan(C.byref(i), None) == N.ATMO_E_ARG
    assert b"atmo_debug_feedback_plan" in N.load().atmo_last_error_string(None)
    assert C.sizeof(N.AtmoFeedbackPlanIn) == 19 * 4 and C.sizeof(N.AtmoFeedbackPlanOut) == 8 * 4   # flat, 32-bit fields only (include/atmo_debug.h)


@pytest.mark.parametrize("batch", [0, 1], ids=["draw", "batch"])
def test_still_camera(batch):
    """The first two draws of a key are not measured, the next four record back to back, then every fb_period-th; never while a sort is pending.  A still
    batch follows the rule of the single draw."""
    for n in (0, 1):
        o = plan(n=n, batch=batch)
        assert (o.order, o.record, o.invalidate_active) == (NONE, 0, 0)
    o = plan(n=2, batch=batch)
    assert (o.order, o.record, o.sort_side, o.sort_instream, o.dil_rx, o.dil_ry, o.reach_px) == (NONE, 1, 1, 0, 0, 0, 0.0)
    o = plan(n=5, last_record=4, active=0, order_born=3, batch=batch)
    assert (o.order, o.record, o.sort_side, o.invalidate_active) == (SIDE, 1, 1, 0)
    assert plan(n=12, last_record=5, batch=batch).record == 0
    assert plan(n=13, last_record=5, batch=batch).record == 1
    for n in (2, 3, 5, 13, 100):
        o = plan(n=n, last_record=0, pending=1, active=1, batch=batch)
        assert (o.order, o.record, o.sort_side, o.sort_instream) == (SIDE, 0, 0, 0), n
    # below FB_STILL_PX the camera counts as still: the period stays fb_period, nothing is dilated
    o = plan(n=13, last_record=6, motion_px=0.5, batch=batch)
    assert (o.record, o.dil_rx, o.dil_ry) == (0, 0, 0)


def test_moving_camera_side_stream():
    # clouds, 1 px per frame: recording period 2, an order has to cover motion x (period + 4) = 6 px -> one tile each way
    o = plan(n=10, last_record=8, motion_px=1.0)
    assert (o.record, o.sort_side, o.sort_instream, o.reach_px, o.dil_rx, o.dil_ry) == (1, 1, 0, 6.0, 1, 1)
    assert plan(n=10, last_record=9, motion_px=1.0).record == 0
    assert plan(n=10, last_record=8, motion_px=1.0, tile_h=4).dil_ry == 2     # tiles half as high: twice as many rows for the same reach
    # 9 px per frame: reach 54 > 48, nothing measured now says anything about the frame it would order
    o = plan(n=12, last_record=2, motion_px=9.0, active=1, order_born=10, order_reach_px=10.0)
    assert (o.order, o.record, o.invalidate_active) == (SIDE, 0, 0)          # moved 9 x 2 = 18 <= 10 + 8: the order in use stays conservative
    o = plan(n=12, last_record=2, motion_px=10.0, active=1, order_born=10, order_reach_px=10.0)
    assert (o.order, o.record, o.invalidate_active) == (NONE, 0, 0)          # 20 > 18: not used (and not thrown away: the camera may stop)
    # short frames (neither clouds nor direct light): recording every other frame costs more than the order brings
    assert plan(n=10, last_record=2, motion_px=1.0, flags=0).record == 0
    assert plan(n=10, last_record=2, motion_px=1.0, flags=KF_LIGHT_DIRECT).record == 1
    assert plan(n=10, last_record=2, motion_px=0.4, flags=0).record == 1     # ... while it moves only


def test_in_stream_sort_of_the_raymarched_light_family():
    o = plan(flags=RM, n=10, last_record=8, motion_px=2.9, sil=(2.0, 0.0))
    assert (o.record, o.sort_side, o.sort_instream, o.invalidate_active) == (1, 1, 0, 0)
    # from 3 px per frame: every draw records and is followed by the sort on its own stream; the window is the silhouette's, one tile at least
    for n, last, is_last, order in ((10, 9, 9, INSTREAM), (10, 9, 8, NONE), (10, 9, NEVER, NONE), (1, 0, 0, INSTREAM)):
        o = plan(flags=RM, n=n, last_record=last, is_last_n=is_last, motion_px=3.0, sil=(2.0, 0.0), active=0, order_born=8, order_reach_px=100.0)
        assert (o.order, o.record, o.sort_side, o.sort_instream, o.invalidate_active) == (order, 1, 0, 1, 1), (n, is_last)
        assert (o.reach_px, o.dil_rx, o.dil_ry) == (4.0, 1, 1)               # ceil(4 / 16) = 1; ceil(0 / 8) = 0, lifted to 1
    o = plan(flags=RM, n=10, motion_px=3.0, sil=(79.0, 0.0))
    assert (o.sort_instream, o.reach_px, o.dil_rx, o.dil_ry) == (1, 158.0, 10, 1)    # ceil(158 / 16) = 10, the upper clamp's value
    o = plan(flags=RM, n=10, motion_px=3.0, sil=(79.0, 100.0))
    assert (o.sort_instream, o.sort_side) == (0, 1)                          # reach 200 > 160 (the faster axis counts)
    o = plan(flags=RM, n=10, motion_px=3.0, sil=(79.0, 60.0))
    assert (o.sort_instream, o.reach_px, o.dil_rx, o.dil_ry) == (1, 158.0, 10, 10)   # ceil(158 / 16) = 10; ceil(120 / 8) = 15, cut to 10
    o = plan(flags=RM, n=10, last_record=2, motion_px=3.0, sil=(81.0, 0.0))
    assert (o.sort_instream, o.sort_side, o.invalidate_active, o.reach_px) == (0, 1, 0, 18.0)   # reach 162 > 160: the side stream's turn
    # a side-stream sort in flight keeps the draw out of the in-stream mode (and of recording)
    o = plan(flags=RM, n=10, motion_px=3.0, sil=(2.0, 0.0), pending=1)
    assert (o.record, o.sort_instream, o.sort_side) == (0, 0, 0)
    assert plan(flags=RM, n=10, motion_px=30.0, sil=(2.0, 0.0), instream=0).sort_instream == 0
    # axis windows off: the isotropic window of the picture's motion, two frames of it, unclamped
    o = plan(flags=RM, n=10, motion_px=20.0, sil=(2.0, 0.0), axis_windows=0)
    assert (o.sort_instream, o.reach_px, o.dil_rx, o.dil_ry) == (1, 40.0, 3, 5)
    assert plan(flags=RM, n=10, motion_px=20.0, sil=(2.0, 0.0), axis_windows=0, tile_h=4).dil_ry == 10
    o = plan(flags=RM, n=10, motion_px=70.0, sil=(2.0, 0.0), axis_windows=0)
    assert (o.sort_instream, o.dil_rx, o.dil_ry) == (1, 9, 18)
    assert plan(flags=RM, n=10, motion_px=81.0, sil=(2.0, 0.0), axis_windows=0).sort_instream == 0   # 162 > 160
    assert plan(flags=RM, n=10, motion_px=3.0, sil=(2.0, 0.0), reach_scale=41.0).sort_instream == 0  # the scale multiplies the reach: 164


def test_in_stream_sort_of_the_other_families():
    long_clouds = dict(flags=KF_CLOUDS | KF_PRECISE, cloud_steps=64, n=10, sil=(2.0, 0.0))
    assert plan(motion_px=8.0, **long_clouds).sort_instream == 1
    assert plan(motion_px=7.9, **long_clouds).sort_instream == 0
    assert plan(motion_px=30.0, axis_windows=0, **long_clouds).sort_instream == 0         # this family came with the per-axis windows
    assert plan(motion_px=30.0, **dict(long_clouds, cloud_steps=63)).sort_instream == 0
    assert plan(motion_px=30.0, **dict(long_clouds, flags=KF_CLOUDS)).sort_instream == 0
    # instream = 2 (an A/B knob): every cloud or direct-light family, from 8 px
    direct = dict(flags=KF_LIGHT_DIRECT, n=10, sil=(2.0, 0.0))
    assert plan(motion_px=8.0, instream=2, **direct).sort_instream == 1
    assert plan(motion_px=7.9, instream=2, **direct).sort_instream == 0
    assert plan(motion_px=30.0, instream=1, **direct).sort_instream == 0
    assert plan(motion_px=30.0, instream=2, **dict(direct, flags=0)).sort_instream == 0
    assert plan(motion_px=3.0, instream=2, flags=RM, n=10, sil=(2.0, 0.0)).sort_instream == 1   # the raymarched family keeps its 3 px


def test_batch_form():
    """While any view moves the batch is neither ordered nor recorded, whatever the family; no in-stream sort, no dilation."""
    for flags in (KF_CLOUDS, RM, KF_LIGHT_DIRECT):
        for motion in (0.51, 3.0, 30.0):
            o = plan(batch=1, flags=flags, n=13, last_record=2, active=1, order_born=10, order_reach_px=100.0, motion_px=motion, sil=(2.0, 0.0))
            assert (o.order, o.record, o.sort_side, o.sort_instream, o.dil_rx, o.dil_ry, o.invalidate_active) == (NONE, 0, 0, 0, 0, 0, 1), (flags, motion)
    # still, however long ago its order was sorted: used
    o = plan(batch=1, flags=RM, n=1000, last_record=999, active=1, order_born=0, order_reach_px=0.0, motion_px=0.5)
    assert (o.order, o.record, o.invalidate_active) == (SIDE, 0, 0)
