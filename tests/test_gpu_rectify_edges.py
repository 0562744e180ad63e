"""GPU: ecal_rectify_batch_dev (eventcalib_amd/csrc/ecal_rectify.hip) on hand-built keyframes (tests/synth_rectify_scene.py),
bit for bit against oracle/rectify_oracle.cpp: both kernel instantiations (8 and 64 flag words) and the hand-over between
them, windows the entry point does not handle, boards from 1 to 128 circles in both trips of the circle loop, the tangential
and fisheye projection at the border of 640 x 480 and 1280 x 720 sensors, every per-circle gate, the frame verdict's exact
boundaries, segment sizes around the 64-point chunk, and the host-buffer form.

Bar, unless a test says otherwise: validity flags, frame verdicts and rectified circles IDENTICAL to the oracle (NaN == NaN).
All points are integer pixels, so fitCircle's sums are exact in any order; the rest is the same f64 / f32 arithmetic without
contraction.  tests/test_rectify_scene_host.py proves on the CPU that each scene has the property its test here relies on (the
numbers quoted in the comments are asserted there).  The outputs are pre-filled with sentinels: a keyframe neither launch
wrote is caught."""
import numpy as np
import pytest

import synth_rectify_scene as RS
from test_rectify_scene_host import VERDICTS, centre_bar

pytestmark = pytest.mark.gpu

F_SENT, U_SENT = 12345.0, 0xFFFFFFFF
ECAL_ERR_INVALID, ECAL_ERR_RANGE = -1, -6


@pytest.fixture
def ctx():
    import eventcalib_amd
    c = eventcalib_amd.Context(0)
    yield c
    c.close()


def run_dev(ctx, bt, b, cam, fit_circle=False):
    """ecal_rectify_batch_dev on a Batch -> (feat [F,n,3], valid [F,n] int32, info [F,2] int64); no sentinel may survive."""
    import torch
    n = b["n"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # (torch has no uint32 arithmetic; the bits go down as int32)
    xy = dev(bt.xy if bt.n_points else np.zeros((1, 2)))
    kept = dev(bt.kept_labels if bt.n_points else np.zeros(1, np.int32))
    off, cnt = dev(bt.seg_off.view(np.int32)), dev(bt.seg_cnt.view(np.int32))
    info_in, fw = dev(bt.win_info.view(np.int32)), dev(bt.frame_window.view(np.int32))
    pose, lm = dev(bt.pose), dev(b["lm"])
    feat = torch.full((bt.F, n, 3), F_SENT, dtype=torch.float64, device="cuda")
    valid = torch.full((bt.F, n), -1, dtype=torch.int32, device="cuda")
    info = torch.full((bt.F, 2), -1, dtype=torch.int32, device="cuda")
    ctx.rectify_batch_dev(xy.data_ptr(), off.data_ptr(), cnt.data_ptr(), kept.data_ptr(), info_in.data_ptr(), fw.data_ptr(),
                          pose.data_ptr(), bt.F, lm.data_ptr(), RS.rectify_params(b, cam, fit_circle), feat.data_ptr(),
                          valid.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    feat, valid, info = feat.cpu().numpy(), valid.cpu().numpy(), info.cpu().numpy()
    assert not (feat == F_SENT).any() and not (valid.view(np.uint32) == U_SENT).any() and not (info.view(np.uint32) == U_SENT).any(), \
        "a keyframe was not written"
    return feat, valid, info.astype(np.int64)


def check(ctx, s, fit_circle=False, expect=None):
    """Run the scene's batch and compare every keyframe with the oracle (or with all-erased where the entry point does not
    handle the window).  expect: per keyframe None or the validity vector written by hand.  Returns the device results."""
    bt, b, cam = s["batch"], s["b"], s["cam"]
    feat, valid, info = run_dev(ctx, bt, b, cam, fit_circle)
    for f in range(bt.F):
        o_feat, o_valid, o_info = RS.oracle(bt, f, b, cam, fit_circle) if RS.handled(bt, f) else RS.all_erased(b["n"])
        tag = "keyframe %d (window %d, kept clusters %s)" % (f, bt.frame_window[f], bt.nk(f))
        assert np.array_equal(valid[f], o_valid), tag + ": validity"
        assert tuple(info[f]) == tuple(o_info), tag + ": verdict"
        assert np.array_equal(feat[f], o_feat, equal_nan=True), tag + ": circles"
        assert np.isnan(feat[f][valid[f] == 0]).all(), tag + ": an erased circle has no value"
        if expect is not None and expect[f] is not None:
            assert valid[f].tolist() == list(np.atleast_1d(expect[f])), tag + ": the verdict written by hand"
    return feat, valid, info


# ---- a. boards -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x4", "8x16", "13x5", "5x4", "1x1"])
@pytest.mark.parametrize("fit_circle", [False, True])
def test_board(ctx, name, fit_circle):
    """n = 36, 128 (the limit: two full trips), 65 (one lane in the second trip), 20 and 1; symmetric and asymmetric; F = 1."""
    s = RS.scene_baseline(name)
    feat, valid, info = check(ctx, s, fit_circle, expect=[np.ones(s["b"]["n"], int)])
    err = np.hypot(*(feat[0, :, :2] - RS.project(s["b"]["lm"], s["pose"], s["cam"])).T)
    assert err.max() <= centre_bar(name)
    if name == "1x1":
        # one valid circle: every edge has size 1, and the border score rejects on 0 >= size - 1 unless fit_circle skips it
        assert tuple(info[0]) == ((1, 0) if fit_circle else (0, 0))
    else:
        assert tuple(info[0]) == (1, 0)


@pytest.mark.parametrize("name", ["8x16", "13x5"])
def test_second_trip_does_not_inherit_the_first(ctx, name):
    """Circles k and k + 64 of one lane with opposite verdicts, both ways: the flags and the verdict of the first trip must not
    leak into the second."""
    s = RS.scene_trips(name)
    check(ctx, s, expect=s["valid"])


# ---- b. both launches ------------------------------------------------------------------------------------------------
def test_both_launches_and_unhandled_windows(ctx):
    """(kept + , kept -) = (256, 256) | (257, 10), (10, 257), (382, 382), (2048, 2048) | (2049, 10) around an ordinary (72, 72),
    interleaved, through a permuted frame_window with repeats: every keyframe is written by exactly one launch.  Status 4,
    0x104 and 2049 clusters: all erased, info (0, n).  Status 0x100 (tie fallback alone): as status 0."""
    s = RS.scene_launches()
    bt = s["batch"]
    feat, valid, info = check(ctx, s)
    big = [f for f in range(bt.F) if RS.handled(bt, f) and max(bt.nk(f)) > 256]
    assert len(big) >= 5 and all(valid[f].any() for f in big)          # the 64-word instantiation found circles
    for f in (0, 6, 9):                                                 # 2049 clusters, status 0x104, status 4
        assert not valid[f].any() and np.isnan(feat[f]).all() and tuple(info[f]) == (0, 36)
    assert RS.LAUNCH_STATUS[bt.frame_window[2]] == 0x100 and valid[2].all() and tuple(info[2]) == (1, 0)
    assert np.array_equal(feat[2], feat[1])                            # ... the same window content with status 0
    check(ctx, s, fit_circle=True)


# ---- c. projection ---------------------------------------------------------------------------------------------------
def test_tangential_distortion_at_the_border(ctx):
    """The 8x16 board over the whole 640 x 480 sensor: zeroing p1 / p2 moves 8 centres by >= 10 px (worst 22.7), swapping them
    29 (worst 48.3), swapping a2 / a3 up to 14.2 px — each erases circles the oracle keeps, and the oracle's centres are
    themselves within 0.305 px of the independent projection."""
    s = RS.scene_baseline("8x16")
    feat, valid, _ = check(ctx, s)
    assert valid.all()
    err = np.hypot(*(feat[0, :, :2] - RS.project(s["b"]["lm"], s["pose"], s["cam"])).T)
    assert err.max() <= centre_bar("8x16")


def test_fisheye_at_wide_angles(ctx):
    """model 1 on 1280 x 720, field angles up to 62.9 degrees."""
    s = RS.scene_fisheye()
    feat, valid, _ = check(ctx, s)
    assert valid.all()
    err = np.hypot(*(feat[0, :, :2] - RS.project(s["b"]["lm"], s["pose"], s["cam"])).T)
    assert err.max() <= centre_bar("fisheye")


@pytest.mark.parametrize("model", [0, 1])
def test_origin_landmark_on_the_optical_axis(ctx, model):
    """x = y = 0: the centre is (cx, cy) to the bit; model 1 takes its r <= 1e-8 branch."""
    s = RS.scene_axis(RS.CAM_VGA if model == 0 else RS.camera(dist=RS.KB, model=1))
    feat, valid, info = check(ctx, s, fit_circle=True, expect=[[1]])
    assert np.abs(feat[0, 0, :2] - [320.0, 240.0]).max() < 1e-9 and tuple(info[0]) == (1, 0)


def test_z_zero_and_board_behind_the_camera(ctx):
    check(ctx, RS.scene_z0(), expect=[np.ones(20, int)])
    check(ctx, RS.scene_behind(), expect=[np.ones(20, int)])


def test_centres_exactly_on_the_image_bounds(ctx):
    """u == width and v == height: erased; u == 0 and v == 0: kept; half a pixel outside each side: erased; half a pixel inside
    the far corner: kept."""
    check(ctx, RS.scene_bounds(), expect=[RS.BOUNDS_VALID])


# ---- d. per-circle gates ---------------------------------------------------------------------------------------------
def test_member_threshold_third_radius_and_collinear_members(ctx):
    """5 against 4 members in either polarity; a fit within 4.5 px of the third-smallest quadrant radius but not of the second
    (kept) and the other way round (erased); members on one row (singular system): whatever the oracle's arithmetic gives."""
    s = RS.scene_gates()
    check(ctx, s, expect=s["valid"])
    check(ctx, s, fit_circle=True, expect=s["valid"])


def test_quadrant_ties_on_the_axes(ctx):
    """A point exactly on a half-axis belongs to the first quadrant of the reference's cascade that takes it (>= / <=): four
    probes that are inliers THERE and outliers of the neighbour by more than 6 px, each with a cluster that wrecks the fit when
    chosen; the same probes one pixel over (not chosen); one on the centre."""
    s = RS.scene_quadrants()
    check(ctx, s, expect=s["valid"])


# ---- e. frame verdict ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5x4", "9x4", "8x16"])
def test_frame_verdict_boundaries(ctx, name):
    """size - 2 and size - 1 erased on each of the four edges, and erased counts on either side of 20 %: info as written by
    hand in test_rectify_scene_host.VERDICTS, and as the oracle gives it."""
    s = RS.scene_verdict(name)
    for fit in (0, 1):
        _, valid, info = check(ctx, s, fit_circle=bool(fit))
        assert [tuple(r) for r in info.tolist()] == VERDICTS[name][fit]
        for f, mask in enumerate(s["masks"]):
            assert sorted(np.nonzero(valid[f] == 0)[0].tolist()) == sorted(mask)


# ---- f. segment shapes -----------------------------------------------------------------------------------------------
def test_segment_sizes_and_odd_offsets(ctx):
    """Polarities of 0, 1, 63, 64, 65, 128 and 1000 points, back to back from an odd offset; every label -1."""
    s = RS.scene_segments()
    check(ctx, s, fit_circle=True, expect=[[v] for v in (0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0)])


# ---- g. host form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["launches", "segments"])
def test_host_form_equals_device_form(ctx, which):
    s = RS.scene_launches(identity=True) if which == "launches" else RS.scene_segments()
    bt, b, cam = s["batch"], s["b"], s["cam"]
    assert bt.frame_window.tolist() == list(range(bt.F)) and not bt.win_info[:, 3].any()
    feat, valid, info = check(ctx, s)
    h_feat, h_valid, h_info = ctx.rectify_batch(bt.xy, bt.seg_off, bt.seg_cnt, bt.kept_labels, bt.pose, b["lm"],
                                                RS.rectify_params(b, cam))
    assert np.array_equal(h_valid.astype(np.int32), valid) and np.array_equal(h_info.astype(np.int64), info)
    assert np.array_equal(h_feat, feat, equal_nan=True)
    if which == "launches":
        f = RS.LAUNCH_NK.index((2049, 10))          # nk derived from the labels on the host: beyond the limit, all erased
        assert not h_valid[f].any() and tuple(h_info[f]) == (0, 36)


def test_host_form_arguments(ctx):
    from eventcalib_amd.capi import EcalError
    s = RS.scene_axis()
    bt, b, cam = s["batch"], s["b"], s["cam"]
    prm = RS.rectify_params(b, cam)
    lm = np.zeros((129, 3))
    for rows, cols in ((0, 1), (1, 0), (129, 1)):
        prm.rows, prm.cols = rows, cols
        with pytest.raises(EcalError) as e:
            ctx.rectify_batch(bt.xy, bt.seg_off, bt.seg_cnt, bt.kept_labels, bt.pose, lm, prm)
        assert e.value.status == ECAL_ERR_INVALID
    prm = RS.rectify_params(b, cam, fit_circle=True)
    for pol in (0, 1):                               # a segment one point past the array
        cnt = bt.seg_cnt.copy()
        cnt[pol] = bt.n_points - bt.seg_off[pol] + 1
        with pytest.raises(EcalError) as e:
            ctx.rectify_batch(bt.xy, bt.seg_off, cnt, bt.kept_labels, bt.pose, b["lm"], prm)
        assert e.value.status == ECAL_ERR_RANGE
    # no points at all (NULL arrays): runs, everything erased
    zero = np.zeros(2, np.uint32)
    feat, valid, info = ctx.rectify_batch(np.zeros((0, 2)), zero, zero, np.zeros(0, np.int32), bt.pose, b["lm"], prm)
    assert np.isnan(feat).all() and not valid.any() and info.tolist() == [[0, 1]]
    # the same call once more with points: the staging is reused
    feat, valid, info = ctx.rectify_batch(bt.xy, bt.seg_off, bt.seg_cnt, bt.kept_labels, bt.pose, b["lm"], prm)
    assert valid.all() and info.tolist() == [[1, 0]]
    # F == 0
    none = np.zeros(0, np.uint32)
    feat, valid, info = ctx.rectify_batch(np.zeros((0, 2)), none, none, np.zeros(0, np.int32), np.zeros((0, 12)), b["lm"], prm)
    assert feat.shape == (0, 1, 3)
