"""CPU: the hand-built keyframes of tests/synth_rectify_scene.py have the properties tests/test_gpu_rectify_edges.py relies on.
Only the oracle (oracle/rectify_oracle.cpp) and the builder's independent float64 projection are used here: a scene that
would not tell a wrong kernel from a right one fails HERE, so a pass on the GPU means something.

Measured values stand beside the bars; none of them was taken from the kernel."""
import numpy as np
import pytest

import synth_rectify_scene as RS

# Worst distance between the oracle's rectified centre and the independent projection of the landmark, per baseline scene, as
# measured here (the pixel rounding of 48 rim samples and the perspective shift of a circle's centre, not arithmetic).  The bar
# in force is twice the measured value.
CENTRE_ERROR = {"9x4": 0.200, "8x16": 0.305, "13x5": 0.332, "5x4": 0.367, "1x1": 1.065, "fisheye": 0.526}


def centre_bar(name):
    return 2 * CENTRE_ERROR[name]


def _centre_error(s, f=0):
    feat, valid, _ = RS.oracle(s["batch"], f, s["b"], s["cam"])
    uv = RS.project(s["b"]["lm"], s["batch"].pose[f], s["cam"])
    return np.hypot(*(feat[:, :2] - uv).T), valid


# ---- the builder itself ----------------------------------------------------------------------------------------------
def test_projection_known_answers():
    """The independent projection against numbers worked out by hand from the documented model."""
    cam = RS.camera(640, 480, fx=400.0, cx=320, cy=240, dist=(0.1, 0.0, 0.01, 0.02, 0.0))
    pose = RS.pose_rt(np.eye(3), (0.0, 0.0, 2.0))
    # x' = 0.5, y' = 0.25: r^2 = 0.3125, radial = 1.03125; x'' = 0.515625 + 2(0.01)(0.125) + 0.02(0.3125 + 0.5) = 0.534375
    #                                                      y'' = 0.2578125 + 0.01(0.3125 + 0.125) + 2(0.02)(0.125) = 0.2671875
    uv = RS.project([[1.0, 0.5, 0.0]], pose, cam)[0]
    assert abs(uv[0] - (320 + 400 * 0.534375)) < 1e-12 and abs(uv[1] - (240 + 400 * 0.2671875)) < 1e-12
    # fisheye: x' = 1, y' = 0: theta = pi/4, theta_d = theta (1 + 0.1 theta^2)
    fish = RS.camera(640, 480, fx=200.0, cx=320, cy=240, dist=(0.1, 0.0, 0.0, 0.0), model=1)
    uv = RS.project([[2.0, 0.0, 0.0]], pose, fish)[0]
    th = np.pi / 4
    assert abs(uv[0] - (320 + 200 * th * (1 + 0.1 * th * th))) < 1e-12 and uv[1] == 240.0


def test_board_layouts():
    """EventCalibIni.cpp:102-106, and the border sets of CirclesEventFrame.cpp:583-594 on the asymmetric board."""
    a = RS.board_9x4(2.0, 0.5)
    assert a["lm"][5].tolist() == [2 * (2 * 1 + 1), 2.0, 0.0] and a["lm"][8].tolist() == [0.0, 4.0, 0.0]
    assert RS.edges(a) == [[0, 1, 2, 3], [32, 33, 34, 35], [0, 8, 16, 24, 32], [7, 15, 23, 31]]
    s = RS.board_13x5()
    assert s["n"] == 65 and s["lm"][64].tolist() == [4.0, 12.0, 0.0]
    assert RS.edges(RS.board_5x4()) == [[0, 1, 2, 3], [16, 17, 18, 19], [0, 4, 8, 12, 16], [3, 7, 11, 15, 19]]
    assert [len(e) for e in RS.edges(RS.board_8x16())] == [16, 16, 8, 8] and RS.board_8x16()["n"] == 128
    assert 0.2 * RS.board_5x4()["n"] == 4.0


def test_packing_and_labels():
    s = RS.scene_segments()
    bt = s["batch"]
    assert bt.seg_off[0] == 1 and (bt.seg_off % 2 == 1).sum() >= 8                 # odd offsets, segments back to back
    ends = bt.seg_off.astype(np.int64) + bt.seg_cnt
    assert (ends[:-1] == bt.seg_off[1:]).all() and ends[-1] == bt.n_points
    assert [(int(bt.seg_cnt[2 * i]), int(bt.seg_cnt[2 * i + 1])) for i in range(len(RS.SEGMENT_COUNTS))] == \
        [(24 if p is None else p, 24 if n is None else n) for p, n in RS.SEGMENT_COUNTS]
    assert (bt.kept_labels[bt.seg_off[20]:] == -1).all()
    assert RS.spread_labels(36, 257)[-1] == 256 and RS.spread_labels(36, 2049)[-1] == 2048 and len(set(RS.spread_labels(36, 256))) == 36


# ---- baseline scenes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x4", "8x16", "13x5", "5x4", "1x1"])
def test_baseline_boards_all_valid_and_centres_near_the_projection(name):
    s = RS.scene_baseline(name)
    err, valid = _centre_error(s)
    assert valid.all() and RS.oracle(s["batch"], 0, s["b"], s["cam"], fit_circle=True)[2] == (1, 0)
    # fit_circle == 0: accepted, except the 1 x 1 board whose every edge has size 1 (0 >= size - 1 rejects)
    assert RS.oracle(s["batch"], 0, s["b"], s["cam"])[2] == ((0, 0) if name == "1x1" else (1, 0))
    print(name, "worst centre error %.3f px" % err.max())
    assert CENTRE_ERROR[name] * 0.5 <= err.max() <= CENTRE_ERROR[name] * 1.01      # the value written above is the measured one
    uv = RS.project(s["b"]["lm"], s["pose"], s["cam"])
    assert (uv >= 0).all() and (uv[:, 0] < s["cam"]["width"]).all() and (uv[:, 1] < s["cam"]["height"]).all()
    if name == "13x5":
        assert s["cam"]["width"] == 1280 and uv[:, 1].max() > 480                    # coordinates beyond the small sensors'


def test_trip_scenes_have_opposite_verdicts_in_one_lane():
    s = RS.scene_trips("8x16")
    _, valid, _ = RS.oracle(s["batch"], 0, s["b"], s["cam"])
    first, second = valid[:64], valid[64:]
    assert ((first == 0) & (second == 1)).sum() >= 16 and ((first == 1) & (second == 0)).sum() >= 16
    assert ((first == 1) & (second == 1)).sum() >= 16                                # (lanes whose flags must be reset, too)
    uv = RS.project(s["b"]["lm"], s["batch"].pose[0], s["cam"])
    assert (uv[:16, 1] < 0).all() and not valid[:16].any()                           # erased by the pose, not by missing points
    s = RS.scene_trips("13x5")
    for f in range(2):
        _, valid, _ = RS.oracle(s["batch"], f, s["b"], s["cam"])
        assert np.array_equal(valid, s["valid"][f])
    assert s["valid"][0][0] == 0 and s["valid"][0][64] == 1 and s["valid"][1][0] == 1 and s["valid"][1][64] == 0


# ---- both launches ---------------------------------------------------------------------------------------------------
def test_launch_scene_cluster_counts_and_verdicts():
    s = RS.scene_launches()
    bt, b, cam = s["batch"], s["b"], s["cam"]
    assert [bt.nk(f) for f in range(bt.F)] == [RS.LAUNCH_NK[w] for w in RS.LAUNCH_FRAMES]
    assert sorted(set(RS.LAUNCH_FRAMES)) == list(range(bt.S)) and len(RS.LAUNCH_FRAMES) > bt.S       # permuted, with repeats
    assert {(256, 256), (257, 10), (10, 257), (382, 382), (2048, 2048), (2049, 10), (72, 72)} == set(RS.LAUNCH_NK)
    assert bt.F <= 16
    for f in range(bt.F):
        w = bt.frame_window[f]
        pos, neg, kp, kn, _ = bt.oracle_args(f)
        assert (kp.max() + 1, kn.max() + 1) == RS.LAUNCH_NK[w] and len(pos) < 2000 and len(neg) < 2000
        _, valid, info = RS.oracle(bt, f, b, cam)
        if 10 in RS.LAUNCH_NK[w]:
            # circles 26..35 alone have both polarities; circle 35 holds the highest label of the large polarity and label
            # 0 of the small one is circle 26's
            assert valid[26:].all() and not valid[:26].any() and info == (0, 26)
            big, small = (kp, kn) if RS.LAUNCH_NK[w][0] > 10 else (kn, kp)
            assert max(RS.LAUNCH_NK[w]) - 1 == big.max() and (small >= 0).all()
        elif f < bt.S:
            assert valid.all() and info == (1, 0)
        else:
            assert info[0] == 1 and valid.sum() >= 30        # the repeats under the second pose: still accepted
    # What an 8-word launch would do to the (257, 10) window: label 256 of the large polarity lies in word 8 = word 0 of the
    # other polarity, bit 0 = that polarity's label 0.  Circle 35 would so collect circle 26's ring as well — which erases it:
    f = RS.LAUNCH_FRAMES.index(RS.LAUNCH_NK.index((257, 10)))
    pos, neg, kp, kn, pose = bt.oracle_args(f)
    assert kp.max() == 256 and 256 // 32 == 8 and (kn == 0).sum() >= 5 and (kn == 9).sum() >= 5
    aliased = np.where(kn == 0, 9, kn)                      # circle 26's points join circle 35's cluster
    import oracle_lib as O
    _, v_alias, _, _ = O.rectify(pos, neg, kp, aliased, pose, RS.intrinsics(cam), cam["dist"], cam["width"], cam["height"], b["lm"],
                                 b["rows"], b["cols"], True, b["radius"])
    assert RS.oracle(bt, f, b, cam)[1][35] == 1 and v_alias[35] == 0
    # what is handled and what is not
    assert [RS.handled(bt, f) for f in range(bt.F)] == [False, True, True, True, True, True, False, True, True, False, True, True]
    assert RS.LAUNCH_STATUS[9] == 0x100 and RS.handled(bt, 2)
    # flag words beyond the eighth really are in use: the labels of the large frames reach word 63
    assert bt.oracle_args(3)[2].max() // 32 == 63 and bt.oracle_args(4)[2].max() // 32 == 11


# ---- projection ------------------------------------------------------------------------------------------------------
def test_tangential_scene_tells_wrong_coefficients():
    s = RS.scene_baseline("8x16")
    b, cam, bt = s["b"], s["cam"], s["batch"]
    uv = RS.project(b["lm"], s["pose"], cam)
    moved = {"zeroed": (22.7, 8, 26), "swapped": (48.3, 29, 56)}      # measured: worst shift px, circles >= 10 px, erased by the oracle
    for name, dist in RS.tangential_variants(cam).items():
        shift = np.hypot(*(RS.project(b["lm"], s["pose"], RS.with_dist(cam, dist)) - uv).T)
        far = shift >= 10.0                                            # beyond the 6 px centre gate plus the ring's width
        _, valid, info = RS.oracle(bt, 0, b, cam, dist=dist)
        print(name, "worst %.1f px, %d circles >= 10 px, oracle erases %d" % (shift.max(), far.sum(), info[1]))
        assert far.sum() >= 4 and not valid[far].any() and info[0] == 0
        assert abs(shift.max() - moved[name][0]) < 0.05 and (far.sum(), info[1]) == moved[name][1:]
    # a2 / a3 swapped acts on the same terms: p1 (r^2 + 2 y'^2) <-> p1 (r^2 + 2 x'^2); on this board |x'| reaches 0.66 and |y'|
    # 0.25, so the two differ by up to 2 p1 |x'^2 - y'^2| fx
    pose = np.asarray(s["pose"])
    Xc = b["lm"] @ pose[:9].reshape(3, 3).T + pose[9:]
    xn, yn = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    a23 = 2 * np.hypot(cam["dist"][2], cam["dist"][3]) * np.abs(xn * xn - yn * yn) * cam["fx"]
    print("a2 / a3 swapped moves up to %.1f px" % a23.max())           # 14.2 px
    assert (a23 >= 10.0).sum() >= 4


def test_fisheye_scene_reaches_wide_angles():
    s = RS.scene_fisheye()
    err, valid = _centre_error(s)
    ang = np.degrees(RS.field_angle(s["b"]["lm"], s["pose"]))
    print("fisheye: widest field angle %.1f deg, worst centre error %.3f px" % (ang.max(), err.max()))   # 62.9 deg, 0.526 px
    assert valid.all() and ang.max() >= 55.0 and (ang >= 55.0).sum() >= 4
    assert CENTRE_ERROR["fisheye"] * 0.5 <= err.max() <= CENTRE_ERROR["fisheye"] * 1.01
    # the pinhole coefficients' model on the same rings is a different camera altogether
    assert RS.oracle(s["batch"], 0, s["b"], RS.camera(1280, 720, fx=520.0, dist=(0.0,) * 5))[2][1] >= 30


def test_axis_circle_projects_to_the_principal_point_in_both_models():
    for cam in (RS.CAM_VGA, RS.camera(dist=RS.KB, model=1)):
        s = RS.scene_axis(cam)
        assert RS.project(s["b"]["lm"], s["pose"], cam)[0].tolist() == [320.0, 240.0]
        feat, valid, info = RS.oracle(s["batch"], 0, s["b"], cam, fit_circle=True)
        assert valid.all() and info == (1, 0) and np.abs(feat[0, :2] - [320.0, 240.0]).max() < 1e-9
        _, radii = RS.quadrant_radii(s["b"], 0, s["pose"], cam)
        print("model %d quadrant radii" % cam["model"], radii.round(2))            # 30.80 18.90 31.48 16.81 / 30.76 18.96 31.44 16.75
        assert np.allclose(radii, [30.8, 18.9, 31.5, 16.8], atol=0.1)


def test_z0_behind_and_bounds_scenes():
    s = RS.scene_z0()
    assert s["pose"][11] == 0.0 and (s["b"]["lm"][:, 2] == 0).all()
    assert RS.oracle(s["batch"], 0, s["b"], s["cam"])[2] == (1, 0)                   # z == 0 -> divided by 1: every circle found
    s = RS.scene_behind()
    pose = s["pose"]
    assert ((s["b"]["lm"] @ pose[:9].reshape(3, 3).T + pose[9:])[:, 2] < 0).all()
    assert abs(np.linalg.det(pose[:9].reshape(3, 3)) - 1) < 1e-12
    assert RS.oracle(s["batch"], 0, s["b"], s["cam"])[2] == (1, 0)
    s = RS.scene_bounds()
    uv = RS.project(s["b"]["lm"], s["pose"], s["cam"])
    assert uv.tolist() == [list(p) for p in RS.BOUNDS_UV]                           # exact: powers of two throughout
    w, h = s["cam"]["width"], s["cam"]["height"]
    by_rule = [int(0 <= u < w and 0 <= v < h) for u, v in RS.BOUNDS_UV]
    assert by_rule == RS.BOUNDS_VALID
    _, valid, info = RS.oracle(s["batch"], 0, s["b"], s["cam"])
    assert valid.tolist() == RS.BOUNDS_VALID and info == (0, 6)
    # the erased ones are erased by the bound alone: on a sensor one pixel larger on each side ... the two ON the far bounds
    # and the two half a pixel beyond them come back
    big = dict(s["cam"], width=w + 1, height=h + 1)
    assert RS.oracle(s["batch"], 0, s["b"], big)[1].tolist() == [1, 1, 1, 0, 0, 1, 1, 1, 1]


# ---- per-circle gates ------------------------------------------------------------------------------------------------
def test_quadrant_probes_discriminate():
    s = RS.scene_quadrants()
    bt, radii, centre = s["batch"], s["radii"], s["centre"]
    assert centre.tolist() == [320.0, 240.0]
    for k, ((dx, dy), picked, other) in enumerate(RS.AXIS_PROBES):
        assert abs(radii[picked] - radii[other]) >= 6.5                             # 11.9 / 14.0 / 14.7 / 12.6 px
        d = np.hypot(*(s["probes"][k] - centre))
        assert abs(d - radii[picked]) <= 3 - 0.4 and abs(d - radii[other]) > 3 + 3   # inlier of one, far outlier of the other
        d1 = np.hypot(*(s["probes"][4 + k] - centre))
        assert abs(d1 - radii[other]) > 3 + 3                                        # one pixel over: the other quadrant, no inlier
        # the far members are outside every search radius
        pos = bt.oracle_args(k)[0]
        assert (np.hypot(*(pos[-5:] - centre).T) > radii.max() + 3 + 100).all()
    for f in range(bt.F):
        _, valid, _ = RS.oracle(bt, f, s["b"], s["cam"])
        assert valid[0] == s["valid"][f], "keyframe %d" % f
    assert s["valid"] == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]


def test_gate_scene_members_and_radii():
    s = RS.scene_gates()
    bt, radii = s["batch"], np.sort(s["radii"])
    second, third = radii[1], radii[2]
    assert s["what"] == ["r 29", "r 21", "pos 5", "pos 4", "neg 5", "neg 4", "collinear"]
    cnt = [(int(bt.seg_cnt[2 * f]), int(bt.seg_cnt[2 * f + 1])) for f in range(bt.F)]
    assert cnt[2:6] == [(5, 24), (4, 24), (24, 5), (24, 4)]
    for f in range(bt.F - 1):
        feat, valid, _ = RS.oracle(bt, f, s["b"], s["cam"])
        assert valid[0] == s["valid"][f], s["what"][f]
    # third-smallest radius: the 29 px ring passes on the third only, the 21 px ring would pass on the second only
    r29 = RS.oracle(bt, 0, s["b"], s["cam"])[0][0, 2]
    assert abs(r29 - third) <= 4.5 and abs(r29 - second) > 4.5                      # r = 29.13: 1.67 and 10.22
    px = np.concatenate(bt.oracle_args(1)[:2])
    r21 = np.hypot(*(px - s["centre"]).T).mean()
    assert abs(r21 - second) <= 4.5 and abs(r21 - third) > 4.5                      # r = 21.1: 2.2 and 9.7
    assert (np.abs(np.hypot(*(px - s["centre"]).T) - second) <= 3).sum() >= 5       # ... and it IS picked up (inliers of 18.9)
    # collinear members: one row, both polarities, inliers among them
    pos, neg = bt.oracle_args(6)[:2]
    assert len(pos) >= 5 and len(neg) >= 5 and set(pos[:, 1]) | set(neg[:, 1]) == {270.0}
    d = np.hypot(*(pos[pos[:, 0] >= 320] - s["centre"]).T)
    assert (np.abs(d - s["radii"][0]) <= 3).all()


# ---- the frame verdict -----------------------------------------------------------------------------------------------
# info per keyframe of RS.scene_verdict, by hand from CirclesEventFrame.cpp:583-621: (fit_circle 0, fit_circle 1).  Edges in the
# order first row, last row, first column, last column; size - 2 erased is below the border score's bar, size - 1 reaches it
# (score >= size - 1); fit_circle skips the border score; erased >= 0.2 n rejects in either mode.
VERDICTS = {
    # 20 circles, 0.2 n = 4: rows of 4, columns of 5 — four erased of a column also is 20 %
    "5x4": ([(1, 2), (0, 3), (1, 2), (0, 3), (1, 3), (0, 4), (1, 3), (0, 4), (0, 3), (0, 4)],
            [(1, 2), (1, 3), (1, 2), (1, 3), (1, 3), (0, 4), (1, 3), (0, 4), (1, 3), (0, 4)]),
    # 36 circles, 0.2 n = 7.2: rows of 4, first column {0 8 16 24 32}, last column {7 15 23 31}
    "9x4": ([(1, 2), (0, 3), (1, 2), (0, 3), (1, 3), (0, 4), (1, 2), (0, 3), (0, 7), (0, 8)],
            [(1, 2), (1, 3), (1, 2), (1, 3), (1, 3), (1, 4), (1, 2), (1, 3), (1, 7), (0, 8)]),
    # 128 circles, 0.2 n = 25.6: rows of 16, columns of 8
    "8x16": ([(1, 14), (0, 15), (1, 14), (0, 15), (1, 6), (0, 7), (1, 6), (0, 7), (0, 25), (0, 26)],
             [(1, 14), (1, 15), (1, 14), (1, 15), (1, 6), (1, 7), (1, 6), (1, 7), (1, 25), (0, 26)]),
}


@pytest.mark.parametrize("name", ["5x4", "9x4", "8x16"])
def test_verdict_scene_matches_the_hand_written_table(name):
    s = RS.scene_verdict(name)
    bt = s["batch"]
    for fit in (0, 1):
        for f in range(bt.F):
            _, valid, info = RS.oracle(bt, f, s["b"], s["cam"], fit_circle=bool(fit))
            assert info == VERDICTS[name][fit][f], "keyframe %d fit_circle %d" % (f, fit)
            assert sorted(np.nonzero(valid == 0)[0].tolist()) == sorted(s["masks"][f])   # exactly the chosen circles are gone


def test_segment_scene_verdicts():
    s = RS.scene_segments()
    bt = s["batch"]
    got = [int(RS.oracle(bt, f, s["b"], s["cam"])[1][0]) for f in range(bt.F)]
    assert got == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0]          # a polarity empty or of one point: erased; labels all -1: erased
