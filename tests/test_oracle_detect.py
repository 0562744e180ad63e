"""CPU suite: known answers for the candidate-extraction oracle (oracle/detect_oracle.cpp)."""
import numpy as np

import oracle_lib as O
import synth_fit_scene as FS
import synth_stream as SS


def test_circle_radius_threshold_kat():
    # shipped config 346x260, 9x4 asymmetric, square 5.5, radius 1.75
    v = O.circle_radius_threshold(346.0, 260.0, 9, 4, True, 5.5, 1.75)
    assert v == 15.511363636363637
    # symmetric branch (CirclesEventFrame.cpp:27-31)
    v2 = O.circle_radius_threshold(346.0, 260.0, 9, 4, False, 5.5, 1.75)
    assert abs(v2 - min(346.0 / 9, 260.0 / 4) / 5.5 * 1.75 * 1.5) < 1e-15


def test_fit_circle_exact_points():
    th = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    pts = np.stack([40 + 7.5 * np.cos(th), 30 + 7.5 * np.sin(th)], 1)
    c, r = O.fit_circle(pts[:12], pts[12:])
    assert np.allclose(c, [40, 30], atol=1e-9) and abs(r - 7.5) < 1e-9


def test_two_half_arcs_make_one_candidate():
    """36 clean circles: every +/- half-arc pair is mutually nearest -> 36 candidates on the grid."""
    rng = np.random.default_rng(3)
    cx, cy = np.meshgrid(30 + 42.0 * np.arange(9), 25 + 45.0 * np.arange(4))   # gap between circles > diameter
    centres = np.stack([cx.ravel(), cy.ravel()], 1)
    r = 9.0
    pos, neg = [], []
    for c in centres:
        th = np.linspace(-1.4, 1.4, 26)
        pos.append(np.unique(np.floor(c + r * np.stack([np.cos(th), np.sin(th)], 1)), axis=0))
        neg.append(np.unique(np.floor(c + r * np.stack([np.cos(th + np.pi), np.sin(th + np.pi)], 1)), axis=0))
    pos = np.concatenate(pos)
    neg = np.concatenate(neg)
    rng.shuffle(pos, axis=0)
    rng.shuffle(neg, axis=0)
    out = O.extract_candidates(pos, neg, 4.0, 2, 5, 36, 15.5)
    assert out["status"] == 0 and out["nk_pos"] == 36 and out["nk_neg"] == 36 and out["n"] == 36
    d = np.linalg.norm(out["xyr"][:, None, :2] - (centres[None] - 0.5), axis=2).min(1)
    # centre = midpoint of the two norm-median pixels: a crude estimate by design (refined by rectifyFeatures)
    assert (d < 8.0).all() and (np.abs(out["xyr"][:, 2] - r) < 4.0).all()
    # fitCircle == 1 path (:180-281): the algebraic fit recovers the true centres / radius much more closely
    fit = O.extract_candidates(pos, neg, 4.0, 2, 5, 36, 15.5, fit_circle=True, knn_num=3)
    assert fit["status"] == 0 and fit["n"] == 36
    d = np.linalg.norm(fit["xyr"][:, None, :2] - (centres[None] - 0.5), axis=2).min(1)
    assert (d < 0.8).all() and (np.abs(fit["xyr"][:, 2] - r) < 0.8).all()
    # too few clusters -> extractFeatures returns false (:127-129)
    out = O.extract_candidates(pos[:200], neg, 4.0, 2, 5, 36, 15.5)
    assert out["status"] == 1 and out["n"] == 0
    out = O.extract_candidates(np.zeros((0, 2)), neg, 4.0, 2, 5, 36, 15.5)
    assert out["status"] == 1 and out["nk_neg"] == 0     # :62-64 returns before DBSCAN


def test_synthetic_window_gives_candidates():
    buf = SS.make_stream(30000, rate=2.0e6)     # denser stream -> complete half arcs
    t, _, _ = SS.unpack_records(buf)
    rec = buf.numpy()
    lo, hi = O.window_bounds(rec, float(t[0]), float(t[0]) + 1.5e-3)
    pos, neg, _ = O.event_frame(rec, lo, hi, "reference")
    out = O.extract_candidates(pos, neg, 4.0, 2, 5, 36, 15.511363636363637)
    assert out["status"] == 0 and out["n"] >= 30


def test_full_window_loop_equals_the_single_window_functions_on_both_kd_trees():
    """oracle_detect_windows_full_mt (the batch checker of the full-size GPU tests) lays out, per window, exactly what
    event_frame + dbscan + extract_candidates give — with the restated kd-tree and with the reference's compiled one
    (oracle/_ref), which must agree with each other in every array."""
    n, rate = 120_000, 2.0e6
    buf = SS.make_stream(n, rate=rate, seed=4)
    rec = buf.numpy()
    t0, t1 = SS.tiled_windows(5.0, 5.0 + (n - 1) / rate)
    t0 = np.concatenate([t0, [t0[3], 1.0]])             # an overlapping window and an empty one
    t1 = np.concatenate([t1, [t1[5], 1.1]])
    S = len(t0)
    bounds = [O.window_bounds(rec, a, b) for a, b in zip(t0, t1)]
    size = np.array([hi - lo for lo, hi in bounds], np.uint64)
    wb = np.concatenate([[0], np.cumsum(size)]).astype(np.uint64)
    outs = {}
    try:
        for ref in ([False, True] if O.have_ref_kdtree() else [False]):
            O.set_kd_backend(ref)
            assert ("reference" in O.kd_backend()) == ref
            outs[ref] = O.detect_windows_full(rec, t0, t1, wb, int(wb[-1]), n_threads=3)
    finally:
        O.set_kd_backend(False)
    f = outs[False]
    assert f["events"] == int(size.sum())
    if True in outs:
        for k, v in f.items():
            assert np.array_equal(v, outs[True][k]), k
    paired = 0
    for s in range(S):
        lo, hi = bounds[s]
        assert (int(f["win_lo"][s]), int(f["win_hi"][s])) == (lo, hi)
        pos, neg, ep = O.event_frame(rec, lo, hi, "reference")
        b = int(wb[s])
        assert (int(f["seg_cnt"][2 * s]), int(f["seg_cnt"][2 * s + 1])) == (len(pos), len(neg))
        assert np.array_equal(f["event_point"][b:b + hi - lo], ep)
        assert np.array_equal(f["xy"][b:b + len(pos)], pos) and np.array_equal(f["xy"][b + len(pos):b + len(pos) + len(neg)], neg)
        assert f["def_pts"][b:b + len(pos) + len(neg)].all() and not f["def_pts"][b + len(pos) + len(neg):int(wb[s + 1])].any()
        for o, pts, k in ((b, pos, 0), (b + len(pos), neg, 1)):
            if len(pts):
                rc, lab, nc = O.dbscan(pts, 4.0, 2)
                assert np.array_equal(f["labels"][o:o + len(pts)], lab) and int(f["n_clusters"][2 * s + k]) == nc
        r = O.extract_candidates(pos, neg, 4.0, 2, 5, 36, 15.511363636363637)
        assert list(f["win_info"][s]) == [r["n"], r["nk_pos"], r["nk_neg"], r["status"]] and bool(f["tie"][s]) == r["tie"]
        if len(pos) and len(neg):
            assert np.array_equal(f["kept_labels"][b:b + len(pos)], r["kept_pos"]) and f["def_kept"][b:b + len(pos)].all()
            assert np.array_equal(f["kept_labels"][b + len(pos):b + len(pos) + len(neg)], r["kept_neg"])
        if not r["status"]:
            paired += 1
            assert np.array_equal(f["rep"][b:b + r["nk_pos"]], r["rep_pos"])
            assert np.array_equal(f["rep"][b + len(pos):b + len(pos) + r["nk_neg"]], r["rep_neg"])
            assert np.array_equal(f["cand_pair"][b:b + r["n"]], r["pair"]) and np.array_equal(f["cand_xyr"][b:b + r["n"]], r["xyr"])
            assert int(f["def_rep"][b:int(wb[s + 1])].sum()) == r["nk_pos"] + r["nk_neg"] and int(f["def_cand"][b:int(wb[s + 1])].sum()) == r["n"]
        else:
            assert not f["def_rep"][b:int(wb[s + 1])].any() and not f["def_cand"][b:int(wb[s + 1])].any()
    assert paired >= S // 2


# ---- the fitCircle == 1 pairing on hand-built windows (synth_fit_scene): what tests/test_gpu_fit_circle.py runs on the GPU ----
def _groups():
    return {g.name: g for g in FS.all_groups()}


def _named(group, K):
    return dict(zip(group.names, FS.oracle_windows(group, K, O)))


def test_fit_scenes_oracle_equals_the_numpy_restatement():
    """Every scene, every knn_num it is run with: pairs, count and circles of oracle/detect_oracle.cpp equal, bit for bit, those of
    synth_fit_scene.pairing_trace — neighbour list by (squared distance, index) ending at the number of clusters, the two gates,
    the fit, first minimum, noise test, back-check, written again in numpy scalars.  Integer pixels: the nine sums are exact in any
    order, the rest is the same sequence of IEEE operations."""
    paired = 0
    for g in FS.all_groups():
        for K in g.knn:
            for name, (pos, neg, ref, tr) in zip(g.names, FS.oracle_windows(g, K, O)):
                if ref["status"]:
                    assert ref["n"] == 0 and (g.name, name) == ("tiny", "two_pixels")
                    continue
                paired += 1
                assert ref["n"] == len(tr["pair"]) and np.array_equal(ref["pair"], tr["pair"]), (g.name, name, K)
                assert np.array_equal(ref["xyr"], tr["xyr"], equal_nan=True), (g.name, name, K)
                assert np.isfinite(ref["xyr"]).all()      # a NaN or inf fit never passes err < 2 / r: no candidate carries one
    assert paired >= 40


def test_fit_scene_knn_lists_grow_with_knn_num():
    """3 x 4 board: the gated list of some + cluster holds 4 neighbours from knn_num = 4 and 5 from knn_num = 5 on, and with
    knn_num = 1 most + arcs find the next ring's - arc first and fail."""
    g = _groups()["knn_board"]
    longest = {}
    for K in g.knn:
        pos, neg, ref, tr = _named(g, K)["board"]
        assert (ref["nk_pos"], ref["nk_neg"]) == (12, 15)
        longest[K] = max(len(s["fwd"]) for s in tr["steps"])
        assert all(len(s["fwd"]) <= K for s in tr["steps"])
        assert ref["n"] == (12 if K >= 2 else 5)
        if K == 1:
            assert sorted(s["end"] for s in tr["steps"]) == ["back"] * 2 + ["noise"] * 5 + ["ok"] * 5
    assert longest == {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 5, 7: 5, 8: 5}


def test_fit_scene_distance_tie_goes_to_the_smaller_cluster_index():
    g = _groups()["tie"]
    for K in (1, 2):
        w = _named(g, K)
        for name in g.names:
            pos, neg, ref, tr = w[name]
            st = tr["steps"][0]
            assert (ref["nk_pos"], ref["nk_neg"]) == (1, 2) and list(st["fwd"]) == list(range(K)) and st["fwd_cut"] is None
            if K == 2:
                assert list(st["fwd_d2"]) == [256.0, 256.0] and ref["n"] == 1            # both fitted: the partner wins on its error
            rp, first = pos[ref["rep_pos"][0]], neg[ref["rep_neg"][0]]
            assert ((first - rp) ** 2).sum() == 256.0
            partner_first = first[0] < rp[0]                                            # the partner is the - arc on the left
            assert partner_first == (name == "partner_first")
            if K == 1:
                assert (ref["n"], st["end"]) == ((1, "ok") if partner_first else (0, "noise"))


def test_fit_scene_ratio_gate_keeps_4_d0_and_cuts_beyond():
    g = _groups()["ratio"]
    for K in g.knn:
        w = _named(g, K)
        pos, neg, ref, tr = w["at_4d0"]
        st = tr["steps"][0]
        assert list(st["fwd_d2"]) == [64.0, 256.0] and len(st["fwd"]) == 2 and st["fwd_cut"] is None and st["nmin"] == 1
        assert ref["n"] == 1 and tuple(neg[ref["rep_neg"][ref["pair"][0, 1]]]) == (22.0, 30.0) and abs(ref["xyr"][0, 2] - 8.0) < 0.1
        pos, neg, ref, tr = w["at_4d0_plus_1"]           # the next squared pixel distance beyond the bound: cut
        st = tr["steps"][0]
        assert list(st["fwd_d2"]) == [64.0, 257.0] and len(st["fwd"]) == 1 and st["fwd_cut"] == "ratio"
        assert ref["n"] == 1 and tuple(neg[ref["rep_neg"][ref["pair"][0, 1]]]) == (30.0, 30.0)      # the block, not the arc at (22, 31)
        assert (22.0, 31.0) in {tuple(neg[i]) for i in ref["rep_neg"]}
        pos, neg, ref, tr = w["beyond_4d0"]
        st = tr["steps"][0]
        assert list(st["fwd_d2"]) == [58.0, 256.0] and len(st["fwd"]) == 1 and st["fwd_cut"] == "ratio"
        assert ref["n"] == 1 and tuple(neg[ref["rep_neg"][ref["pair"][0, 1]]]) == (31.0, 27.0)      # the block inside the ring
        pos, neg, ref, tr = w["adjacent"]
        st = tr["steps"][0]
        assert list(st["fwd_d2"]) == [1.0, 256.0] and len(st["fwd"]) == 1 and st["fwd_cut"] == "ratio" and ref["n"] == 0


def test_fit_scene_distance_gate_keeps_4_thr2_and_cuts_below():
    gs = _groups()
    assert 4 * FS.T_AT * FS.T_AT == 324.0 and 4 * FS.T_BELOW * FS.T_BELOW < 324.0
    pos, neg, ref, tr = _named(gs["gate_at"], 2)["tees"]
    st = tr["steps"][0]
    assert list(st["fwd_d2"]) == [324.0] and st["fwd_cut"] is None and st["end"] == "ok" and ref["n"] == 1
    assert st["fits"][0][1] < FS.T_BELOW                              # (the radius test r > thr is not what tells the two runs apart)
    pos, neg, ref, tr = _named(gs["gate_below"], 2)["tees"]
    st = tr["steps"][0]
    assert list(st["fwd_d2"]) == [324.0] and st["fwd_cut"] == "gate" and st["end"] == "empty" and ref["n"] == 0


def test_fit_scene_back_check_rejects_the_second_claim():
    pos, neg, ref, tr = _named(_groups()["back"], 3)["two_plus_one_minus"]
    ends = sorted(s["end"] for s in tr["steps"])
    assert ends == ["back", "ok"] and ref["n"] == 1
    loser = [s for s in tr["steps"] if s["end"] == "back"][0]
    best = loser["fits"][loser["nmin"]]
    assert best[0] < 2 / best[1] and len(loser["back"]) == 2           # its own forward fit passes; the - arc's back list holds both
    assert abs(ref["xyr"][0, 2] - 8.0) < 0.1


def test_fit_scene_degenerate_fits_are_rejected_through_nan_comparisons():
    gs = _groups()
    for K in (1, 3):
        w = _named(gs["collinear"], K)
        for name in ("row", "diagonal"):
            pos, neg, ref, tr = w[name]
            st = tr["steps"][0]
            assert np.isnan(st["fits"][0][1]) and np.isnan(st["fits"][0][0])      # NaN radius: r > thr is false, the error is NaN
            assert st["end"] == "noise" and ref["n"] == 0                         # ... and NaN < 2 / NaN is false
        for name in ("among_rings", "among_rings_duplicated"):
            pos, neg, ref, tr = w[name]
            assert (ref["nk_pos"], ref["nk_neg"]) == (5, 5) and ref["n"] == (4 if K == 3 else 1)
        a, b = w["among_rings"], w["among_rings_duplicated"]                      # duplicated events change nothing
        assert {tuple(q) for q in a[0]} == {tuple(q) for q in b[0]} and a[2]["n"] == b[2]["n"]
        w = _named(gs["tiny"], K)
        assert w["two_pixels"][2]["status"] == 1 and (w["two_pixels"][2]["nk_pos"], w["two_pixels"][2]["nk_neg"]) == (0, 0)
        pos, neg, ref, tr = w["two_pairs_square"]
        assert ref["n"] == 1 and np.allclose(ref["xyr"][0], [10.5, 11.5, np.sqrt(2.5)], atol=1e-9)
        assert w["two_pairs_collinear"][2]["n"] == 0


def test_fewer_clusters_than_knn_num_ends_the_list_at_the_count():
    """The contract below knn_num kept clusters (include/ecal.h at knn_num): the neighbour list ends at the number of kept
    clusters of the other polarity — the oracle against the numpy restatement, which sorts by (d2, index), cuts at the count and
    applies the two gates."""
    gs = _groups()
    seen = 0
    for name in ("short_2x2", "short_2x3", "short_one_side"):
        g = gs[name]
        for K in g.knn:
            pos, neg, ref, tr = FS.oracle_windows(g, K, O)[0]
            assert min(ref["nk_pos"], ref["nk_neg"]) < K and ref["status"] == 0
            for st in tr["steps"]:
                assert len(st["fwd_d2"]) == min(K, ref["nk_neg"]) and len(st["back_d2"]) == min(K, ref["nk_pos"])
                assert len(set(st["fwd"])) == len(st["fwd"]) and len(set(st["back"])) == len(st["back"])    # no cluster twice
            assert np.array_equal(ref["pair"], tr["pair"]) and np.array_equal(ref["xyr"], tr["xyr"])
            assert ref["n"] == ref["nk_pos"]                  # every ring is found
            seen += 1
    assert seen == 5
    assert gs["short_one_side"].knn == (8,) and FS.oracle_windows(gs["short_one_side"], 8, O)[0][2]["nk_neg"] == 9


def test_fit_scene_coincident_representatives_cut_every_other_neighbour():
    """d0 = 0 (point sets handed to the stages directly; no event window can hold them): 4 d0 = 0, so the partner at 256 is cut
    and the + arc is left with the block on top of it."""
    pos, neg = FS.coincident_points()
    g = FS.Group("coincident", [], [], knn=(3,))
    ref = FS.extract(O, pos, neg, g, 3)
    tr = FS.pairing_trace(pos, neg, ref, g.thr, 3)
    st = tr["steps"][0]
    assert (ref["nk_pos"], ref["nk_neg"]) == (1, 2) and list(st["fwd_d2"]) == [0.0, 256.0] and len(st["fwd"]) == 1 and st["fwd_cut"] == "ratio"
    assert ref["n"] == len(tr["pair"]) == 0 and st["end"] == "noise"
