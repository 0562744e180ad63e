"""GPU parity: the fitCircle == 1 pairing (CirclesEventFrame.cpp:180-281 — fit_pair, knn_gated and the FIT branch of
extract_window in extract_window.hpp) on hand-built windows of integer pixels (synth_fit_scene) against the CPU oracle and
against the numpy restatement of the pairing: every knn_num, distance ties, the two gates at and beside their boundaries, the
back-check, degenerate (singular) fits, fewer kept clusters than knn_num, and every tier of the extraction with its FIT kernels.

Every window goes records -> slicer -> DBSCAN -> extraction and is checked as test_gpu_detect._check_windows checks it (status,
kept labels, representatives, count, pairs, circles to 1e-9) and then once more with the circles compared BIT FOR BIT: on
integer pixels the nine sums of the fit are exact in any order and everything after them is the same sequence of IEEE operations
in the kernel (built with -ffp-contract=off), in oracle/detect_oracle.cpp and in synth_fit_scene.fit_circle.  What the scenes are
built to reach — which rule ends which + cluster — is asserted from the oracle alone in tests/test_oracle_detect.py."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import synth_fit_scene as FS
import test_gpu_detect as TD

pytestmark = pytest.mark.gpu
GROUPS = {g.name: g for g in FS.all_groups()}


@pytest.fixture(scope="module")
def env():
    import torch
    import eventcalib_amd
    from eventcalib_amd.pipeline import DetectPipeline
    ctx = eventcalib_amd.Context(0)
    yield ctx, DetectPipeline(ctx), torch
    ctx.close()


def _limits():
    """DET_LDS_PTS, DET_LDS_MAXC, DET_LDS_PTS2, DET_LDS_MAXC2 and DET_KNN_MAX as extract_window.hpp states them."""
    src = open(os.path.join(O.ROOT, "eventcalib_amd", "csrc", "extract_window.hpp")).read()
    return {k: int(re.search(r"\b%s = (\d+)\b" % k, src).group(1)) for k in ("DET_LDS_PTS", "DET_LDS_MAXC", "DET_LDS_PTS2", "DET_LDS_MAXC2", "DET_KNN_MAX")}


def _run(pipe, torch, g, K, exact_ties=True, fused=False, built=None):
    b = built or g.build()
    pipe.set_windows(b["t0"], b["t1"])
    pipe.set_detect_params(g.cluster_min, g.need, g.thr, fit_circle=True, knn_num=K)
    pipe.run(b["buf"].cuda(), 4.0, g.minpts, exact_ties=exact_ties, fused=fused)
    torch.cuda.synchronize()
    assert not pipe.overflowed()
    return b


def _check(pipe, torch, g, b, K, exact_ties=True):
    """Every window of the group: as _check_windows (where the DBSCAN runs with its minpts = 2), then everything again with
    the circles bit for bit, against the oracle and against the numpy restatement.  Returns the oracle's results."""
    S = len(b["t0"])
    if g.minpts == 2:
        TD._check_windows(pipe, torch, b["buf"].numpy(), b["t0"], b["t1"], g.cluster_min, g.need, g.thr, True, K, exact_ties)
    info = pipe.win_info[:S].cpu().numpy().astype(np.int64)
    off = pipe.seg_off[:2 * S].cpu().numpy().astype(np.int64)
    cnt = pipe.seg_cnt[:2 * S].cpu().numpy().astype(np.int64)
    xy, kept, rep = pipe.xy.cpu().numpy(), pipe.kept_labels.cpu().numpy(), pipe.rep.cpu().numpy()
    pair, xyr = pipe.cand_pair.cpu().numpy(), pipe.cand_xyr.cpu().numpy()
    refs = []
    for s in range(S):
        op, on = off[2 * s], off[2 * s + 1]
        pos, neg = xy[op:op + cnt[2 * s]], xy[on:on + cnt[2 * s + 1]]
        for got, want in zip((pos, neg), b["points"][s]):                      # the window holds the scene's pixels, each once
            assert len(got) == len(want) and {tuple(q) for q in got} == {tuple(q) for q in want}, (g.name, g.names[s])
        ref = FS.extract(O, pos, neg, g, K)
        what = (g.name, g.names[s], K, exact_ties)
        assert info[s, 3] == ref["status"] and (info[s, 1], info[s, 2]) == (ref["nk_pos"], ref["nk_neg"]), what
        assert np.array_equal(kept[op:op + len(pos)], ref["kept_pos"]) and np.array_equal(kept[on:on + len(neg)], ref["kept_neg"]), what
        refs.append(ref)
        if ref["status"]:
            assert info[s, 0] == 0, what
            continue
        if ref["tie"] and not exact_ties:      # the smaller pid at a tied median: the member of rank size / 2 by (norm, pid) ...
            for o, pts, lab, nk in ((op, pos, ref["kept_pos"], ref["nk_pos"]), (on, neg, ref["kept_neg"], ref["nk_neg"])):
                for k in range(nk):
                    m = np.nonzero(lab == k)[0]
                    by = m[np.lexsort((m, (pts[m] ** 2).sum(1)))]
                    assert rep[o + k] == by[len(m) // 2], what
            # ... and with the build's representatives handed to the oracle everything downstream
            ref = FS.extract(O, pos, neg, g, K, rep[op:op + ref["nk_pos"]].astype(np.uint32), rep[on:on + ref["nk_neg"]].astype(np.uint32))
            refs[-1] = ref
        assert np.array_equal(rep[op:op + ref["nk_pos"]], ref["rep_pos"]) and np.array_equal(rep[on:on + ref["nk_neg"]], ref["rep_neg"]), what
        n = ref["n"]
        tr = FS.pairing_trace(pos, neg, ref, g.thr, K)
        assert info[s, 0] == n == len(tr["pair"]), what
        assert np.array_equal(pair[op:op + n], ref["pair"]) and np.array_equal(pair[op:op + n], tr["pair"]), what
        assert np.array_equal(xyr[op:op + n], ref["xyr"], equal_nan=True), what            # bit for bit (NaNs where the oracle's are)
        assert np.array_equal(xyr[op:op + n], tr["xyr"], equal_nan=True), what
    return refs


@pytest.mark.parametrize("knn_num", list(range(1, 9)))
def test_every_knn_num_on_a_3x4_board(env, knn_num):
    """knn_num 1 .. DET_KNN_MAX on 12 rings and three decoys: 12 and 15 kept clusters, so every list is full; gated lists of
    up to five neighbours (test_oracle_detect.test_fit_scene_knn_lists_grow_with_knn_num)."""
    ctx, pipe, torch = env
    assert _limits()["DET_KNN_MAX"] == 8
    g = GROUPS["knn_board"]
    for exact_ties in ((True, False) if knn_num in (1, 5, 8) else (True,)):
        ref = _check(pipe, torch, g, _run(pipe, torch, g, knn_num, exact_ties), knn_num, exact_ties)[0]
        if exact_ties:       # (with the smaller pid at the board's tied medians the representatives, and so the lists, are others)
            assert ref["n"] == (12 if knn_num >= 2 else 5)


@pytest.mark.parametrize("name", ["tie", "ratio", "gate_at", "gate_below", "back"])
def test_distance_ties_gate_boundaries_and_the_back_check(env, name):
    """Equal distances on both sides of a + representative (the smaller cluster index first), a neighbour at exactly 4 d0, one
    at 4 d0 + 1 and one further off, a - representative next to the + one (d0 = 1; d0 = 0 cannot occur: a pixel of both polarities is erased from
    both sets, EventFrame.cpp:24-32), a neighbour at exactly 4 thr^2 and the next threshold below, two + clusters after one
    - cluster."""
    ctx, pipe, torch = env
    g = GROUPS[name]
    counts = {}
    for K in g.knn:
        for exact_ties in (True, False):
            counts[K] = [r["n"] for r in _check(pipe, torch, g, _run(pipe, torch, g, K, exact_ties), K, exact_ties)]
    want = {"tie": {1: [1, 0], 2: [1, 1]}, "ratio": {2: [1, 1, 1, 0], 3: [1, 1, 1, 0]}, "gate_at": {2: [1]}, "gate_below": {2: [0]}, "back": {3: [1]}}
    assert counts == want[name]


@pytest.mark.parametrize("name", ["collinear", "tiny"])
def test_degenerate_fits(env, name):
    """Singular systems — both clusters on one row, on one diagonal, such a pair beside good rings, with duplicated events —
    and the smallest clusters (minpts = 1, cluster_min = 1): NaN and inf fits are rejected by the same comparisons as in the
    oracle, pairs and count equal, no NaN reaches a circle."""
    ctx, pipe, torch = env
    g = GROUPS[name]
    for K in g.knn:
        for exact_ties in (True, False):
            refs = _check(pipe, torch, g, _run(pipe, torch, g, K, exact_ties), K, exact_ties)
            if name == "collinear":
                assert [r["n"] for r in refs[:2]] == [0, 0]
                if exact_ties:   # (the rings' medians are tied: other representatives with the smaller pid)
                    assert [r["n"] for r in refs[2:]] == ([4, 4] if K == 3 else [1, 1])
            else:
                assert [r["status"] for r in refs] == [1, 0, 0] and [r["n"] for r in refs] == [0, 1, 0]
            S = len(refs)
            off = pipe.seg_off[:2 * S:2].cpu().numpy()
            got = pipe.cand_xyr.cpu().numpy()
            assert all(np.isfinite(got[o:o + r["n"]]).all() for o, r in zip(off, refs))


@pytest.mark.parametrize("name", ["short_2x2", "short_2x3", "short_one_side"])
def test_fewer_kept_clusters_than_knn_num(env, name):
    """The neighbour list ends at the number of kept clusters present, then the two gates apply (include/ecal.h at knn_num):
    4 and 4 clusters with knn_num 5, 6, 8; 6 and 6 with 8; 4 and 9 with 8 — against the oracle and against the numpy
    restatement (sort by (d2, index), cut at the count, the two gates)."""
    ctx, pipe, torch = env
    g = GROUPS[name]
    for K in g.knn:
        for exact_ties in (True, False):
            ref = _check(pipe, torch, g, _run(pipe, torch, g, K, exact_ties), K, exact_ties)[0]
            assert min(ref["nk_pos"], ref["nk_neg"]) < K and (ref["n"] == ref["nk_pos"] or not exact_ties)


def _sizes(pipe):
    cnt = pipe.seg_cnt[:2].cpu().numpy().astype(np.int64)
    return int(cnt.sum()), int(pipe.n_clusters[:2].cpu().numpy().max()), int(pipe.win_info[0, 1:3].cpu().numpy().max())


@pytest.mark.parametrize("form", ["inline", "listed", "smaller_pid"])
@pytest.mark.parametrize("kind", ["first", "points", "clusters", "global"])
def test_every_tier_with_the_circle_fit(env, kind, form, monkeypatch):
    """The 3 x 4 board alone and with lattice noise around it: the first pass (extract_kernel<true, .>), the second pass for
    its point count and for its cluster count (extract_list_kernel<true, .>) and the global-scratch path.  The tier is stated
    from the sizes read back against the header's constants.  The board's arcs (23 pixels) have tied medians; what the exact
    extraction does with them is stated by the count of windows it leaves on its tie list (ecal_debug_tie_list_count):
      inline   the <true, 2> pass resolves the ties of an LDS-staged window itself (resolve_ties_inline, on the kd-trees the
               pixel DBSCAN exported) and lists nothing — the <true, 1> kernels find an empty list; the global-scratch window
               (doubles, no inline form) is listed and extracted again by extract_first_list_kernel<true, 1>;
      listed   ECAL_FORCE=extract_no_inline_ties: every tier's window is listed and extracted again in member order (ORD) with
               the fit — extract_first_list_kernel<true, 1> for the first pass's staging, which hands the 'points' and
               'clusters' windows on to extract_list_kernel<true, 1>: fit_pair on each tier's st.sorted / koff / ksize;
      smaller_pid  ecal_extract_batch_dev alone, the <true, 0> kernels."""
    ctx, pipe, torch = env
    from eventcalib_amd.capi import sync_env
    L = _limits()
    g = GROUPS["tier_" + kind]
    exact_ties = form != "smaller_pid"
    if form == "listed":
        monkeypatch.setenv("ECAL_FORCE", "extract_no_inline_ties")
    else:
        monkeypatch.delenv("ECAL_FORCE", raising=False)
    sync_env()
    ctx.set_tail_mode("tiered")      # (every size tier of the pixel DBSCAN launched: its passes export the trees)
    try:
        b = _run(pipe, torch, g, 3, exact_ties)
        listed = TD._tie_list_count(ctx, torch) if exact_ties else None
        n_all, n_raw, n_kept = _sizes(pipe)
        ref = _check(pipe, torch, g, b, 3, exact_ties)[0]
    finally:
        ctx.set_tail_mode("auto")
        monkeypatch.delenv("ECAL_FORCE", raising=False)
        sync_env()
    print("tier %s form %s: tie list %s, points %d, clusters %d raw %d kept" % (kind, form, listed, n_all, n_raw, n_kept))
    assert ref["tie"] and (ref["n"] == 12 or not exact_ties)
    assert not (pipe.win_info[0, 3].item() & 0x100)                    # no fallback to the smaller pid
    if form == "listed" or (form == "inline" and kind == "global"):
        assert listed == 1
    elif form == "inline":
        assert listed == 0
    if kind == "first":
        assert n_all <= L["DET_LDS_PTS"] and n_raw <= L["DET_LDS_MAXC"]
    elif kind == "points":       # over DET_LDS_PTS, within DET_LDS_PTS2 / DET_LDS_MAXC2
        assert L["DET_LDS_PTS"] < n_all <= L["DET_LDS_PTS"] + 64 and n_all <= L["DET_LDS_PTS2"] and n_raw <= L["DET_LDS_MAXC"]
    elif kind == "clusters":     # within DET_LDS_PTS, over DET_LDS_MAXC kept clusters, within DET_LDS_MAXC2
        assert n_all <= L["DET_LDS_PTS"] and L["DET_LDS_MAXC"] < n_kept <= n_raw <= L["DET_LDS_MAXC2"]
    else:                        # over DET_LDS_PTS2
        assert L["DET_LDS_PTS2"] < n_all <= L["DET_LDS_PTS2"] + 64


def test_packed_plain_and_fused_forms_agree_with_the_circle_fit(env):
    """The board with fit_circle set through the packed-points stage calls (DetectPipeline's default) and the plain ones, with
    either tie rule, and through ecal_detect_fused_dev (the plain stage calls in one: the smaller pid at tied medians): every
    result equal bit for bit within a tie rule, and equal to the oracle's."""
    ctx, _pipe, torch = env
    from eventcalib_amd.pipeline import DetectPipeline
    g = GROUPS["knn_board"]
    b = g.build()
    for exact_ties, forms in ((True, ((True, False), (False, False))), (False, ((True, False), (False, False), (False, True)))):
        outs = []
        for packed, fused in forms:
            pipe = DetectPipeline(ctx, packed=packed)
            _run(pipe, torch, g, 4, exact_ties, fused=fused, built=b)
            ref = _check(pipe, torch, g, b, 4, exact_ties)[0]
            off, cnt = pipe.seg_off[:2].cpu().numpy().astype(np.int64), pipe.seg_cnt[:2].cpu().numpy().astype(np.int64)
            o, n = off[0], ref["n"]
            outs.append(dict(off=off, cnt=cnt, info=pipe.win_info[:1].cpu().numpy().copy(), pts=pipe.xy.cpu().numpy()[o:o + cnt.sum()].copy(),
                             kept=pipe.kept_labels.cpu().numpy()[o:o + cnt.sum()].copy(), pair=pipe.cand_pair.cpu().numpy()[o:o + n].copy(),
                             xyr=pipe.cand_xyr.cpu().numpy()[o:o + n].copy(),
                             rep=np.concatenate([pipe.rep.cpu().numpy()[off[h]:off[h] + ref["nk_pos" if h == 0 else "nk_neg"]] for h in (0, 1)])))
        assert outs[0]["info"][0, 0] == 12 or not exact_ties
        for other in outs[1:]:
            for k, v in outs[0].items():
                assert np.array_equal(v, other[k]), (k, exact_ties)


def test_coincident_representatives_through_the_stage_calls(env):
    """d0 = 0: a - cluster whose representative is the + representative's own pixel.  An event window cannot hold that pixel in
    both sets, so the point sets go to ecal_dbscan_batch_dev and to both extraction calls directly: every other neighbour is
    cut (d > 4 d0 = 0), as in the oracle and in the restatement."""
    ctx, _pipe, torch = env
    pos, neg = FS.coincident_points()
    g = FS.Group("coincident", [], [], knn=(3,))
    ref = FS.extract(O, pos, neg, g, 3)
    tr = FS.pairing_trace(pos, neg, ref, g.thr, 3)
    assert ref["status"] == 0 and not ref["tie"] and tr["steps"][0]["fwd_d2"][0] == 0.0
    n = len(pos) + len(neg)
    dev = torch.device("cuda", ctx.device)
    xy = torch.tensor(np.concatenate([pos, neg]), dtype=torch.float64, device=dev)
    off = torch.tensor([0, len(pos)], dtype=torch.int32, device=dev)
    cnt = torch.tensor([len(pos), len(neg)], dtype=torch.int32, device=dev)
    labels, kept, rep = (torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(3))
    ncl = torch.zeros(2, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ctx.dbscan_batch_dev(xy.data_ptr(), off.data_ptr(), cnt.data_ptr(), 2, n, 0, 4.0, 2, labels.data_ptr(), ncl.data_ptr(), st)
    for exact in (False, True):
        info = torch.full((1, 4), -7, dtype=torch.int32, device=dev)
        pair = torch.full((n, 2), -7, dtype=torch.int32, device=dev)
        xyr = torch.full((n, 3), -7.0, dtype=torch.float64, device=dev)
        args = (g.cluster_min, g.need, g.thr, info.data_ptr(), pair.data_ptr(), xyr.data_ptr(), kept.data_ptr(), rep.data_ptr(), st)
        if exact:
            ctx.extract_batch_exact_dev(xy.data_ptr(), off.data_ptr(), cnt.data_ptr(), labels.data_ptr(), ncl.data_ptr(), 1, n, 4.0, *args,
                                        fit_circle=True, knn_num=3)
        else:
            ctx.extract_batch_dev(xy.data_ptr(), off.data_ptr(), cnt.data_ptr(), labels.data_ptr(), ncl.data_ptr(), 1, n, *args,
                                  fit_circle=True, knn_num=3)
        torch.cuda.synchronize()
        assert info.cpu().numpy().tolist() == [[ref["n"], ref["nk_pos"], ref["nk_neg"], 0]] and ref["n"] == 0
        k = kept.cpu().numpy()
        assert np.array_equal(k[:len(pos)], ref["kept_pos"]) and np.array_equal(k[len(pos):], ref["kept_neg"])
        r = rep.cpu().numpy()
        assert np.array_equal(r[:1], ref["rep_pos"]) and np.array_equal(r[len(pos):len(pos) + 2], ref["rep_neg"])
        assert tuple(pos[r[0]]) == (38.0, 30.0) and (38.0, 30.0) in {tuple(neg[i]) for i in r[len(pos):len(pos) + 2]}
