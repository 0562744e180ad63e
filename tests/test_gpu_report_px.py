"""GPU: the report in pixels (include/ecal.h, "report in pixels": ecal_residuals_px[_dev], ecal_solver_report_px[_dev]) through
the C ABI via capi.

Per-event form.  r_px = r / |d r / d (u, v)| against r / hypot(J[:, 2], J[:, 3]) of Solver.residuals(y, True), existing code.
The project's stated bounds (tests/test_gpu_solver.py): r is known to 1e-11 absolute, a Jacobian row to 1e-11 of its largest
entry j_max.  With |g| = hypot(J2, J3):  d r_px <= d r / |g| + |r| d|g| / |g|^2 = 1e-11 / |g| + |r_px| * 1e-11 * j_max / |g|.
The degenerate flags and their count are exact.

Report.  Against numpy float64 binning of what Solver.residuals_px returns, by the method and with the tolerance forms of
tests/test_gpu_report.py (TOL = 1e-11; the two kernels evaluate one sequence of operations and can differ by the contraction
choices of two compilations, a few ulp of intermediates of size ~70 carried through 1 / |g| ~ 5: ~1e-13):
    n, n_degenerate, and the sums of n over every family        exact
    max_abs                                                     TOL absolute
    sum_abs, sum_r      TOL * sum|r| + n_b * TOL
    sum_r2              TOL * sum r^2 + 2 TOL * sum|r|
    sum_px_per_unit     TOL relative
    n_out, hist         per bin as many may differ as reference values lie within TOL of the threshold / of one of the bin's
                        edges; that slack, summed, must stay below 0.1 % of the residuals (the test's own precondition).

Known answer.  At the ground truth with pixel noise sigma the distance of an event to the projected rim IS the noise's component
across the rim: rms_px = sigma within 5 / sqrt(2 n) (five standard deviations of an RMS of n normal samples) + sigma / rho (the
curvature term: the rim is a closed curve of radius rho ~ 9.5 px, not a line), relative.
"""
import functools

import numpy as np
import pytest

import synth_solver as SV

pytestmark = pytest.mark.gpu

TOL = 1e-11
NE_T = 256          # threads per workgroup (ecal_solver_state.hpp)
RHO_PX = 9.5        # the projected rim radius on these problems, pixels


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    c = eventcalib_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _problem(n_res, n_cp, n_segments=1, use_so3=False, fisheye=False):
    """(problem, ground truth, perturbed parameters).  Made once per case."""
    prob, x = SV.make_problem(n_res, n_cp=n_cp, seed=n_res + n_cp, pixel_noise=0.5, n_segments=n_segments, use_so3=use_so3, fisheye=fisheye)
    y = SV.perturb(x, n_cp * n_segments, np.random.default_rng(n_res), intr_rel=0.01, rot=0.005, trans=0.2)
    return prob, x, y


def _kf_4ms(prob):
    t = prob["time"]
    return np.arange(t.min() + 2e-3, t.max() + 4e-3, 4e-3)


def _keyframe_of(kf, t):
    """the association's rule: first index with kf >= t against its predecessor, ties to the predecessor"""
    K = len(kf)
    a = np.searchsorted(kf, t, side="left")
    k = np.minimum(a, K - 1)
    mid = (a > 0) & (a < K)
    d0 = t[mid] - kf[a[mid] - 1]
    d1 = kf[a[mid]] - t[mid]
    k[mid] = np.where(d0 * d0 <= d1 * d1, a[mid] - 1, a[mid])
    return k


def _keyframes_per_chunk(prob, kf):
    """how many keyframes of the table the records of each chunk (= each knot span of the one segment) lie across"""
    t = prob["time"]
    span = np.searchsorted(prob["knots"], t, side="right") - 1
    k = _keyframe_of(np.asarray(kf, np.float64), t)
    return np.array([k[span == sp].max() - k[span == sp].min() + 1 for sp in np.unique(span)])


def _check_per_event(s, y):
    """residuals_px against r / hypot(J2, J3) of the existing per-residual seam; returns (r_px, grad, flag)"""
    r, J, _ = s.residuals(y, True)
    r_px, g, flag = s.residuals_px(y, with_gradient=True)
    assert r_px.shape == r.shape and g.shape == (len(r), 2) and flag.dtype == np.uint8
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g2 = J[:, 2] * J[:, 2] + J[:, 3] * J[:, 3]
        ref_deg = ~np.isfinite(r) | ~np.isfinite(g2) | ~(g2 > 0)
        ok = ~ref_deg
        norm = np.hypot(J[ok, 2], J[ok, 3])
        ref = r[ok] / norm
        j_max = np.abs(J[ok]).max(axis=1)
    assert np.array_equal(flag, ref_deg.astype(np.uint8))
    assert (r_px[ref_deg] == 0.0).all()
    bound = TOL / norm + np.abs(ref) * TOL * j_max / norm
    err = np.abs(r_px[ok] - ref)
    print("per event: n %d degenerate %d, max |r_px - ref| %.3g, worst err / bound %.3g, |g| in [%.3g, %.3g]" % (
        len(r), int(ref_deg.sum()), err.max(initial=0.0), (err / bound).max(initial=0.0), norm.min(initial=np.inf), norm.max(initial=0.0)))
    assert (err <= bound).all()
    # the gradient is minus the (cx, cy) columns, to the Jacobian's own bound
    assert (np.abs(g[ok] + J[ok, 2:4]) <= TOL * j_max[:, None]).all()
    # the per-event form without the optional outputs gives the same values
    assert np.array_equal(s.residuals_px(y)[0], r_px)
    return r_px, g, flag


def _bin_stats(idx, n_bins, r, thresh):
    a = np.abs(r)
    out = {"n": np.bincount(idx, minlength=n_bins), "n_out": np.bincount(idx, weights=(a > thresh), minlength=n_bins),
           "sum_r": np.bincount(idx, weights=r, minlength=n_bins), "sum_r2": np.bincount(idx, weights=r * r, minlength=n_bins),
           "sum_abs": np.bincount(idx, weights=a, minlength=n_bins), "max_abs": np.zeros(n_bins),
           "slack_out": np.bincount(idx, weights=(np.abs(a - thresh) <= TOL), minlength=n_bins)}
    np.maximum.at(out["max_abs"], idx, a)
    return out


def _check_bins(name, got, ref):
    print("%s: bins %d, non-empty %d, max |d sum_r2| %.3g, max |d max_abs| %.3g" % (
        name, len(ref["n"]), int((ref["n"] > 0).sum()), np.abs(got["sum_r2"] - ref["sum_r2"]).max(initial=0.0),
        np.abs(got["max_abs"] - ref["max_abs"]).max(initial=0.0)))
    assert np.array_equal(got["n"].astype(np.int64), ref["n"].astype(np.int64)), name
    n = ref["n"].astype(np.float64)
    assert (np.abs(got["max_abs"] - ref["max_abs"]) <= TOL).all(), name
    assert (np.abs(got["sum_abs"] - ref["sum_abs"]) <= TOL * ref["sum_abs"] + n * TOL).all(), name
    assert (np.abs(got["sum_r"] - ref["sum_r"]) <= TOL * ref["sum_abs"] + n * TOL).all(), name
    assert (np.abs(got["sum_r2"] - ref["sum_r2"]) <= TOL * ref["sum_r2"] + 2 * TOL * ref["sum_abs"]).all(), name
    assert (np.abs(got["n_out"].astype(np.int64) - ref["n_out"].astype(np.int64)) <= ref["slack_out"]).all(), name


def _check_report(s, prob, y, kf_time, per_event=None, **options):
    """one pixel report with every family on, against the numpy binning of residuals_px; returns the report"""
    r_all, g_all, flag = per_event if per_event is not None else s.residuals_px(y, with_gradient=True)
    n_res = len(r_all)
    ok = flag == 0
    r, g = r_all[ok], g_all[ok]
    n_ok = len(r)
    rep = s.report_px(y, kf_time, **options)
    o = rep["options"]
    thresh = o.outlier_thresh if o.outlier_thresh > 0 else 1.0
    tot = _bin_stats(np.zeros(n_ok, np.int64), 1, r, thresh)
    assert 1000 * tot["slack_out"][0] <= n_res          # (the test's own validity, see the module's docstring)
    got_tot = {k: np.array([rep["totals"]["all"][k]]) for k in ("n", "n_out", "sum_r", "sum_r2", "sum_abs", "max_abs")}
    _check_bins("totals", got_tot, tot)
    assert rep["n_degenerate"] == int((~ok).sum()) == int(rep["totals"]["n_degenerate"])
    assert int(rep["totals"]["all"]["n"]) + rep["n_degenerate"] == n_res == s.n_res
    ppu = (1.0 / np.hypot(g[:, 0], g[:, 1])).sum()
    print("sum_px_per_unit %.17g numpy %.17g; px_per_unit %.6g rms_px %.6g" % (rep["totals"]["sum_px_per_unit"], ppu, rep["px_per_unit"], rep["rms_px"]))
    assert abs(rep["totals"]["sum_px_per_unit"] - ppu) <= TOL * ppu
    # per keyframe, per landmark
    K = len(kf_time)
    _check_bins("keyframes", rep["kf"], _bin_stats(_keyframe_of(np.asarray(kf_time, np.float64), prob["time"][ok]), K, r, thresh))
    n_lm = len(prob["landmarks"])
    _check_bins("landmarks", rep["lm"], _bin_stats(prob["lm_id"][ok].astype(np.int64), n_lm, r, thresh))
    # coverage
    cy, cx = rep["cell_n"].shape
    assert (cy, cx) == (-(-o.height // o.cell_px), -(-o.width // o.cell_px))
    px = np.maximum(prob["obs"][ok], 0.0).astype(np.uint32) // o.cell_px
    cell = np.minimum(px[:, 1], cy - 1).astype(np.int64) * cx + np.minimum(px[:, 0], cx - 1)
    ref_n = np.bincount(cell, minlength=cy * cx)
    ref_s = np.bincount(cell, weights=r * r, minlength=cy * cx)
    ref_a = np.bincount(cell, weights=np.abs(r), minlength=cy * cx)
    assert np.array_equal(rep["cell_n"].ravel().astype(np.int64), ref_n)
    assert (np.abs(rep["cell_sum_r2"].ravel() - ref_s) <= TOL * ref_s + 2 * TOL * ref_a).all()
    assert rep["empty_cell_frac"] == (ref_n == 0).mean()
    # histogram: the bins' edges in units of the bin width, the first and last bin open-ended
    bins = o.hist_bins
    hr = o.hist_range if o.hist_range > 0 else 4.0
    assert rep["hist_edges"][-1] == hr
    pos = (r + hr) * bins / (2 * hr)
    ref_h = np.bincount(np.clip(np.floor(pos), 0, bins - 1).astype(np.int64), minlength=bins)
    edges = np.arange(1, bins) * (2 * hr / bins) - hr                      # the inner edges, in pixels
    near = np.abs(r[:, None] - edges[None, :]) <= TOL if bins > 1 else np.zeros((n_ok, 0), bool)
    edge_cnt = np.concatenate([[0], near.sum(axis=0), [0]])                # values near edge j = the border of bins j - 1 and j
    slack_h = edge_cnt[:-1] + edge_cnt[1:]
    assert 1000 * slack_h.sum() <= n_res
    assert (np.abs(rep["hist"].astype(np.int64) - ref_h) <= slack_h).all()
    # every record with a distance lands in exactly one bin of every family
    for fam in (rep["kf"]["n"], rep["lm"]["n"], rep["cell_n"], rep["hist"]):
        assert int(fam.sum()) == n_ok
    # derived figures
    if n_ok:
        assert abs(rep["rms_px"] - np.sqrt((r * r).mean())) <= 1e-9 * rep["rms_px"] and rep["rms"] == rep["rms_px"]
        assert abs(rep["px_per_unit"] - ppu / n_ok) <= 1e-9 * rep["px_per_unit"]
        assert abs(rep["outlier_frac"] - tot["n_out"][0] / n_ok) <= 1e-12 + tot["slack_out"][0] / n_ok
    assert "cost" not in rep
    # a second call gives the same counts: the call zeroes its outputs itself
    rep2 = s.report_px(y, kf_time, **options)
    for key in ("kf", "lm"):
        assert np.array_equal(rep2[key]["n"], rep[key]["n"]) and np.array_equal(rep2[key]["n_out"], rep[key]["n_out"])
    assert np.array_equal(rep2["cell_n"], rep["cell_n"]) and np.array_equal(rep2["hist"], rep["hist"])
    assert rep2["totals"]["all"]["n"] == rep["totals"]["all"]["n"] and rep2["n_degenerate"] == rep["n_degenerate"]
    return rep


@pytest.mark.parametrize("n_res,n_cp,kw", [
    (1, 4, {}),
    (NE_T - 1, 4, {}),                   # one chunk of one span: the workgroup's last thread idle,
    (NE_T, 4, {}),                       # every thread one record,
    (NE_T + 1, 4, {}),                   # thread 0 a second one
    (2500, 7, {}),                       # four chunks, several keyframes per chunk
    (20000, 4, {}),                      # ONE span cut at the 16384-record chunk limit: two workgroups add into the same keyframes
    (1200, 6, {"n_segments": 2}),
    (600, 6, {"use_so3": True}),
    (600, 6, {"fisheye": True}),
    (600, 6, {"use_so3": True, "fisheye": True}),
])
def test_per_event_and_report_match_the_existing_seam(ctx, n_res, n_cp, kw):
    from eventcalib_amd.capi import Solver
    prob, _, y = _problem(n_res, n_cp, **kw)
    s = Solver(ctx, prob)
    if n_res == 20000:
        assert s.n_chunks == 2
    elif n_cp == 4:
        assert s.n_chunks == 1
    per_event = _check_per_event(s, y)
    assert not per_event[2].any()
    _check_report(s, prob, y, _kf_4ms(prob), per_event=per_event)
    s.close()


def test_degenerate_records_are_counted_and_enter_no_bin(ctx):
    """observations that are not numbers: r is NaN, the record is flagged, counted in n_degenerate and binned nowhere"""
    from eventcalib_amd.capi import Solver
    prob, _, y = _problem(2500, 7)
    obs = prob["obs"].copy()
    bad = np.array([0, 3, 255, 256, 1000, 2499])
    obs[bad[:3], 0] = np.nan
    obs[bad[3:], 1] = np.nan
    prob = dict(prob, obs=obs)
    s = Solver(ctx, prob)
    per_event = _check_per_event(s, y)
    assert np.array_equal(np.flatnonzero(per_event[2]), bad)
    rep = _check_report(s, prob, y, _kf_4ms(prob), per_event=per_event)
    assert rep["n_degenerate"] == len(bad)
    s.close()


@pytest.mark.parametrize("table", ["single", "dense", "ends"])
def test_keyframe_tables(ctx, table):
    """4 ms tables (above) stage a chunk's keyframes in LDS; `dense` makes one chunk meet hundreds — more than RP_KF_LDS = 64 —
    and takes the unstaged global path"""
    from eventcalib_amd.capi import Solver
    prob, _, y = _problem(2500, 7)
    t0, t1 = prob["time"].min(), prob["time"].max()
    kf = {"single": np.array([0.5 * (t0 + t1)]),
          "dense": np.linspace(t0 - 0.1, t1 + 0.1, 4000),
          "ends": np.array([t0 - 0.3, t0 - 0.2, t0 - 0.1, t1 + 0.1])}[table]
    s = Solver(ctx, prob)
    rep = _check_report(s, prob, y, kf)
    if table == "dense":
        assert _keyframes_per_chunk(prob, kf).min() > 64 + 2
    if table == "ends":
        assert rep["kf"]["n"][:2].sum() == 0 and rep["kf"]["n"][2:].sum() == 2500 and (rep["kf"]["n"][2:] > 0).all()
    s.close()


def test_keyframe_tie_goes_to_the_predecessor(ctx):
    from eventcalib_amd.capi import Solver
    prob, _, y = _problem(2500, 7)
    t = prob["time"].copy()
    tie = (t >= 5.12) & (t <= 5.13)
    assert tie.sum() >= 10
    t[tie] = 5.125                                   # (a run of equal times: still sorted)
    prob = dict(prob, time=t)
    kf = np.array([5.0, 5.25, 5.5])
    assert (_keyframe_of(kf, t[tie]) == 0).all()
    s = Solver(ctx, prob)
    rep = _check_report(s, prob, y, kf)
    assert rep["kf"]["n"][0] == (t <= 5.125).sum()
    s.close()


def test_options_and_families(ctx):
    """other options; every family alone gives what it gives with all together; a value <= 0 means the pixel defaults"""
    from eventcalib_amd.capi import Solver
    prob, _, y = _problem(2500, 7)
    s = Solver(ctx, prob)
    kf = _kf_4ms(prob)
    per_event = s.residuals_px(y, with_gradient=True)
    assert _keyframes_per_chunk(prob, kf).max() <= 64 - 2          # every chunk stages its keyframes in LDS (RP_KF_LDS)
    full = _check_report(s, prob, y, kf, per_event=per_event)
    o = full["options"]
    assert (o.width, o.height, o.cell_px, o.hist_bins, o.hist_range, o.outlier_thresh) == (346, 260, 16, 64, 4.0, 1.0)
    _check_report(s, prob, y, kf, per_event=per_event, hist_bins=1)
    _check_report(s, prob, y, kf, per_event=per_event, hist_bins=256, hist_range=0.5, outlier_thresh=0.25, width=64, height=64, cell_px=1)
    zero = s.report_px(y, kf, hist_range=0.0, outlier_thresh=-1.0)
    assert np.array_equal(zero["hist"], full["hist"]) and zero["totals"]["all"]["n_out"] == full["totals"]["all"]["n_out"]
    assert zero["hist_edges"][-1] == 4.0
    for fam, keys in (("kf", ("kf",)), ("lm", ("lm",)), ("cells", ("cell_n", "cell_sum_r2")), ("hist", ("hist",))):
        one = s.report_px(y, kf, families=(fam,))
        assert set(one) & {"kf", "lm", "cell_n", "cell_sum_r2", "hist"} == set(keys), fam
        assert one["totals"]["all"]["n"] == 2500 and one["totals"]["all"]["n_out"] == full["totals"]["all"]["n_out"]
        assert abs(one["totals"]["sum_px_per_unit"] - full["totals"]["sum_px_per_unit"]) <= TOL * full["totals"]["sum_px_per_unit"]
        for key in keys:
            a, b = one[key], full[key]
            if a.dtype.names:
                assert np.array_equal(a["n"], b["n"]) and np.array_equal(a["n_out"], b["n_out"]), key
                assert (np.abs(a["sum_r2"] - b["sum_r2"]) <= TOL * b["sum_r2"] + 2 * TOL * b["sum_abs"]).all(), key
                assert (np.abs(a["max_abs"] - b["max_abs"]) <= TOL).all(), key
            elif a.dtype == np.uint64:
                assert np.array_equal(a, b), key
            else:                                     # (cell_sum_r2 has no sum|r| beside it: sum|r| <= sqrt(n sum r^2))
                assert (np.abs(a - b) <= TOL * b + 2 * TOL * np.sqrt(b * full["cell_n"])).all(), key
    none = s.report_px(y, None, families=())
    assert none["totals"]["all"]["n"] == 2500 and not set(none) & {"kf", "lm", "cell_n", "hist"}
    s.close()


def test_null_families_touch_no_memory(ctx):
    """report_px_dev with output families left out: one arena filled with a canary, the outputs carved out of it side by side —
    only what was asked for is written"""
    import torch
    from eventcalib_amd import capi
    from eventcalib_amd.capi import Solver
    prob, _, y = _problem(2500, 7)
    s = Solver(ctx, prob)
    kf = _kf_4ms(prob)
    K, n_lm, bins = len(kf), s.n_landmarks, 64
    o = s.report_px_options()
    n_cells = 22 * 17
    full = s.report_px(y, kf)
    sizes = dict(total=8, kf=6 * K, lm=6 * n_lm, cell_n=n_cells, cell_s=n_cells, hist=bins)
    assert capi.REPORT_PX_TOTALS.itemsize == 64
    off, at = {}, 3
    for name, w in sizes.items():
        off[name] = at
        at += w + 3                                   # three canary words between neighbours and at both ends
    canary = -7.25e77
    d_y = torch.as_tensor(y, device="cuda")
    d_kf = torch.as_tensor(kf, device="cuda")
    for asked in (("hist",), ("kf", "cell_n"), ("lm", "cell_s"), ()):
        arena = torch.full((at,), canary, dtype=torch.float64, device="cuda")

        def p(name):
            return arena.data_ptr() + 8 * off[name] if name in asked or name == "total" else None
        s.report_px_dev(d_y.data_ptr(), d_kf.data_ptr(), K, o, p("total"), p("kf"), p("lm"), p("cell_n"), p("cell_s"), p("hist"),
                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        host = arena.cpu().numpy()
        written = np.zeros(at, bool)
        for name in asked + ("total",):
            written[off[name]: off[name] + sizes[name]] = True
        assert (host[~written] == canary).all(), asked
        assert not (host[written] == canary).any(), asked
        tot = host[off["total"]: off["total"] + 8].view(capi.REPORT_PX_TOTALS)[0]
        assert tot["all"]["n"] == 2500 and tot["n_degenerate"] == 0
        assert abs(tot["sum_px_per_unit"] - full["totals"]["sum_px_per_unit"]) <= TOL * full["totals"]["sum_px_per_unit"]
        if "hist" in asked:
            assert np.array_equal(host[off["hist"]: off["hist"] + bins].view(np.uint64), full["hist"])
        if "kf" in asked:
            assert np.array_equal(host[off["kf"]: off["kf"] + 6 * K].view(capi.BIN_STATS)["n"], full["kf"]["n"])
            assert np.array_equal(host[off["cell_n"]: off["cell_n"] + n_cells].view(np.uint64), full["cell_n"].ravel())
        if "lm" in asked:
            assert np.array_equal(host[off["lm"]: off["lm"] + 6 * n_lm].view(capi.BIN_STATS)["n"], full["lm"]["n"])
    s.close()


def test_known_answer_pixel_noise(ctx):
    """pixel_noise = 0.5 at the ground-truth vector, n = 20 000: the report says 0.5 px; the board-unit report of the same
    call does not"""
    from eventcalib_amd.capi import Solver
    n, sigma = 20000, 0.5
    prob, x, _ = _problem(n, 4)
    s = Solver(ctx, prob)
    rep = s.report_px(x, _kf_4ms(prob))
    board = s.report(x, _kf_4ms(prob))
    margin = 5.0 / np.sqrt(2 * n) + sigma / RHO_PX
    print("rms_px %.6f (sigma %.3f, relative margin %.4f), board-unit rms %.6f, px_per_unit %.6f, n_degenerate %d" % (
        rep["rms_px"], sigma, margin, board["rms"], rep["px_per_unit"], rep["n_degenerate"]))
    assert rep["n_degenerate"] == 0 and int(rep["totals"]["all"]["n"]) == n
    assert abs(rep["rms_px"] - sigma) <= margin * sigma
    s.close()


def test_invalid_arguments_and_empty_solver(ctx):
    """the error codes of the board-unit call for the same mistakes; a solver without residuals gives zeros"""
    from eventcalib_amd.capi import EcalError, Solver
    prob, _, y = _problem(600, 6, use_so3=True)
    s = Solver(ctx, prob)
    kf = _kf_4ms(prob)

    def status(call, *a, **k):
        try:
            call(*a, **k)
        except EcalError as e:
            return e.status
        return 0
    for bad in (dict(cell_px=0), dict(width=1000, height=1000, cell_px=8), dict(hist_bins=0), dict(hist_bins=257)):
        assert status(s.report_px, y, kf, **bad) == status(s.report, y, kf, **bad) == -1, bad
    assert status(s.report_px, y, np.zeros(0)) == status(s.report, y, np.zeros(0)) == -1      # a keyframe output without keyframes
    assert s.report_px(y, kf, width=1280, height=720)["cell_n"].shape == (45, 80)     # 3600 cells
    # the refused options belong to families that are not asked for: fine
    assert int(s.report_px(y, None, families=("lm",), cell_px=0, hist_bins=0)["lm"]["n"].sum()) == 600
    s.close()
    # more landmarks than the LDS bins hold: ECAL_ERR_RANGE from both, and only when the landmark family is asked for
    many = dict(prob, landmarks=np.concatenate([prob["landmarks"], np.zeros((1025 - len(prob["landmarks"]), 3))]))
    s = Solver(ctx, many)
    assert s.n_landmarks == 1025
    assert status(s.report_px, y, kf) == status(s.report, y, kf) != 0
    assert status(s.report_px, y, kf) not in (0, -1)
    assert int(s.report_px(y, kf, families=("kf", "cells", "hist"))["hist"].sum()) == 600
    s.close()
    empty = dict(prob, obs=prob["obs"][:0], time=prob["time"][:0], lm_id=prob["lm_id"][:0])
    s = Solver(ctx, empty)
    rep = s.report_px(y, kf)
    assert rep["totals"]["all"]["n"] == 0 and rep["n_degenerate"] == 0 and rep["totals"]["sum_px_per_unit"] == 0.0
    assert rep["totals"]["all"]["max_abs"] == 0.0
    assert not rep["kf"]["n"].any() and not rep["lm"]["n"].any() and not rep["cell_n"].any() and not rep["hist"].any()
    assert rep["empty_cell_frac"] == 1.0
    r_px, g, flag = s.residuals_px(y, with_gradient=True)
    assert r_px.shape == (0,) and g.shape == (0, 2) and flag.shape == (0,)
    s.close()
