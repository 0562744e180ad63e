"""GPU: the calibration quality report (ecal_solver_report[_dev]: residual statistics per keyframe, per landmark, per sensor
cell and a histogram, binned on the GPU in one pass over the solver's records) against numpy float64 binning of the residuals
that Solver.residuals returns — existing code, one double per residual — by the rules stated in include/ecal.h.

Tolerances (f64; the project's stated bounds, tests/test_gpu_solver.py): a residual is known to 1e-11 absolute, a sum of n terms
added in another order to 1e-11 relative.  Per bin with n_b members:
    n, and the sums of n over every family                      exact
    max_abs                                                     1e-11 absolute
    sum_abs, sum_r      1e-11 * sum|r| + n_b * 1e-11
    sum_r2              1e-11 * sum r^2 + 2e-11 * sum|r|
    cost                1e-11 relative of Solver.evaluate(y, False)[0]
    n_out, hist         threshold decisions on a value known to 1e-11: per bin, as many may differ as reference residuals lie within
                        1e-11 of the threshold / of one of the bin's edges; that slack, summed, must stay below 0.1 % of the residuals
                        for the test to say anything (on these continuous random inputs it is 0).
"""
import functools

import numpy as np
import pytest

import synth_solver as SV

pytestmark = pytest.mark.gpu

TOL = 1e-11


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    c = eventcalib_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _problem(n_res, n_cp, n_segments=1, use_so3=False, fisheye=False):
    """(problem, perturbed parameters): residuals on the Huber tail, as tests/test_gpu_solver.py:31.  Made once per case."""
    prob, x = SV.make_problem(n_res, n_cp=n_cp, seed=n_res + n_cp, pixel_noise=0.5, n_segments=n_segments, use_so3=use_so3, fisheye=fisheye)
    y = SV.perturb(x, n_cp * n_segments, np.random.default_rng(n_res), intr_rel=0.01, rot=0.005, trans=0.2)
    return prob, y


def _kf_4ms(prob):
    t = prob["time"]
    return np.arange(t.min() + 2e-3, t.max() + 4e-3, 4e-3)


def _keyframe_of(kf, t):
    """the association's rule (ecal_associate.hip:40-51): first index with kf >= t against its predecessor, ties to the predecessor"""
    K = len(kf)
    a = np.searchsorted(kf, t, side="left")
    k = np.minimum(a, K - 1)
    mid = (a > 0) & (a < K)
    d0 = t[mid] - kf[a[mid] - 1]
    d1 = kf[a[mid]] - t[mid]
    k[mid] = np.where(d0 * d0 <= d1 * d1, a[mid] - 1, a[mid])
    return k


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


def _check_report(s, prob, y, kf_time, **options):
    """one report with every family on, against the numpy binning; returns the report"""
    r = s.residuals(y, with_jacobian=False)[0]
    n_res = len(r)
    rep = s.report(y, kf_time, **options)
    o = rep["options"]
    thresh = o.outlier_thresh if o.outlier_thresh > 0 else prob["huber_a"]
    zero = np.zeros(n_res, np.int64)
    # totals
    tot = _bin_stats(zero, 1, r, thresh)
    assert 1000 * tot["slack_out"][0] <= n_res          # (the test's own validity, see the module's docstring)
    got_tot = {k: np.array([rep["totals"]["all"][k]]) for k in ("n", "n_out", "sum_r", "sum_r2", "sum_abs", "max_abs")}
    _check_bins("totals", got_tot, tot)
    cost = s.evaluate(y, False)[0]
    print("cost %.17g evaluate %.17g" % (rep["cost"], cost))
    assert abs(rep["cost"] - cost) <= TOL * abs(cost)
    # per keyframe, per landmark
    K = len(kf_time)
    _check_bins("keyframes", rep["kf"], _bin_stats(_keyframe_of(np.asarray(kf_time, np.float64), prob["time"]), K, r, thresh))
    n_lm = len(prob["landmarks"])
    _check_bins("landmarks", rep["lm"], _bin_stats(prob["lm_id"].astype(np.int64), n_lm, r, thresh))
    # coverage
    cy, cx = rep["cell_n"].shape
    assert (cy, cx) == (-(-o.height // o.cell_px), -(-o.width // o.cell_px))
    px = np.maximum(prob["obs"], 0.0).astype(np.uint32) // o.cell_px
    cell = np.minimum(px[:, 1], cy - 1).astype(np.int64) * cx + np.minimum(px[:, 0], cx - 1)
    ref_n = np.bincount(cell, minlength=cy * cx)
    ref_s = np.bincount(cell, weights=r * r, minlength=cy * cx)
    ref_a = np.bincount(cell, weights=np.abs(r), minlength=cy * cx)
    assert np.array_equal(rep["cell_n"].ravel().astype(np.int64), ref_n)
    assert (np.abs(rep["cell_sum_r2"].ravel() - ref_s) <= TOL * ref_s + 2 * TOL * ref_a).all()
    assert rep["empty_cell_frac"] == (ref_n == 0).mean()
    # histogram: the bins' edges in units of the bin width, the first and last bin open-ended
    bins = o.hist_bins
    hr = o.hist_range if o.hist_range > 0 else 4.0 * prob["huber_a"]
    pos = (r + hr) * bins / (2 * hr)
    ref_h = np.bincount(np.clip(np.floor(pos), 0, bins - 1).astype(np.int64), minlength=bins)
    edges = np.arange(1, bins) * (2 * hr / bins) - hr                      # the inner edges, in residual units
    near = np.abs(r[:, None] - edges[None, :]) <= TOL if bins > 1 else np.zeros((n_res, 0), bool)
    edge_cnt = np.concatenate([[0], near.sum(axis=0), [0]])                # residuals near edge j = the border of bins j - 1 and j
    slack_h = edge_cnt[:-1] + edge_cnt[1:]
    assert 1000 * slack_h.sum() <= n_res
    assert (np.abs(rep["hist"].astype(np.int64) - ref_h) <= slack_h).all()
    # every residual lands in exactly one bin of every family
    assert int(rep["totals"]["all"]["n"]) == n_res == s.n_res
    for fam in (rep["kf"]["n"], rep["lm"]["n"], rep["cell_n"], rep["hist"]):
        assert int(fam.sum()) == n_res
    # derived figures
    assert abs(rep["rms"] - np.sqrt((r * r).mean())) <= 1e-9 * rep["rms"] and abs(rep["outlier_frac"] - tot["n_out"][0] / n_res) <= 1e-12
    # a second call gives the same counts: the call zeroes its outputs itself
    rep2 = s.report(y, kf_time, **options)
    for key in ("kf", "lm"):
        assert np.array_equal(rep2[key]["n"], rep[key]["n"]) and np.array_equal(rep2[key]["n_out"], rep[key]["n_out"])
    assert np.array_equal(rep2["cell_n"], rep["cell_n"]) and np.array_equal(rep2["hist"], rep["hist"])
    assert rep2["totals"]["all"]["n"] == rep["totals"]["all"]["n"]
    return rep


@pytest.mark.parametrize("n_res,n_cp,kw", [
    (2500, 7, {}),                       # many chunks, several keyframes per chunk
    (40000, 4, {}),                      # ONE span cut at the 16384-residual chunk limit: several workgroups add into the same keyframes
    (1200, 6, {"n_segments": 2}),
    (1, 4, {}),
    (600, 6, {"use_so3": True}),
    (600, 6, {"fisheye": True}),
])
def test_report_matches_numpy_binning(ctx, n_res, n_cp, kw):
    from eventcalib_amd.capi import Solver
    prob, y = _problem(n_res, n_cp, **kw)
    s = Solver(ctx, prob)
    if n_res == 40000:
        assert s.n_chunks > n_cp - 3
    _check_report(s, prob, y, _kf_4ms(prob))
    s.close()


@pytest.mark.parametrize("table", ["single", "dense", "ends"])
def test_keyframe_tables(ctx, table):
    from eventcalib_amd.capi import Solver
    prob, y = _problem(2500, 7)
    t0, t1 = prob["time"].min(), prob["time"].max()
    kf = {"single": np.array([0.5 * (t0 + t1)]),
          "dense": np.linspace(t0 - 0.1, t1 + 0.1, 4000),                          # more keyframes than residuals: a chunk meets hundreds
          "ends": np.array([t0 - 0.3, t0 - 0.2, t0 - 0.1, t1 + 0.1])}[table]     # every residual between the last two
    s = Solver(ctx, prob)
    rep = _check_report(s, prob, y, kf)
    if table == "ends":
        assert rep["kf"]["n"][:2].sum() == 0 and rep["kf"]["n"][2:].sum() == 2500 and (rep["kf"]["n"][2:] > 0).all()
    s.close()


def test_keyframe_tie_goes_to_the_predecessor(ctx):
    """keyframes at 5.0 and 5.25 and residuals at exactly 5.125 (binary fractions: both distances are 0.125): d0 * d0 <= d1 * d1"""
    from eventcalib_amd.capi import Solver
    prob, y = _problem(2500, 7)
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


@pytest.mark.parametrize("case", ["crop_1px", "clamped_obs"])
def test_coverage_clamps(ctx, case):
    from eventcalib_amd.capi import Solver
    prob, y = _problem(2500, 7)
    if case == "crop_1px":               # a 64 x 64 crop in 1-pixel cells: what lies beyond it counts in the last column / row
        s = Solver(ctx, prob)
        rep = _check_report(s, prob, y, _kf_4ms(prob), width=64, height=64, cell_px=1)
        assert rep["cell_n"].shape == (64, 64)
    else:                                # observations left of / above the sensor and beyond its far edges
        obs = prob["obs"].copy()
        obs[:7, 0] = [-3.5, -0.25, 346.0, 400.75, 345.999, 0.0, 420.0]
        obs[7:12, 1] = [-1.0, 260.0, 259.5, 300.0, -1e-9]
        prob = dict(prob, obs=obs)
        s = Solver(ctx, prob)
        rep = _check_report(s, prob, y, _kf_4ms(prob))        # 346 x 260 in 16-pixel cells: 22 x 17, the last column and row partial
        assert rep["cell_n"].shape == (17, 22)
    s.close()


def test_options_histogram_and_threshold(ctx):
    from eventcalib_amd.capi import Solver
    prob, y = _problem(2500, 7)
    s = Solver(ctx, prob)
    _check_report(s, prob, y, _kf_4ms(prob), hist_bins=1)
    _check_report(s, prob, y, _kf_4ms(prob), hist_bins=256, hist_range=0.05, outlier_thresh=0.01)   # most residuals in the tail bins
    s.close()


def test_invalid_arguments_and_empty_solver(ctx):
    from eventcalib_amd.capi import EcalError, Solver
    prob, y = _problem(600, 6, use_so3=True)
    s = Solver(ctx, prob)
    kf = _kf_4ms(prob)
    for bad in (dict(cell_px=0), dict(width=1000, height=1000, cell_px=8), dict(hist_bins=0), dict(hist_bins=257)):
        with pytest.raises(EcalError) as e:
            s.report(y, kf, **bad)
        assert e.value.status == -1, bad
    with pytest.raises(EcalError) as e:
        s.report(y, np.zeros(0))                       # a keyframe output without keyframes
    assert e.value.status == -1
    assert s.report(y, kf, width=1280, height=720)["cell_n"].shape == (45, 80)     # 3600 cells
    # the refused options belong to families that are not asked for: fine
    assert int(s.report(y, None, families=("lm",), cell_px=0, hist_bins=0)["lm"]["n"].sum()) == 600
    s.close()
    empty = dict(prob, obs=prob["obs"][:0], time=prob["time"][:0], lm_id=prob["lm_id"][:0])
    s = Solver(ctx, empty)
    rep = s.report(y, kf)
    assert rep["totals"]["all"]["n"] == 0 and rep["cost"] == 0.0 and rep["totals"]["all"]["max_abs"] == 0.0
    assert not rep["kf"]["n"].any() and not rep["lm"]["n"].any() and not rep["cell_n"].any() and not rep["hist"].any()
    assert rep["empty_cell_frac"] == 1.0
    s.close()


def test_null_families_touch_no_memory(ctx):
    """report_dev with output families left out: one arena filled with a canary, the outputs carved out of it side by side —
    only what was asked for is written"""
    import torch
    from eventcalib_amd import capi
    from eventcalib_amd.capi import Solver
    prob, y = _problem(2500, 7)
    s = Solver(ctx, prob)
    kf = _kf_4ms(prob)
    K, n_lm, bins = len(kf), s.n_landmarks, 64
    o = s.report_options()
    n_cells = 22 * 17
    full = s.report(y, kf)
    sizes = dict(total=7, kf=6 * K, lm=6 * n_lm, cell_n=n_cells, cell_s=n_cells, hist=bins)
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
        s.report_dev(d_y.data_ptr(), d_kf.data_ptr(), K, o, p("total"), p("kf"), p("lm"), p("cell_n"), p("cell_s"), p("hist"),
                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        host = arena.cpu().numpy()
        written = np.zeros(at, bool)
        for name in asked + ("total",):
            written[off[name]: off[name] + sizes[name]] = True
        assert (host[~written] == canary).all(), asked
        assert not (host[written] == canary).any(), asked
        tot = host[off["total"]: off["total"] + 7].view(capi.REPORT_TOTALS)[0]
        assert tot["all"]["n"] == 2500 and abs(tot["cost"] - full["cost"]) <= TOL * full["cost"]
        if "hist" in asked:
            assert np.array_equal(host[off["hist"]: off["hist"] + bins].view(np.uint64), full["hist"])
        if "kf" in asked:
            assert np.array_equal(host[off["kf"]: off["kf"] + 6 * K].view(capi.BIN_STATS)["n"], full["kf"]["n"])
            assert np.array_equal(host[off["cell_n"]: off["cell_n"] + n_cells].view(np.uint64), full["cell_n"].ravel())
        if "lm" in asked:
            assert np.array_equal(host[off["lm"]: off["lm"] + 6 * n_lm].view(capi.BIN_STATS)["n"], full["lm"]["n"])
    s.close()
