"""GPU: ecal_solver_uncertainty (the evaluation and the chunk scores on the device, arrow_covariance.hpp on the host) against numpy.

Dense oracle: H assembled densely from ecal_solver_evaluate's buffer, np.linalg.inv, the chunk scores summed in numpy from
ecal_residuals' rows (uncertainty_oracle.py); n_cp = 6 and 12, cluster_spans = 1, 2 and 1000 (one cluster: robust_valid = 0).
The bar is 100 n eps kappa_2 of the Jacobi-scaled H, applied in that scaled system (tests/cpp/check_covariance.cpp derives it):
  Sigma_ii, cov / s2      |error| / (d_i d_j) <= bar max |Hs^-1|
  cov_robust              |error| / (d_i d_j) <= G / (G - 1) sum_c ((2 bar + bar^2) B_c^2 + 2 B_c M |D e_c|_1),  B_c = M |D g_c|_1,
                          M = max |Hs^-1|, e_c the summation bound of the cluster's scores (test_gpu_chunk_scores.py): the product
                          rule on s_c s_c^T with s_c = P g_c, for the error of P and for that of g_c.
Duplication: every record stored twice leaves cov_robust where it was and takes Sigma_ii to one half, cov to 1/2 s2' / s2 — the
formal figure believes the second copy, the robust one does not.  Held to the same bars (measured: 1e-16 and 7e-7 of them).
Monte Carlo: one noise-free problem (1024 residuals, n_cp = 8) and K = 256 seeded draws of iid pixel noise of 0.005 px (no residual
near the Huber corner, asserted), each solved from the truth: the mean of (x - truth)^T cov^-1 (x - truth) over the draws must lie
in 9 +- 4 sqrt(18 / K), the sampling band of the mean of a chi^2_9.  Seeds 1000 .. 1255; tests/ref_lm.py with the numpy covariance
gives MC_ORACLE_MEAN = 9.279 for them (tools/uncertainty_mc_oracle.py 1024 0.005 1000 reproduces it), inside the band (at 0.05 px the same seeds give 11.18 and a standard deviation of 8.4 where a
chi^2_9 has 4.24: the estimate is no longer linear in the noise there, which is not what this test is about).
A gap in time that leaves a control point without residuals: positive_definite = 0."""
import numpy as np
import pytest

import synth_solver as SV
import uncertainty_oracle as UO

pytestmark = pytest.mark.gpu
EPS = UO.EPS
MC_K, MC_SEED0, MC_SIGMA, MC_RES, MC_CP = 256, 1000, 0.005, 1024, 8
MC_ORACLE_MEAN = 9.279


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    with eventcalib_amd.Context(0) as c:
        yield c


def _scaled_err(a, b, d):
    return float((np.abs(a - b) / np.outer(d[:9], d[:9])).max())


class Oracle:
    """everything numpy of one (problem, x): dense H, its scaled condition, the chunk scores and their summation bound"""

    def __init__(self, ctx, prob, x):
        from eventcalib_amd import capi, uncertainty
        self.n_cp = int(prob["seg_cp_off"][-1])
        self.n_res = len(prob["time"])
        self.solver = capi.Solver(ctx, prob)
        self.x = x
        self.cost, _, self.H = capi.unpack_normal(self.solver.evaluate(x), self.n_cp)
        self.table = uncertainty.chunk_table(self.solver)
        terms, _, self.tail, _ = UO.record_terms(self.solver, x)
        self.score, mag, _ = UO.chunk_sums(terms, self.table)
        self.score_bound = (self.table[:, 1:2] + 33.0) * EPS * mag
        self.kappa, self.d = UO.scaled_condition(self.H)
        self.n = 9 + 6 * self.n_cp
        self.bar = 100.0 * self.n * EPS * self.kappa
        Hi = np.linalg.inv(self.H)
        self.M = float((np.abs(Hi) / np.outer(self.d, self.d)).max())

    def robust_limit(self, cluster_spans):
        ids = [(int(t[2]), (int(t[3]) - 3) // cluster_spans) for t in self.table]
        uniq = sorted(set(ids))
        G = len(uniq)
        g = UO.scatter(self.score, self.table, self.n_cp)
        e = UO.scatter(self.score_bound, self.table, self.n_cp)
        tot = 0.0
        for u in uniq:
            rows = [i for i, k in enumerate(ids) if k == u]
            B = self.M * float((np.abs(g[rows].sum(axis=0)) * self.d).sum())
            E = float((e[rows].sum(axis=0) * self.d).sum())
            tot += (2 * self.bar + self.bar ** 2) * B * B + 2 * B * self.M * E
        return G / (G - 1) * tot if G >= 2 else np.nan


def _check_against_oracle(o, u, cluster_spans, factor=1.0):
    ref = UO.covariance(o.cost, o.H, o.n_res, o.score, o.table, o.n_cp, cluster_spans)
    assert u["positive_definite"] and u["formal_valid"]
    assert u["n_res"] == o.n_res and u["n_unknowns"] == o.n and u["n_cp"] == o.n_cp and u["n_chunks"] == len(o.table)
    assert u["n_clusters"] == ref["n_clusters"]
    assert abs(u["cost"] - o.cost) <= 2 * (o.n_res + 33.0) * EPS * o.cost          # (two evaluations: the order of the atomics)
    assert abs(u["s2"] - ref["s2"]) <= 4 * (o.n_res + 33.0) * EPS * ref["s2"]
    lim = factor * o.bar * o.M
    e_sig = _scaled_err(u["cov"] / u["s2"], ref["Sii"], o.d)
    e_cov = _scaled_err(u["cov"], ref["cov"], o.d)
    print("n_cp %d cluster_spans %d: kappa %.3e bar %.3e | Sigma_ii %.3e of its limit, cov %.3e, G %d" % (
        o.n_cp, cluster_spans, o.kappa, o.bar, e_sig / lim, e_cov / (lim * ref["s2"]), u["n_clusters"]), end="")
    ds2 = 4 * (o.n_res + 33.0) * EPS                                               # (s2 of another evaluation, see above)
    assert e_sig <= lim and e_cov <= ref["s2"] * (lim + ds2 * o.M)
    assert np.abs(u["sigma"] / ref["sigma"] - 1).max() <= lim / (np.diag(ref["Sii"]) / o.d[:9] ** 2).min() + ds2
    assert np.array_equal(u["sigma"], np.sqrt(np.diag(u["cov"]))) and np.allclose(np.diag(u["corr"]), 1.0, rtol=0, atol=4 * EPS)
    assert np.array_equal(u["corr"], u["corr"].T) and np.abs(u["corr"]).max() <= 1 + 4 * EPS
    if ref["n_clusters"] >= 2:
        assert u["robust_valid"]
        r_lim = factor * o.robust_limit(cluster_spans)
        e_rob = _scaled_err(u["cov_robust"], ref["cov_robust"], o.d)
        print(", cov_robust %.3e of its limit; inflation %.3g .. %.3g" % (e_rob / r_lim, u["inflation"].min(), u["inflation"].max()))
        assert e_rob <= r_lim
        assert np.array_equal(u["sigma_robust"], np.sqrt(np.diag(u["cov_robust"])))
        assert np.array_equal(u["inflation"], u["sigma_robust"] / u["sigma"])
    else:
        print(", one cluster")
        assert not u["robust_valid"]
        assert np.isnan(u["cov_robust"]).all() and np.isnan(u["sigma_robust"]).all() and np.isnan(u["inflation"]).all()
    return ref


@pytest.fixture(scope="module")
def problems(ctx):
    out = {}
    for n_cp in (6, 12):
        prob, x_gt = SV.make_problem(1200, n_cp=n_cp, seed=20 + n_cp, pixel_noise=0.3)
        out[n_cp] = (prob, Oracle(ctx, prob, x_gt))
    yield out
    for _, o in out.values():
        o.solver.close()


@pytest.mark.parametrize("cluster_spans", [1, 2, 1000])
@pytest.mark.parametrize("n_cp", [6, 12])
def test_uncertainty_against_the_dense_oracle(problems, n_cp, cluster_spans):
    from eventcalib_amd import uncertainty
    _, o = problems[n_cp]
    u = uncertainty.solver_uncertainty(o.solver, o.x, cluster_spans=cluster_spans)
    assert u["cluster_spans"] == cluster_spans
    _check_against_oracle(o, u, cluster_spans)
    assert o.solver.uncertainty(o.x, cluster_spans=cluster_spans)["n_clusters"] == u["n_clusters"]     # (the method form)


def test_storing_every_record_twice(ctx, problems):
    from eventcalib_amd import uncertainty
    prob, o = problems[12]
    twice = dict(prob, obs=np.repeat(prob["obs"], 2, axis=0), time=np.repeat(prob["time"], 2), lm_id=np.repeat(prob["lm_id"], 2))
    o2 = Oracle(ctx, twice, o.x)
    try:
        u1 = uncertainty.solver_uncertainty(o.solver, o.x)
        u2 = uncertainty.solver_uncertainty(o2.solver, o.x)
    finally:
        o2.solver.close()
    assert np.array_equal(o2.table[:, 1], 2 * o.table[:, 1]) and np.array_equal(o2.table[:, 2:], o.table[:, 2:])   # duplicates share a chunk
    assert u1["robust_valid"] and u2["robust_valid"] and u1["n_clusters"] == u2["n_clusters"]
    lim, r_lim = o.bar * o.M, o.robust_limit(1)                               # the dense-oracle test's bars, as they are
    e_rob = _scaled_err(u2["cov_robust"], u1["cov_robust"], o.d)
    e_sig = _scaled_err(2 * u2["cov"] / u2["s2"], u1["cov"] / u1["s2"], o.d)
    e_cov = _scaled_err(u2["cov"], 0.5 * (u2["s2"] / u1["s2"]) * u1["cov"], o.d)
    print("twice: cov_robust moved by %.3e of its limit, 2 Sigma_ii' - Sigma_ii by %.3e; s2' / s2 %.6f, sigma' / sigma %.4f .. %.4f, inflation' / inflation %.4f" % (
        e_rob / r_lim, e_sig / lim, u2["s2"] / u1["s2"], (u2["sigma"] / u1["sigma"]).min(), (u2["sigma"] / u1["sigma"]).max(),
        (u2["inflation"] / u1["inflation"]).mean()))
    assert e_rob <= r_lim and e_sig <= lim and e_cov <= lim * u2["s2"]


def test_monte_carlo_coverage_of_the_formal_covariance(ctx):
    from eventcalib_amd import capi, uncertainty
    prob, x_gt = SV.make_problem(MC_RES, n_cp=MC_CP, seed=9, pixel_noise=0.0)
    stats, worst_r = [], 0.0
    for k in range(MC_K):
        rng = np.random.default_rng(MC_SEED0 + k)
        p = dict(prob, obs=prob["obs"] + MC_SIGMA * rng.normal(size=prob["obs"].shape))
        s = capi.Solver(ctx, p)
        try:
            x, summary = s.solve(x_gt)
            u = uncertainty.solver_uncertainty(s, x)
            worst_r = max(worst_r, float(np.abs(s.residuals(x, with_jacobian=False)[0]).max()))
        finally:
            s.close()
        assert u["positive_definite"] and u["formal_valid"]
        d = x[:9] - x_gt[:9]
        stats.append(float(d @ np.linalg.solve(u["cov"], d)))
    stats = np.array(stats)
    half = 4 * np.sqrt(18.0 / MC_K)
    print("Monte Carlo: K %d, mean %.4f (band %.4f .. %.4f; the CPU oracle's mean for these seeds: %s), std %.3f, largest |r| seen %.4f of huber_a %.4f" % (
        MC_K, stats.mean(), 9 - half, 9 + half, MC_ORACLE_MEAN, stats.std(), worst_r, prob["huber_a"]))
    assert worst_r < 0.5 * prob["huber_a"], "no residual on the Huber tail"
    assert 9 - half <= stats.mean() <= 9 + half
    assert abs(stats.mean() - MC_ORACLE_MEAN) <= 0.05          # (the same data and estimator as the CPU oracle: two solvers' last digits)


def test_a_gap_in_time_is_not_positive_definite(ctx):
    from eventcalib_amd import capi, uncertainty
    prob, x = SV.make_problem(1200, n_cp=12, seed=3, pixel_noise=0.1)
    span = np.array([SV.find_span(prob["knots"], 12, t) for t in prob["time"]])
    keep = (span < 5) | (span > 8)                       # control point 5 is reached from the spans 5 .. 8 alone
    gap = dict(prob, obs=prob["obs"][keep], time=prob["time"][keep], lm_id=prob["lm_id"][keep])
    assert 0 < keep.sum() < len(keep)
    s = capi.Solver(ctx, gap)
    try:
        u = uncertainty.solver_uncertainty(s, x)
    finally:
        s.close()
    assert not u["positive_definite"] and not u["formal_valid"] and not u["robust_valid"]
    assert u["n_res"] == int(keep.sum()) and np.isfinite(u["cost"])
    for k in ("cov", "corr", "cov_robust", "sigma", "sigma_robust", "inflation"):
        assert np.isnan(u[k]).all(), k
    assert np.isnan(u["s2"])
