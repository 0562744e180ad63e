"""GPU: the per-chunk score sums (ecal_solver_chunk_scores, eventcalib_amd/csrc/ecal_uncertainty.hip) on synth_solver problems.

The oracle is sum rho' r J per chunk in numpy from ecal_residuals' own r and J (the parent's kernel) with the Huber loss restated
(uncertainty_oracle.py).  The bar of an entry is the summation bound (count + 33) eps sum |terms|: `count` additions, and 33 for the
row itself, whose entries the two kernels reach through differently placed roundings (the score kernel scales the row by sqrt(rho')
at its root, as the normal equations do).

Cases: one record; chunks of 255, 256 and 257 records (one short, one exact and one started second turn of the workgroup's 256
threads; n_cp = 4 is one knot span, so the problem is one chunk); 16385 records in one span (two chunks of one cluster); two
segments; the four use_so3 x fisheye kernels; pixel noise large enough for both Huber branches (asserted).  For each: the scores
scattered and summed over the chunks against the gradient in ecal_solver_evaluate's buffer, sum half_rho against its [0], and a
second call bit for bit.

The gradient's bar: both sides are computed sums of the same n_k terms of entry k (the evaluation adds them on the matrix cores and
by atomics, in another order), each within (n_k + 33) eps sum |terms| of the exact sum: twice that between them."""
import numpy as np
import pytest

import synth_solver as SV
import uncertainty_oracle as UO
from oracle_chain import dense_from_arrow

pytestmark = pytest.mark.gpu
EPS = UO.EPS


def _one_span(n_res, seed=3, pixel_noise=0.2, **kw):
    """n_res records in ONE knot span (n_cp = 4): generated 2048 at most and repeated in place (times stay sorted)"""
    base = min(n_res, 2048)
    prob, x = SV.make_problem(base, n_cp=4, seed=seed, pixel_noise=pixel_noise, **kw)
    if n_res > base:
        rep = -(-n_res // base)
        for k in ("obs", "time", "lm_id"):
            prob[k] = np.repeat(prob[k], rep, axis=0)[:n_res]
    return prob, x


CASES = {
    "one_record": lambda: _one_span(1),
    "chunk_255": lambda: _one_span(255),
    "chunk_256": lambda: _one_span(256),
    "chunk_257": lambda: _one_span(257),
    "span_16385": lambda: _one_span(16385),
    "two_segments": lambda: SV.make_problem(900, n_cp=6, seed=4, pixel_noise=0.2, n_segments=2),
    "quat_radial": lambda: SV.make_problem(700, n_cp=7, seed=5, pixel_noise=0.2),
    "quat_fisheye": lambda: SV.make_problem(700, n_cp=7, seed=5, pixel_noise=0.2, fisheye=True),
    "so3_radial": lambda: SV.make_problem(700, n_cp=7, seed=5, pixel_noise=0.2, use_so3=True),
    "so3_fisheye": lambda: SV.make_problem(700, n_cp=7, seed=5, pixel_noise=0.2, use_so3=True, fisheye=True),
    "huber_both": lambda: SV.make_problem(1500, n_cp=9, seed=6, pixel_noise=2.0),
}
EXPECT_CHUNKS = {"one_record": [1], "chunk_255": [255], "chunk_256": [256], "chunk_257": [257]}


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.mark.parametrize("case", list(CASES))
def test_chunk_scores_against_the_residuals_own_rows(ctx, case):
    from eventcalib_amd import capi, uncertainty
    prob, x_gt = CASES[case]()
    n_cp = int(prob["seg_cp_off"][-1])
    x = SV.perturb(x_gt, n_cp, np.random.default_rng(11), intr_rel=0.002, rot=0.001, trans=0.03)   # (off the solution: a gradient to speak of)
    s = capi.Solver(ctx, prob)
    try:
        score, half_rho, table = uncertainty.chunk_scores(s, x)
        score2, half_rho2, table2 = s.chunk_scores(x)                 # the method form, a second call
        acc = s.evaluate(x)
        terms, hr_rec, tail, cp0 = UO.record_terms(s, x)
    finally:
        s.close()
    n_res = len(prob["time"])
    assert score.shape == (s.n_chunks, 33) and half_rho.shape == (s.n_chunks,) and table.shape == (s.n_chunks, 4)
    assert int(table[:, 1].sum()) == n_res
    if case in EXPECT_CHUNKS:
        assert list(table[:, 1]) == EXPECT_CHUNKS[case]
        assert len(set(map(tuple, table[:, 2:]))) == 1                                   # one span: one cluster
    if case == "span_16385":                                                             # one span, more than a chunk holds
        assert len(table) == 2 and table[:, 1].max() <= 16384 and len(set(map(tuple, table[:, 2:]))) == 1
    if case == "two_segments":
        assert set(table[:, 2]) == {0, 1}
    if case == "huber_both":
        assert 0.05 * n_res < int(tail.sum()) < 0.95 * n_res, "the numpy side sees residuals on both Huber branches"
    # a second call gives the same bits
    assert np.array_equal(score, score2) and np.array_equal(half_rho, half_rho2) and np.array_equal(table, table2)
    want, mag, start = UO.chunk_sums(terms, table)
    for c in range(len(table)):                                                          # the table's cp0 is the records' cp0
        assert (cp0[start[c]:start[c + 1]] == table[c, 0]).all()
        assert table[c, 0] == prob["seg_cp_off"][table[c, 2]] + table[c, 3] - 3
    bar = (table[:, 1].astype(np.float64)[:, None] + 33.0) * EPS * mag
    err = np.abs(score - want)
    worst = float((err / np.maximum(bar, 1e-300)).max())
    print("%s: %d chunks, %d records (%d on the Huber tail); largest |score - oracle| / bar %.3g" % (
        case, len(table), n_res, int(tail.sum()), worst))
    assert (err <= bar).all(), worst
    # sum half_rho: the chunks against their records, and their total against the evaluation's cost
    hr_want, hr_mag, _ = UO.chunk_sums(hr_rec[:, None], table)
    assert (np.abs(half_rho - hr_want[:, 0]) <= (table[:, 1] + 33.0) * EPS * hr_mag[:, 0]).all()
    assert abs(half_rho.sum() - acc[0]) <= 2 * (n_res + 33.0) * EPS * hr_rec.sum()
    # scattered and summed over the chunks: the gradient of ecal_solver_evaluate
    _, g, _ = dense_from_arrow(acc, n_cp)
    full = UO.scatter(score, table, n_cp).sum(axis=0)
    count = (UO.scatter(np.ones_like(score), table, n_cp) * table[:, 1:2]).sum(axis=0)
    g_bar = 2 * (count + 33.0) * EPS * UO.scatter(mag, table, n_cp).sum(axis=0)
    g_err = np.abs(full - g)
    print("   gradient: largest |sum of scores - evaluate| / bar %.3g" % float((g_err / np.maximum(g_bar, 1e-300)).max()))
    assert (g_err <= g_bar).all()


def test_a_solver_without_residuals_has_no_chunks(ctx):
    from eventcalib_amd import capi, uncertainty
    prob, x = SV.make_problem(8, n_cp=5, seed=1)
    empty = dict(prob, obs=prob["obs"][:0], time=prob["time"][:0], lm_id=prob["lm_id"][:0])
    s = capi.Solver(ctx, empty)
    try:
        assert s.n_chunks == 0
        score, half_rho, table = uncertainty.chunk_scores(s, x)
        assert score.shape == (0, 33) and half_rho.shape == (0,) and table.shape == (0, 4)
        u = uncertainty.solver_uncertainty(s, x)
        assert not u["positive_definite"] and u["n_clusters"] == 0 and np.isnan(u["cov"]).all() and np.isnan(u["cov_robust"]).all()
    finally:
        s.close()
