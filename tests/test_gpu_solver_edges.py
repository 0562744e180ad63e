"""GPU: the continuous-time solve where its code branches — small relative rotations and sign-flipped control points, pixels on
and around the principal point, event times on knots, chunk tables at their limits, both regimes of the robust loss.  Everything
goes through the C ABI (Solver.residuals / .evaluate / n_chunks); the reference is the oracle's forward-mode dual numbers
(oracle_find_span, oracle_basis, oracle_residual*_cam, oracle_evaluate_mode), which tests/test_residual_edges_host.py holds to a
60-digit restatement at the same edges.  The data come from tests/synth_solver_edges.py (explicit times, pixels, control points).

Tolerances, f64: per-residual rows as test_per_residual_rows_match_dual_numbers — 1e-11 absolute on r (cm), 1e-11 on a row
relative to its largest entry (1e-10 with the fisheye camera, test_fisheye_rows_match_dual_numbers); normal equations as
test_so3_normal_equations_match_oracle — 1e-11 relative on the cost, 1e-9 of the largest entry on g and H; a host-built and a
device-built solver of the same problem — residuals() bit-equal (the same kernel over the same table), evaluate() to rtol 1e-12,
atol 1e-9 of the largest entry (the atomics' accumulation order differs from launch to launch).

Where a ray would run along the board (|Y_z| < 0.2; depth = -T_z / Y_z) the rotation directions are redrawn: the residual is
singular there and amplifies rounding by 1 / Y_z^2, which none of these tests is about."""
import numpy as np
import pytest

import oracle_lib as O
import synth_solver as SV
import synth_solver_edges as E

pytestmark = pytest.mark.gpu

TOL_R, TOL_ROW, TOL_ROW_FISHEYE = 1e-11, 1e-11, 1e-10
TOL_COST, TOL_GH = 1e-11, 1e-9


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    c = eventcalib_amd.Context(0)
    yield c
    c.close()


def _intr(fisheye, rng=None):
    intr = (SV.GT_INTR_FISHEYE if fisheye else SV.GT_INTR).copy()
    if rng is not None:       # (the principal point of the parameter vector under evaluation is not a round number)
        intr[:4] *= 1 + 0.01 * rng.uniform(-1, 1, 4)
        intr[4:9] += 0.005 * rng.uniform(-1, 1, 5)
    return intr


def _rows_against_oracle(s, prob, y, label):
    """r, the 33-entry row and cp0 of EVERY residual against the oracle's dual numbers; returns (r, J, worst |dr|, worst row error)"""
    r, J, cp0 = s.residuals(y)
    ro, Jo, co = E.oracle_rows(prob, y)
    assert np.isfinite(ro).all() and np.isfinite(Jo).all(), label
    assert np.isfinite(r).all() and np.isfinite(J).all(), label
    assert np.array_equal(cp0, co), (label, cp0, co)
    err_r = float(np.abs(r - ro).max()) if len(r) else 0.0
    err_row = float((np.abs(J - Jo).max(axis=1) / np.abs(Jo).max(axis=1)).max()) if len(r) else 0.0
    tol_row = TOL_ROW_FISHEYE if prob["fisheye"] else TOL_ROW
    print("%-60s n=%5d worst |dr| %.2e  worst row %.2e" % (label, len(r), err_r, err_row))
    assert err_r <= TOL_R and err_row <= tol_row, (label, err_r, err_row)
    r0, none, _ = s.residuals(y, with_jacobian=False)
    assert none is None and r0.tobytes() == r.tobytes(), label
    return r, J, err_r, err_row


def _normal_against_oracle(s, prob, y, label):
    from eventcalib_amd.capi import unpack_normal
    n_cp = int(prob["seg_cp_off"][-1])
    acc = s.evaluate(y, True)
    assert np.isfinite(acc).all(), label
    cost, g, H = unpack_normal(acc, n_cp)
    oc, og, oH = O.solver_evaluate(prob, y)
    assert np.isfinite(oc) and np.isfinite(og).all() and np.isfinite(oH).all(), label
    e_c, e_g, e_H = abs(cost - oc) / abs(oc), np.abs(g - og).max() / np.abs(og).max(), np.abs(H - oH).max() / np.abs(oH).max()
    print("%-60s cost %.2e  g %.2e  H %.2e" % (label, e_c, e_g, e_H))
    assert e_c <= TOL_COST and e_g <= TOL_GH and e_H <= TOL_GH, (label, e_c, e_g, e_H)
    assert abs(s.evaluate(y, False)[0] - oc) <= TOL_COST * abs(oc), label
    return acc


def _device_built(ctx, prob, pad=0):
    """the same problem through ecal_solver_create_dev: residual arrays and their count on the device (pad: unused capacity behind
    the count, filled with records that would be refused if they were read)"""
    import torch
    from eventcalib_amd.capi import Solver
    n = len(prob["time"])
    cap = n + pad
    obs = torch.full((cap, 2), -1.0, dtype=torch.float64)
    tm = torch.full((cap,), -1.0, dtype=torch.float64)
    lm = torch.full((cap,), 1 << 20, dtype=torch.int32)
    sg = torch.zeros(cap, dtype=torch.int32)
    obs[:n] = torch.from_numpy(np.ascontiguousarray(prob["obs"], np.float64).reshape(n, 2))
    tm[:n] = torch.from_numpy(np.ascontiguousarray(prob["time"], np.float64))
    lm[:n] = torch.from_numpy(np.ascontiguousarray(prob["lm_id"]).astype(np.int32))
    if prob["seg_id"] is not None:
        sg[:n] = torch.from_numpy(np.ascontiguousarray(prob["seg_id"]).astype(np.int32))
    d = [a.cuda() for a in (obs, tm, lm, sg)]
    cnt = torch.tensor([n], dtype=torch.int32).cuda()
    layout = {k: prob[k] for k in ("seg_cp_off", "knots", "landmarks", "circle_radius", "huber_a", "use_so3", "fisheye")}
    s = Solver(ctx, layout, device_arrays=(d[0].data_ptr() if cap else 0, d[1].data_ptr() if cap else 0, d[2].data_ptr() if cap else 0,
                                           d[3].data_ptr() if cap and prob["seg_id"] is not None else 0, cap, cnt.data_ptr()))
    torch.cuda.synchronize()
    return s


def _host_and_device_built_agree(ctx, prob, y, label, pad=0):
    """returns the host-built solver (the caller closes it)"""
    from eventcalib_amd.capi import Solver
    hs = Solver(ctx, prob)
    ds = _device_built(ctx, prob, pad)
    try:
        assert ds.n_res == hs.n_res == len(prob["time"]), (label, ds.n_res, hs.n_res)
        assert ds.n_chunks == hs.n_chunks, (label, ds.n_chunks, hs.n_chunks)
        rh, Jh, ch = hs.residuals(y)
        rd, Jd, cd = ds.residuals(y)
        assert rh.tobytes() == rd.tobytes() and Jh.tobytes() == Jd.tobytes() and np.array_equal(ch, cd), label
        for with_jacobian in (True, False):
            a, b = ds.evaluate(y, with_jacobian), hs.evaluate(y, with_jacobian)
            assert np.isfinite(a).all() and np.isfinite(b).all(), label
            assert np.allclose(a, b, rtol=1e-12, atol=1e-9 * np.abs(b).max()), (label, np.abs(a - b).max(), np.abs(b).max())
    finally:
        ds.close()
    return hs


def _chain(n_cp, angle, rng, prob, intr, t, tries=400):
    """rotation control points `angle` apart whose rays all meet the board at a fair angle.  Up to 0.1 rad the directions are
    uniform on the sphere; at 1 and 3 rad they stay within ~0.1 rad of the optical axis (a roll), or three such factors in a row
    turn the camera away from the board for some time of every span."""
    for _ in range(tries):
        dirs = None
        if angle >= 1.0:
            dirs = [np.array([0.0, 0.0, 1.0]) + 0.05 * rng.normal(size=3) for _ in range(n_cp - 1)]
            dirs = [d / np.linalg.norm(d) for d in dirs]
        q = E.rotation_chain(n_cp, angle, rng, directions=dirs)
        y = E.params(intr, q, t)
        if np.abs(E.ray_yz(prob, y)).min() >= 0.2:
            return q, y
    raise AssertionError("no well-conditioned control points at %g rad" % angle)


# ---- a. small relative rotations and sign-flipped control points ----
@pytest.mark.parametrize("fisheye", [False, True])
@pytest.mark.parametrize("use_so3", [False, True])
def test_small_angles_and_sign_flips(ctx, use_so3, fisheye):
    """Neighbouring rotation control points 0, 1e-12, 0.9e-10, 1.1e-10, 1e-8, 0.9e-6, 1.1e-6, 0.9e-4, 1.1e-4, 1e-3, 0.1, 1 and 3 rad
    apart (both sides of every small-angle threshold of so3_log / so3_exp / so3_rotate / so3_jl / so3_jinv), n_cp = 6, 40 residuals over
    the three spans with times on the spans' ends (basis values 0 and 1) — one thread per row.  The sweep stops at 3.0 rad: so3_log
    folds at pi and the HOST code itself is at 1.7e-11 there (3.14159 rad), so angles beyond are out of scope.
    SO3 spline: q and -q are the same rotation — negating any ONE control point leaves r and the row unchanged (a property; within
    the row tolerance).  Quaternion blend: -q is another function (the blend is linear in q); it is held to the oracle, on the
    residuals whose blend keeps a norm >= 0.2.
    Measured on an MI355X, worst over the sweep (design/08_solver.md, "Edges of the residual's branches"): SO3 |dr| 4.3e-14, row
    1.0e-12 (pinhole) / 9.6e-13 (fisheye), both at 1.1e-4 rad, just above the 1e-8 threshold of so3_jl / so3_jinv where
    (1 - cos t) / t^2 cancels (host: 4e-13 there), <= 1.1e-13 at every other angle; g and H 3.7e-13.  Blend |dr| 3.6e-14, row 3.1e-15.
    SO3 under -q: r and row bit-equal.  Blend through -q: |dr| 2.5e-14, row 3.2e-15."""
    from eventcalib_amd.capi import Solver
    rng = np.random.default_rng(100 + 2 * use_so3 + fisheye)
    n_cp = 6
    knots = E.jittered_knots(n_cp, 5.0, 5.5, rng)
    times = E.span_times(knots, n_cp, 13, rng)
    n = len(times)
    assert n == 40
    prob = E.problem(knots, times, E.random_pixels(n, rng), E.random_landmarks(n, rng), use_so3=use_so3, fisheye=fisheye)
    intr = _intr(fisheye, rng)
    s = Solver(ctx, prob)
    worst = [0.0, 0.0, 0.0]
    for angle in E.ANGLES:
        t = E.translations(n_cp, rng, still=angle < 1e-9)       # (a camera that stands still: equal translations as well)
        q, y = _chain(n_cp, angle, rng, prob, intr, t)
        label = "angles so3=%d fisheye=%d %g rad" % (use_so3, fisheye, angle)
        r, J, e_r, e_row = _rows_against_oracle(s, prob, y, label)
        _normal_against_oracle(s, prob, y, label)
        worst[0], worst[1] = max(worst[0], e_r), max(worst[1], e_row)
        if use_so3:
            scale = np.abs(J).max(axis=1)
            for j in range(n_cp):
                qf = q.copy()
                qf[j] = -qf[j]
                r2, J2, _ = s.residuals(E.params(intr, qf, t))
                d_r, d_row = float(np.abs(r2 - r).max()), float((np.abs(J2 - J).max(axis=1) / scale).max())
                worst[2] = max(worst[2], d_row)
                assert d_r <= TOL_R and d_row <= (TOL_ROW_FISHEYE if fisheye else TOL_ROW), (label, j, d_r, d_row)
    s.close()
    print("angles so3=%d fisheye=%d: worst |dr| %.2e, row %.2e, row change under -q %.2e" % (use_so3, fisheye, *worst))
    if not use_so3:
        # the blend through one negated control point, each in turn, at 0 and at 0.05 rad: against the oracle only
        for angle in (0.0, 0.05):
            t = E.translations(n_cp, rng)
            q = E.rotation_chain(n_cp, angle, rng)
            for j in range(n_cp):
                qf = q.copy()
                qf[j] = -qf[j]
                y = E.params(intr, qf, t)
                keep = np.abs(E.ray_yz(prob, y)) >= 0.2
                assert keep.sum() >= 10
                pj = E.problem(knots, times[keep], prob["obs"][keep], prob["lm_id"][keep], fisheye=fisheye)
                sj = Solver(ctx, pj)
                label = "blend -q%d fisheye=%d %g rad" % (j, fisheye, angle)
                _rows_against_oracle(sj, pj, y, label)
                _normal_against_oracle(sj, pj, y, label)
                sj.close()


# ---- b. pixels on and around the principal point ----
@pytest.mark.parametrize("fisheye", [False, True])
@pytest.mark.parametrize("use_so3", [False, True])
def test_pixels_at_the_principal_point(ctx, use_so3, fisheye):
    """Pixels at (cx, cy) of the parameter vector under evaluation and 1e-9, 3e-6, 4e-6, 0.03, 0.04 and 1 px away from it, six
    directions each: r2 on both sides of the fisheye branches r2 > 1e-16 (value) and r2 > 1e-8 (derivative, with its limit
    poly' + poly^3 / 3), and at exactly 0.  Rows and normal equations against the oracle (whose fisheye functor takes the series of
    tan(r poly) / r below r2 = 1e-10: other thresholds, another expansion); every value finite.
    Measured on an MI355X, worst of the four variants: |dr| 1.1e-14, row 3.9e-15, cost 3.7e-16, g 2.0e-15, H 9.3e-15."""
    from eventcalib_amd.capi import Solver
    rng = np.random.default_rng(200 + 2 * use_so3 + fisheye)
    n_cp = 6
    knots = E.jittered_knots(n_cp, 5.0, 5.5, rng)
    intr = _intr(fisheye, rng)
    offs = np.repeat(np.array(E.PIXEL_OFFSETS), 6)
    ang = rng.uniform(0, 2 * np.pi, len(offs))
    pix = np.stack([intr[2] + offs * np.cos(ang), intr[3] + offs * np.sin(ang)], axis=1)
    pix[offs == 0.0] = intr[2:4]
    order = rng.permutation(len(offs))           # (every offset in every span)
    pix = pix[order]
    n = len(pix)
    times = np.sort(rng.uniform(knots[3], knots[n_cp], n))
    prob = E.problem(knots, times, pix, E.random_landmarks(n, rng), use_so3=use_so3, fisheye=fisheye)
    fx2 = ((pix[:, 0] - intr[2]) / intr[0]) ** 2 + ((pix[:, 1] - intr[3]) / intr[1]) ** 2
    assert (fx2 == 0).sum() == 6 and ((fx2 > 0) & (fx2 < 1e-16)).sum() == 12 and ((fx2 > 1e-16) & (fx2 < 1e-8)).sum() == 12 and (fx2 > 1e-8).sum() == 12
    t = E.translations(n_cp, rng)
    q, y = _chain(n_cp, 0.05, rng, prob, intr, t)
    s = Solver(ctx, prob)
    label = "pixels so3=%d fisheye=%d" % (use_so3, fisheye)
    _rows_against_oracle(s, prob, y, label)
    _normal_against_oracle(s, prob, y, label)
    s.close()


# ---- c. times on knots ----
@pytest.mark.parametrize("use_so3", [False, True])
def test_times_on_knots(ctx, use_so3):
    """One segment, n_cp = 8, jittered knots; times = the first knot, every interior knot exactly and the doubles just below and
    above it, the last knot, each three times over.  cp0 of every row == oracle_find_span - 3 (spline_find_span's u == last knot
    case, the [u_span, u_span+1) cuts of ecal_solver_create and of solver_span_kernel, spline_basis_inv with left / right = 0), rows
    and normal equations against the oracle, and the solver built by ecal_solver_create_dev from device arrays equal to the
    host-built one.  Measured on an MI355X: |dr| 1.8e-14, row 2.6e-15, cost 3.2e-16, g 1.6e-15, H 5.9e-15."""
    rng = np.random.default_rng(300 + use_so3)
    n_cp = 8
    knots = E.jittered_knots(n_cp, 5.0, 5.5, rng)
    times = E.knot_times(knots, n_cp)
    n = len(times)
    assert n == 3 * (2 + 3 * (n_cp - 4)) and (np.diff(times) >= 0).all()
    prob = E.problem(knots, times, E.random_pixels(n, rng), E.random_landmarks(n, rng), use_so3=use_so3)
    intr = _intr(False, rng)
    q, y = _chain(n_cp, 0.05, rng, prob, intr, E.translations(n_cp, rng))
    label = "knot times so3=%d" % use_so3
    s = _host_and_device_built_agree(ctx, prob, y, label, pad=3)
    # the spans as findSpan has them: a time on an interior knot opens the span to its right, the last knot closes the last span
    want = np.array([SV.find_span(knots, n_cp, u) - 3 for u in times], np.uint32)
    assert want[0] == 0 and want[-1] == n_cp - 4 and set(want) == set(range(n_cp - 3))
    assert np.array_equal(s.residuals(y)[2], want)
    _rows_against_oracle(s, prob, y, label)
    _normal_against_oracle(s, prob, y, label)
    s.close()


# ---- d. chunk tables at their limits, host and device creation side by side ----
@pytest.mark.parametrize("m", [1, 255, 256, 257, 16384, 16385, 32769])
def test_span_of_exactly_m_residuals(ctx, m):
    """A span of exactly NE_T - 1, NE_T, NE_T + 1, NE_CHUNK, NE_CHUNK + 1 and 2 NE_CHUNK + 1 residuals (and of 1), followed by a span
    of 7: n_chunks by the formula of ecal_solver_create (parts = ceil(m / 16384) equal parts, each rounded up to whole batches of
    256), the same table from the device, the sums against the oracle.  Measured on an MI355X, worst over the seven sizes: cost
    3.3e-15, g 3.7e-15, H 7.4e-15."""
    rng = np.random.default_rng(400 + m)
    n_cp = 5
    knots = E.jittered_knots(n_cp, 5.0, 5.5, rng)
    times = E.counted_span_times(knots, n_cp, [m, 7], rng)
    n = len(times)
    prob = E.problem(knots, times, E.random_pixels(n, rng), E.random_landmarks(n, rng))
    y = E.params(_intr(False, rng), E.rotation_chain(n_cp, 0.05, rng), E.translations(n_cp, rng))
    label = "span of %d" % m
    s = _host_and_device_built_agree(ctx, prob, y, label)
    assert {1: 1, 255: 1, 256: 1, 257: 1, 16384: 1, 16385: 2, 32769: 3}[m] == E.expected_chunks(m)
    assert s.n_chunks == E.expected_chunks(m) + 1, (m, s.n_chunks)
    _normal_against_oracle(s, prob, y, label)
    s.close()


def test_empty_spans_and_an_empty_segment(ctx):
    """A segment whose first, two middle and last spans hold no residual; three segments of which the middle one holds none.
    Measured on an MI355X: |dr| 3.6e-14, row 4.1e-15, cost 3.7e-16, g 5.2e-16, H 4.7e-16."""
    rng = np.random.default_rng(410)
    n_cp = 10
    knots = E.jittered_knots(n_cp, 5.0, 5.5, rng)
    counts = [0, 5, 0, 0, 300, 9, 0]
    times = E.counted_span_times(knots, n_cp, counts, rng)
    n = len(times)
    prob = E.problem(knots, times, E.random_pixels(n, rng), E.random_landmarks(n, rng), use_so3=True)
    y = E.params(_intr(False, rng), E.rotation_chain(n_cp, 0.05, rng), E.translations(n_cp, rng))
    s = _host_and_device_built_agree(ctx, prob, y, "empty spans", pad=2)
    assert s.n_chunks == sum(E.expected_chunks(c) for c in counts) == 3
    _rows_against_oracle(s, prob, y, "empty spans")
    _normal_against_oracle(s, prob, y, "empty spans")
    s.close()
    # three segments, the middle one empty
    ncp = [5, 4, 6]
    kn = [E.jittered_knots(c, 5.0 + g, 5.5 + g, rng) for g, c in enumerate(ncp)]
    t0 = E.counted_span_times(kn[0], ncp[0], [40, 0], rng)
    t2 = E.counted_span_times(kn[2], ncp[2], [3, 300, 20], rng)
    times = np.concatenate([t0, t2])
    n = len(times)
    seg = np.concatenate([np.zeros(len(t0)), np.full(len(t2), 2)]).astype(np.uint32)
    prob = E.problem(kn, times, E.random_pixels(n, rng), E.random_landmarks(n, rng), seg_ids=seg)
    y = E.params(_intr(False, rng), E.rotation_chain(sum(ncp), 0.05, rng), E.translations(sum(ncp), rng))
    s = _host_and_device_built_agree(ctx, prob, y, "empty middle segment")
    assert s.n_chunks == 1 + 3                                                    # (one occupied span, then three)
    r, J, _, _ = _rows_against_oracle(s, prob, y, "empty middle segment")
    cp0 = s.residuals(y)[2]
    assert set(cp0[:len(t0)]) == {0} and set(cp0[len(t0):]) == {9, 10, 11}        # (segment 2's control points start at 5 + 4)
    # nothing is accumulated on the empty segment's control points, nor between segments
    from eventcalib_amd.capi import unpack_normal
    cost, g, H = unpack_normal(s.evaluate(y, True), sum(ncp))
    assert cost > 0 and np.abs(g[9 + 6 * 5: 9 + 6 * 9]).max() == 0.0 and np.abs(H[9 + 6 * 5: 9 + 6 * 9]).max() == 0.0
    assert np.abs(H[9: 9 + 6 * 5, 9 + 6 * 9:]).max() == 0.0
    s.close()


@pytest.mark.parametrize("capacity", [0, 8])
def test_zero_residuals(ctx, capacity):
    """No residual at all (device arrays of capacity 0, and of capacity 8 with a count of 0): cost 0, the accumulation buffer all
    zeros, no chunk."""
    rng = np.random.default_rng(420)
    n_cp = 6
    knots = E.jittered_knots(n_cp, 5.0, 5.5, rng)
    prob = E.problem(knots, [], np.zeros((0, 2)), [])
    y = E.params(_intr(False), E.rotation_chain(n_cp, 0.05, rng), E.translations(n_cp))
    s = _host_and_device_built_agree(ctx, prob, y, "zero residuals", pad=capacity)
    assert s.n_res == 0 and s.n_chunks == 0
    acc = s.evaluate(y, True)
    assert acc.shape[0] == 91 + 204 * n_cp and (acc == 0.0).all() and s.evaluate(y, False)[0] == 0.0
    r, J, cp0 = s.residuals(y)
    assert len(r) == 0 and J.shape == (0, 33) and len(cp0) == 0
    oc, og, oH = O.solver_evaluate(prob, y)
    assert oc == 0.0 and not og.any() and not oH.any()
    s.close()


def _acc_fields(acc, n_cp):
    """the defined entries of an accumulation buffer by kind (arrow_layout.hpp), as tests/test_gpu_solver.py reads them"""
    rec = acc[91:].reshape(n_cp, 204)
    hi = acc[10:91].reshape(9, 9)[np.triu_indices(9)]
    blocks = rec[:, 60:].reshape(n_cp, 4, 6, 6).copy()
    iu = np.tril_indices(6, -1)
    blocks[:, 0, iu[0], iu[1]] = 0.0
    for d in range(1, 4):
        blocks[n_cp - d:, d] = 0.0
    return {"cost": acc[:1], "g_intr": acc[1:10], "H_intr": hi, "g_cp": rec[:, :6], "H_cp_intr": rec[:, 6:60], "H_band": blocks}


def test_more_spans_than_one_round_of_the_chunk_scan(ctx):
    """n_cp = 1100: 1097 spans, more than the 1024 threads of solver_chunks_kernel — its carry loop runs a second round — with
    3000 residuals (most spans hold 0 to 6), through ecal_solver_create_dev, against the host-built table and the oracle's sums
    (oracle_evaluate_arrow_mt: the accumulation buffer's own layout; 1e-9 of the largest entry of each kind)."""
    rng = np.random.default_rng(430)
    n_cp, n = 1100, 3000
    knots = E.jittered_knots(n_cp, 5.0, 16.0, rng)
    times = np.sort(rng.uniform(knots[3], knots[n_cp], n))
    prob = E.problem(knots, times, E.random_pixels(n, rng), E.random_landmarks(n, rng))
    y = E.params(_intr(False, rng), E.rotation_chain(n_cp, 0.002, rng), E.translations(n_cp, rng))
    s = _host_and_device_built_agree(ctx, prob, y, "1097 spans", pad=5)
    spans = np.array([SV.find_span(knots, n_cp, u) for u in times])
    occupied = len(set(spans))
    assert s.n_chunks == occupied and occupied > 900 and (spans >= 3 + 1024).any()
    assert np.array_equal(s.residuals(y, with_jacobian=False)[2], (spans - 3).astype(np.uint32))
    got, ref = _acc_fields(s.evaluate(y, True), n_cp), _acc_fields(O.solver_evaluate_arrow(prob, y, 4), n_cp)
    for k in ref:
        assert np.abs(got[k] - ref[k]).max() <= TOL_GH * np.abs(ref[k]).max(), k
    assert abs(got["cost"][0] - ref["cost"][0]) <= TOL_COST * ref["cost"][0]
    s.close()


# ---- e. both regimes of the robust loss ----
@pytest.mark.parametrize("use_so3", [False, True])
def test_loss_regimes(ctx, use_so3):
    """The same 200 residuals with huber_a far below every |r| (all on the linear tail: rho = 2 a |r| - a^2, rows scaled by
    sqrt(a / |r|)) and far above every |r| (all quadratic), |r| read back from residuals().  The boundary |r| == a itself is not
    tested: cost, gradient and J^T J are continuous there, so no test could tell the branches apart.
    Measured on an MI355X: cost 4.0e-16, g 7.4e-16, H 1.4e-14 (tail) / 8.6e-16 (quadratic)."""
    from eventcalib_amd.capi import Solver
    rng = np.random.default_rng(500 + use_so3)
    n_cp, n = 6, 200
    knots = E.jittered_knots(n_cp, 5.0, 5.5, rng)
    times = np.sort(rng.uniform(knots[3], knots[n_cp], n))
    prob = E.problem(knots, times, E.random_pixels(n, rng), E.random_landmarks(n, rng), use_so3=use_so3)
    intr = _intr(False, rng)
    q, y = _chain(n_cp, 0.05, rng, prob, intr, E.translations(n_cp, rng))
    s = Solver(ctx, prob)
    r = np.abs(s.residuals(y, with_jacobian=False)[0])
    s.close()
    assert r.min() > 1e-4 and r.max() < 1e3, (r.min(), r.max())
    costs = {}
    for name, a in (("tail", 1e-3 * r.min()), ("quadratic", 1e3 * r.max())):
        p = dict(prob, huber_a=float(a))
        s = Solver(ctx, p)
        acc = _normal_against_oracle(s, p, y, "loss %s so3=%d" % (name, use_so3))
        costs[name] = acc[0]
        s.close()
    # the regimes are the ones meant: all quadratic -> cost = sum r^2 / 2; all tail -> cost = sum (a |r| - a^2 / 2)
    a = 1e-3 * r.min()
    assert abs(costs["quadratic"] - 0.5 * (r ** 2).sum()) <= 1e-12 * costs["quadratic"]
    assert abs(costs["tail"] - (a * r - 0.5 * a * a).sum()) <= 1e-12 * costs["tail"]
