"""Keeps tests/ref_calib.py honest (CPU only): its autograd blocks against the oracle's finite differences, its dense step
against Schur elimination + back-substitution, its extended-precision solvers against numpy's."""
import numpy as np
import pytest

import ref_calib as RC
from ref_calib import CO, SC


def _state(model, V, seed, obj=None, noise=0.3):
    obj, img, rv, tv = SC.make_views(V, model, seed=seed, noise_px=noise, obj=obj)
    intr = (SC.GT_PINHOLE if model == 0 else SC.GT_FISHEYE).copy()
    if model == 0:
        intr[6:8] = 1e-3, -2e-3
        intr[9:12] = 0.01, -0.02, 0.005
    else:
        intr[4] = 0.01
    p = np.concatenate([intr] + [np.concatenate([rv[v], tv[v]]) for v in range(V)])
    p[12:] += 1e-3 * np.random.default_rng(0).normal(size=6 * V)
    return obj, img, p


@pytest.mark.parametrize("model,flags,aspect", [(0, SC.FLAGS_EXAMPLE, 1.0), (0, CO.FIX_ASPECT_RATIO, 1.3), (0, 0, 0.0),
                                                (1, SC.FLAGS_FISHEYE, 0.0), (1, 0, 0.0)])
def test_autograd_blocks_match_the_oracles_finite_differences(model, flags, aspect):
    """2e-6 of sqrt(Haa * Hbb) per entry (the finite-difference bound of tests/test_gpu_calib.py; measured: at most 2.1e-8),
    gradient in sqrt(Haa * cost), cost 1e-12 relative."""
    obj, img, p = _state(model, 2, seed=3)
    worst = 0.0
    for v in range(2):
        B = RC.view_blocks(model, flags, aspect, p, obj, img, v)
        Hii, Hiv, Hvv, gi, gv, cost = CO.view_blocks(model, flags, aspect, p, obj, img, v)
        d = np.sqrt(np.concatenate([np.diag(Hii), np.diag(Hvv)]))
        di, dv = d[:12], d[12:]
        for got, ref, scale in ((B[:144].reshape(12, 12), Hii, np.outer(di, di)), (B[144:216].reshape(12, 6), Hiv, np.outer(di, dv)),
                                (B[216:252].reshape(6, 6), Hvv, np.outer(dv, dv)), (B[252:264], gi, di * np.sqrt(cost)),
                                (B[264:270], gv, dv * np.sqrt(cost))):
            fixed = scale == 0
            assert (got[fixed] == 0).all() and (ref[fixed] == 0).all()
            ratio = np.abs(got - ref)[~fixed] / scale[~fixed]
            worst = max(worst, ratio.max())
            assert ratio.max() <= 2e-6, (model, flags, v, ratio.max())
        assert abs(B[270] - cost) <= 1e-12 * cost and B[271] == 0
    print("autograd vs finite differences, worst ratio: %.2e" % worst)


def test_projection_matches_the_oracle():
    for model in (0, 1):
        obj, img, p = _state(model, 2, seed=5)
        r = RC.view_residuals(model, 0, 0.0, p, obj, img, 1)
        ref = CO.residuals(model, 0, 0.0, np.concatenate([p[:12], p[18:24]]), obj, img[1:2])
        assert np.abs(r - ref).max() <= 1e-11


def test_extended_solvers_solve():
    rng = np.random.default_rng(1)
    M = rng.normal(size=(9, 9))
    A, b = M @ M.T + 9 * np.eye(9), rng.normal(size=9)
    x = np.linalg.solve(A, b)
    assert np.abs(RC.cholesky_solve_ld(A, b).astype(float) - x).max() <= 1e-13 * np.abs(x).max()
    assert np.abs(RC.gauss_solve_ld(M, b).astype(float) - np.linalg.solve(M, b)).max() <= 1e-11 * np.abs(np.linalg.solve(M, b)).max()
    B2 = rng.normal(size=(9, 3))
    assert np.abs(RC.cholesky_solve_ld(A, B2).astype(float) - np.linalg.solve(A, B2)).max() <= 1e-13


@pytest.mark.parametrize("case", [RC.STEP_CASES[k] for k in (0, 5, 6, 7, 8)], ids=RC.step_case_id)
def test_dense_step_equals_schur_elimination_and_lowers_the_cost(case):
    """step() (one dense solve of the damped system) == eliminate the views, solve the head, back-substitute, within
    1e-9 * max|x| (measured 1e-14 ... 2e-11); the reduced record's two precisions agree; and on the inputs of the GPU's
    first-step test the step lowers the cost from the oracle's initial poses (the GPU test relies on an accepted first step)."""
    model, flags, aspect, _, V = case
    obj, img, guess = RC.step_inputs(case)
    poses = [np.concatenate(CO.view_pose(model, guess, obj, img[v])) for v in range(V)]
    p0 = np.concatenate([guess] + poses)
    lam = 1e-3 if model == 0 else 0.0
    jr = RC.all_view_blocks(model, flags, aspect, p0, obj, img)
    x64, xld = RC.step(jr, lam, model, flags)
    xs = RC.step_by_schur(jr, lam, model, flags)
    assert np.abs(x64 - xs).max() <= 1e-9 * np.abs(x64).max(), np.abs(x64 - xs).max() / np.abs(x64).max()
    assert np.abs(x64 - xld.astype(float)).max() <= 1e-9 * np.abs(x64).max()
    fixed = np.flatnonzero(CO.free_mask(model, flags) == 0)
    assert (x64[fixed] == 0).all()
    r64, rld = RC.reduced_record(jr, lam, obj.shape[0])
    assert r64[RC.R_NPTS] == V * obj.shape[0]
    D = r64[RC.R_D:RC.R_COST]
    tol, _ = RC.group_tolerance(r64[:144], rld[:144], np.sqrt(np.outer(D, D)).ravel(), factor=1.0, floor=1e-9)
    assert tol == 1e-9
    cand = p0 - (x64 if model == 0 else 0.4 * x64)
    cand[:12] = RC.effective_intr(model, flags, aspect, cand[:12])
    assert RC.cost(model, flags, aspect, cand, obj, img) < RC.cost(model, flags, aspect, p0, obj, img)
