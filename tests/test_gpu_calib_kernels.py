"""The init calibration's kernels one by one (ecal_calib.hip) against tests/ref_calib.py — float64 autograd blocks, the
reduced record and the damped step solved in float64 AND in numpy.longdouble — on boards from 4 to 128 points, every flag
bit, validity masks, and the entry-point options.  Tolerances are stated per test; those of the record and the step come
from the reference's own float64-versus-longdouble spread."""
import numpy as np
import pytest

import ref_calib as RC
from ref_calib import CO, SC

pytestmark = pytest.mark.gpu

BOARD_IDS = ["%dx%d" % b for b in RC.BOARDS]


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    c = eventcalib_amd.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- 1. calib_eval_kernel ----------------------------------------------------------------------------------------------
def _eval_state(model, rows, cols, V, seed):
    """Noisy views (0.3 px), nonzero tangential / rational / skew terms, poses off by 1e-3."""
    obj, img, rv, tv = SC.make_views(V, model, seed=seed, noise_px=0.3, obj=RC.board(rows, cols))
    intr = (SC.GT_PINHOLE if model == 0 else SC.GT_FISHEYE).copy()
    if model == 0:
        intr[6:8] = 1e-3, -2e-3
        intr[9:12] = 0.01, -0.02, 0.005
    else:
        intr[4] = 0.01
    p = np.concatenate([intr] + [np.concatenate([rv[v], tv[v]]) for v in range(V)])
    p[12:] += 1e-3 * np.random.default_rng(0).normal(size=6 * V)
    return obj, img, p


def _gpu_blocks(ctx, model, flags, aspect, p, obj, img, with_jac=1):
    import torch
    from eventcalib_amd import capi
    V = img.shape[0]
    d_blocks = torch.zeros(V, capi.CALIB_BLOCK_DOUBLES, dtype=torch.float64, device="cuda:0")
    d_obj, d_img, d_intr, d_view = _dev(obj), _dev(img), _dev(p[:12]), _dev(p[12:])
    capi.calib_view_blocks_dev(ctx, d_obj.data_ptr(), obj.shape[0], d_img.data_ptr(), V, model, flags, aspect,
                               d_intr.data_ptr(), d_view.data_ptr(), with_jac, d_blocks.data_ptr(), _stream())
    torch.cuda.synchronize()
    return d_blocks.cpu().numpy()


def _check_blocks(B, model, flags, aspect, p, obj, img, tag):
    """Every entry of Hii, Hiv, Hvv within 1e-10 * sqrt(Haa * Hbb), of gi, gv within 1e-10 * sqrt(Haa * cost), cost 1e-12
    relative; rows and columns of fixed slots exactly 0.0.  Returns the worst ratio (in units of the scale)."""
    fixed = CO.free_mask(model, flags) == 0
    worst = 0.0
    for v in range(img.shape[0]):
        R = RC.view_blocks(model, flags, aspect, p, obj, img, v)
        cost = R[RC.O_COST]
        d = np.sqrt(np.concatenate([np.diag(R[:144].reshape(12, 12)), np.diag(R[216:252].reshape(6, 6))]))
        di, dv = d[:12], d[12:]
        assert (di[fixed] == 0).all() and (di[~fixed] > 0).all() and (dv > 0).all()
        for name, sl, shape, scale in (("Hii", slice(0, 144), (12, 12), np.outer(di, di)), ("Hiv", slice(144, 216), (12, 6), np.outer(di, dv)),
                                       ("Hvv", slice(216, 252), (6, 6), np.outer(dv, dv)), ("gi", slice(252, 264), (12,), di * np.sqrt(cost)),
                                       ("gv", slice(264, 270), (6,), dv * np.sqrt(cost))):
            got, ref = B[v, sl].reshape(shape), R[sl].reshape(shape)
            zero = scale == 0
            assert (got[zero] == 0.0).all(), (tag, v, name, "a fixed slot's row / column is not exactly zero")
            ratio = float((np.abs(got - ref)[~zero] / scale[~zero]).max())
            worst = max(worst, ratio)
            assert ratio <= 1e-10, (tag, v, name, ratio)
        assert abs(B[v, 270] - cost) <= 1e-12 * cost, (tag, v, B[v, 270], cost)
    print("%s: worst block ratio %.2e" % (tag, worst))
    return worst


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("rows,cols", RC.BOARDS, ids=BOARD_IDS)
def test_view_blocks_match_autograd_on_every_board_size(ctx, rows, cols, model):
    """4, 9, 63, 64, 65, 100, 128 points (one trip per lane, exactly one, a second trip for one lane, for most, for all): the
    analytic rows' Gram matrix == J^T J of the float64 autograd Jacobian at 1e-10 of the block scale — the project's bound
    for analytic rows against dual numbers.  Cost-only mode writes the bit-identical cost and nothing else."""
    obj, img, p = _eval_state(model, rows, cols, 3, seed=3 + rows)
    B = _gpu_blocks(ctx, model, 0, 0.0, p, obj, img)
    _check_blocks(B, model, 0, 0.0, p, obj, img, "%dx%d model %d" % (rows, cols, model))
    C = _gpu_blocks(ctx, model, 0, 0.0, p, obj, img, with_jac=0)
    assert _bits(C[:, 270]) == _bits(B[:, 270])
    assert (np.delete(C, 270, axis=1) == 0).all()


PINHOLE_BITS = [("FIX_ASPECT_RATIO", 1.0), ("FIX_ASPECT_RATIO", 1.3), ("FIX_PRINCIPAL_POINT", 0.0), ("ZERO_TANGENT_DIST", 0.0)] + [
    ("FIX_K%d" % k, 0.0) for k in range(1, 7)]
FISHEYE_BITS = ["FIX_PRINCIPAL_POINT", "FIX_SKEW", "FIX_K1", "FIX_K2", "FIX_K3", "FIX_K4"]


@pytest.mark.parametrize("bit,aspect", PINHOLE_BITS, ids=["%s-%g" % b for b in PINHOLE_BITS])
def test_every_pinhole_flag_bit_on_its_own(ctx, bit, aspect):
    """The fixed slot's rows and columns are exactly 0.0, everything else at the 1e-10 bound; a fixed aspect ratio (1.0 and 1.3)
    puts both focal lengths' derivatives into column 1."""
    flags = getattr(CO, bit)
    obj, img, p = _eval_state(0, 9, 4, 2, seed=3)
    B = _gpu_blocks(ctx, 0, flags, aspect, p, obj, img)
    _check_blocks(B, 0, flags, aspect, p, obj, img, "pinhole %s %g" % (bit, aspect))


@pytest.mark.parametrize("bit", FISHEYE_BITS)
def test_every_fisheye_flag_bit_on_its_own(ctx, bit):
    flags = getattr(CO, bit)
    obj, img, p = _eval_state(1, 9, 4, 2, seed=3)
    B = _gpu_blocks(ctx, 1, flags, 0.0, p, obj, img)
    _check_blocks(B, 1, flags, 0.0, p, obj, img, "fisheye %s" % bit)


def test_pinhole_only_bits_change_nothing_for_the_fisheye(ctx):
    obj, img, p = _eval_state(1, 9, 4, 2, seed=3)
    plain = _gpu_blocks(ctx, 1, 0, 0.0, p, obj, img)
    for bit, aspect in ((CO.FIX_ASPECT_RATIO, 1.3), (CO.ZERO_TANGENT_DIST, 0.0), (CO.FIX_K5, 0.0), (CO.FIX_K6, 0.0)):
        assert _bits(_gpu_blocks(ctx, 1, bit, aspect, p, obj, img)) == _bits(plain), bit


def test_point_counts_outside_the_kernels_range_are_refused(ctx):
    """n_pts = 129 on all three entry points, 3 on PnP and calibrate, 0 on blocks: EcalError, no launch (the buffers passed
    are large enough for the count all the same)."""
    import torch
    from eventcalib_amd import capi
    obj = np.zeros((129, 3))
    obj[:, 0], obj[:, 1] = np.arange(129) % 13, np.arange(129) // 13
    img = np.random.default_rng(0).uniform(10, 200, size=(2, 129, 2))
    d_obj, d_img, d_intr, d_view = _dev(obj), _dev(img), _dev(SC.GT_PINHOLE), _dev(np.tile([0.1, 0.2, 0.3, 0, 0, 60.0], 2))
    d_blocks = torch.zeros(2, capi.CALIB_BLOCK_DOUBLES, dtype=torch.float64, device="cuda:0")
    d_pose = torch.zeros(2, 6, dtype=torch.float64, device="cuda:0")
    for n in (129, 0):
        with pytest.raises(capi.EcalError):
            capi.calib_view_blocks_dev(ctx, d_obj.data_ptr(), n, d_img.data_ptr(), 2, 0, 0, 0.0, d_intr.data_ptr(), d_view.data_ptr(), 1,
                                       d_blocks.data_ptr(), _stream())
    for n in (129, 3):
        with pytest.raises(capi.EcalError):
            capi.pnp_batch_dev(ctx, d_obj.data_ptr(), n, d_img.data_ptr(), None, 2, 0, d_intr.data_ptr(), 4.0, 3, 0, d_pose.data_ptr(),
                               stream=_stream())
        with pytest.raises(capi.EcalError):
            capi.pnp_batch(ctx, obj[:n], img[:, :n], None, 0, SC.GT_PINHOLE, 4.0, 3, 0)
        with pytest.raises(capi.EcalError):
            capi.calibrate_views(ctx, obj[:n], img[:, :n], SC.WIDTH, SC.HEIGHT)
    torch.cuda.synchronize()
    assert (d_blocks == 0).all() and (d_pose == 0).all()


# ---- 2. + 3. the first reduced record and the first step --------------------------------------------------------------
def _pnp_dev(ctx, obj, img, valid, model, intr, thresh, rounds, refine_iters):
    import torch
    from eventcalib_amd import capi
    F, n = img.shape[0], obj.shape[0]
    d_pose = torch.zeros(F, 6, dtype=torch.float64, device="cuda:0")
    d_inl = torch.zeros(F, n, dtype=torch.int32, device="cuda:0")
    d_err = torch.zeros(F, dtype=torch.float64, device="cuda:0")
    d_ok = torch.zeros(F, dtype=torch.int32, device="cuda:0")
    d_obj, d_img, d_intr = _dev(obj), _dev(img), _dev(np.asarray(intr, np.float64))
    d_valid = None if valid is None else _dev(np.ascontiguousarray(valid, np.uint32).view(np.int32))
    capi.pnp_batch_dev(ctx, d_obj.data_ptr(), n, d_img.data_ptr(), None if valid is None else d_valid.data_ptr(), F, model,
                       d_intr.data_ptr(), thresh, rounds, refine_iters, d_pose.data_ptr(), d_inl.data_ptr(), d_err.data_ptr(),
                       d_ok.data_ptr(), _stream())
    torch.cuda.synchronize()
    return {"pose": d_pose.cpu().numpy(), "inlier": d_inl.cpu().numpy().view(np.uint32), "err": d_err.cpu().numpy(),
            "ok": d_ok.cpu().numpy().view(np.uint32)}


@pytest.fixture(scope="module", params=RC.STEP_CASES, ids=RC.step_case_id)
def first_step(request, ctx):
    """One ecal_calibrate_views run of max_iter = 1 from a guess, with a Python all-reduce hook that records every buffer it
    is handed, and the reference at the state p0 the run starts from: the guess + the poses of the pose kernel at the
    guess (the same kernel on the same inputs as the run's own initial poses: bit-identical)."""
    import torch
    from eventcalib_amd import capi
    case = request.param
    model, flags, aspect, _, V = case
    obj, img, guess = RC.step_inputs(case)
    poses = _pnp_dev(ctx, obj, img, None, model, guess, 0.0, 1, 20)
    assert poses["ok"].all()
    p0 = np.concatenate([guess, poses["pose"].ravel()])
    records = []

    def hook(user, d_buf, n, stream):
        try:
            t = torch.empty(n, dtype=torch.float64, device="cuda:0")
            ctx._check(ctx._L.ecal_copy_dev(ctx._h, t.data_ptr(), d_buf, n * 8, stream, 1))
            records.append(t.cpu().numpy())
            return 0
        except Exception as e:  # never let an exception cross the C boundary
            print("hook failed:", e)
            return 1

    cb = capi.ALLREDUCE_FN(hook)
    out = capi.calibrate_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, model, flags | capi.CALIB_USE_INTRINSIC_GUESS, aspect, max_iter=1,
                               allreduce=cb, intr_guess=guess)
    lam = 1e-3 if model == 0 else 0.0
    jr = RC.all_view_blocks(model, flags, aspect, p0, obj, img)
    return dict(case=case, obj=obj, img=img, guess=guess, p0=p0, records=records, out=out, lam=lam, jr=jr,
                rec=RC.reduced_record(jr, lam, obj.shape[0]), x=RC.step(jr, lam, model, flags))


def _cost_only(rec):
    return (np.delete(rec, [RC.R_COST, RC.R_NPTS]) == 0).all() and rec[RC.R_COST] > 0


def test_first_reduced_record_matches_the_reference(first_step):
    """calib_schur_kernel + calib_reduce_kernel.  The hook sees exactly 170 (cost only), 170 (full record, lambda 1e-3), 170
    (the candidate's cost), 2 (stop test) for the radial model — anything else means the first step was rejected, and the
    test fails —; 170 (full record, lambda 0), 170 (final cost) for the fisheye model.  The full record against
    ref_calib.reduced_record at p0, group by group: S in sqrt(D_a D_b), g in sqrt(D_a cost), D and cost relative;
    tolerance 16 x the reference's own float64-versus-longdouble spread in that scale (the kernel sums in another order —
    256 rows in sequence, four interleaved partial sums over the views — and divides through its own Cholesky), floor
    1e-13; without an extended type 1e-9 of the group scale."""
    fs = first_step
    model, flags, aspect, _, V = fs["case"]
    n = fs["obj"].shape[0]
    lens = [len(r) for r in fs["records"]]
    if model == 0:
        assert lens == [170, 170, 170, 2], lens
        assert _cost_only(fs["records"][0]) and _cost_only(fs["records"][2])
        assert fs["records"][0][RC.R_NPTS] == V * n and fs["records"][2][RC.R_NPTS] == V * n
        assert fs["records"][2][RC.R_COST] <= fs["records"][0][RC.R_COST]
        got = fs["records"][1]
    else:
        assert lens == [170, 170], lens
        assert _cost_only(fs["records"][1])
        got = fs["records"][0]
    r64, rld = fs["rec"]
    D, cost = r64[RC.R_D:RC.R_COST], r64[RC.R_COST]
    fixed = CO.free_mask(model, flags) == 0
    assert (D[fixed] == 0).all() and (D[~fixed] > 0).all()
    note = "" if RC.HAVE_EXTENDED else " (no extended type on this machine: fixed 1e-9 of the group scale)"
    for name, sl, scale in (("S", slice(0, RC.R_G), np.sqrt(np.outer(D, D)).ravel()), ("g", slice(RC.R_G, RC.R_D), np.sqrt(D * cost)),
                            ("D", slice(RC.R_D, RC.R_COST), D), ("cost", slice(RC.R_COST, RC.R_NPTS), np.array([cost]))):
        tol, spread = RC.group_tolerance(r64[sl], rld[sl], scale)
        zero = scale == 0
        assert (got[sl][zero] == 0.0).all(), (name, "fixed slots are not exactly zero")
        ratio = float((np.abs(got[sl] - rld[sl].astype(np.float64))[~zero] / scale[~zero]).max())
        print("%s %s: reference spread %.2e, kernel vs reference %.2e, tolerance %.2e" % (RC.step_case_id(fs["case"]), name, spread, ratio, tol))
        assert ratio <= tol, (name, ratio, tol, spread, note)
    assert got[RC.R_NPTS] == V * n


def test_first_step_matches_the_dense_solve(first_step):
    """calib_update_kernel + the host LU.  With max_iter = 1 the result IS the first candidate: p0 - x (fisheye: p0 - 0.4 x,
    the first smoothing factor), x the solution of the damped dense system (ref_calib.step); fx = aspect * fy under a fixed
    aspect ratio; fixed slots unchanged bit for bit.  Bound per group (intrinsics, rvecs, tvecs): 16 x the reference's
    float64-versus-longdouble spread of x + 1e-12 max|x|."""
    fs = first_step
    model, flags, aspect, _, V = fs["case"]
    out, guess, p0 = fs["out"], fs["guess"], fs["p0"]
    n = fs["obj"].shape[0]
    x64, xld = fs["x"]
    a = 1.0 if model == 0 else 0.4
    want = (p0.astype(RC.LD) - a * xld).astype(np.float64)
    fix_aspect = model == 0 and bool(flags & CO.FIX_ASPECT_RATIO)
    if fix_aspect:
        want[0] = want[1] * aspect
    got = np.concatenate([out["intr"], np.concatenate([out["rvecs"], out["tvecs"]], 1).ravel()])
    fixed = np.flatnonzero(CO.free_mask(model, flags) == 0)
    for j in fixed:
        if not (fix_aspect and j == 0):
            assert _bits(got[j]) == _bits(guess[j]), ("fixed slot moved", j, got[j], guess[j])
    if fix_aspect:
        assert got[0] == got[1] * aspect
    views = np.arange(12, 12 + 6 * V).reshape(V, 6)
    note = "" if RC.HAVE_EXTENDED else " (no extended type on this machine: fixed 1e-9 of the group scale)"
    for name, idx in (("intrinsics", np.arange(12)), ("rvecs", views[:, :3].ravel()), ("tvecs", views[:, 3:].ravel())):
        xmax = float(np.abs(x64[idx]).max())
        spread = float(np.abs(x64[idx].astype(RC.LD) - xld[idx]).max())
        tol = a * (16 * spread + 1e-12 * xmax) if RC.HAVE_EXTENDED else RC.FALLBACK_TOL * xmax
        err = float(np.abs(got[idx] - want[idx]).max())
        print("%s %s: max|x| %.3e, reference spread %.2e, kernel vs reference %.2e, tolerance %.2e"
              % (RC.step_case_id(fs["case"]), name, xmax, spread, err, tol))
        assert xmax > 0 and err <= tol, (name, err, tol, note)
    rms = np.sqrt(RC.cost(model, flags, aspect, got, fs["obj"], fs["img"]) / (V * n))
    assert abs(out["rms"] - rms) <= 1e-10 * rms, (out["rms"], rms)
    assert out["iterations"] == 1
    # radial: the start and the candidate are evaluated with their Jacobians (hook calls 1 and 3 carry their costs);
    # fisheye: one Jacobian evaluation for the step, one cost-only evaluation at the end
    assert (out["jacobian_evaluations"], out["error_evaluations"]) == ((2, 0) if model == 0 else (1, 1))


# ---- 4. view_pose_kernel: board sizes, d_err, validity masks ----------------------------------------------------------
def _reproj_err(model, intr, pose, inl, obj, img):
    e = np.zeros(len(pose))
    for f in range(len(pose)):
        r = CO.project(model, intr, pose[f, :3], pose[f, 3:], obj) - img[f]
        e[f] = (r[inl[f] != 0] ** 2).sum()
    return e


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("rows,cols", [(2, 2), (13, 5), (16, 8)], ids=["2x2", "13x5", "16x8"])
def test_pnp_on_small_and_large_boards(ctx, rows, cols, model):
    """test_pnp_recovers_pose_and_flags_outliers' assertions, at its bounds, on 4, 65 and 128 points (16x8: one corrupted
    index below 64 and one above; 2x2: none, four points have no redundancy).  d_err == the squared reprojection residuals
    of the returned pose over the returned inliers (1e-9 relative) — on 0.3 px noisy views as well, where the residuals
    are far from rounding level, with and without refinement."""
    F = 16
    gt = SC.GT_PINHOLE if model == 0 else SC.GT_FISHEYE
    obj, img, rv, tv = SC.make_views(F, model, seed=5, obj=RC.board(rows, cols))
    n = obj.shape[0]
    img = img.copy()
    bad = [] if n == 4 else [(3, 7), (9, 30)] if n < 128 else [(3, 7), (9, 100)]
    for (f, k), d in zip(bad, ((9.0, -7.0), (-12.0, 5.0))):
        img[f, k] += d
    res = _pnp_dev(ctx, obj, img, None, model, gt, 4.0, 3, 0)
    pose, inl = res["pose"], res["inlier"]
    assert res["ok"].all()
    exp_inl = np.ones_like(inl)
    for f, k in bad:
        exp_inl[f, k] = 0
    assert (inl == exp_inl).all()
    print("%dx%d model %d: |rvec - gt| %.2e, |tvec - gt| %.2e" % (rows, cols, model, np.abs(pose[:, :3] - rv).max(), np.abs(pose[:, 3:] - tv).max()))
    assert np.abs(pose[:, :3] - rv).max() < 5e-5 and np.abs(pose[:, 3:] - tv).max() < 2e-3
    for f in (0, 3, 9):
        r_o, t_o, inl_o = CO.pnp_consensus(model, gt, obj, img[f])
        assert (inl_o == inl[f].astype(bool)).all()
        print("  frame %d vs oracle: rvec %.2e tvec %.2e" % (f, np.abs(pose[f, :3] - r_o).max(), np.abs(pose[f, 3:] - t_o).max()))
        assert np.abs(pose[f, :3] - r_o).max() < 1e-9 and np.abs(pose[f, 3:] - t_o).max() < 1e-8
    res = _pnp_dev(ctx, obj, img, None, model, gt, 4.0, 3, 20)
    assert np.abs(res["pose"][:, :3] - rv).max() < 1e-7 and np.abs(res["pose"][:, 3:] - tv).max() < 1e-5
    # d_err on noisy views
    noisy = img + 0.3 * np.random.default_rng(1).normal(size=img.shape)
    for refine in (0, 20):
        res = _pnp_dev(ctx, obj, noisy, None, model, gt, 4.0, 3, refine)
        assert res["ok"].all()
        want = _reproj_err(model, gt, res["pose"], res["inlier"], obj, noisy)
        assert (want > 0).all() and np.abs(res["err"] / want - 1).max() <= 1e-9, (refine, res["err"], want)


def _mask_case(model, rows, cols):
    """F = 8 noise-free frames: 0 all valid; 1 exactly four valid points, not collinear; 2 three valid points; 3 a random mask
    and two corrupted detections among the valid; 4 a random mask with the corrupted detection masked out; 5-7 random masks
    that drop about a quarter."""
    F = 8
    obj, img, rv, tv = SC.make_views(F, model, seed=7, obj=RC.board(rows, cols))
    n = obj.shape[0]
    rng = np.random.default_rng(rows)
    valid = (rng.uniform(size=(F, n)) > 0.25).astype(np.uint32)
    valid[0] = 1
    valid[1] = 0
    valid[1, [0, cols - 1, n - cols, n - 2]] = 1          # two on the first row, two on the last
    valid[2] = 0
    valid[2, [0, cols - 1, n - 1]] = 1
    img = img.copy()
    a, b = np.flatnonzero(valid[3])[[2, -3]]
    img[3, a] += (9.0, -7.0)
    img[3, b] += (-12.0, 5.0)
    c = np.flatnonzero(valid[4] == 0)[1]
    img[4, c] += (15.0, 11.0)
    return obj, img, valid, rv, tv


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("rows,cols", [(9, 4), (10, 10)], ids=["9x4", "10x10"])
def test_pnp_with_validity_masks(ctx, rows, cols, model):
    """d_valid != NULL.  A masked point is read into nothing: NaN or 1e6 in its image coordinates give bit-identical pose,
    inlier, err and ok, with and without refinement, and it is never an inlier.  Fewer than four valid points: ok = 0, pose,
    inliers and err all zero, the neighbours' results those of a run without that frame.  Every other frame: the oracle's
    consensus on the compacted arrays (inliers equal, pose 1e-9 / 1e-8).  The host form uploads the mask and returns the
    device form's bits; rounds = 0 and model = 2 are refused."""
    from eventcalib_amd import capi
    gt = SC.GT_PINHOLE if model == 0 else SC.GT_FISHEYE
    obj, img, valid, rv, tv = _mask_case(model, rows, cols)
    F, n = valid.shape
    masked = valid == 0
    img_a, img_b = img.copy(), img.copy()
    img_a[masked] = np.nan
    img_b[masked] = 1e6
    keep = [f for f in range(F) if f != 2]
    for refine in (0, 20):
        A = _pnp_dev(ctx, obj, img_a, valid, model, gt, 4.0, 3, refine)
        B = _pnp_dev(ctx, obj, img_b, valid, model, gt, 4.0, 3, refine)
        H = capi.pnp_batch(ctx, obj, img_a, valid, model, gt, 4.0, 3, refine)
        W = _pnp_dev(ctx, obj, img_a[keep], valid[keep], model, gt, 4.0, 3, refine)
        for k in ("pose", "inlier", "err", "ok"):
            assert _bits(A[k]) == _bits(B[k]), (refine, k, "a masked point was read")
            assert _bits(A[k]) == _bits(H[k]), (refine, k, "host form differs from the device form")
            assert _bits(A[k][keep]) == _bits(W[k]), (refine, k, "the refused frame changed its neighbours")
        assert np.isfinite(A["pose"]).all() and np.isfinite(A["err"]).all()
        assert (A["inlier"][masked] == 0).all()
        assert A["ok"][2] == 0 and (A["pose"][2] == 0).all() and (A["inlier"][2] == 0).all() and A["err"][2] == 0
        assert (A["ok"][keep] == 1).all()
        if refine == 0:
            for f in keep:
                sel = valid[f] != 0
                r_o, t_o, inl_o = CO.pnp_consensus(model, gt, obj[sel], img[f][sel])
                back = np.zeros(n, bool)
                back[sel] = inl_o
                assert (back == (A["inlier"][f] != 0)).all(), f
                assert np.abs(A["pose"][f, :3] - r_o).max() < 1e-9 and np.abs(A["pose"][f, 3:] - t_o).max() < 1e-8, f
            assert A["inlier"][3].sum() == valid[3].sum() - 2 and (A["inlier"][4] == valid[4]).all()
    for rounds, mdl in ((0, model), (3, 2)):
        with pytest.raises(capi.EcalError):
            _pnp_dev(ctx, obj, img_b, valid, mdl, gt, 4.0, rounds, 0)
        with pytest.raises(capi.EcalError):
            capi.pnp_batch(ctx, obj, img_b, valid, mdl, gt, 4.0, rounds, 0)


# ---- 5. entry points --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,flags,aspect", [(0, SC.FLAGS_EXAMPLE, 1.0), (1, SC.FLAGS_FISHEYE, 0.0)])
def test_intrinsic_guess_arrives_at_the_same_minimum(ctx, model, flags, aspect):
    """CALIB_USE_INTRINSIC_GUESS with fx, fy 2 % wrong == the run without a guess, at the bounds of
    test_calibrate_matches_oracle_on_noisy_views (the guess's principal point is the image centre the run without a guess
    starts from: FLAGS_EXAMPLE fixes it, so another one would be another problem); fx <= 0 or a NaN principal point in the
    guess is refused."""
    from eventcalib_amd import capi
    obj, img, rv, tv = SC.make_views(10, model, seed=21, noise_px=0.2)
    ref = capi.calibrate_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, model, flags, aspect)
    guess = (SC.GT_PINHOLE if model == 0 else SC.GT_FISHEYE).copy()
    guess[:2] *= 1.02
    assert guess[2] == (SC.WIDTH - 1) * 0.5 and guess[3] == (SC.HEIGHT - 1) * 0.5
    out = capi.calibrate_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, model, flags | capi.CALIB_USE_INTRINSIC_GUESS, aspect, intr_guess=guess)
    assert abs(out["rms"] - ref["rms"]) < 1e-7
    assert np.abs(out["intr"][:4] / ref["intr"][:4] - 1).max() < 1e-5
    assert np.abs(out["intr"][4:] - ref["intr"][4:]).max() < 1e-4
    assert np.abs(out["per_view_err"]).max() < 1.0
    for j, bad in ((0, 0.0), (1, -300.0), (2, np.nan), (3, np.nan)):
        g = guess.copy()
        g[j] = bad
        with pytest.raises(capi.EcalError):
            capi.calibrate_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, model, flags | capi.CALIB_USE_INTRINSIC_GUESS, aspect, intr_guess=g)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_fisheye_start_is_the_references_on_a_wide_lens(ctx, seed):
    """ecal_calibrate_fisheye_views on GT_FISHEYE views: the reference's own start (f = max(w, h) / pi) converges,
    start_used == 0; with a guess: one run, start_used == 2; both recover the ground truth."""
    from eventcalib_amd import capi
    obj, img, rv, tv = SC.make_views(16, 1, seed=seed)
    out = capi.calibrate_fisheye_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, SC.FLAGS_FISHEYE)
    assert out["start_used"] == 0
    assert np.abs(out["intr"][:4] / SC.GT_FISHEYE[:4] - 1).max() < 1e-7 and out["rms"] < 1e-8
    guess = SC.GT_FISHEYE.copy()
    guess[:2] *= 1.02
    out = capi.calibrate_fisheye_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, SC.FLAGS_FISHEYE | capi.CALIB_USE_INTRINSIC_GUESS,
                                       intr_guess=guess)
    assert out["start_used"] == 2
    assert np.abs(out["intr"][:4] / SC.GT_FISHEYE[:4] - 1).max() < 1e-7 and out["rms"] < 1e-8


NARROW_FISHEYE = np.array([359.7, 359.7, 172.5, 129.5, 0.0, 0.02, -0.005, 0.0, 0.0, 0, 0, 0])


def test_fisheye_start_falls_back_on_a_narrow_lens(ctx):
    """A 55-degree lens under the fisheye model (poses of the radial generator, projected with model 1, noise-free): the
    180-degree start is far off and ends singular on some view sets (marginal per seed: the oracle's restatement of that
    start ends singular on seeds 12 and 13 and converges on 11).  Whichever branch is taken, fx and fy come back within 1e-6
    relative; and at least one seed takes the fallback (start_used == 1), so that branch is exercised."""
    from eventcalib_amd import capi
    used = []
    for seed in (11, 12, 13):
        obj, _, rv, tv = SC.make_views(16, 0, seed=seed)
        img = np.array([SC.project(1, NARROW_FISHEYE, rv[v], tv[v], obj) for v in range(16)])
        out = capi.calibrate_fisheye_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, SC.FLAGS_FISHEYE)
        used.append(out["start_used"])
        print("seed %d: start_used %d, fx fy %r, rms %.2e, %d iterations" % (seed, out["start_used"], out["intr"][:2], out["rms"], out["iterations"]))
        assert out["start_used"] in (0, 1)
        assert np.abs(out["intr"][:2] / NARROW_FISHEYE[:2] - 1).max() < 1e-6, (seed, out["start_used"], out["intr"])
    assert 1 in used, used


def test_calibrate_on_a_128_point_board(ctx):
    """test_calibrate_recovers_ground_truth and test_calibrate_matches_oracle_on_noisy_views at 16x8, V = 8, with their bounds."""
    from eventcalib_amd import capi
    board = RC.board(16, 8)
    obj, img, rv, tv = SC.make_views(8, 0, seed=11, obj=board)
    out = capi.calibrate_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, 0, SC.FLAGS_EXAMPLE, 1.0)
    gt = SC.GT_PINHOLE
    assert out["rms"] < 1e-8
    assert np.abs(out["intr"][:4] / gt[:4] - 1).max() < 1e-7
    assert np.abs(out["intr"][4:] - gt[4:]).max() < 1e-6
    assert np.abs(out["rvecs"] - rv).max() < 1e-7 and np.abs(out["tvecs"] - tv).max() < 1e-5
    obj, img, rv, tv = SC.make_views(8, 0, seed=21, noise_px=0.2, obj=board)
    out = capi.calibrate_views(ctx, obj, img, SC.WIDTH, SC.HEIGHT, 0, SC.FLAGS_EXAMPLE, 1.0)
    intr, rvs, tvs, rms, it = CO.calibrate(0, obj, img, SC.WIDTH, SC.HEIGHT, SC.FLAGS_EXAMPLE, 1.0)
    assert abs(out["rms"] - rms) < 1e-7
    assert np.abs(out["intr"][:4] / intr[:4] - 1).max() < 1e-5
    assert np.abs(out["intr"][4:] - intr[4:]).max() < 1e-4
    assert np.abs(out["per_view_err"]).max() < 1.0
