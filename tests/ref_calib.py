"""TEST INFRASTRUCTURE ONLY — a plain high-precision reference of the init calibration's arithmetic (ecal_calib.hip):
projection, per-view normal-equation blocks, the Schur-reduced record and one damped step.  CPU only, torch.float64 on
"cpu" for the derivatives (autograd, no finite differences, no hand-written Jacobian), numpy for the linear algebra.

Everything that is solved is solved twice: in float64 with numpy.linalg and in numpy.longdouble with a hand-written
Cholesky / Gauss elimination.  The difference between the two is this reference's own error; the GPU tests derive their
tolerances from it (tests/test_gpu_calib_kernels.py).  Where the machine has no extended type (HAVE_EXTENDED False) the
second computation is a float64 one too and the tests fall back to a fixed 1e-9 of the group scale.

Parameter vector p = [intr 12 | V x (rvec 3, tvec 3)], as oracle/calib_oracle.py."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import calib_oracle as CO  # noqa: E402
import synth_calib as SC  # noqa: E402

NI = 12
BLOCK_DOUBLES = 272     # Hii 144 | Hiv 72 | Hvv 36 | gi 12 | gv 6 | cost | pad
RED_DOUBLES = 170       # S 144 | g 12 | diag sum Hii 12 | cost | points
O_HIV, O_HVV, O_GI, O_GV, O_COST = 144, 216, 252, 264, 270
R_G, R_D, R_COST, R_NPTS = 144, 156, 168, 169

LD = np.longdouble
HAVE_EXTENDED = bool(np.finfo(LD).eps < 1e-17)
FALLBACK_TOL = 1e-9     # of the group scale, as tests/test_gpu_solver.py holds its normal equations

BOARDS = [(2, 2), (3, 3), (9, 7), (8, 8), (13, 5), (10, 10), (16, 8)]


def board(rows, cols):
    """A rows x cols asymmetric board scaled to the footprint of the 9 x 4 one (44 x 38.5), so that synth_calib.make_views'
    poses still keep the whole board inside the image."""
    return SC.board(rows, cols, square=44.0 / max(rows - 1, 2 * cols - 1))


# ---- projection (torch, float64) ---------------------------------------------------------------------------------------
def rodrigues(rvec):
    th = torch.sqrt((rvec * rvec).sum())
    r = rvec / th
    z = torch.zeros((), dtype=rvec.dtype)
    K = torch.stack([torch.stack([z, -r[2], r[1]]), torch.stack([r[2], z, -r[0]]), torch.stack([-r[1], r[0], z])])
    c, s = torch.cos(th), torch.sin(th)
    return c * torch.eye(3, dtype=rvec.dtype) + (1 - c) * torch.outer(r, r) + s * K


def project(model, intr, rvec, tvec, obj):
    """Pixels [n][2] of obj [n][3]; the formulas of oracle/calib_oracle.py::project on torch tensors."""
    X = obj @ rodrigues(rvec).T + tvec
    x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    if model == 0:
        fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = [intr[j] for j in range(12)]
        r2 = x * x + y * y
        r4, r6 = r2 * r2, r2 * r2 * r2
        g = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
        xd = x * g + p1 * 2 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * g + p1 * (r2 + 2 * y * y) + p2 * 2 * x * y
        return torch.stack([fx * xd + cx, fy * yd + cy], 1)
    fx, fy, cx, cy, alpha, k1, k2, k3, k4 = [intr[j] for j in range(9)]
    r = torch.sqrt(x * x + y * y)
    th = torch.atan(r)
    th2 = th * th
    sc = th * (1 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4)))) / r
    xp, yp = sc * x, sc * y
    return torch.stack([fx * (xp + alpha * yp) + cx, fy * yp + cy], 1)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float64), dtype=torch.float64, device="cpu")


def effective_intr(model, flags, aspect, intr):
    intr = np.array(intr, np.float64)
    if model == 0 and (flags & CO.FIX_ASPECT_RATIO):
        intr[0] = aspect * intr[1]
    return intr


def view_residuals(model, flags, aspect, p, obj, img, v):
    """projected - measured of view v, [2n] (u0 v0 u1 v1 ...), float64 numpy."""
    intr = effective_intr(model, flags, aspect, p[:NI])
    q = p[NI + 6 * v: NI + 6 * v + 6]
    with torch.no_grad():
        r = project(model, _t(intr), _t(q[:3]), _t(q[3:]), _t(obj)) - _t(img[v])
    return r.reshape(-1).numpy()


def cost(model, flags, aspect, p, obj, img):
    return float(sum((view_residuals(model, flags, aspect, p, obj, img, v).astype(LD) ** 2).sum() for v in range(img.shape[0])))


def view_jacobian(model, flags, aspect, p, obj, img, v):
    """(J [2n][18], r [2n]) of view v over its 18 parameters (12 intrinsics, rvec, tvec), autograd in float64.  Fixed
    intrinsics columns are zero (CO.free_mask); with a fixed aspect ratio fx = aspect * fy: column 0 is zero and column 1
    carries both focal lengths' derivatives."""
    intr = effective_intr(model, flags, aspect, p[:NI])
    pv = _t(np.concatenate([intr, p[NI + 6 * v: NI + 6 * v + 6]]))
    tobj, timg = _t(obj), _t(img[v])

    def f(z):
        return (project(model, z[:NI], z[NI:NI + 3], z[NI + 3:], tobj) - timg).reshape(-1)

    J = torch.autograd.functional.jacobian(f, pv).numpy().copy()
    r = f(pv).detach().numpy().copy()
    if model == 0 and (flags & CO.FIX_ASPECT_RATIO):
        J[:, 1] += aspect * J[:, 0]
        J[:, 0] = 0.0
    J[:, :NI] *= CO.free_mask(model, flags)
    return J, r


def _blocks_of(J, r, dtype):
    J, r = J.astype(dtype), r.astype(dtype)
    H = J.T @ J
    g = J.T @ r
    return H, g, r @ r


def view_blocks(model, flags, aspect, p, obj, img, v, dtype=np.float64):
    """The 272 doubles ecal_calib_view_blocks_dev writes for view v (pad slot zero), accumulated in dtype."""
    H, g, c = _blocks_of(*view_jacobian(model, flags, aspect, p, obj, img, v), dtype)
    out = np.zeros(BLOCK_DOUBLES, dtype)
    out[:O_HIV] = H[:NI, :NI].ravel()
    out[O_HIV:O_HVV] = H[:NI, NI:].ravel()
    out[O_HVV:O_GI] = H[NI:, NI:].ravel()
    out[O_GI:O_GV] = g[:NI]
    out[O_GV:O_COST] = g[NI:]
    out[O_COST] = c
    return out


def all_view_blocks(model, flags, aspect, p, obj, img):
    """[(J, r)] of every view: the autograd part, computed once and shared by normal_matrix / reduced_record / step."""
    return [view_jacobian(model, flags, aspect, p, obj, img, v) for v in range(img.shape[0])]


def normal_matrix(jr, dtype=np.float64):
    """Full (12 + 6V)-square normal matrix, gradient and cost from all_view_blocks' list."""
    V = len(jr)
    H, g, c = np.zeros((NI + 6 * V, NI + 6 * V), dtype), np.zeros(NI + 6 * V, dtype), dtype(0)
    for v, (J, r) in enumerate(jr):
        Hv, gv, cv = _blocks_of(J, r, dtype)
        s = slice(NI + 6 * v, NI + 6 * v + 6)
        H[:NI, :NI] += Hv[:NI, :NI]
        H[:NI, s] = Hv[:NI, NI:]
        H[s, :NI] = Hv[NI:, :NI]
        H[s, s] = Hv[NI:, NI:]
        g[:NI] += gv[:NI]
        g[s] = gv[NI:]
        c += cv
    return H, g, c


# ---- hand-written extended-precision linear algebra --------------------------------------------------------------------
def cholesky_solve_ld(A, B):
    """X = A^-1 B for SPD A, numpy.longdouble, Cholesky A = L L^T then two triangular solves."""
    A, X = np.array(A, LD), np.array(B, LD).reshape(A.shape[0], -1)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    for i in range(n):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X.reshape(np.shape(B))


def gauss_solve_ld(A, b):
    """x = A^-1 b, numpy.longdouble, Gauss elimination with partial pivoting."""
    A, b = np.array(A, LD), np.array(b, LD)
    n = A.shape[0]
    for c in range(n):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        if piv != c:
            A[[c, piv]] = A[[piv, c]]
            b[[c, piv]] = b[[piv, c]]
        for r in range(c + 1, n):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    for r in range(n - 1, -1, -1):
        b[r] = (b[r] - A[r, r + 1:] @ b[r + 1:]) / A[r, r]
    return b


# ---- reduced record and step -------------------------------------------------------------------------------------------
def _reduced(jr, lam, n_pts, dtype):
    S, g, d, c = np.zeros((NI, NI), dtype), np.zeros(NI, dtype), np.zeros(NI, dtype), dtype(0)
    for J, r in jr:
        H, gg, cv = _blocks_of(J, r, dtype)
        Hii, Hiv, Hvv = H[:NI, :NI], H[:NI, NI:], H[NI:, NI:].copy()
        Hvv[np.diag_indices(6)] *= dtype(1) + dtype(lam)
        if dtype is np.float64:
            Wt = np.linalg.solve(Hvv, np.column_stack([Hiv.T, gg[NI:]]))      # Hvv'^-1 [Hvi | gv]
        else:
            Wt = cholesky_solve_ld(Hvv, np.column_stack([Hiv.T, gg[NI:]]))
        S += Hii - Hiv @ Wt[:, :NI]
        g += gg[:NI] - Hiv @ Wt[:, NI]
        d += np.diag(Hii)
        c += cv
    return np.concatenate([S.ravel(), g, d, [c, dtype(len(jr) * n_pts)]])


def reduced_record(jr, lam, n_pts):
    """The 170 doubles the ranks all-reduce: S = sum_v Hii - Hiv Hvv'^-1 Hvi | g = sum_v gi - Hiv Hvv'^-1 gv | diag sum Hii |
    cost | points, with Hvv' = Hvv damped as Hvv * (1 + lam) on the diagonal.  Returns (float64 / numpy.linalg,
    longdouble / hand-written Cholesky)."""
    return _reduced(jr, lam, n_pts, np.float64), _reduced(jr, lam, n_pts, LD if HAVE_EXTENDED else np.float64)


def free_slots(model, flags, V):
    return np.flatnonzero(np.concatenate([CO.free_mask(model, flags), np.ones(6 * V)]))


def step(jr, lam, model, flags):
    """x of (H + lam diag H) x = g over the free slots (zero elsewhere), [12 + 6V].  Returns (float64 / numpy.linalg.solve,
    longdouble / hand-written Gauss elimination)."""
    idx = free_slots(model, flags, len(jr))
    out = []
    for dtype in (np.float64, LD if HAVE_EXTENDED else np.float64):
        H, g, _ = normal_matrix(jr, dtype)
        A = H[np.ix_(idx, idx)].copy()
        A[np.diag_indices_from(A)] *= dtype(1) + dtype(lam)
        x = np.zeros(H.shape[0], dtype)
        x[idx] = np.linalg.solve(A, g[idx]) if dtype is np.float64 else gauss_solve_ld(A, g[idx])
        out.append(x)
    return out[0], out[1]


def step_by_schur(jr, lam, model, flags):
    """The same step the way the GPU path takes it — eliminate every view, solve the 12 x 12 head, back-substitute — in plain
    numpy float64.  tests/test_ref_calib.py holds step() against it."""
    V = len(jr)
    rec = _reduced(jr, lam, 1, np.float64)
    idx = np.flatnonzero(CO.free_mask(model, flags))
    A = rec[:R_G].reshape(NI, NI)[np.ix_(idx, idx)].copy()
    A[np.diag_indices_from(A)] += lam * rec[R_D:R_COST][idx]
    x = np.zeros(NI + 6 * V)
    x[idx] = np.linalg.solve(A, rec[R_G:R_D][idx])
    for v, (J, r) in enumerate(jr):
        H, g, _ = _blocks_of(J, r, np.float64)
        Hvv = H[NI:, NI:].copy()
        Hvv[np.diag_indices(6)] *= 1 + lam
        x[NI + 6 * v: NI + 6 * v + 6] = np.linalg.solve(Hvv, g[NI:] - H[NI:, :NI] @ x[:NI])
    return x


def group_tolerance(a64, ald, scale, factor=16.0, floor=1e-13):
    """(tolerance, spread): spread = the largest |float64 - longdouble| of the reference in units of scale (entries whose scale is
    zero are exact zeros and do not count); tolerance = max(factor * spread, floor), or FALLBACK_TOL without an extended type."""
    scale = np.asarray(scale, np.float64)
    d = np.abs(np.asarray(a64, LD) - np.asarray(ald, LD)).astype(np.float64)
    nz = scale > 0
    spread = float((d[nz] / scale[nz]).max()) if nz.any() else 0.0
    if not HAVE_EXTENDED:
        return FALLBACK_TOL, spread
    return max(factor * spread, floor), spread


# ---- the inputs of the first-step tests (shared by tests/test_ref_calib.py and tests/test_gpu_calib_kernels.py) ------------
FISHEYE_STEP_FLAGS = CO.FIX_SKEW | CO.FIX_K4      # no RECOMPUTE_EXTRINSIC: the poses take the back-substituted step
# (model, flags, aspect, (rows, cols), V)
STEP_CASES = [(0, SC.FLAGS_EXAMPLE, 1.0, (9, 4), V) for V in (1, 2, 3, 4, 5, 9)] + [
    (0, 0, 0.0, (16, 8), 3), (0, SC.FLAGS_EXAMPLE, 1.0, (3, 3), 9), (1, FISHEYE_STEP_FLAGS, 0.0, (13, 5), 4)]


def step_case_id(case):
    model, flags, _, (rows, cols), V = case
    return "%s-flags%x-%dx%d-V%d" % ("pinhole" if model == 0 else "fisheye", flags, rows, cols, V)


def step_inputs(case):
    """(obj, img, guess): 0.3 px noisy views of the ground-truth camera and the guess the run starts from — the ground truth
    with fx, fy off by 1 % (fx = aspect * fy kept when the aspect ratio is fixed)."""
    model, flags, aspect, (rows, cols), V = case
    obj, img, _, _ = SC.make_views(V, model, seed=40 + V + rows, noise_px=0.3, obj=board(rows, cols))
    guess = (SC.GT_PINHOLE if model == 0 else SC.GT_FISHEYE).copy()
    guess[:2] *= 1.01
    guess = effective_intr(model, flags, aspect, guess)
    return obj, img, guess
