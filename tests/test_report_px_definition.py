"""CPU: what the report in pixels MEANS (include/ecal.h, "report in pixels") — a numpy restatement of the rule,
r_px = r / |d r / d (u, v)|, against the brute-force distance from the event to the projected rim of its circle.  This pins the
definition, not the kernels: tests/test_gpu_report_px.py holds the kernels to the existing residual and Jacobian.

The restatement: the residual of spline_residual.hpp (quaternion spline; radial or fisheye inverse polynomial) as a numpy function
of the event's pixel, its gradient by central differences (step 1e-4 px: the truncation error is a third derivative times 1e-8).
The brute force: the rim of the landmark's circle on the board, forward-projected through the ground-truth pose and camera by
synth_solver's Newton iteration, sampled in two levels — 720 angles, then 2001 angles across the two coarse steps around the
nearest — so that neighbouring samples are ~8e-5 px apart and the nearest sample is within 4e-5 px (< 1e-4) of the nearest point
of the curve; the distance takes the sign of r.

Data: synth_solver problems at the ground truth, radial and fisheye, pixel noise 0.5 and 2 px, 300 residuals, n_cp = 8.

|r_px - d_true| is a SECOND-order quantity (curvature of the projected rim and of the camera model across the distance) and no
bound on it is derived here.  GAP_MEASURED holds what this restatement measured when the test was written (design/23_report_px.md
has the table); the test asserts the gap with a margin of 2 on those figures.  The statistical statement is derived: at the
ground truth with pixel noise sigma, r_px is the noise's component across the rim, so its RMS over n records is sigma within
5 / sqrt(2 n) (five standard deviations of an RMS of n normal samples) + sigma / rho (the curvature term, rho ~ 9.5 px the
projected rim radius) relative.
"""
import functools

import numpy as np
import pytest

import synth_solver as SV

N_RES, N_CP = 300, 8
RHO_PX = 9.5
# max |r_px - d_true| in pixels per (fisheye, pixel noise), measured by this file's restatement (seed as below)
GAP_MEASURED = {(False, 0.5): 0.00201, (True, 0.5): 0.00138, (False, 2.0): 0.04645, (True, 2.0): 0.02238}


def _poly(intr, r2):
    return 1 + intr[4] * r2 + intr[5] * r2 ** 2 + intr[6] * r2 ** 3 + intr[7] * r2 ** 4 + intr[8] * r2 ** 5


def _rotate(q, v):
    """R(q) v for unit quaternions q [..., 4] (xyzw) and vectors v [..., 3]"""
    u, w = q[..., :3], q[..., 3:4]
    uv = 2.0 * np.cross(u, v)
    return v + w * uv + np.cross(u, uv)


def _poses(prob, x):
    """the pose (unit quaternion, translation) of every record: spline_residual's blend and normalisation"""
    kn, n_cp = prob["knots"], N_CP
    q_cp, t_cp = x[9:9 + 4 * n_cp].reshape(n_cp, 4), x[9 + 4 * n_cp:].reshape(n_cp, 3)
    Q, T = [], []
    for u in prob["time"]:
        sp = SV.find_span(kn, n_cp, u)
        b = SV.basis(kn, sp, u)
        qv = b @ q_cp[sp - 3: sp + 1]
        Q.append(qv / np.linalg.norm(qv))
        T.append(b @ t_cp[sp - 3: sp + 1])
    return np.array(Q), np.array(T)


def _residual(px, intr, fisheye, Q, T, lm):
    """r of the rule for pixels px [n, 2]: inverse camera model, rotation, ray / plane z = 0, |Xw - lm| - radius"""
    xy = (px - intr[2:4]) / intr[0:2]
    r2 = (xy * xy).sum(axis=1)
    poly = _poly(intr, r2)
    if fisheye:
        r = np.sqrt(r2)
        c = np.where(r2 > 1e-16, np.tan(r * poly) / np.where(r > 0, r, 1.0), poly)
    else:
        c = poly
    p = np.concatenate([xy * c[:, None], np.ones((len(px), 1))], axis=1)
    Y = _rotate(Q, p)
    s = -T[:, 2] / Y[:, 2]
    Xw = T + s[:, None] * Y
    return np.linalg.norm(Xw - lm, axis=1) - SV.RADIUS


def _sampson(px, *a):
    """(r, r_px, |g|): the rule with central differences"""
    h = 1e-4
    r = _residual(px, *a)
    gu = (_residual(px + [h, 0.0], *a) - _residual(px - [h, 0.0], *a)) / (2 * h)
    gv = (_residual(px + [0.0, h], *a) - _residual(px - [0.0, h], *a)) / (2 * h)
    g2 = gu * gu + gv * gv
    assert np.isfinite(r).all() and np.isfinite(g2).all() and (g2 > 0).all()      # no degenerate record on these problems
    return r, r / np.sqrt(g2), np.sqrt(g2)


def _project(Xw, intr, fisheye, Q, T):
    """forward projection of board points Xw [n, m, 3] through pose n: synth_solver.make_problem's Newton, vectorised"""
    Qc = Q * np.array([-1.0, -1.0, -1.0, 1.0])
    Xc = _rotate(Qc[:, None, :], Xw - T[:, None, :])
    assert (Xc[..., 2] > 1e-6).all()
    pu = Xc[..., :2] / Xc[..., 2:3]
    ru = np.linalg.norm(pu, axis=-1)
    target = np.arctan(ru) if fisheye else ru
    rd = target.copy()
    for _ in range(50):
        r2 = rd * rd
        c = _poly(intr, r2)
        dc = 2 * rd * (intr[4] + 2 * intr[5] * r2 + 3 * intr[6] * r2 ** 2 + 4 * intr[7] * r2 ** 3 + 5 * intr[8] * r2 ** 4)
        rd = rd - (rd * c - target) / (c + rd * dc)
    assert np.abs(rd * _poly(intr, rd * rd) - target).max() < 1e-13
    pd = pu * (rd / np.where(ru > 0, ru, 1.0))[..., None]
    return pd * intr[0:2] + intr[2:4]


def _brute_force(px, intr, fisheye, Q, T, lm):
    """(distance from px to the nearest sample of the projected rim, the largest spacing of the fine samples)"""
    def rim(ang):
        return lm[:, None, :] + SV.RADIUS * np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], axis=-1)
    n = len(px)
    coarse = np.broadcast_to(np.linspace(0.0, 2 * np.pi, 720, endpoint=False), (n, 720))
    d = np.linalg.norm(_project(rim(coarse), intr, fisheye, Q, T) - px[:, None, :], axis=-1)
    best = coarse[np.arange(n), d.argmin(axis=1)]
    step = 2 * np.pi / 720
    fine = best[:, None] + np.linspace(-step, step, 2001)[None, :]
    pts = _project(rim(fine), intr, fisheye, Q, T)
    d = np.linalg.norm(pts - px[:, None, :], axis=-1)
    k = d.argmin(axis=1)
    assert ((k > 0) & (k < 2000)).all()                     # the minimum lies inside the refined arc
    return d.min(axis=1), np.linalg.norm(np.diff(pts, axis=1), axis=-1).max()


@functools.lru_cache(maxsize=None)
def _case(fisheye, noise):
    prob, x = SV.make_problem(N_RES, n_cp=N_CP, seed=23, pixel_noise=noise, fisheye=fisheye)
    intr = x[:9]
    Q, T = _poses(prob, x)
    lm = prob["landmarks"][prob["lm_id"]]
    args = (intr, fisheye, Q, T, lm)
    r, r_px, gnorm = _sampson(prob["obs"], *args)
    d, spacing = _brute_force(prob["obs"], *args)
    return r, r_px, gnorm, np.sign(r) * d, spacing


CASES = [(False, 0.5), (True, 0.5), (False, 2.0), (True, 2.0)]


@pytest.mark.parametrize("fisheye,noise", CASES)
def test_first_order_distance_is_the_distance_to_the_projected_rim(fisheye, noise):
    r, r_px, gnorm, d_true, spacing = _case(fisheye, noise)
    assert 0.5 * spacing < 1e-4                            # the brute force's own error, pixels
    gap = np.abs(r_px - d_true).max()
    rms = lambda a: float(np.sqrt((a * a).mean()))         # noqa: E731
    print("%s noise %.1f px: rms r_px %.4f, rms brute force %.4f, rms board units %.4f, max |r_px - d_true| %.5f px, px per unit %.3f, "
          "sample spacing %.2g px" % ("fisheye" if fisheye else "radial", noise, rms(r_px), rms(d_true), rms(r), gap, (1 / gnorm).mean(), spacing))
    assert gap <= 2.0 * GAP_MEASURED[(fisheye, noise)]
    # second order: a quarter of the noise makes the gap much smaller than a quarter (what a first-order error would not do)
    if noise == 2.0:
        small = np.abs(_case(fisheye, 0.5)[1] - _case(fisheye, 0.5)[3]).max()
        assert small < gap / 4.0


@pytest.mark.parametrize("fisheye,noise", CASES)
def test_rms_in_pixels_is_the_pixel_noise(fisheye, noise):
    r, r_px, gnorm, _, _ = _case(fisheye, noise)
    rms_px = float(np.sqrt((r_px * r_px).mean()))
    margin = 5.0 / np.sqrt(2 * N_RES) + noise / RHO_PX
    print("noise %.1f px: rms r_px %.4f, relative deviation %.4f, margin %.4f; the board-unit rms %.4f says nothing of the kind" % (
        noise, rms_px, abs(rms_px - noise) / noise, margin, float(np.sqrt((r * r).mean()))))
    assert abs(rms_px - noise) <= margin * noise
