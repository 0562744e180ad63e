"""CPU: the sigma map's Jacobian and sigma_px on the host (ecal_uncertainty_map_host: eventcalib_amd/csrc/uncertainty_point.hpp, no
device) against torch.autograd.functional.jacobian in f64 on a torch restatement of the ray (X, Y) = (x, y) g(rho) of
include/ecal_uncertainty.h — both camera models, a sensor wide enough that the model turns invalid inside it, the pixel at the
principal point (rho = 0), the four corners, the pixels on both sides of the validity edge and a coarse grid.

The figures: per pixel and row of J the largest |difference| over the largest |entry| of that row; for sigma_px the relative
difference.  MEASURED holds the largest value over this grid as measured on the CPU (printed by every run); the test allows 16 x
that, because autograd orders the operations differently (design/24_uncertainty.md records the values)."""
import numpy as np
import pytest
import torch

import synth_solver as SV
from eventcalib_amd import capi, uncertainty

W, H = 900, 640
# fx fy cx cy k1..k5: tests/synth_solver.py's cameras with a principal point ON a pixel, so that rho = 0 is on the grid (the fisheye lens
# shorter, so that theta reaches pi / 2 inside the sensor)
INTR = {"radial": np.r_[359.67525, 361.25, 440.0, 300.0, SV.GT_INTR[4:]], "fisheye": np.r_[250.5, 251.25, 440.0, 300.0, SV.GT_INTR_FISHEYE[4:]]}
MEASURED = {"radial": (3.11e-16, 5.01e-16), "fisheye": (2.61e-15, 2.54e-15)}   # (J, sigma_px)
ALLOW = 16.0


def _cov():
    rng = np.random.default_rng(5)
    a = np.diag([0.5, 0.4, 0.3, 0.35, 1e-3, 5e-3, 2e-2, 5e-2, 1e-1]) @ rng.normal(size=(9, 12))
    return a @ a.T / 12.0


def _ray(intr, u, v, fisheye):
    """(X, Y) [2, N] and the validity of include/ecal_uncertainty.h, in torch"""
    fx, fy, cx, cy = intr[0], intr[1], intr[2], intr[3]
    x, y = (u - cx) / fx, (v - cy) / fy
    rho = x * x + y * y
    P = 1.0 + intr[4] * rho + intr[5] * rho ** 2 + intr[6] * rho ** 3 + intr[7] * rho ** 4 + intr[8] * rho ** 5
    if fisheye:
        small = rho <= 1e-16
        td = torch.sqrt(torch.where(small, torch.ones_like(rho), rho))
        theta = td * P
        g = torch.where(small, P, torch.tan(theta) / td)
        ok = torch.where(small, P > 0, (theta >= 0) & (theta < np.pi / 2))
    else:
        g = P
        ok = P > 0
    return torch.stack([x * g, y * g]), ok


def _pixels(flag):
    """principal point, corners, both sides of the validity edge, a coarse grid: (cols, rows)"""
    pts = {(440, 300), (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}
    edge = (flag[:, 1:] != flag[:, :-1])
    rows, cols = np.nonzero(edge)
    for r, c in list(zip(rows, cols))[::7]:
        pts.add((int(c), int(r)))
        pts.add((int(c) + 1, int(r)))
    for r in range(0, H, 41):
        for c in range(0, W, 43):
            pts.add((c, r))
    p = np.array(sorted(pts))
    return p[:, 0], p[:, 1]


@pytest.mark.parametrize("model", ["radial", "fisheye"])
def test_host_jacobian_and_sigma_against_autograd(model):
    fisheye = model == "fisheye"
    intr, cov = INTR[model], _cov()
    sig, flag, jac = uncertainty.uncertainty_map(capi.CAMERA_FISHEYE if fisheye else capi.CAMERA_RADIAL, intr, cov, W, H, jacobian=True)
    assert sig.shape == (H, W) and flag.shape == (H, W) and jac.shape == (H, W, 2, 9)
    assert 0 < int(flag.sum()) < W * H, "the validity edge lies inside the sensor"
    cols, rows = _pixels(flag)
    u, v = torch.tensor(cols, dtype=torch.float64), torch.tensor(rows, dtype=torch.float64)
    k = torch.tensor(intr, dtype=torch.float64)
    _, ok = _ray(k, u, v, fisheye)
    ok = ok.numpy()
    assert np.array_equal(flag[rows, cols] == 0, ok), "flags differ from the restated validity"
    assert (sig[flag == 1] == 0).all() and (jac[flag == 1] == 0).all()
    assert flag[300, 440] == 0                                                       # rho = 0 is a valid pixel
    J_ref = torch.autograd.functional.jacobian(lambda kk: _ray(kk, u, v, fisheye)[0], k, vectorize=True).numpy()   # [2, N, 9]
    J_ref = np.transpose(J_ref, (1, 0, 2))[ok]
    J = jac[rows, cols][ok]
    assert np.isfinite(J_ref).all() and np.isfinite(J).all()
    scale = np.abs(J_ref).max(axis=2, keepdims=True)
    assert (scale > 0).all()
    dJ = float((np.abs(J - J_ref) / scale).max())
    # sigma_px from the autograd Jacobian: E = diag(fx, fy) J, C = E cov E^T, the larger eigenvalue
    E = J_ref * intr[:2][None, :, None]
    C = E @ cov @ np.transpose(E, (0, 2, 1))
    lam = np.linalg.eigvalsh(C)[:, 1]
    s_ref = np.sqrt(lam)
    s = sig[rows, cols][ok]
    assert (s_ref > 0).all()
    dS = float((np.abs(s - s_ref) / s_ref).max())
    print("%s: %d pixels (%d valid), largest difference J %.3e sigma_px %.3e; sigma_px from %.4g to %.4g" % (
        model, len(cols), int(ok.sum()), dJ, dS, s.min(), s.max()))
    assert dJ <= ALLOW * MEASURED[model][0], (dJ, MEASURED[model][0])
    assert dS <= ALLOW * MEASURED[model][1], (dS, MEASURED[model][1])


def test_host_map_refuses_what_the_header_refuses():
    cov = _cov()
    for bad in (dict(width=0), dict(height=8193), dict(intr=np.r_[0.0, INTR["radial"][1:]]), dict(intr=np.r_[np.nan, INTR["radial"][1:]])):
        a = dict(intr=INTR["radial"], width=4, height=4)
        a.update(bad)
        with pytest.raises(capi.EcalError):
            uncertainty.uncertainty_map(capi.CAMERA_RADIAL, a["intr"], cov, a["width"], a["height"])
    # a NaN covariance stays visible
    sig, flag = uncertainty.uncertainty_map(capi.CAMERA_RADIAL, INTR["radial"], np.full((9, 9), np.nan), 3, 2)
    assert np.isnan(sig[flag == 0]).all()
