"""GPU: the sigma map on the device (ecal_uncertainty_map_dev, one thread a pixel) against the host twin (ecal_uncertainty_map_host):
both compile eventcalib_amd/csrc/uncertainty_point.hpp without contraction, so RADIAL agrees bit for bit; FISHEYE goes through tan,
which the two math libraries round differently, and is held to 16 x MEASURED_FISHEYE, the largest relative difference of sigma_px
measured over these maps on the MI355X (printed by every run; design/24_uncertainty.md records it).  Sizes 1 x 1, 65 x 3 and
346 x 260 (the last two not multiples of the 256-thread block); the flags are equal in every case."""
import numpy as np
import pytest

import synth_solver as SV

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (65, 3), (346, 260)]
MEASURED_FISHEYE = 8.66e-16
ALLOW = 16.0


def _cov():
    rng = np.random.default_rng(5)
    a = np.diag([0.5, 0.4, 0.3, 0.35, 1e-3, 5e-3, 2e-2, 5e-2, 1e-1]) @ rng.normal(size=(9, 12))
    return a @ a.T / 12.0


def _intr(model, width, height):
    """the synthetic cameras, the principal point on a pixel; the fisheye lens short enough that theta passes pi / 2 at 346 x 260"""
    k = (SV.GT_INTR_FISHEYE if model == "fisheye" else SV.GT_INTR)[4:]
    f = 95.0 if model == "fisheye" else 359.67525
    return np.r_[f, f * 1.004, float(width // 2), float(height // 2), k]


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("model", ["radial", "fisheye"])
def test_device_map_against_the_host_map(ctx, model, size):
    import torch
    from eventcalib_amd import capi, uncertainty
    w, h = size
    cam = capi.CAMERA_FISHEYE if model == "fisheye" else capi.CAMERA_RADIAL
    intr, cov = _intr(model, w, h), _cov()
    sig_h, flag_h = uncertainty.uncertainty_map(cam, intr, cov, w, h)
    d_sig, d_flag = uncertainty.uncertainty_map_dev(ctx, cam, intr, cov, w, h)
    torch.cuda.synchronize()
    sig_d, flag_d = d_sig.cpu().numpy(), d_flag.cpu().numpy()
    assert sig_d.shape == (h, w) and flag_d.shape == (h, w) and sig_d.dtype == np.float64 and flag_d.dtype == np.uint8
    assert np.array_equal(flag_d, flag_h)
    assert (sig_d[flag_d == 1] == 0).all() and (sig_d[flag_d == 0] > 0).all() and flag_h[h // 2, w // 2] == 0
    if (w, h) == (346, 260) and model == "fisheye":
        assert 0 < int(flag_h.sum()) < w * h, "the validity edge lies inside the sensor"
    if model == "radial":
        assert np.array_equal(sig_d, sig_h)
        return
    ok = flag_h == 0
    rel = float((np.abs(sig_d[ok] - sig_h[ok]) / sig_h[ok]).max())
    print("fisheye %d x %d: largest relative difference of sigma_px, device against host, %.3e (%d of %d pixels differ)" % (
        w, h, rel, int((sig_d != sig_h).sum()), w * h))
    assert rel <= ALLOW * MEASURED_FISHEYE
