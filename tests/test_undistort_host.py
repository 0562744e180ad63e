"""CPU: the undistortion rule (include/ecal.h, "undistortion").  ecal_undistort_points_host and a plain-g++ build of
eventcalib_amd/csrc/undistort_point.hpp (tests/cpp/check_undistort.cpp) against the numpy restatement tests/undistort_oracle.py:
RADIAL bit for bit; FISHEYE the same flags and coordinates within 1e-9 px (tan is the only operation that is not correctly rounded;
libm, numpy and the device library differ by a few ulp there, the chain amplifies that by less than 10 at th <= 1.2, the result is a
few hundred px: a few 1e-13 px are expected).  The rounding, the reference canvas, every refusal's text, and a round trip through the
forward model as a sanity check of the rule itself."""
import os
import subprocess

import numpy as np
import pytest

import undistort_oracle as UO
from eventcalib_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_undistort.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-O2"]

RADIAL_INTR = [251.3, 249.8, 171.2, 129.9, -0.21, 0.07, -0.012, 0.0011, -0.00004]
FISHEYE_INTR = [180.0, 180.0, 175.5, 127.5, -0.02, 0.003, 0.0, 0.0, 0.0]
ZERO_K_INTR = [2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
FISHEYE_TOL_PX = 1e-9


def case_points():
    """20 000 seeded grid pixels of 346 x 260, half-pixel inputs, negative coordinates, NaN, +-inf"""
    rng = np.random.default_rng(20261020)
    grid = np.stack([rng.integers(0, 346, 20000), rng.integers(0, 260, 20000)], axis=1).astype(np.float64)
    half = grid[:2000] + 0.5
    neg = -grid[:2000] - np.array([1.0, 0.25])
    inf, nan = np.inf, np.nan
    odd = np.array([[nan, 10.0], [10.0, nan], [nan, nan], [inf, 10.0], [10.0, -inf], [-inf, inf], [171.2, 129.9], [175.5, 127.5],
                    [0.0, 0.0], [-0.0, -0.0], [1e300, 1e300], [-1e300, 5.0], [1e-300, 1e-300], [345.0, 259.0]])
    return np.concatenate([grid, half, neg, odd])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("undistort") / "check_undistort")
    subprocess.check_call(["g++"] + FLAGS + ["-o", path, SRC])
    return path


def gxx_points(exe, tmp_path, cam, uv):
    uv = np.ascontiguousarray(uv, np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(bytes(cam))
        f.write(np.uint64(uv.shape[0]).tobytes())
        f.write(uv.tobytes())
    r = subprocess.run([exe, "points", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    n = uv.shape[0]
    return np.frombuffer(raw[: n * 16], np.float64).reshape(n, 2), np.frombuffer(raw[n * 16:], np.uint8)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("intr,out_k", [(RADIAL_INTR, None), (RADIAL_INTR, [300.0, 310.0, 200.5, 150.25]), (ZERO_K_INTR, [1.0, 1.0, 0.0, 0.0]),
                                        ([250.0, 250.0, 175.5, 127.5, -50.0, 0.0, 0.0, 0.0, 0.0], None)])
def test_radial_is_bit_for_bit_the_numpy_rule(exe, tmp_path, intr, out_k):
    uv = case_points()
    cam = capi.undistort_camera(intr, capi.CAMERA_RADIAL, out_k=out_k)
    want, want_flag = UO.points(UO.camera(UO.RADIAL, intr, out_k), uv)
    for name, (got, flag) in (("library", capi.undistort_points_host(cam, uv)), ("g++", gxx_points(exe, tmp_path, cam, uv))):
        assert (flag == want_flag).all(), name
        assert (bits(got) == bits(want)).all(), name
    assert want_flag[-14:-8].all(), "NaN and inf inputs are invalid"
    if intr[4] == -50.0:
        assert want_flag.mean() > 0.9   # (poly <= 0 everywhere but around the principal point)
    else:
        assert want_flag[:20000].sum() == 0


def test_fisheye_flags_equal_and_coordinates_within_1e_9(exe, tmp_path):
    uv = case_points()
    cam = capi.undistort_camera(FISHEYE_INTR, capi.CAMERA_FISHEYE)
    want, want_flag = UO.points(UO.camera(UO.FISHEYE, FISHEYE_INTR), uv)
    assert want_flag[:20000].sum() == 0 and want_flag.sum() > 0
    for name, (got, flag) in (("library", capi.undistort_points_host(cam, uv)), ("g++", gxx_points(exe, tmp_path, cam, uv))):
        assert (flag == want_flag).all(), name
        worst = float(np.abs(got - want).max())
        print("fisheye, %s against numpy: largest difference %.3e px" % (name, worst))
        assert worst <= FISHEYE_TOL_PX, name
    # at the principal point the small-radius branch decides (r2 <= 1e-16): c = poly = 1
    got, flag = capi.undistort_points_host(cam, [[175.5, 127.5]])
    assert flag[0] == 0 and got[0, 0] == 175.5 and got[0, 1] == 127.5


def test_round_half_away(exe):
    below_half = 0.49999999999999994
    assert below_half + 0.5 == 1.0   # (why floor(a + 0.5) is wrong)
    cases = [(0.5, 1.0), (-0.5, -1.0), (1.5, 2.0), (-1.5, -2.0), (below_half, 0.0), (-below_half, 0.0), (2.0 ** 52 + 1.0, 2.0 ** 52 + 1.0),
             (2.5, 3.0), (-2.5, -3.0)]
    for a, want in cases:
        assert capi.undistort_round_half_away(a) == want, a
        assert float(UO.round_half_away(a)) == want, a
    r = subprocess.run([exe, "self"], capture_output=True, text=True)
    assert r.returncode == 0 and "self ok" in r.stdout, r.stdout + r.stderr


def test_reference_canvas():
    for (w, h), (cw, ch) in (((346, 260), (415, 312)), ((640, 480), (768, 576)), ((1280, 720), (1536, 864)), ((5, 3), (6, 4))):
        o = capi.undistort_reference_canvas(w, h)
        assert (o.mode, o.out_width, o.out_height, o.reserved) == (capi.UNDISTORT_PIXEL, cw, ch, 0)
        assert o.off_x == w * 0.1 and o.off_y == h * 0.1
        assert UO.reference_canvas(w, h) == (cw, ch, w * 0.1, h * 0.1)
        assert capi.undistort_options_error(o) is None
    o = capi.undistort_reference_canvas(346, 260)
    assert (o.off_x, o.off_y) == (34.6, 26.0)


def test_every_refusal_names_its_field():
    def cam(**change):
        c = capi.undistort_camera(RADIAL_INTR, change.pop("model", capi.CAMERA_RADIAL), reserved=change.pop("reserved", 0))
        for k, v in change.items():
            arr, i = k.split("_")
            getattr(c, "intr" if arr == "i" else "out_k")[int(i)] = v
        return c

    assert capi.undistort_camera_error(cam()) is None
    for change, word in ([dict(i_0=v) for v in (0.0, -1.0, np.nan, np.inf)], "fx "), ([dict(i_1=v) for v in (0.0, -2.0, np.nan, -np.inf)], "fy "), \
                        ([dict(o_0=v) for v in (0.0, -1.0, np.nan, np.inf)], "fx'"), ([dict(o_1=v) for v in (0.0, -1.0, np.nan, np.inf)], "fy'"), \
                        ([dict(i_4=np.nan), dict(i_4=np.inf)], "k1"), ([dict(i_5=np.nan)], "k2"), ([dict(i_6=-np.inf)], "k3"), \
                        ([dict(i_7=np.nan)], "k4"), ([dict(i_8=np.inf)], "k5"), ([dict(reserved=1)], "reserved"), \
                        ([dict(model=2), dict(model=-1)], "model"):
        for ch in change:
            c = cam(**ch)
            err = capi.undistort_camera_error(c)
            assert err is not None and word in err, (ch, err)
            with pytest.raises(capi.EcalError) as e:
                capi.undistort_points_host(c, [[1.0, 2.0]])
            assert e.value.status == -1 and word in str(e.value)
    # a principal point or an ideal principal point may be anything finite or not: the rule's own validity takes care of it
    assert capi.undistort_camera_error(cam(i_2=-5.0, o_3=1e9)) is None
    ok = capi.undistort_reference_canvas(346, 260)
    assert capi.undistort_options_error(ok) is None and capi.undistort_options_error(capi.undistort_options()) is None
    for change, word in ((dict(mode=2), "mode"), (dict(out_width=0), "out_width"), (dict(out_width=8193), "out_width"),
                         (dict(out_height=0), "out_height"), (dict(out_height=8193), "out_height"), (dict(reserved=3), "reserved"),
                         (dict(off_x=np.nan), "off_x"), (dict(off_y=np.inf), "off_y")):
        o = capi.undistort_options(sensor=(346, 260), **change)
        err = capi.undistort_options_error(o)
        assert err is not None and word in err, (change, err)
    assert capi.undistort_options_error(capi.undistort_options(sensor=(346, 260), out_width=8192, out_height=1)) is None


def test_gxx_stream_form_is_the_oracle(exe, tmp_path):
    """the sequential statement of the stream form (ud_events_sequential) against the oracle, both modes"""
    rng = np.random.default_rng(5)
    n = 5000
    rec = np.zeros(n, UO.RECORD)
    rec["t"] = np.sort(rng.random(n))
    rec["x"] = rng.integers(-300, 646, n)
    rec["y"] = rng.integers(-300, 560, n)
    rec["p"] = rng.choice([0, 1, 7], n)
    rec["x"][::97] = np.nan
    cam = capi.undistort_camera(RADIAL_INTR, capi.CAMERA_RADIAL)
    for o in (capi.undistort_options(), capi.undistort_reference_canvas(346, 260)):
        fin, fout = str(tmp_path / "ev_in.bin"), str(tmp_path / "ev_out.bin")
        with open(fin, "wb") as f:
            f.write(bytes(cam) + bytes(o) + np.uint64(n).tobytes() + rec.tobytes())
        r = subprocess.run([exe, "events", fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
        tot = np.frombuffer(raw[:32], np.uint64)
        want, want_tot = UO.events(UO.camera(UO.RADIAL, RADIAL_INTR), o.as_dict(), np.frombuffer(rec.tobytes(), np.uint8))
        assert [int(v) for v in tot] == [want_tot[k] for k in ("n_events", "n_invalid", "n_outside", "n_kept")]
        assert raw[32:] == want.tobytes()
        assert want_tot["n_invalid"] > 0 and (o.mode == 0 or want_tot["n_outside"] > 0)


def test_header_under_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (its own main: nothing is preloaded)"""
    exe = str(tmp_path / "check_undistort_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    r = subprocess.run([exe, "self"], capture_output=True, text=True)
    assert r.returncode == 0 and "self ok" in r.stdout, r.stdout + r.stderr
    uv = case_points()
    for model, intr in ((capi.CAMERA_RADIAL, RADIAL_INTR), (capi.CAMERA_FISHEYE, FISHEYE_INTR)):
        cam = capi.undistort_camera(intr, model)
        got, flag = gxx_points(exe, tmp_path, cam, uv)
        want, want_flag = capi.undistort_points_host(cam, uv)
        assert (flag == want_flag).all() and np.abs(got - want).max() <= (0.0 if model == capi.CAMERA_RADIAL else FISHEYE_TOL_PX)


def test_round_trip_through_the_forward_model():
    """A sanity check of the rule, not a tolerance of the code under test: forward radial k = (-0.1, 0.01), fx = fy = 250, principal
    point (175.5, 127.5); the inverse coefficients from ecal_inverse_radial_distortion; the numpy rule brings every distorted pixel of
    the sensor back within 0.02 px of where the forward model took it from (0.0107 px worst, measured on the CPU).  Stronger
    distortion is the five-term series' own error (14 px at k = (-0.3, 0.1)): the reference's property."""
    k1, k2, f, cx, cy = -0.1, 0.01, 250.0, 175.5, 127.5
    b5 = capi.inverse_radial_distortion([k1, k2, 0.0, 0.0])
    cam = UO.camera(UO.RADIAL, [f, f, cx, cy] + [float(v) for v in b5])
    ys, xs = np.mgrid[0:260, 0:346]
    uv = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64)   # the distorted pixels
    xd, yd = (uv[:, 0] - cx) / f, (uv[:, 1] - cy) / f
    rd = np.sqrt(xd * xd + yd * yd)
    ru = rd.copy()   # Newton on ru * (1 + k1 ru^2 + k2 ru^4) = rd
    for _ in range(60):
        g = ru * (1.0 + k1 * ru * ru + k2 * ru * ru * ru * ru) - rd
        dg = 1.0 + 3.0 * k1 * ru * ru + 5.0 * k2 * ru * ru * ru * ru
        ru = ru - g / dg
    assert np.abs(ru * (1.0 + k1 * ru * ru + k2 * ru ** 4) - rd).max() < 1e-14
    scale = np.where(rd > 0.0, ru / np.where(rd > 0.0, rd, 1.0), 1.0)
    ideal = np.stack([f * (xd * scale) + cx, f * (yd * scale) + cy], axis=1)
    got, flag = UO.points(cam, uv)
    assert flag.sum() == 0
    worst = float(np.sqrt(((got - ideal) ** 2).sum(axis=1)).max())
    print("round trip: worst %.4f px" % worst)
    assert worst <= 0.02
