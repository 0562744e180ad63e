"""GPU: the calibration report at the end of the whole chain — calibrate_stream(report=True) and the driver's opt-in settings key
`CalibrationReport: 1` (host/event_camera_calib_main.cpp: saveDir/CalibrationReport.txt and one `report ...` line on stdout;
without the key neither appears) — on one synthetic stream.

The stream is the tilted-view ("orbit") one of test_gpu_shims.py::test_cpp_driver_chain, 2 M events: the 600 k-event stream of
test_gpu_end_to_end.py keeps the board fronto-parallel and is fed to the solver with ground-truth circles there; through the
whole chain its init stage accepts fewer than the 11 frames the spline stage needs (RuntimeError: too few frames in the map,
with or without a report)."""
import os
import subprocess

import numpy as np
import pytest

import synth_stream as SS
from test_gpu_shims import SETTINGS_YAML

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(path):
    lines = open(path).read().splitlines()
    rep, i = {}, 0
    while i < len(lines):
        w = lines[i].split()
        i += 1
        if not w or w[0] == "#":
            continue
        if w[0] == "totals":
            rep["totals"] = {w[k]: float(w[k + 1]) for k in range(1, len(w), 2)}
        elif w[0] == "worst_keyframes":
            rows = [lines[i + k].split() for k in range(int(w[1]))]
            i += len(rows)
            rep["n_keyframes"] = int(w[3])
            rep["worst"] = [{"t": float(r[1]), "id": int(r[3]), **{r[k]: float(r[k + 1]) for k in range(4, len(r), 2)}} for r in rows]
        elif w[0] == "landmarks":
            rows = [lines[i + k].split() for k in range(int(w[1]))]
            i += len(rows)
            assert [int(r[1]) for r in rows] == list(range(len(rows)))          # grid order
            rep["lm"] = [{r[k]: float(r[k + 1]) for k in range(2, len(r), 2)} for r in rows]
        elif w[0] == "coverage":
            cy, cx = int(w[1]), int(w[2])
            rep["cell_n"] = np.array([[int(v) for v in lines[i + k].split()] for k in range(cy)])
            assert rep["cell_n"].shape == (cy, cx)
            i += cy
        elif w[0] == "empty_cells":
            rep["empty_cells"] = float(w[1])
        elif w[0] == "histogram":
            rep["hist"] = np.array([int(v) for v in lines[i].split()])
            assert len(rep["hist"]) == int(w[1])
            rep["hist_range"] = float(w[3])
            i += 1
    return rep


N_EVENTS = 2_000_000


@pytest.fixture(scope="module")
def chain():
    """the stream, and the Python chain on it without and with the report"""
    import eventcalib_amd
    from eventcalib_amd.calibrate import calibrate_stream
    SS.TRAJECTORY = "orbit"
    try:
        buf = SS.make_stream(N_EVENTS, rate=1.0e6, t_start=5.0, device="cpu", seed=21)
    finally:
        SS.TRAJECTORY = "hover"
    d_buf = buf.cuda()
    with eventcalib_amd.Context(0) as ctx:
        plain = calibrate_stream(ctx, d_buf, 5.0, 5.0 + (N_EVENTS - 1) / 1e6)
        out = calibrate_stream(ctx, d_buf, 5.0, 5.0 + (N_EVENTS - 1) / 1e6, report=True)
    return buf, plain, out


def test_calibrate_stream_report(chain):
    """calibrate_stream(report=True): the report describes the solution.  final_cost is the cost of the solver's OWN last
    accepted evaluation at the returned parameters (the normal-equation kernel or the cost kernel of that Levenberg-Marquardt
    step); the report's cost is one more pass of another kernel over the same records: 1e-9 relative, not the 1e-11 of two
    kernels compared at one call."""
    _, plain, out = chain
    assert "report" not in plain and "report" not in plain["stage_seconds"]
    rep = out["report"]
    n_res = out["spline"]["residuals"]
    print("residuals %d rms %.6g outliers %.4f empty cells %.3f cost %.17g final_cost %.17g" % (
        n_res, rep["rms"], rep["outlier_frac"], rep["empty_cell_frac"], rep["cost"], out["spline"]["final_cost"]))
    assert int(rep["totals"]["all"]["n"]) == n_res > 0
    assert abs(rep["cost"] - out["spline"]["final_cost"]) <= 1e-9 * out["spline"]["final_cost"]
    assert len(rep["kf"]) == len(out["trajectory"]) and int(rep["kf"]["n"].sum()) == n_res
    assert len(rep["lm"]) == 36 and int(rep["lm"]["n"].sum()) == n_res
    assert rep["cell_n"].shape == (17, 22) and int(rep["cell_n"].sum()) == n_res and int(rep["hist"].sum()) == n_res
    assert set(plain["stage_seconds"]) | {"report"} == set(out["stage_seconds"])
    assert set(plain) | {"report"} == set(out)
    assert np.abs(plain["intrinsics"] / out["intrinsics"] - 1).max() < 1e-6        # (FP64 atomics: equal up to the order of the sums)


def test_driver_writes_the_report_only_when_asked(tmp_path, chain):
    buf, _, py_out = chain
    n = N_EVENTS
    exe = os.path.join(ROOT, "eventcalib_amd", "unit_test_eventCameraCalib")
    if not os.path.exists(exe):      # (it travels to the GPU box prebuilt, like libecal.so)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eventcalib_amd", "csrc"), "driver"])
    binf = str(tmp_path / "events.bin")
    buf.numpy().tofile(binf)
    settings = SETTINGS_YAML % dict(start=5, end=8)
    outs = {}
    for key in (False, True):
        d = tmp_path / ("with" if key else "without")
        d.mkdir()
        yamlf = str(d / "settings.yaml")
        open(yamlf, "w").write(settings + ("CalibrationReport: 1\n" if key else ""))
        # ("batch": the same chain without the keyframe images)
        out = subprocess.run([exe, yamlf, binf, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[key] = ([ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")], d)
    plain, d0 = outs[False]
    assert not any(ln.startswith("report") for ln in plain) and not os.path.exists(str(d0 / "CalibrationReport.txt"))
    lines, d1 = outs[True]
    assert [ln for ln in lines if not ln.startswith("report")][:2] == plain[:2]      # keyframes, init calibration: the same chain
    said = [ln.split() for ln in lines if ln.startswith("report ")]
    assert len(said) == 1 and said[0][1::2] == ["rms", "outliers", "empty_cells"]
    rep = _parse(str(d1 / "CalibrationReport.txt"))
    tot = rep["totals"]
    n_res = int([ln for ln in lines if ln.startswith("refined ")][0].split()[11])
    # the file is consistent with itself and with the driver's other lines
    assert tot["n"] == n_res > 0
    assert abs(tot["rms"] - np.sqrt(tot["sum_r2"] / tot["n"])) <= 1e-8 * tot["rms"]
    assert abs(float(said[0][2]) - tot["rms"]) <= 1e-8 * tot["rms"] and abs(float(said[0][4]) - tot["n_out"] / tot["n"]) <= 1e-6
    assert len(rep["lm"]) == 36 and sum(b["n"] for b in rep["lm"]) == n_res
    assert rep["cell_n"].shape == (17, 22) and rep["cell_n"].sum() == n_res and rep["hist"].sum() == n_res and len(rep["hist"]) == 64
    assert abs(rep["empty_cells"] - (rep["cell_n"] == 0).mean()) <= 1e-6 and abs(float(said[0][6]) - rep["empty_cells"]) <= 1e-6
    assert len(rep["worst"]) == 10 and all(a["rms"] >= b["rms"] for a, b in zip(rep["worst"], rep["worst"][1:]))
    assert rep["worst"][0]["rms"] >= tot["rms"] and all(0 <= w["id"] < rep["n_keyframes"] for w in rep["worst"])
    # ... and with the Python chain's report on the same stream.  The two chains select the same keyframes and are held to 1e-3
    # on the refined camera (test_cpp_driver_chain); their rectified circles agree to the last digits only, so single rim events
    # may associate differently: the residual count to 1e-3 relative, the rms to 1e-2
    py = py_out["report"]
    print("driver n %d rms %.9g | python n %d rms %.9g" % (n_res, tot["rms"], int(py["totals"]["all"]["n"]), py["rms"]))
    assert abs(tot["n"] - int(py["totals"]["all"]["n"])) <= 1e-3 * tot["n"]
    assert abs(tot["rms"] - py["rms"]) <= 1e-2 * py["rms"]
    assert rep["n_keyframes"] == len(py["kf"])
    assert abs(rep["hist_range"] - py["hist_edges"][-1]) <= 1e-9
