"""GPU: the report in pixels at the end of the whole chain — calibrate_stream(report_px=True) and the driver's opt-in settings key
`CalibrationReportPixels: 1` (host/event_camera_calib_main.cpp: saveDir/CalibrationReportPixels.txt and one `report_px ...` line
on stdout; without the key neither appears) — on the stream and settings of tests/test_gpu_report_driver.py: the tilted-view
("orbit") stream of test_gpu_shims.py::test_cpp_driver_chain, 2 M events.

What can be held exactly is held exactly: the file against itself and against the driver's stdout line to the printed digits,
the set of files and the lines of the chain before the solve with and without the key.  The driver keeps its solution vector and
its residual records to itself, so Solver.report_px cannot be called on the driver's own solution from here, and two solves of one
problem differ in the last digits (FP64 atomics: 1e-6 of the scale, test_gpu_board_image_driver.py); the driver's totals are
therefore held against the Python chain's report_px on the same stream to the figures test_gpu_report_driver.py uses for the
board-unit report of the two chains: the count to 1e-3 relative, the rms to 1e-2."""
import os
import subprocess

import numpy as np
import pytest

import synth_stream as SS
from test_gpu_shims import SETTINGS_YAML
from test_gpu_report_driver import _parse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 2_000_000


@pytest.fixture(scope="module")
def chain():
    """the stream, and the Python chain on it without and with the two reports"""
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
        out = calibrate_stream(ctx, d_buf, 5.0, 5.0 + (N_EVENTS - 1) / 1e6, report=True, report_px=True)
    return buf, plain, out


def test_calibrate_stream_report_px(chain):
    _, plain, out = chain
    assert "report_px" not in plain and "report_px" not in plain["stage_seconds"]
    assert set(plain["stage_seconds"]) | {"report", "report_px"} == set(out["stage_seconds"])
    assert set(plain) | {"report", "report_px"} == set(out)
    assert np.abs(plain["intrinsics"] / out["intrinsics"] - 1).max() < 1e-6        # (FP64 atomics: equal up to the order of the sums)
    rep, board = out["report_px"], out["report"]
    n_res = out["spline"]["residuals"]
    print("residuals %d rms_px %.6g px_per_unit %.6g outliers %.4f degenerate %d | board-unit rms %.6g (x px_per_unit = %.6g)" % (
        n_res, rep["rms_px"], rep["px_per_unit"], rep["outlier_frac"], rep["n_degenerate"], board["rms"], board["rms"] * rep["px_per_unit"]))
    assert int(rep["totals"]["all"]["n"]) + rep["n_degenerate"] == n_res > 0 and rep["n_degenerate"] == 0
    assert len(rep["kf"]) == len(out["trajectory"]) and int(rep["kf"]["n"].sum()) == n_res
    assert len(rep["lm"]) == 36 and int(rep["lm"]["n"].sum()) == n_res
    assert rep["cell_n"].shape == (17, 22) and int(rep["cell_n"].sum()) == n_res and int(rep["hist"].sum()) == n_res
    # the same records in both reports: every count of a family that does not depend on the unit
    assert np.array_equal(rep["kf"]["n"], board["kf"]["n"]) and np.array_equal(rep["lm"]["n"], board["lm"]["n"])
    assert np.array_equal(rep["cell_n"], board["cell_n"])
    assert rep["hist_edges"][-1] == 4.0 and rep["options"].outlier_thresh == 1.0
    # a sensor of this size sees the board's unit as a few pixels, and the solved chain fits to a fraction of a pixel .. a few
    assert 1.0 < rep["px_per_unit"] < 20.0 and 0.0 < rep["rms_px"] < 5.0


def test_driver_writes_the_pixel_report_only_when_asked(tmp_path, chain):
    buf, _, py_out = chain
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
        open(yamlf, "w").write(settings + ("CalibrationReportPixels: 1\n" if key else ""))
        out = subprocess.run([exe, yamlf, binf, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[key] = ([ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")], d)
    plain, d0 = outs[False]
    lines, d1 = outs[True]
    # without the key: no line, no file — the parent's output
    assert not any(ln.startswith("report") for ln in plain)
    assert sorted(os.listdir(str(d0))) == sorted(set(os.listdir(str(d1))) - {"CalibrationReportPixels.txt"})
    assert not os.path.exists(str(d1 / "CalibrationReport.txt"))          # the board-unit report has its own key
    rest = [ln for ln in lines if not ln.startswith("report_px")]
    assert [ln.split()[0] for ln in plain] == [ln.split()[0] for ln in rest]
    assert rest[:2] == plain[:2]                                              # keyframes, init calibration: byte for byte
    ref_a = np.array([float(v) for v in [ln for ln in plain if ln.startswith("refined ")][0].split()[1:10]])
    ref_b = np.array([float(v) for v in [ln for ln in rest if ln.startswith("refined ")][0].split()[1:10]])
    assert (np.abs(ref_a - ref_b) <= 1e-6 * np.maximum(np.abs(ref_a), 1.0)).all()   # two solves: equal up to the order of the sums
    said = [ln.split() for ln in lines if ln.startswith("report_px ")]
    assert len(said) == 1 and said[0][1::2] == ["rms_px", "px_per_unit", "outliers", "degenerate"]
    path = str(d1 / "CalibrationReportPixels.txt")
    head = open(path).readline()
    assert head.startswith("# residuals in pixels") and "px_per_unit" in head
    rep = _parse(path)                     # CalibrationReport.txt's layout: that file's parser reads it
    tot = rep["totals"]
    n_res = int([ln for ln in lines if ln.startswith("refined ")][0].split()[11])
    # the file is consistent with itself and with the driver's other lines, to the printed digits
    assert tot["n"] + tot["n_degenerate"] == n_res > 0
    assert "%.9g" % np.sqrt(tot["sum_r2"] / tot["n"]) == "%.9g" % tot["rms"] == said[0][2]
    assert "%.9g" % (tot["sum_px_per_unit"] / tot["n"]) == said[0][4] == head.split("px_per_unit")[1].split(";")[0].strip()
    assert "%.6f" % (tot["n_out"] / tot["n"]) == said[0][6] and int(said[0][8]) == tot["n_degenerate"]
    assert len(rep["lm"]) == 36 and sum(b["n"] for b in rep["lm"]) == tot["n"]
    assert rep["cell_n"].shape == (17, 22) and rep["cell_n"].sum() == tot["n"] and rep["hist"].sum() == tot["n"] and len(rep["hist"]) == 64
    assert abs(rep["empty_cells"] - (rep["cell_n"] == 0).mean()) <= 1e-6 and rep["hist_range"] == 4.0
    assert len(rep["worst"]) == 10 and all(a["rms"] >= b["rms"] for a, b in zip(rep["worst"], rep["worst"][1:]))
    assert rep["worst"][0]["rms"] >= tot["rms"] and all(0 <= w["id"] < rep["n_keyframes"] for w in rep["worst"])
    # ... and with the Python chain's pixel report on the same stream (the module's docstring has the figures' origin)
    py = py_out["report_px"]
    print("driver n %d rms_px %.9g px_per_unit %s | python n %d rms_px %.9g px_per_unit %.9g" % (
        tot["n"], tot["rms"], said[0][4], int(py["totals"]["all"]["n"]), py["rms_px"], py["px_per_unit"]))
    assert abs(tot["n"] - int(py["totals"]["all"]["n"])) <= 1e-3 * tot["n"]
    assert abs(tot["rms"] - py["rms_px"]) <= 1e-2 * py["rms_px"]
    assert abs(float(said[0][4]) - py["px_per_unit"]) <= 1e-2 * py["px_per_unit"]
    assert rep["n_keyframes"] == len(py["kf"])
