"""GPU: the opt-in refinement round at the end of the whole chain — calibrate_stream(refine_rounds=1) and the driver's settings key
`RefineRounds: 1` (host/event_camera_calib_main.cpp: one `refine round k ...` line on stdout per round; without the key nothing
changes) — on the stream and settings of tests/test_gpu_board_image_driver.py: the tilted-view ("orbit") stream, 2 M events.

A round re-associates EVERY event of the stream through the solution (capi.Solver.reassociated: the events within the Huber width
of a circle's rim, wherever they sit relative to a keyframe) and solves again from that solution.  Whether that makes the camera
more accurate is not known, and this test does not assume it: it prints the largest relative error of fx, fy, cx, cy against
synth_stream's ground truth without (err0) and with (err1) the round, and the kept count against the keyframe association's
residual count, and asserts only err1 <= 2 err0 — a guard against a refinement that wrecks the fit.  The figures of the run that
introduced the feature are in design/09_measured.md.

The driver and the Python chain are two implementations of the chain, held to 1e-3 on the refined camera
(test_gpu_shims.py::test_cpp_driver_chain): their rounds' counts agree to 1e-3 (+ 2), the figure of the other driver tests."""
import os
import subprocess

import numpy as np
import pytest

import synth_stream as SS
from test_gpu_shims import SETTINGS_YAML

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 2_000_000


@pytest.fixture(scope="module")
def chain():
    """the stream, and the Python chain on it: as it is called today, with refine_rounds=0 spelled out, and with one round"""
    import eventcalib_amd
    from eventcalib_amd.calibrate import calibrate_stream
    SS.TRAJECTORY = "orbit"
    try:
        buf = SS.make_stream(N_EVENTS, rate=1.0e6, t_start=5.0, device="cpu", seed=21)
    finally:
        SS.TRAJECTORY = "hover"
    d_buf = buf.cuda()
    t_last = 5.0 + (N_EVENTS - 1) / 1e6
    with eventcalib_amd.Context(0) as ctx:
        plain = calibrate_stream(ctx, d_buf, 5.0, t_last)
        zero = calibrate_stream(ctx, d_buf, 5.0, t_last, refine_rounds=0)
        one = calibrate_stream(ctx, d_buf, 5.0, t_last, refine_rounds=1)
    return buf, plain, zero, one


def _same_calibration(a_out, b_out):
    """every array and number the chain returns: counts equal, arrays within 1e-6 of their scale (the solve sums with FP64 atomics,
    so two runs agree up to the order of the sums: the rule of test_gpu_board_image_driver.py)"""
    for key in ("keyframes", "fisheye_start"):
        assert a_out.get(key) == b_out.get(key), key
    for key in ("splines", "control_points", "residuals", "unknowns"):
        assert a_out["spline"][key] == b_out["spline"][key], key
    pairs = {key: (a_out[key], b_out[key]) for key in ("intrinsics", "trajectory", "init_trajectory")}
    pairs["init.intr"] = (a_out["init"]["intr"], b_out["init"]["intr"])
    pairs["init.rms"] = ([a_out["init"]["rms"]], [b_out["init"]["rms"]])
    for key, (a, b) in pairs.items():
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert a.shape == b.shape, key
        scale = np.maximum(np.abs(a).max(axis=0) if a.ndim == 2 else np.abs(a), 1e-300)
        print("%s: max deviation / scale %.3g" % (key, (np.abs(a - b) / scale).max()))
        assert (np.abs(a - b) <= 1e-6 * scale).all(), key
    assert abs(a_out["spline"]["final_cost"] - b_out["spline"]["final_cost"]) <= 1e-6 * a_out["spline"]["final_cost"]


def test_zero_rounds_change_nothing(chain):
    _, plain, zero, _ = chain
    assert set(plain) == set(zero) and "refine" not in zero
    assert set(plain["stage_seconds"]) == set(zero["stage_seconds"]) and "refine" not in zero["stage_seconds"]
    assert set(plain["spline"]) == set(zero["spline"]) and set(plain["init"]) == set(zero["init"])
    _same_calibration(plain, zero)


def _intrinsics_error(intr):
    gt = np.array([SS.FX, SS.FY, SS.CX, SS.CY])
    return float(np.abs(np.asarray(intr[:4]) / gt - 1).max())


def test_one_round(chain):
    _, plain, _, one = chain
    assert set(plain) | {"refine"} == set(one) and set(plain["stage_seconds"]) | {"refine"} == set(one["stage_seconds"])
    # the keyframe-gated solve in front of the round is the same one
    for key in ("splines", "control_points", "residuals", "unknowns"):
        assert plain["spline"][key] == one["spline"][key], key
    assert abs(plain["spline"]["final_cost"] - one["spline"]["final_cost"]) <= 1e-6 * plain["spline"]["final_cost"]
    assert len(one["refine"]) == 1
    r = one["refine"][0]
    tot = r["totals"]
    assert int(tot["n_events"]) == N_EVENTS == int(tot["n_outside_time"] + tot["n_behind"] + tot["n_off_ring"] + tot["n_kept"])
    assert r["residuals"] == int(tot["n_kept"]) > 0
    assert r["iterations"] >= 1 and np.isfinite(r["initial_cost"]) and 0 <= r["final_cost"] <= r["initial_cost"]
    assert one["trajectory"].shape == plain["trajectory"].shape and np.isfinite(one["intrinsics"]).all()
    err0, err1 = _intrinsics_error(plain["intrinsics"]), _intrinsics_error(one["intrinsics"])
    print("largest relative error of fx fy cx cy: %.4g without the round, %.4g with it" % (err0, err1))
    print("records: %d kept of %d events (outside time %d, behind %d, off ring %d) against %d from the keyframe association" % (
        int(tot["n_kept"]), N_EVENTS, int(tot["n_outside_time"]), int(tot["n_behind"]), int(tot["n_off_ring"]), plain["spline"]["residuals"]))
    print("round: cost %.6g -> %.6g in %d iterations; keyframe-gated solve: %.6g -> %.6g" % (
        r["initial_cost"], r["final_cost"], r["iterations"], plain["spline"]["initial_cost"], plain["spline"]["final_cost"]))
    assert err1 <= 2 * err0


def test_driver_refines_only_when_asked(tmp_path, chain):
    buf, _, _, one = chain
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
        open(yamlf, "w").write(settings + ("RefineRounds: 1\n" if key else ""))
        out = subprocess.run([exe, yamlf, binf, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[key] = ([ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")], sorted(os.listdir(str(d))))
    plain, files0 = outs[False]
    lines, files1 = outs[True]
    # without the key: the parent's lines and files
    assert [ln.split()[0] for ln in plain] == ["keyframes", "init", "refined"]
    assert files0 == ["TrajectoryByEvent.txt", "settings.yaml"] == files1
    # with it: the same chain in front, one line for the round
    assert [ln.split()[0] for ln in lines] == ["keyframes", "init", "refined", "refine"] and lines[:2] == plain[:2]
    said = [ln.split() for ln in lines if ln.startswith("refine round 0 ")]
    assert len(said) == 1 and len([ln for ln in lines if ln.startswith("refine round")]) == 1
    w = said[0]
    assert [w[3], w[5], w[7], w[9], w[11]] == ["events", "kept", "cost", "->", "iterations"] and len(w) == 13
    events, kept, iterations = int(w[4]), int(w[6]), int(w[12])
    py = one["refine"][0]
    print("driver: %s | python: kept %d, cost %.6g -> %.6g, iterations %d" % (" ".join(w), int(py["totals"]["n_kept"]), py["initial_cost"],
                                                                            py["final_cost"], py["iterations"]))
    assert events == N_EVENTS == int(py["totals"]["n_events"])
    assert abs(kept - int(py["totals"]["n_kept"])) <= 1e-3 * int(py["totals"]["n_kept"]) + 2
    assert iterations >= 1 and float(w[8]) >= float(w[10]) >= 0
    drv = np.array([float(v) for v in lines[2].split()[1:5]])      # (the `refined` line carries the round's camera)
    print("refined fx fy cx cy, driver against python: %.3g relative" % np.abs(drv / one["intrinsics"][:4] - 1).max())
