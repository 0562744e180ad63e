"""GPU: the hot-pixel filter at the front of the whole chain — calibrate_stream(hot_pixels=True) and the driver's settings key
`HotPixels: 1` (host/event_camera_calib_main.cpp: one `hot pixels: ...` line on stdout and saveDir/HotPixels.txt; without the key
nothing changes) — on the stream and settings of tests/test_gpu_refine_driver.py: the tilted-view ("orbit") stream, 2 M events.

Five hot pixels are injected (tests/hot_pixel_oracle.py: the first five pixels in row-major order that the clean stream never
touches, 10 000 events each at even spacing over the stream with alternating polarity, merged by a stable sort on time with the clean
event first on ties).  The filter with its defaults must give the clean stream back byte for byte, so the calibration of the
filtered dirty stream must be the calibration of the clean stream — under the rule of tests/test_gpu_refine_driver.py: counts
equal, arrays within 1e-6 of their scale (the solve sums with FP64 atomics).  What the dirty stream gives unfiltered is printed, not
asserted (design/09_measured.md has the figures of the run that introduced the feature)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hot_pixel_oracle as HP  # noqa: E402
import synth_stream as SS  # noqa: E402
from test_gpu_refine_driver import _same_calibration  # noqa: E402
from test_gpu_shims import SETTINGS_YAML  # noqa: E402

pytestmark = pytest.mark.gpu
N_EVENTS = 2_000_000
W, H = 346, 260


@pytest.fixture(scope="module")
def streams():
    SS.TRAJECTORY = "orbit"
    try:
        clean = SS.make_stream(N_EVENTS, rate=1.0e6, t_start=5.0, device="cpu", seed=21).numpy()
    finally:
        SS.TRAJECTORY = "hover"
    dirty, where, per = HP.inject_hot_pixels(clean, W, H, n_pixels=5, per_pixel=10000)
    return clean, dirty, where, per


@pytest.fixture(scope="module")
def chain(streams):
    """the Python chain: on the clean stream as it is called today and with hot_pixels=None spelled out, on the dirty stream with the
    filter and without it"""
    import torch
    import eventcalib_amd
    from eventcalib_amd.calibrate import calibrate_stream
    clean, dirty, _, _ = streams
    t_last = 5.0 + (N_EVENTS - 1) / 1e6
    d_clean, d_dirty = torch.from_numpy(clean).cuda(), torch.from_numpy(dirty).cuda()
    with eventcalib_amd.Context(0) as ctx:
        plain = calibrate_stream(ctx, d_clean, 5.0, t_last)
        off = calibrate_stream(ctx, d_clean, 5.0, t_last, hot_pixels=None)
        filtered = calibrate_stream(ctx, d_dirty, 5.0, t_last, hot_pixels=True)
        try:
            unfiltered = calibrate_stream(ctx, d_dirty, 5.0, t_last)
        except Exception as e:   # (printed, not asserted: the unfiltered run is nobody's contract)
            unfiltered = e
    return plain, off, filtered, unfiltered


def test_the_filter_gives_the_clean_stream_back(streams):
    import torch
    import eventcalib_amd
    from eventcalib_amd.calibrate import remove_hot_pixels
    clean, dirty, where, per = streams
    with eventcalib_amd.Context(0) as ctx:
        out, info = remove_hot_pixels(ctx, torch.from_numpy(dirty).cuda())
        assert torch.equal(out.cpu(), torch.from_numpy(clean))
    assert info["n_hot_pixels"] == 5 == info["n_masked_pixels"] and info["n_removed"] == 50000
    assert info["n_events"] == N_EVENTS + 50000 and info["n_kept"] == N_EVENTS and info["n_off_grid"] == 0
    ys, xs = np.nonzero(info["mask"])
    assert sorted(zip(xs.tolist(), ys.tolist())) == sorted(where)
    assert [(int(info["counts"][0, y, x]), int(info["counts"][1, y, x])) for x, y in where] == per
    assert info["max_count"] == 10000 and info["max_kept_count"] < info["quantile_count"] * 8


def test_off_switch_changes_nothing(chain):
    plain, off, _, _ = chain
    assert set(plain) == set(off) and "hot_pixels" not in off
    assert set(plain["stage_seconds"]) == set(off["stage_seconds"]) and "hot_pixels" not in off["stage_seconds"]
    assert set(plain["spline"]) == set(off["spline"]) and set(plain["init"]) == set(off["init"])
    _same_calibration(plain, off)


def _intrinsics_error(intr):
    gt = np.array([SS.FX, SS.FY, SS.CX, SS.CY])
    return float(np.abs(np.asarray(intr[:4]) / gt - 1).max())


def test_filtered_dirty_stream_calibrates_as_the_clean_one(chain):
    plain, _, filtered, unfiltered = chain
    assert set(plain) | {"hot_pixels"} == set(filtered) and set(plain["stage_seconds"]) | {"hot_pixels"} == set(filtered["stage_seconds"])
    info = filtered["hot_pixels"]
    assert info["n_hot_pixels"] == 5 and info["n_removed"] == 50000 and info["n_kept"] == N_EVENTS
    _same_calibration(plain, filtered)
    print("clean: %d keyframes, %d residuals, final cost %.6g, largest relative error of fx fy cx cy %.4g" % (
        plain["keyframes"], plain["spline"]["residuals"], plain["spline"]["final_cost"], _intrinsics_error(plain["intrinsics"])))
    if isinstance(unfiltered, Exception):
        print("dirty, unfiltered: the chain raised %r" % (unfiltered,))
    else:
        print("dirty, unfiltered: %d keyframes, %d residuals, final cost %.6g, largest relative error of fx fy cx cy %.4g" % (
            unfiltered["keyframes"], unfiltered["spline"]["residuals"], unfiltered["spline"]["final_cost"],
            _intrinsics_error(unfiltered["intrinsics"])))


def test_driver_filters_only_when_asked(tmp_path, streams):
    _, dirty, where, per = streams
    exe = os.path.join(ROOT, "eventcalib_amd", "unit_test_eventCameraCalib")
    if not os.path.exists(exe):      # (it travels to the GPU box prebuilt, like libecal.so)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eventcalib_amd", "csrc"), "driver"])
    binf = str(tmp_path / "events.bin")
    dirty.tofile(binf)
    settings = SETTINGS_YAML % dict(start=5, end=8)
    outs = {}
    for key in (False, True):
        d = tmp_path / ("with" if key else "without")
        d.mkdir()
        yamlf = str(d / "settings.yaml")
        open(yamlf, "w").write(settings + ("HotPixels: 1\n" if key else ""))
        out = subprocess.run([exe, yamlf, binf, str(d), "batch"], capture_output=True, text=True, timeout=600)
        if key:
            assert out.returncode == 0, out.stdout + out.stderr
        outs[key] = (out.returncode, [ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")], sorted(os.listdir(str(d))))
    rc0, plain, files0 = outs[False]
    _, lines, files1 = outs[True]
    # without the key: no line, no file (what the unfiltered chain makes of the dirty stream is not this test's business)
    print("without the key: exit status %d, lines %r" % (rc0, [ln.split()[0] for ln in plain]))
    assert not [ln for ln in plain if ln.startswith("hot pixels")] and "HotPixels.txt" not in files0
    # with it: the line in front of the chain's, the file beside the trajectory
    assert [ln.split()[0] for ln in lines] == ["hot", "keyframes", "init", "refined"]
    assert lines[0] == "hot pixels: 5 pixels, 50000 of %d events removed" % (N_EVENTS + 50000)
    assert files1 == ["HotPixels.txt", "TrajectoryByEvent.txt", "settings.yaml"]
    listed = [tuple(int(v) for v in ln.split()) for ln in open(str(tmp_path / "with" / "HotPixels.txt")).read().splitlines()]
    assert sorted(listed) == sorted((x, y, neg, pos) for (x, y), (neg, pos) in zip(where, per))
