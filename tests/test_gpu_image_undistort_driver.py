"""GPU: image undistortion behind the upper layers, in the manner of tests/test_gpu_undistort_driver.py — the PinholeCamera shim
(host/pinhole_camera.hpp) from a small C++ program, calibrate_stream(undistort_maps=...) and the driver's settings keys UndistortMaps /
UndistortMaps_Reference on the tilted-view "orbit" stream (2 M events).

The shim's picture is Context.image_plan's on the reference canvas, its maps are calibrate.undistort_maps', its plan is built once for
two pictures and again when the camera changes, and one channel is refused with the reference's words.  The driver with the keys at 0
writes what a plain run writes; with them on, undistort_map_x.npy / _y.npy load with numpy.load and equal calibrate.undistort_maps for
the camera the run solved (the 17-digit intrinsics of UndistortMaps.txt), and UndistortMaps.txt carries the options and the plan's info."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_undistort_oracle as IO  # noqa: E402
import synth_stream as SS  # noqa: E402
from test_gpu_shims import SETTINGS_YAML  # noqa: E402

pytestmark = pytest.mark.gpu
N_EVENTS = 2_000_000
W, H = 346, 260


@pytest.fixture(scope="module")
def stream():
    SS.TRAJECTORY = "orbit"
    try:
        return SS.make_stream(N_EVENTS, rate=1.0e6, t_start=5.0, device="cpu", seed=21).numpy()
    finally:
        SS.TRAJECTORY = "hover"


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    with eventcalib_amd.Context(0) as c:
        yield c


def b32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_pinhole_camera_shim(tmp_path, ctx):
    from eventcalib_amd import calibrate, capi
    cam, w, h = IO.camera("B64")
    c = capi.undistort_camera(cam["intr"], cam["model"])
    frame = np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8)
    camf, framef = str(tmp_path / "camera.bin"), str(tmp_path / "frame.rgb")
    open(camf, "wb").write(bytes(c))
    frame.tofile(framef)
    exe = str(tmp_path / "test_image_shims")
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_image_shims.cpp"),
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    out = subprocess.run([exe, camf, str(w), str(h), framef, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "shims ok" in out.stdout, out.stdout + out.stderr
    said = {ln.split()[0]: [float(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines() if ln.split()[0] in ("point", "inverse")}
    p = np.array([[w * 0.75, h * 0.25]])
    ideal, flag = capi.undistort_points_host(c, p)
    back, bflag = capi.distort_points_host(c, w, h, ideal)
    assert said["point"] == [ideal[0, 0], ideal[0, 1], back[0, 0], back[0, 1], 1.0] and flag[0] == 0 and bflag[0] == 0
    assert np.abs(back - p).max() <= 1e-9
    assert said["inverse"] == [float(v) for v in capi.inverse_radial_distortion([-0.1, 0.01, 0.0, 0.0])]
    raw = open(str(tmp_path / "picture.rgb"), "rb").read()
    with ctx.image_plan(c, w, h, capi.image_reference_options(w, h)) as plan:
        want = plan.apply(frame)
    assert struct.unpack("<II", raw[:8]) == (want.shape[1], want.shape[0]) == (77, 58)
    assert raw[8:] == want.tobytes() and want.any()
    raw = open(str(tmp_path / "maps.bin"), "rb").read()
    m = calibrate.undistort_maps(ctx, cam["intr"], capi.CAMERA_RADIAL, w, h)
    assert struct.unpack("<II", raw[:8]) == (w, h)
    assert raw[8:] == m["map_x"].tobytes() + m["map_y"].tobytes()


def test_chain_returns_the_maps(ctx, stream):
    import torch
    from eventcalib_amd import calibrate
    t_last = 5.0 + (N_EVENTS - 1) / 1e6
    out = calibrate.calibrate_stream(ctx, torch.from_numpy(stream).cuda(), 5.0, t_last, undistort_maps=dict(canvas="reference"))
    assert "undistort_maps" in out and "undistort_maps" in out["stage_seconds"]
    got = out["undistort_maps"]
    want = calibrate.undistort_maps(ctx, out["intrinsics"], 0, W, H, canvas="reference")
    assert got["map_x"].shape == (312, 415) and got["map_x"].dtype == np.float32
    for k in ("map_x", "map_y", "valid"):
        assert got[k].tobytes() == want[k].tobytes()
    info = got["info"]
    print("solved camera %s: r_lim %.6f truncated %d, %d invalid, %d not converged of %d canvas pixels"
          % (np.array2string(out["intrinsics"], precision=6), info["r_lim"], info["truncated"], info["n_invalid"], info["n_not_converged"], 312 * 415))
    # (the solver's free k2..k5 may turn g' negative inside 1.05 x the corner radius: `truncated` says so, and is no error)
    assert info == want["info"] and info["n_invalid"] == int((got["valid"] == 0).sum()) and info["n_invalid"] < 0.5 * 312 * 415
    centre = got["valid"][26 + H // 4:26 + 3 * H // 4, 35 + W // 4:35 + 3 * W // 4]
    assert centre.all(), "the middle of the sensor's own frame has sensor positions"


def _files(d):
    return sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs)


def test_driver_keys(tmp_path, ctx, stream):
    from eventcalib_amd import calibrate
    exe = os.path.join(ROOT, "eventcalib_amd", "unit_test_eventCameraCalib")
    if not os.path.exists(exe):      # (it travels to the GPU box prebuilt, like libecal.so)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eventcalib_amd", "csrc"), "driver"])
    binf = str(tmp_path / "events.bin")
    stream.tofile(binf)
    settings = SETTINGS_YAML % dict(start=5, end=8)
    keys = "UndistortMaps: %d\nUndistortMaps_Reference: %d\n"
    outs = {}
    for name, extra in (("zero", keys % (0, 0)), ("sensor", keys % (1, 0)), ("reference", keys % (1, 1))):
        d = tmp_path / name
        d.mkdir()
        yamlf = str(d / "settings.yaml")
        open(yamlf, "w").write(settings + extra)
        out = subprocess.run([exe, yamlf, binf, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[name] = ([ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")], d)
    zero, dz = outs["zero"]
    assert [ln.split()[0] for ln in zero] == ["keyframes", "init", "refined"]
    assert _files(dz) == ["TrajectoryByEvent.txt", "settings.yaml"]
    for name, shape, off in (("sensor", (H, W), (0.0, 0.0)), ("reference", (312, 415), (35.0, 26.0))):
        lines, d = outs[name]
        assert [ln.split()[0] for ln in lines] == ["keyframes", "init", "refined", "undistort"]
        assert lines[0] == zero[0] and lines[1] == zero[1]
        assert _files(d) == sorted(["TrajectoryByEvent.txt", "settings.yaml", "UndistortMaps.txt", "undistort_map_x.npy", "undistort_map_y.npy"])
        said = {ln.split()[0]: ln.split()[1:] for ln in open(str(d / "UndistortMaps.txt")).read().splitlines()}
        intr = [float(v) for v in said["intrinsics"]]
        assert [float("%.9g" % v) for v in intr] == [float(v) for v in lines[2].split()[1:10]] and said["model"] == ["0"]
        assert [float(v) for v in said["out_k"]] == intr[:4]
        mx, my = np.load(str(d / "undistort_map_x.npy")), np.load(str(d / "undistort_map_y.npy"))
        assert mx.dtype == my.dtype == np.float32 and mx.shape == my.shape == shape
        want = calibrate.undistort_maps(ctx, intr, 0, W, H, canvas="reference" if name == "reference" else "sensor")
        assert (b32(mx) == b32(want["map_x"])).all() and (b32(my) == b32(want["map_y"])).all()
        opt, info = dict(zip(said["options"][::2], said["options"][1::2])), dict(zip(said["info"][::2], said["info"][1::2]))
        assert (int(opt["method"]), int(opt["channels"]), int(opt["out_width"]), int(opt["out_height"]), int(opt["normalize"])) == (1, 1, shape[1], shape[0], 0)
        assert (float(opt["off_x"]), float(opt["off_y"])) == off
        wi = want["info"]
        assert (int(info["width"]), int(info["height"]), int(info["truncated"]), int(info["n_invalid"]), int(info["n_not_converged"])) == \
            (W, H, wi["truncated"], wi["n_invalid"], wi["n_not_converged"])
        assert float(info["r_lim"]) == wi["r_lim"] and int(info["n_invalid"]) == int((want["valid"] == 0).sum())
        assert lines[3] == "undistort maps %d x %d invalid %d" % (shape[1], shape[0], wi["n_invalid"])
