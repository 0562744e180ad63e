"""GPU: undistortion behind the whole chain — calibrate_stream(undistort=...), the C++ shims (EventContainer::undistorted,
EventFrame::undistortedImage) and the driver's settings keys UndistortedEvents / UndistortedEvents_Pixel / UndistortedImages — on the
stream and settings of tests/test_gpu_noise_filter_driver.py (the tilted-view "orbit" stream, 2 M events).

calibrate_stream(undistort=True) returns the records Context.undistort_events gives with the parameters that run solved, and the
oracle's; off (None, False) nothing changes.  The driver with the three keys writes events_undistorted.bin equal to
Context.undistort_events with the intrinsics it wrote (17 digits) into Undistorted.txt, one PNG per accepted keyframe under
undistortedImage/ with names the reference's parser (visulization_eventCalib.cpp:85-93) accepts, and Undistorted.txt; with the keys 0
or absent its lines and files are a plain run's — compared as tests/test_gpu_noise_filter_driver.py compares two runs of the same
chain (the solve sums with FP64 atomics: the refined line within 1e-9 * 400, everything else equal)."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth_stream as SS  # noqa: E402
import undistort_oracle as UO  # noqa: E402
from test_gpu_refine_driver import _same_calibration  # noqa: E402
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


@pytest.fixture(scope="module")
def chain(ctx, stream):
    import torch
    from eventcalib_amd.calibrate import calibrate_stream
    t_last = 5.0 + (N_EVENTS - 1) / 1e6
    d = torch.from_numpy(stream).cuda()
    plain = calibrate_stream(ctx, d, 5.0, t_last)
    off = calibrate_stream(ctx, d, 5.0, t_last, undistort=False)
    on = calibrate_stream(ctx, d, 5.0, t_last, undistort=True)
    pixel = calibrate_stream(ctx, d, 5.0, t_last, undistort=dict(sensor=(W, H)))
    return plain, off, on, pixel


def test_off_switch_changes_nothing(chain):
    plain, off, _, _ = chain
    assert set(plain) == set(off) and "undistorted_events" not in off and "undistort" not in off["stage_seconds"]
    _same_calibration(plain, off)


def test_chain_returns_what_undistort_events_gives(ctx, chain, stream):
    from eventcalib_amd import capi
    plain, _, on, pixel = chain
    for out, opt in ((on, capi.undistort_options()), (pixel, capi.undistort_options(sensor=(W, H)))):
        assert set(plain) | {"undistorted_events", "undistort"} == set(out) and "undistort" in out["stage_seconds"]
        _same_calibration(plain, out)
        cam = capi.undistort_camera(out["intrinsics"], capi.CAMERA_RADIAL)
        want, tot = ctx.undistort_events(cam, stream, opt)
        got = out["undistorted_events"]
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        info = out["undistort"]
        assert {k: info[k] for k in tot.dtype.names} == {k: int(tot[k]) for k in tot.dtype.names}
        assert {k: info[k] for k in opt.as_dict()} == opt.as_dict()
        oracle, oracle_tot = UO.events(UO.camera(UO.RADIAL, out["intrinsics"]), opt.as_dict(), stream)
        assert oracle.tobytes() == want.cpu().numpy().tobytes() and {k: info[k] for k in oracle_tot} == oracle_tot
        assert info["n_events"] == N_EVENTS and info["n_kept"] > 0.9 * N_EVENTS
        print("undistort (mode %d): %d invalid, %d outside, %d kept" % (opt.mode, info["n_invalid"], info["n_outside"], info["n_kept"]))


def test_cpp_shims(tmp_path, ctx):
    """EventContainer::undistorted and EventFrame::undistortedImage against the Python layer on a small stream: three windows as
    in tests/test_gpu_undistort.py (both polarities, none, one polarity)"""
    from eventcalib_amd import capi
    from test_gpu_undistort import FRAME_CASES, frame_stream
    (w, h), intr, out_k, n_per = FRAME_CASES["346x260"]
    rec, t0, t1 = frame_stream(np.random.default_rng(3), w, h, n_per)
    binf, camf = str(tmp_path / "events.bin"), str(tmp_path / "camera.bin")
    rec.tofile(binf)
    cam = capi.undistort_camera(intr, capi.CAMERA_RADIAL, out_k=out_k)
    open(camf, "wb").write(bytes(cam))
    exe = str(tmp_path / "test_undistort_shims")
    lib_dir = os.path.join(ROOT, "eventcalib_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_undistort_shims.cpp"),
                           "-L" + lib_dir, "-lecal", "-Wl,-rpath," + lib_dir, "-lpthread"])
    out = subprocess.run([exe, binf, camf, repr(float(t0[0])), repr(float(t1[0])), repr(float(t0[2])), repr(float(t1[2])), str(tmp_path)], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "shims ok" in out.stdout, out.stdout + out.stderr
    said = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines() if ln.split()[0] in ("sub", "pixel", "frame")}
    for name, opt in (("sub", capi.undistort_options()), ("pixel", capi.undistort_options(sensor=(w, h)))):
        want, tot = ctx.undistort_events(cam, rec, opt)
        assert open(str(tmp_path / (name + ".bin")), "rb").read() == want.cpu().numpy().tobytes()
        assert said[name] == [int(tot[k]) for k in ("n_events", "n_invalid", "n_outside", "n_kept")] and 0 < said[name][3] < said[name][0]
    rgb, tot = ctx.undistorted_frames(cam, rec, t0[:1], t1[:1], capi.undistort_options(sensor=(w, h)))
    raw = open(str(tmp_path / "frame.rgb"), "rb").read()
    assert struct.unpack("<II", raw[:8]) == (rgb.shape[2], rgb.shape[1]) == (415, 312)
    assert raw[8:] == rgb[0].tobytes() and rgb.any()
    assert said["frame"] == [int(v) for v in tot[0]]


def _files(d):
    return sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs)


def _png_rgb(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(raw):
        n, kind = struct.unpack(">I4s", raw[at: at + 8])
        body = raw[at + 8: at + 8 + n]
        if kind == b"IHDR":
            size = struct.unpack(">II", body[:8])
            assert body[8:10] == b"\x08\x02"   # 8 bits, RGB
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[1], 1 + 3 * size[0])
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(size[1], size[0], 3)


def test_driver_keys(tmp_path, ctx, stream):
    from eventcalib_amd import capi
    exe = os.path.join(ROOT, "eventcalib_amd", "unit_test_eventCameraCalib")
    if not os.path.exists(exe):      # (it travels to the GPU box prebuilt, like libecal.so)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eventcalib_amd", "csrc"), "driver"])
    binf = str(tmp_path / "events.bin")
    stream.tofile(binf)
    settings = SETTINGS_YAML % dict(start=5, end=8)
    keys = "UndistortedEvents: %d\nUndistortedEvents_Pixel: %d\nUndistortedImages: %d\n"
    outs = {}
    for name, extra in (("without", ""), ("zero", keys % (0, 0, 0)), ("on", keys % (1, 1, 1))):
        d = tmp_path / name
        d.mkdir()
        yamlf = str(d / "settings.yaml")
        open(yamlf, "w").write(settings + extra)
        out = subprocess.run([exe, yamlf, binf, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[name] = ([ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")], d)
    # the keys at 0 are a run without them
    (a, da), (b, db) = outs["zero"], outs["without"]
    assert [ln.split()[0] for ln in a] == ["keyframes", "init", "refined"] == [ln.split()[0] for ln in b]
    assert _files(da) == _files(db) == ["TrajectoryByEvent.txt", "settings.yaml"]
    assert a[0] == b[0] and a[1] == b[1]
    ra, rb = a[2].split(), b[2].split()
    assert np.abs(np.array([float(v) for v in ra[1:10]]) - np.array([float(v) for v in rb[1:10]])).max() < 1e-9 * 400 and ra[10:] == rb[10:]
    ta, tb = (open(str(x / "TrajectoryByEvent.txt")).read().split("\n") for x in (da, db))
    assert len(ta) == len(tb) > 20 and [ln.split()[:1] for ln in ta] == [ln.split()[:1] for ln in tb]
    # with the keys: the chain's lines as they were, two lines more, the files
    lines, d = outs["on"]
    print("\n".join(lines))
    assert [ln.split()[0] for ln in lines] == ["keyframes", "init", "refined", "undistorted", "undistorted"]
    assert lines[0] == b[0] and lines[1] == b[1]
    accepted = int(lines[1].split()[lines[1].split().index("accepted") + 1])
    pngs = [f for f in _files(d) if f.startswith("undistortedImage" + os.sep)]
    assert _files(d) == sorted(["TrajectoryByEvent.txt", "settings.yaml", "Undistorted.txt", "events_undistorted.bin"] + pngs)
    said = {}
    for ln in open(str(d / "Undistorted.txt")).read().splitlines():
        said.setdefault(ln.split()[0], []).append(ln.split()[1:])
    intr = [float(v) for v in said["intrinsics"][0]]
    assert [float("%.9g" % v) for v in intr] == [float(v) for v in lines[2].split()[1:10]] and said["model"] == [["0"]]
    # the stream: Context.undistort_events with those intrinsics on the reference canvas
    opt = capi.undistort_options(sensor=(W, H))
    want, tot = ctx.undistort_events(capi.undistort_camera(intr, capi.CAMERA_RADIAL), stream, opt)
    assert open(str(d / "events_undistorted.bin"), "rb").read() == want.cpu().numpy().tobytes()
    ev_opt, ev_tot = (dict(zip(row[::2], row[1::2])) for row in said["events"])
    assert {k: int(ev_tot[k]) for k in tot.dtype.names} == {k: int(tot[k]) for k in tot.dtype.names}
    assert (int(ev_opt["mode"]), int(ev_opt["out_width"]), int(ev_opt["out_height"]), float(ev_opt["off_x"]), float(ev_opt["off_y"])) == (1, 415, 312, 34.6, 26.0)
    assert lines[3] == "undistorted events %d of %d kept" % (int(tot["n_kept"]), N_EVENTS) and int(tot["n_kept"]) > 0.9 * N_EVENTS
    # the pictures: one per accepted keyframe, names the reference's parser reads (the stamp in front of the last '_', no 'd' behind it)
    assert len(pngs) == accepted > 10 and lines[4] == "undistorted images %d" % accepted
    stamps = set()
    for f in pngs:
        path = str(d / f)
        end = path.rfind("_")
        assert path[end + 1] != "d" and path.endswith("_undistorted.png")
        stamps.add(float(path[path.rfind("/") + 1: end]))
    assert len(stamps) == accepted and all(5.0 <= s <= 8.0 for s in stamps)
    head = ["images"] + said["images"][0]
    img_opt, img_tot = dict(zip(head[::2], head[1::2])), dict(zip(said["images"][1][::2], said["images"][1][1::2]))
    assert int(img_opt["images"]) == accepted and (int(img_opt["out_width"]), int(img_opt["out_height"])) == (415, 312)
    painted = 0
    for f in pngs[:3] + pngs[-1:]:
        rgb = _png_rgb(str(d / f))
        assert rgb.shape == (312, 415, 3) and not rgb[:, :, 2].any() and set(np.unique(rgb)) <= {0, 255}
        red, green = (rgb[:, :, 0] == 255), (rgb[:, :, 1] == 255)
        assert red.any() and green.any() and not (red & green).any()
        painted += int(red.sum() + green.sum())
    assert 0 < painted <= int(img_tot["n_pos"]) + int(img_tot["n_neg"])
