"""GPU: the board-frame event image at the end of the whole chain — calibrate_stream(board_image=True) and the driver's opt-in
settings key `BoardImage: 1` (host/event_camera_calib_main.cpp: saveDir/board_image.png, saveDir/BoardImage.txt and one
`board_image ...` line on stdout; without the key none of them appears) — on the stream and settings of
tests/test_gpu_report_driver.py: the tilted-view ("orbit") stream of test_gpu_shims.py::test_cpp_driver_chain, 2 M events.

The driver and the Python chain are two implementations of the chain, held to 1e-3 on the refined camera
(test_cpp_driver_chain), so their board images are images of two slightly different solutions: the event count must be equal,
every other total agrees to 1e-3 of itself, the per-circle counts, spreads and means to 1e-2 — the figures to which
test_gpu_report_driver.py holds the two reports; what the driver's files say is held exactly against each other."""
import os
import subprocess

import numpy as np
import pytest

import synth_stream as SS
from test_gpu_shims import SETTINGS_YAML
from test_png_writer import decode_png

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 2_000_000


def _parse(path):
    out = {"circles": []}
    for ln in open(path).read().splitlines():
        w = ln.split()
        if not w or w[0] == "#":
            continue
        if w[0] == "totals":
            out["totals"] = {w[k]: int(w[k + 1]) for k in range(1, len(w), 2)}
        elif w[0] == "image":
            out["image"] = {w[k]: float(w[k + 1]) for k in range(1, len(w), 2)}
        elif w[0] == "circles":
            out["n_circles"] = int(w[1])
        elif w[0] == "circle":
            assert int(w[1]) == len(out["circles"])          # grid order
            out["circles"].append({w[k]: float(w[k + 1]) for k in range(2, len(w), 2)})
    return out


@pytest.fixture(scope="module")
def chain():
    """the stream, and the Python chain on it without and with the board image"""
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
        out = calibrate_stream(ctx, d_buf, 5.0, 5.0 + (N_EVENTS - 1) / 1e6, board_image=True)
    return buf, plain, out


def test_calibrate_stream_board_image(chain):
    _, plain, out = chain
    assert "board_image" not in plain and "board_image" not in plain["stage_seconds"]
    assert set(plain["stage_seconds"]) | {"board_image"} == set(out["stage_seconds"])
    assert set(plain) | {"board_image"} == set(out)
    # the same calibration with and without the flag: every array and number the chain returns.  The solve sums with FP64 atomics,
    # so two runs agree up to the order of the sums (1e-6 of the array's scale, the figure test_gpu_report_driver.py uses for the
    # intrinsics); every count is equal
    for key in ("keyframes", "fisheye_start"):
        assert plain.get(key) == out.get(key), key
    for key in ("splines", "control_points", "residuals", "unknowns"):
        assert plain["spline"][key] == out["spline"][key], key
    pairs = {key: (plain[key], out[key]) for key in ("intrinsics", "trajectory", "init_trajectory")}
    pairs["init.intr"] = (plain["init"]["intr"], out["init"]["intr"])
    pairs["init.rms"] = ([plain["init"]["rms"]], [out["init"]["rms"]])
    for key, (a, b) in pairs.items():
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert a.shape == b.shape, key
        scale = np.maximum(np.abs(a).max(axis=0) if a.ndim == 2 else np.abs(a), 1e-300)
        print("%s: max deviation / scale %.3g" % (key, (np.abs(a - b) / scale).max()))
        assert (np.abs(a - b) <= 1e-6 * scale).all(), key
    assert abs(plain["spline"]["final_cost"] - out["spline"]["final_cost"]) <= 1e-6 * plain["spline"]["final_cost"]
    bi = out["board_image"]
    tot = bi["totals"]
    o = bi["options"]
    print("events %d outside time %d behind %d outside image %d image %s ring %d; mean ring_std %.4g" % (
        int(tot["n_events"]), int(tot["n_outside_time"]), int(tot["n_behind"]), int(tot["n_outside_image"]), tot["n_image"].tolist(),
        int(tot["n_ring"]), float(np.nanmean(bi["ring_std"]))))
    assert int(tot["n_events"]) == N_EVENTS
    assert bi["image"].shape == (2, o.height, o.width)
    assert (bi["image"].sum(axis=(1, 2)) == tot["n_image"]).all()
    assert int(tot["n_outside_time"] + tot["n_behind"] + tot["n_outside_image"] + tot["n_image"].sum()) == N_EVENTS
    assert int(bi["ring_hist"].sum()) == int(tot["n_ring"]) == int(bi["ring_stats"]["n"].sum())
    assert len(bi["ring_std"]) == 36 and bi["ring_hist"].shape == (36, 64)
    # the stream shows the board: most events in time land in the image, and the rings are narrower than the histogram's range
    assert tot["n_image"].sum() > 0.5 * (N_EVENTS - int(tot["n_outside_time"])) and np.nanmean(bi["ring_std"]) < 0.5 * o.ring_range


def test_driver_writes_the_board_image_only_when_asked(tmp_path, chain):
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
        open(yamlf, "w").write(settings + ("BoardImage: 1\n" if key else ""))
        out = subprocess.run([exe, yamlf, binf, str(d), "batch"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[key] = ([ln for ln in out.stdout.splitlines() if not ln.startswith("stage ")], d)
    plain, d0 = outs[False]
    lines, d1 = outs[True]
    # without the key: no line, no file — the parent's output
    assert not any(ln.startswith("board_image") for ln in plain)
    assert sorted(os.listdir(str(d0))) == sorted(set(os.listdir(str(d1))) - {"board_image.png", "BoardImage.txt"})
    assert [ln.split()[0] for ln in plain] == [ln.split()[0] for ln in lines if not ln.startswith("board_image")]
    assert [ln for ln in lines if not ln.startswith("board_image")][:2] == plain[:2]      # keyframes, init calibration: the same chain
    said = [ln.split() for ln in lines if ln.startswith("board_image ")]
    assert len(said) == 1 and said[0][1::2] == ["events", "in_image", "ring", "ring_mean", "ring_std"]
    rep = _parse(str(d1 / "BoardImage.txt"))
    tot, im = rep["totals"], rep["image"]
    # the file is consistent with itself, with the stdout line and with the PNG
    assert tot["n_events"] == N_EVENTS == int(said[0][2])
    assert tot["n_outside_time"] + tot["n_behind"] + tot["n_outside_image"] + tot["n_image_neg"] + tot["n_image_pos"] == N_EVENTS
    assert int(said[0][4]) == tot["n_image_neg"] + tot["n_image_pos"] and int(said[0][6]) == tot["n_ring"]
    assert rep["n_circles"] == 36 == len(rep["circles"])
    assert sum(c["neg_n"] + c["pos_n"] for c in rep["circles"]) == tot["n_ring"]
    rgb = decode_png(str(d1 / "board_image.png"))
    assert rgb.shape == (int(im["height"]), int(im["width"]), 3)
    assert not rgb[:, :, 2].any() and rgb[:, :, :2].max() == 255       # red positive, green negative; the counts above p99 saturate
    assert (rgb[:, :, 0] > 0).sum() > 1000 and (rgb[:, :, 1] > 0).sum() > 1000
    # ... and with the Python chain's board image on the same stream
    py = py_out["board_image"]
    po, pt = py["options"], py["totals"]
    assert (int(im["width"]), int(im["height"])) == (po.width, po.height)
    assert (im["x0"], im["y0"], im["bin"]) == (po.x0, po.y0, po.bin)
    print("driver %s | python %s" % (tot, pt))
    assert tot["n_events"] == int(pt["n_events"])
    # The two chains select the same keyframes and are held to 1e-3 on the refined camera (test_cpp_driver_chain), and
    # test_gpu_report_driver.py holds their residual counts to 1e-3 relative and their rms to 1e-2: the same figures here — every
    # total to 1e-3 of itself (+ 2 events), per circle and polarity the count to 1e-2 (+ 2), the ring's spread to 1e-2 and its
    # mean to 1e-2 of the spread
    for name, mine in (("n_outside_time", tot["n_outside_time"]), ("n_behind", tot["n_behind"]), ("n_outside_image", tot["n_outside_image"]),
                       ("n_ring", tot["n_ring"])):
        print("%s driver %d python %d" % (name, mine, int(pt[name])))
        assert abs(mine - int(pt[name])) <= 1e-3 * int(pt[name]) + 2, name
    for k, name in enumerate(("n_image_neg", "n_image_pos")):
        assert abs(tot[name] - int(pt["n_image"][k])) <= 1e-3 * int(pt["n_image"][k]) + 2, name
    st = py["ring_stats"]
    worst = [0.0, 0.0, 0.0]
    for c, line in enumerate(rep["circles"]):
        for k, pol in enumerate(("neg", "pos")):
            n = float(st["n"][c, k])
            assert abs(line[pol + "_n"] - n) <= 1e-2 * n + 2, (c, pol)
            if n < 100:
                continue
            mean = st["sum_d"][c, k] / n
            std = np.sqrt(max(st["sum_d2"][c, k] / n - mean * mean, 0.0))
            worst = [max(worst[0], abs(line[pol + "_n"] - n) / n), max(worst[1], abs(line[pol + "_ring_std"] - std) / std),
                     max(worst[2], abs(line[pol + "_ring_mean"] - mean) / std)]
            assert abs(line[pol + "_ring_std"] - std) <= 1e-2 * std, (c, pol, line[pol + "_ring_std"], std)
            assert abs(line[pol + "_ring_mean"] - mean) <= 1e-2 * std, (c, pol, line[pol + "_ring_mean"], mean)
    print("per circle and polarity, driver against python: worst count %.3g, ring_std %.3g relative, ring_mean %.3g of the spread" % tuple(worst))
    py_n = float(st["n"].sum())
    py_mean = st["sum_d"].sum() / py_n
    py_std = np.sqrt(st["sum_d2"].sum() / py_n - py_mean ** 2)
    assert abs(float(said[0][10]) - py_std) <= 1e-2 * py_std and abs(float(said[0][8]) - py_mean) <= 1e-2 * py_std
