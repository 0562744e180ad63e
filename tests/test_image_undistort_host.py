"""CPU: image undistortion (include/ecal.h, "image undistortion").  ecal_undistort_image_host, ecal_image_table_host,
ecal_image_maps_host, ecal_distort_points_host and a plain-g++ build of eventcalib_amd/csrc/image_undistort.hpp
(tests/cpp/check_image_undistort.cpp) against the numpy restatement tests/image_undistort_oracle.py.

RADIAL (cameras B, P, I) bit for bit: the neighbour tables (indices, order, weight bits), the u8 pictures of both methods and both
normalize values, the forward projection's coordinates and flags, the f32 maps.  FISHEYE (camera F): tan and atan are the operations
that are not correctly rounded, so positions agree to ~1e-13 px (design/20_undistort.md derives 1e-9 px as the bar); the tables must
still be the same because the smallest |d2 - 4| of any candidate pair is four orders of magnitude above that (asserted as the
precondition), weights within 1e-9 relative, maps within one f32 ulp, pictures at most one level apart in at most 0.5 % of the pixels.
Known answers, round trips through ud_point, an independent bilinear (scipy.ndimage.map_coordinates in f64), every refusal's text and
the header under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import image_undistort_oracle as IO
import undistort_oracle as UO
from eventcalib_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_image_undistort.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-O2"]
RADIAL_NAMES = ["B346", "B64", "B37", "P64", "I40"]
ALL_NAMES = RADIAL_NAMES + ["F64"]
POSITION_TOL_PX = 1e-9       # design/20_undistort.md: host, numpy and device agree on a FISHEYE position within this
LEVEL_SHARE = 0.005          # pictures: at most one level apart in at most 0.5 % of the pixels


def lib_camera(name):
    cam, W, H = IO.camera(name)
    return capi.undistort_camera(cam["intr"], cam["model"]), cam, W, H


def lib_options(d):
    return capi.image_options(method=d["method"], channels=d["channels"], out_width=d["out_width"], out_height=d["out_height"],
                              normalize=d["normalize"], off_x=d["off_x"], off_y=d["off_y"])


def frames(name, C, n=1):
    _, W, H = IO.camera(name)
    rng = np.random.default_rng(sum(name.encode()) * 8 + C)
    return rng.integers(0, 256, (n, H, W, C), dtype=np.uint8)


_TABLES, _MAPS = {}, {}


def oracle_table(name):
    """the numpy table on the reference canvas, computed once per camera"""
    if name not in _TABLES:
        cam, W, H = IO.camera(name)
        _TABLES[name] = IO.table(cam, W, H, IO.reference_options(W, H))
    return _TABLES[name]


def oracle_maps(name):
    if name not in _MAPS:
        cam, W, H = IO.camera(name)
        _MAPS[name] = IO.maps(cam, W, H, IO.reference_options(W, H))
    return _MAPS[name]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("image_undistort") / "check_image_undistort")
    subprocess.check_call(["g++"] + FLAGS + ["-o", path, SRC])
    return path


def gxx(exe, tmp_path, what, c, W, H, payload):
    fin, fout = str(tmp_path / (what + "_in.bin")), str(tmp_path / (what + "_out.bin"))
    with open(fin, "wb") as f:
        f.write(bytes(c) + np.array([W, H], np.uint32).tobytes() + payload)
    r = subprocess.run([exe, what, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(fout, "rb").read()


def gxx_table(exe, tmp_path, c, W, H, o):
    raw = gxx(exe, tmp_path, "table", c, W, H, bytes(o))
    n, n_inv, n_empty, most = [int(v) for v in np.frombuffer(raw[:32], np.uint64)]
    npix = int(o.out_width) * int(o.out_height)
    a = 32 + 4 * (npix + 1)
    return (np.frombuffer(raw[32:a], np.uint32), np.frombuffer(raw[a:a + 4 * n], np.uint32), np.frombuffer(raw[a + 4 * n:], np.float64),
            {"n_invalid_sources": n_inv, "n_empty": n_empty, "max_neighbours": most, "n_entries": n})


def gxx_maps(exe, tmp_path, c, W, H, o):
    raw = gxx(exe, tmp_path, "maps", c, W, H, bytes(o))
    npix = int(o.out_width) * int(o.out_height)
    shape = (int(o.out_height), int(o.out_width))
    return (np.frombuffer(raw[:4 * npix], np.float32).reshape(shape), np.frombuffer(raw[4 * npix:8 * npix], np.float32).reshape(shape),
            np.frombuffer(raw[8 * npix:9 * npix], np.uint8).reshape(shape))


def gxx_image(exe, tmp_path, c, W, H, o, frame):
    raw = gxx(exe, tmp_path, "image", c, W, H, bytes(o) + np.ascontiguousarray(frame).tobytes())
    n = int(o.out_width) * int(o.out_height) * int(o.channels)
    return np.frombuffer(raw[:n], np.uint8).reshape(int(o.out_height), int(o.out_width), int(o.channels)), np.frombuffer(raw[n:], np.float32)


def gxx_points(exe, tmp_path, c, W, H, uv):
    uv = np.ascontiguousarray(uv, np.float64)
    raw = gxx(exe, tmp_path, "points", c, W, H, np.uint64(uv.shape[0]).tobytes() + uv.tobytes())
    n = uv.shape[0]
    return np.frombuffer(raw[:16 * n], np.float64).reshape(n, 2), np.frombuffer(raw[16 * n:], np.uint8)


def b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def b32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def canvas_points(d):
    X, Y = np.meshgrid(np.arange(d["out_width"], dtype=np.float64), np.arange(d["out_height"], dtype=np.float64))
    return np.stack([X.ravel() - np.float64(d["off_x"]), Y.ravel() - np.float64(d["off_y"])], axis=1)


ODD_POINTS = np.array([[np.nan, 1.0], [1.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [-np.inf, np.inf], [1e300, 1e300], [1e6, -1e6],
                       [1e-300, 1e-300], [-0.0, 0.0], [17.25, 9.75], [-3.5, 40.125]])


def test_reference_options_are_rounded_unlike_the_event_frames():
    for (w, h), (cw, ch, ox, oy) in (((346, 260), (415, 312, 35.0, 26.0)), ((64, 48), (77, 58, 6.0, 5.0)), ((37, 29), (44, 35, 4.0, 3.0)),
                                     ((1280, 720), (1536, 864, 128.0, 72.0)), ((5, 3), (6, 4, 1.0, 0.0))):
        o = capi.image_reference_options(w, h)
        assert (o.method, o.channels, o.out_width, o.out_height, o.normalize, o.reserved) == (capi.IMAGE_REFERENCE, 3, cw, ch, 1, 0)
        assert (o.off_x, o.off_y) == (ox, oy)
        want = IO.reference_options(w, h)
        assert o.as_dict() == want
        assert capi.image_options_error(o) is None
    assert capi.undistort_reference_canvas(346, 260).off_x == 34.6   # (the event frames' offset is not rounded)


@pytest.mark.parametrize("name", RADIAL_NAMES)
def test_radial_tables_are_bit_for_bit_the_numpy_rule(exe, tmp_path, name):
    c, cam, W, H = lib_camera(name)
    o = capi.image_reference_options(W, H)
    want = oracle_table(name)
    lib = capi.image_table_host(c, W, H, o)
    for who, (off, idx, w, info) in (("library", lib), ("g++", gxx_table(exe, tmp_path, c, W, H, o))):
        assert (off == want["off"]).all(), who
        assert idx.size == want["idx"].size and (idx == want["idx"]).all(), who
        assert (b64(w) == b64(want["w"])).all(), who
        for k in ("n_invalid_sources", "n_empty", "max_neighbours"):
            assert int(info[k]) == want[k], (who, k)
        assert int(info["n_entries"]) == want["idx"].size
    print("%s: %d entries, %.2f a canvas pixel, %d at most, %.1f %% empty" % (name, want["idx"].size, want["idx"].size / (want["off"].size - 1),
                                                                             want["max_neighbours"], 100.0 * want["n_empty"] / (want["off"].size - 1)))


def test_the_prototype_figures_of_the_reference_canvases():
    """what the issue measured: the most neighbours of a canvas pixel and the share of empty pixels"""
    for name, most, empty_percent in (("B346", 23, 41), ("B64", 21, 35), ("B37", 19, 28), ("P64", 13, 12), ("F64", 13, 0)):
        t = oracle_table(name)
        assert t["max_neighbours"] == most, name
        assert round(100.0 * t["n_empty"] / (t["off"].size - 1)) == empty_percent, name
    assert abs(oracle_table("B346")["idx"].size / (415 * 312) - 8.7) < 0.05


@pytest.mark.parametrize("name", RADIAL_NAMES)
@pytest.mark.parametrize("channels", [1, 3])
def test_radial_pictures_are_bit_for_bit_the_numpy_rule(exe, tmp_path, name, channels):
    c, cam, W, H = lib_camera(name)
    frame = frames(name, channels)[0]
    for method in (IO.REFERENCE, IO.BILINEAR):
        for normalize in (0, 1):
            d = dict(IO.reference_options(W, H), method=method, channels=channels, normalize=normalize)
            o = lib_options(d)
            want, (mn, mx) = IO.undistort(cam, W, H, d, frame, tab=oracle_table(name), mp=oracle_maps(name))
            got, mm, info = capi.undistort_image_host(c, W, H, frame, o)
            assert (got == want).all(), (method, normalize)
            assert b32(mm).tolist() == b32([mn, mx]).tolist()
            if name != "B346" or channels == 3:   # (the big case once through the g++ build)
                g_pic, g_mm = gxx_image(exe, tmp_path, c, W, H, o, frame)
                assert (g_pic == want).all() and b32(g_mm).tolist() == b32([mn, mx]).tolist()
            if method == IO.REFERENCE:
                assert int(info["n_empty"]) == oracle_table(name)["n_empty"]
            else:
                assert int(info["n_empty"]) == int((oracle_maps(name)[2] == 0).sum()) == int(info["n_invalid"])
    # (H, W) in, (oh, ow) out
    if channels == 1:
        got2, _, _ = capi.undistort_image_host(c, W, H, frame[:, :, 0], o)
        assert got2.shape == (d["out_height"], d["out_width"]) and (got2 == got[:, :, 0]).all()


@pytest.mark.parametrize("name", RADIAL_NAMES)
def test_radial_forward_projection_and_maps_are_bit_for_bit(exe, tmp_path, name):
    c, cam, W, H = lib_camera(name)
    d = IO.reference_options(W, H)
    uv = np.concatenate([canvas_points(d), canvas_points(d)[::7] + 0.37, ODD_POINTS])
    want, want_flag = IO.distort_points(cam, W, H, uv)
    for who, (got, flag) in (("library", capi.distort_points_host(c, W, H, uv)), ("g++", gxx_points(exe, tmp_path, c, W, H, uv))):
        assert (flag == want_flag).all(), who
        assert (b64(got) == b64(want)).all(), who
    assert (want_flag[-11:-5] == IO.DISTORT_INVALID).all(), "NaN, +-inf and far points are invalid"
    assert (want_flag == IO.DISTORT_NOT_CONVERGED).sum() == 0
    r_lim, truncated = capi.camera_monotone_radius(c, W, H)
    assert (r_lim, truncated) == IO.monotone_radius(cam, W, H) and truncated == 0
    o = lib_options(dict(d, method=IO.BILINEAR))
    wx, wy, wvalid, _ = oracle_maps(name)
    for who, (mx, my, valid) in (("library", capi.image_maps_host(c, W, H, o)[:3]), ("g++", gxx_maps(exe, tmp_path, c, W, H, o))):
        assert (b32(mx) == b32(wx)).all() and (b32(my) == b32(wy)).all() and (valid == wvalid).all(), who
    assert ((wx == -1.0) & (wy == -1.0))[wvalid == 0].all()
    info = capi.image_maps_host(c, W, H, o)[3]
    assert info["r_lim"] == r_lim and info["n_not_converged"] == 0 and int(info["n_invalid"]) == int((wvalid == 0).sum())


def test_fisheye_against_numpy_under_the_stated_bars(exe, tmp_path):
    name = "F64"
    c, cam, W, H = lib_camera(name)
    d = IO.reference_options(W, H)
    o = capi.image_reference_options(W, H)
    want = oracle_table(name)
    margin = float(np.abs(want["all_d2"] - 4.0).min())
    print("fisheye: smallest |d2 - 4| of a candidate pair %.2e" % margin)
    # the precondition: a position error of POSITION_TOL_PX moves d2 by at most 2 * 2.9 * 1e-9 (|d| < 2.9 among the candidates)
    assert margin > 1e4 * POSITION_TOL_PX
    for who, (off, idx, w, info) in (("library", capi.image_table_host(c, W, H, o)), ("g++", gxx_table(exe, tmp_path, c, W, H, o))):
        assert (off == want["off"]).all() and (idx == want["idx"]).all(), who
        worst = float(np.abs(w / want["w"] - 1.0).max())
        print("fisheye, %s against numpy: weights within %.2e relative" % (who, worst))
        assert worst <= 1e-9, who
    wx, wy, wvalid, _ = oracle_maps(name)
    om = lib_options(dict(d, method=IO.BILINEAR))
    for who, (mx, my, valid) in (("library", capi.image_maps_host(c, W, H, om)[:3]), ("g++", gxx_maps(exe, tmp_path, c, W, H, om))):
        assert (valid == wvalid).all(), who
        ulps = max(int(np.abs(b32(mx).astype(np.int64) - b32(wx).astype(np.int64)).max()), int(np.abs(b32(my).astype(np.int64) - b32(wy).astype(np.int64)).max()))
        print("fisheye, %s against numpy: maps within %d f32 ulp" % (who, ulps))
        assert ulps <= 1, who
    uv = canvas_points(d)
    want_uv, want_flag = IO.distort_points(cam, W, H, uv)
    got_uv, flag = capi.distort_points_host(c, W, H, uv)
    assert (flag == want_flag).all() and float(np.abs(got_uv - want_uv).max()) <= POSITION_TOL_PX
    for channels in (1, 3):
        frame = frames(name, channels)[0]
        for method in (IO.REFERENCE, IO.BILINEAR):
            for normalize in (0, 1):
                dd = dict(d, method=method, channels=channels, normalize=normalize)
                ref, _ = IO.undistort(cam, W, H, dd, frame, tab=want, mp=oracle_maps(name))
                for who, got in (("library", capi.undistort_image_host(c, W, H, frame, lib_options(dd))[0]),
                                 ("g++", gxx_image(exe, tmp_path, c, W, H, lib_options(dd), frame)[0])):
                    diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
                    share = float((diff > 0).mean())
                    print("fisheye, %s, method %d, %d channel(s), normalize %d: %d of %d values differ (%.4f %%), at most %d level(s)"
                          % (who, method, channels, normalize, int((diff > 0).sum()), diff.size, 100.0 * share, int(diff.max())))
                    assert diff.max() <= 1 and share <= LEVEL_SHARE, (who, method, channels, normalize)


@pytest.mark.parametrize("method", [IO.REFERENCE, IO.BILINEAR])
def test_identity_camera_shifts_the_picture_by_the_offsets(method):
    c, cam, W, H = lib_camera("I40")
    d = dict(IO.reference_options(W, H), method=method, normalize=0)
    ox, oy = int(d["off_x"]), int(d["off_y"])
    for channels in (1, 3):
        frame = frames("I40", channels)[0]
        got, _, info = capi.undistort_image_host(c, W, H, frame, lib_options(dict(d, channels=channels)))
        assert (got[oy:oy + H, ox:ox + W] == frame).all()
        # black elsewhere: BILINEAR everywhere off the sensor; REFERENCE from 2 px off the sensor on (d2 < 4 is strict; a pixel 1 px
        # off has neighbours)
        far = np.ones(got.shape[:2], bool)
        m = 0 if method == IO.BILINEAR else 1
        far[oy - m:oy + H + m, ox - m:ox + W + m] = False
        assert far.any() and (got[far] == 0).all()
        if method == IO.REFERENCE:
            assert int(info["n_empty"]) == oracle_table("I40")["n_empty"] == int(far.sum())


def test_one_value_frames_and_flat_frames():
    for name in ("B37", "F64"):
        c, cam, W, H = lib_camera(name)
        d = IO.reference_options(W, H)
        tab = oracle_table(name)
        covered = (np.diff(tab["off"].astype(np.int64)) > 0).reshape(d["out_height"], d["out_width"])
        frame = np.full((H, W, 3), 77, np.uint8)
        got, mm, _ = capi.undistort_image_host(c, W, H, frame, lib_options(d))
        if covered.all():   # (F64: no empty pixel, the averages of one value span a few f32 ulp — far more than DBL_EPSILON)
            assert mm[0] > 76.99 and mm[1] < 77.01
        else:
            assert (got[covered] == 255).all() and (got[~covered] == 0).all() and mm[0] == 0.0
        # max - min <= DBL_EPSILON: all 0
        got0, mm0, _ = capi.undistort_image_host(c, W, H, np.zeros((H, W, 3), np.uint8), lib_options(d))
        assert (got0 == 0).all() and mm0.tolist() == [0.0, 0.0]
    # BILINEAR on the identity camera, canvas = sensor: every value is the frame's one value exactly, min == max
    c, cam, W, H = lib_camera("I40")
    flat = np.full((H, W, 1), 200, np.uint8)
    got, mm, _ = capi.undistort_image_host(c, W, H, flat, capi.image_options(sensor=(W, H), normalize=1))
    assert mm.tolist() == [200.0, 200.0] and (got == 0).all()
    got, _, _ = capi.undistort_image_host(c, W, H, flat, capi.image_options(sensor=(W, H), normalize=0))
    assert (got == 200).all()


@pytest.mark.parametrize("name", ALL_NAMES)
def test_round_trip_through_ud_point(name):
    c, cam, W, H = lib_camera(name)
    d = IO.reference_options(W, H)
    uv = canvas_points(d)
    out, flag = capi.distort_points_host(c, W, H, uv)
    ok = flag != capi.DISTORT_INVALID
    assert ok.sum() > 0.8 * W * H and (flag == capi.DISTORT_NOT_CONVERGED).sum() == 0
    back, bad = capi.undistort_points_host(c, out[ok])
    assert bad.sum() == 0
    worst = float(np.abs(back - uv[ok]).max())
    print("%s: round trip %.2e px over %d valid canvas pixels of %d" % (name, worst, int(ok.sum()), ok.size))
    assert worst <= 1e-9
    # every sensor pixel is inside the limit: its ideal position projects back onto it
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    px = np.stack([cols.ravel(), rows.ravel()], axis=1)
    ideal, inv = capi.undistort_points_host(c, px)
    again, fl = capi.distort_points_host(c, W, H, ideal[inv == 0])
    assert inv.sum() == 0 and (fl == 0).all() and float(np.abs(again - px).max()) <= 1e-9


def test_points_beyond_the_limit_and_a_truncated_camera():
    c, cam, W, H = lib_camera("B64")
    r_lim, truncated = capi.camera_monotone_radius(c, W, H)
    g_lim = float(IO.g(cam, np.float64(r_lim)))
    fx, fy, cx, cy = cam["intr"][:4]
    just_in, just_out = g_lim * (1.0 - 1e-12), g_lim * (1.0 + 1e-12)
    uv = np.array([[cx + fx * just_in, cy], [cx + fx * just_out, cy], [cx, cy - fy * just_out], [cx, cy - fy * just_in]])
    _, flag = capi.distort_points_host(c, W, H, uv)
    assert flag.tolist() == [0, capi.DISTORT_INVALID, capi.DISTORT_INVALID, 0] and truncated == 0
    _, flag = capi.distort_points_host(c, W, H, ODD_POINTS[:7])
    assert (flag == capi.DISTORT_INVALID).all()
    # g' = 1 - 150 r^2 turns negative at r = 0.0816, well inside the sensor
    intr = [48.0, 47.5, 31.2, 23.9, -50.0, 0.0, 0.0, 0.0, 0.0]
    cam50 = UO.camera(UO.RADIAL, intr)
    c50 = capi.undistort_camera(intr, capi.CAMERA_RADIAL)
    r50, t50 = capi.camera_monotone_radius(c50, 64, 48)
    assert t50 == 1 and (r50, t50) == IO.monotone_radius(cam50, 64, 48) and 0.08 < r50 < (1.0 / 150.0) ** 0.5
    uv = canvas_points(IO.reference_options(64, 48))
    out, flag = capi.distort_points_host(c50, 64, 48, uv)
    want, want_flag = IO.distort_points(cam50, 64, 48, uv)
    assert (flag == want_flag).all() and (b64(out) == b64(want)).all()
    ok = flag != capi.DISTORT_INVALID
    assert 0 < ok.sum() < ok.size
    r = np.sqrt(((out[ok, 0] - intr[2]) / intr[0]) ** 2 + ((out[ok, 1] - intr[3]) / intr[1]) ** 2)
    assert r.max() <= r50 * (1.0 + 1e-12), "no valid point lies beyond r_lim"
    info = capi.image_maps_host(c50, 64, 48, capi.image_options(sensor=(64, 48)))[3]
    assert info["truncated"] == 1 and info["r_lim"] == r50


@pytest.mark.parametrize("name", ALL_NAMES)
def test_an_independent_bilinear(name):
    """scipy.ndimage.map_coordinates(order=1) in f64 on the same maps, on the canvas pixels whose four taps lie on the sensor: the f32
    arithmetic of the rule (24-bit weights, three rounded sums) moves a value by a few 1e-5 of a level, so a picture differs from the
    f64 one only where a value falls that close to a half: at most one level, in at most 0.5 % of those pixels"""
    from scipy import ndimage
    c, cam, W, H = lib_camera(name)
    d = dict(IO.reference_options(W, H), method=IO.BILINEAR, normalize=0)
    mx, my, valid, _ = capi.image_maps_host(c, W, H, lib_options(dict(d, channels=1)))
    inner = (valid == 1) & (mx >= 0.0) & (mx <= W - 1.0) & (my >= 0.0) & (my <= H - 1.0)
    assert inner.sum() > 0.7 * W * H
    for channels in (1, 3):
        frame = frames(name, channels)[0]
        got, _, _ = capi.undistort_image_host(c, W, H, frame, lib_options(dict(d, channels=channels)))
        coords = np.stack([my[inner].astype(np.float64), mx[inner].astype(np.float64)])
        total = differ = 0
        for ch in range(channels):
            ref = ndimage.map_coordinates(frame[:, :, ch].astype(np.float64), coords, order=1, mode="constant", cval=0.0)
            ref = np.clip(UO.round_half_away(ref), 0, 255).astype(np.int32)
            diff = np.abs(got[:, :, ch][inner].astype(np.int32) - ref)
            assert diff.max() <= 1
            total += diff.size
            differ += int((diff > 0).sum())
        print("%s, %d channel(s): %d of %d inner values differ from the f64 bilinear by one level (%.4f %%)"
              % (name, channels, differ, total, 100.0 * differ / total))
        assert differ <= LEVEL_SHARE * total


def test_every_refusal_names_its_field():
    c, cam, W, H = lib_camera("B37")
    ok = capi.image_reference_options(W, H)
    assert capi.image_options_error(ok) is None and capi.image_options_error(None) == "null options"
    frame = frames("B37", 3)[0]
    for change, text in ((dict(method=2), "method must be ECAL_IMAGE_REFERENCE or ECAL_IMAGE_BILINEAR"), (dict(channels=2), "channels must be 1 or 3"),
                         (dict(channels=0), "channels must be 1 or 3"), (dict(channels=4), "channels must be 1 or 3"),
                         (dict(out_width=0), "out_width from 1 to 8192"), (dict(out_width=8193), "out_width from 1 to 8192"),
                         (dict(out_height=0), "out_height from 1 to 8192"), (dict(out_height=8193), "out_height from 1 to 8192"),
                         (dict(normalize=2), "normalize must be 0 or 1"), (dict(reserved=1), "options reserved must be 0"),
                         (dict(off_x=np.nan), "off_x must be finite"), (dict(off_x=np.inf), "off_x must be finite"),
                         (dict(off_y=-np.inf), "off_y must be finite")):
        o = capi.image_options(sensor=(W, H), reference_canvas=True, **change)
        assert capi.image_options_error(o) == text, change
        for call in (lambda: capi.undistort_image_host(c, W, H, frame, o), lambda: capi.image_table_host(c, W, H, o),
                     lambda: capi.image_maps_host(c, W, H, o)):
            with pytest.raises(capi.EcalError) as e:
                call()
            assert e.value.status == -1 and text in str(e.value)
    assert capi.image_options_error(capi.image_options(sensor=(W, H), out_width=8192, out_height=1)) is None
    # the sensor, the camera
    for w, h, text in ((0, 29, "width from 1 to 8192"), (8193, 29, "width from 1 to 8192"), (37, 0, "height from 1 to 8192"), (37, 8193, "height from 1 to 8192")):
        for call in (lambda: capi.camera_monotone_radius(c, w, h), lambda: capi.distort_points_host(c, w, h, [[1.0, 2.0]]),
                     lambda: capi.image_maps_host(c, w, h, ok)):
            with pytest.raises(capi.EcalError) as e:
                call()
            assert e.value.status == -1 and text in str(e.value)
    bad = capi.undistort_camera(cam["intr"], capi.CAMERA_RADIAL)
    bad.intr[0] = 0.0
    for call in (lambda: capi.camera_monotone_radius(bad, W, H), lambda: capi.distort_points_host(bad, W, H, [[1.0, 2.0]]),
                 lambda: capi.undistort_image_host(bad, W, H, frame, ok), lambda: capi.image_table_host(bad, W, H, ok)):
        with pytest.raises(capi.EcalError) as e:
            call()
        assert e.value.status == -1 and "fx must be finite and above 0" in str(e.value)
    # the table is REFERENCE's
    with pytest.raises(capi.EcalError):
        capi.image_table_host(c, W, H, capi.image_options(sensor=(W, H)))
    with pytest.raises(ValueError):
        capi.undistort_image_host(c, W, H, frame[:, :-1], ok)
    with pytest.raises(ValueError):
        capi.undistort_image_host(c, W, H, frame.astype(np.float32), ok)


def test_the_driver_s_npy_writer_loads_with_numpy(tmp_path):
    """host/npy_writer.hpp, what the driver writes undistort_map_x.npy / _y.npy with, from a program of its own"""
    exe = str(tmp_path / "check_npy_writer")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "check_npy_writer.cpp")])
    for rows, cols in ((312, 415), (1, 1), (3, 100000), (29, 37)):   # (header dicts of different lengths)
        path = str(tmp_path / ("a_%d_%d.npy" % (rows, cols)))
        assert subprocess.run([exe, str(rows), str(cols), path]).returncode == 0
        a = np.load(path)
        assert a.dtype == np.float32 and a.shape == (rows, cols) and a.flags["C_CONTIGUOUS"]
        want = (np.arange(rows, dtype=np.float32)[:, None] * 1000 + np.arange(cols, dtype=np.float32)[None, :]).astype(np.float32) + np.float32(0.25)
        want[-1, -1] = -1.0
        assert (a == want).all()
        assert (os.path.getsize(path) - rows * cols * 4) % 64 == 0


def test_header_under_sanitizers(tmp_path):
    """the stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (its own main: nothing is preloaded): its own known
    answers, and the 37 x 29 case of both methods against the library"""
    exe = str(tmp_path / "check_image_undistort_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, SRC])
    r = subprocess.run([exe, "self"], capture_output=True, text=True)
    assert r.returncode == 0 and "self ok" in r.stdout, r.stdout + r.stderr
    c, cam, W, H = lib_camera("B37")
    frame = frames("B37", 3)[0]
    for method in (IO.REFERENCE, IO.BILINEAR):
        o = lib_options(dict(IO.reference_options(W, H), method=method))
        got, mm = gxx_image(exe, tmp_path, c, W, H, o, frame)
        want, want_mm, _ = capi.undistort_image_host(c, W, H, frame, o)
        assert (got == want).all() and b32(mm).tolist() == b32(want_mm).tolist()
    off, idx, w, _ = gxx_table(exe, tmp_path, c, W, H, capi.image_reference_options(W, H))
    want = capi.image_table_host(c, W, H, capi.image_reference_options(W, H))
    assert (off == want[0]).all() and (idx == want[1]).all() and (b64(w) == b64(want[2])).all()
    uv = np.concatenate([canvas_points(IO.reference_options(W, H)), ODD_POINTS])
    got, flag = gxx_points(exe, tmp_path, c, W, H, uv)
    want, want_flag = capi.distort_points_host(c, W, H, uv)
    assert (flag == want_flag).all() and (b64(got) == b64(want)).all()
