"""GPU: the undistortion kernels (eventcalib_amd/csrc/ecal_undistort.hip) through capi.Context, against the numpy restatement of the
rule (tests/undistort_oracle.py) and the host entry point.

Points: RADIAL bit for bit ecal_undistort_points_host, FISHEYE the same flags and coordinates within 1e-9 px (tan is the one operation
that is not correctly rounded: tests/test_undistort_host.py has the reasoning), sizes around the wave, the block of 4096 and three
blocks, the records at 0, 1, 7 and 15 bytes past a 16-byte boundary with nothing behind them.
Events, SUBPIXEL and PIXEL: the output is the oracle's, record for record — stamps and polarity bytes (0, 1, 7) untouched, the order
kept, the count and the totals exact, nothing stored behind the last kept record; all kept, all invalid, all outside, kept runs that
straddle every block edge, the exact halves, the fisheye case on the reference canvas.
Frames: S in {1, 3} with an empty window and one that has a single polarity, 346 x 260 on the reference canvas (presence bits in LDS),
640 x 480 (presence bits in context scratch) and a 5 x 3 sensor on 6 x 4; the RGB bytes and the per-window totals equal the numpy
rule exactly, packed and double segments give the same bytes, ecal_stream_undistorted_frames equals the staged calls."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import undistort_oracle as UO  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCK = 4096
RADIAL_INTR = [251.3, 249.8, 171.2, 129.9, -0.21, 0.07, -0.012, 0.0011, -0.00004]
FISHEYE_INTR = [180.0, 180.0, 175.5, 127.5, -0.02, 0.003, 0.0, 0.0, 0.0]
FISHEYE_TOL_PX = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    with eventcalib_amd.Context(0) as c:
        yield c


def records(t, x, y, p):
    n = len(t)
    rec = np.zeros(n, UO.RECORD)
    rec["t"], rec["x"], rec["y"], rec["p"] = t, x, y, p
    return np.frombuffer(rec.tobytes(), np.uint8).copy()


def random_records(rng, n, lo=(-40, -40), hi=(400, 300), nan_every=0):
    x = rng.integers(lo[0], hi[0], n).astype(np.float64)
    y = rng.integers(lo[1], hi[1], n).astype(np.float64)
    if nan_every:
        x[::nan_every] = np.nan
    return records(5.0 + np.arange(n) * 1e-6, x, y, rng.choice([0, 1, 7], n))


def cams(intr, model, out_k=None):
    from eventcalib_amd import capi
    return capi.undistort_camera(intr, model, out_k=out_k), UO.camera(model, intr, out_k)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- points ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def point_streams():
    rng = np.random.default_rng(31)
    n = 3 * BLOCK + 7
    rec = random_records(rng, n, nan_every=211)
    r = rec.reshape(-1, 25)
    r[5, 8:16] = np.frombuffer(np.float64(np.inf).tobytes(), np.uint8)
    r[6, 16:24] = np.frombuffer(np.float64(-np.inf).tobytes(), np.uint8)
    r[7, 8:24] = np.frombuffer(np.array([100.5, 77.25]).tobytes(), np.uint8)   # a sub-pixel input
    return rec


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
def test_points_against_the_host_function(ctx, point_streams, n, shift):
    import torch
    from eventcalib_amd import capi
    rec = point_streams[: n * 25]
    uv_in = np.frombuffer(rec.tobytes(), UO.RECORD)
    uv_in = np.stack([uv_in["x"], uv_in["y"]], axis=1) if n else np.zeros((0, 2))
    arena = torch.full((16 + shift + n * 25,), 0xEE, dtype=torch.uint8, device="cuda")   # the records end the allocation
    view = arena[16 + shift:]
    view.copy_(torch.from_numpy(rec.copy()))
    assert arena.data_ptr() % 16 == 0 and view.numel() == n * 25
    st = torch.cuda.current_stream().cuda_stream
    for model, intr in ((capi.CAMERA_RADIAL, RADIAL_INTR), (capi.CAMERA_FISHEYE, FISHEYE_INTR)):
        cam, ocam = cams(intr, model)
        want, want_flag = capi.undistort_points_host(cam, uv_in)
        uv = torch.full((2 * n + 4,), -7.0, dtype=torch.float64, device="cuda")
        flag = torch.full((n + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        ctx.undistort_points_dev(cam, view.data_ptr() if n else None, n, uv.data_ptr() if n else None, flag.data_ptr() if n else None, st)
        torch.cuda.synchronize()
        got, got_flag = uv[: 2 * n].cpu().numpy().reshape(n, 2), flag[:n].cpu().numpy()
        assert (uv[2 * n:] == -7.0).all() and (flag[n:] == 0xEE).all()   # nothing behind n records' worth is stored
        assert (got_flag == want_flag).all()
        oracle, oracle_flag = UO.points(ocam, uv_in)
        assert (oracle_flag == want_flag).all()
        if model == capi.CAMERA_RADIAL:
            assert (bits(got) == bits(want)).all() and (bits(got) == bits(oracle)).all()
        elif n:
            worst = float(np.abs(got - want).max())
            print("fisheye, device against host, n = %d: largest difference %.3e px" % (n, worst))
            assert worst <= FISHEYE_TOL_PX and float(np.abs(got - oracle).max()) <= FISHEYE_TOL_PX
        if n > 1000:
            assert 0 < want_flag.sum() < n
    assert (arena[: 16 + shift] == 0xEE).all() and torch.equal(view.cpu(), torch.from_numpy(rec.copy()))


# ---- events ------------------------------------------------------------------------------------------------------------------------------
def check_events(ctx, cam, ocam, opt, rec, exact=True):
    """Context.undistort_events against the oracle applied to the input; returns the totals"""
    want, want_tot = UO.events(ocam, opt.as_dict(), rec)
    out, tot = ctx.undistort_events(cam, rec, opt)
    got = out.cpu().numpy()
    assert {k: int(tot[k]) for k in tot.dtype.names} == want_tot
    assert got.size == want.size == want_tot["n_kept"] * 25
    if exact:
        assert got.tobytes() == want.tobytes()
    else:
        g, w = np.frombuffer(got.tobytes(), UO.RECORD), np.frombuffer(want.tobytes(), UO.RECORD)
        assert (bits(g["t"]) == bits(w["t"])).all() and (g["p"] == w["p"]).all()
        assert max(np.abs(g["x"] - w["x"]).max(), np.abs(g["y"] - w["y"]).max()) <= FISHEYE_TOL_PX
    kept = np.frombuffer(got.tobytes(), UO.RECORD)
    if kept.size:
        assert (np.diff(kept["t"]) > 0).all()          # the order is kept (the stamps of these streams ascend strictly)
        assert set(np.unique(kept["p"])) <= {0, 1, 7}
    return want_tot


def pixel_options(w=346, h=260, **change):
    from eventcalib_amd import capi
    return capi.undistort_options(sensor=(w, h), **change)


@pytest.mark.parametrize("n", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
def test_events_sizes_both_modes(ctx, n):
    from eventcalib_amd import capi
    rng = np.random.default_rng(100 + n)
    rec = random_records(rng, n, lo=(-300, -300), hi=(650, 560), nan_every=97)
    cam, ocam = cams(RADIAL_INTR, capi.CAMERA_RADIAL)
    tot = check_events(ctx, cam, ocam, capi.undistort_options(), rec)
    assert tot["n_outside"] == 0 and (n < 100 or 0 < tot["n_invalid"] < n)
    tot = check_events(ctx, cam, ocam, pixel_options(), rec)
    assert n < 100 or (tot["n_outside"] > 0 and tot["n_invalid"] > 0 and tot["n_kept"] > 0)
    if n:
        p = np.frombuffer(rec.tobytes(), UO.RECORD)["p"]
        assert n < 100 or set(np.unique(p)) == {0, 1, 7}


def test_all_kept_all_invalid_all_outside(ctx):
    from eventcalib_amd import capi
    rng = np.random.default_rng(7)
    n = 2 * BLOCK + 77
    rec = random_records(rng, n, lo=(0, 0), hi=(346, 260))
    cam, ocam = cams(RADIAL_INTR, capi.CAMERA_RADIAL)
    assert check_events(ctx, cam, ocam, capi.undistort_options(), rec)["n_kept"] == n
    corner = random_records(rng, n, lo=(0, 0), hi=(50, 50))
    cam, ocam = cams([250.0, 250.0, 175.5, 127.5, -50.0, 0.0, 0.0, 0.0, 0.0], capi.CAMERA_RADIAL)
    for opt in (capi.undistort_options(), pixel_options()):
        assert check_events(ctx, cam, ocam, opt, corner)["n_invalid"] == n
    cam, ocam = cams(RADIAL_INTR, capi.CAMERA_RADIAL)
    assert check_events(ctx, cam, ocam, pixel_options(off_x=1e6), rec)["n_outside"] == n
    assert check_events(ctx, cam, ocam, pixel_options(off_y=-1e6), rec)["n_outside"] == n


def test_kept_runs_that_straddle_every_block_edge(ctx):
    from eventcalib_amd import capi
    rng = np.random.default_rng(8)
    n = 4 * BLOCK + 100
    rec = np.frombuffer(random_records(rng, n, lo=(0, 0), hi=(346, 260)).tobytes(), UO.RECORD).copy()
    i = np.arange(n)
    near_edge = np.abs(((i + BLOCK // 2) % BLOCK) - BLOCK // 2) <= 20     # 20 events either side of every multiple of 4096
    near_chunk = np.abs(((i + 512) % 1024) - 512) <= 3                     # ... and a few around the staging chunks of 1024
    rec["x"][~(near_edge | near_chunk)] = np.nan
    rec = np.frombuffer(rec.tobytes(), np.uint8)
    cam, ocam = cams(RADIAL_INTR, capi.CAMERA_RADIAL)
    tot = check_events(ctx, cam, ocam, capi.undistort_options(), rec)
    assert tot["n_kept"] == int((near_edge | near_chunk).sum()) and tot["n_kept"] > 4 * 41
    check_events(ctx, cam, ocam, pixel_options(), rec)


def test_exact_halves(ctx):
    """k = 0, fx = fy = 2, cx = cy = 0, the ideal camera (1, 1, 0, 0), no offset: u' = u / 2 exactly"""
    from eventcalib_amd import capi
    cam, ocam = cams([2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], capi.CAMERA_RADIAL, out_k=[1.0, 1.0, 0.0, 0.0])
    opt = capi.undistort_options(mode="pixel", out_width=8, out_height=8, off_x=0.0, off_y=0.0)
    u = np.array([1.0, 3.0, -1.0, 5.0, 0.0, 15.0, 16.0, 0.99999999999999989])
    rec = records(np.arange(u.size) + 1.0, u, np.full(u.size, 3.0), [1, 0, 1, 7, 0, 1, 0, 1])
    out, tot = ctx.undistort_events(cam, rec, opt)
    kept = np.frombuffer(out.cpu().numpy().tobytes(), UO.RECORD)
    # 0.5 -> 1, 1.5 -> 2, -0.5 -> -1: outside, 2.5 -> 3, 0 -> 0, 7.5 -> 8: outside, 8 -> outside, 0.49999999999999994 -> 0
    assert list(kept["x"]) == [1.0, 2.0, 3.0, 0.0, 0.0] and list(kept["y"]) == [2.0] * 5
    assert list(kept["t"]) == [1.0, 2.0, 4.0, 5.0, 8.0] and list(kept["p"]) == [1, 0, 7, 0, 1]
    assert (int(tot["n_events"]), int(tot["n_invalid"]), int(tot["n_outside"]), int(tot["n_kept"])) == (8, 0, 3, 5)
    check_events(ctx, cam, ocam, opt, rec)


def test_fisheye_on_the_reference_canvas(ctx):
    """346 x 260, fx = fy = 180, principal point (175.5, 127.5), k = (-0.02, 0.003, 0, 0, 0), 20 000 pixels of default_rng(20261020).
    Events whose oracle value lies within 1e-6 of a rounding half (a canvas edge is one) are left out of the input, 1 % at most
    (none on the CPU that wrote this test; 81 % land inside the canvas; the largest th is 1.19)."""
    from eventcalib_amd import capi
    rng = np.random.default_rng(20261020)
    n = 20000
    x = rng.integers(0, 346, n).astype(np.float64)
    y = rng.integers(0, 260, n).astype(np.float64)
    cam, ocam = cams(FISHEYE_INTR, capi.CAMERA_FISHEYE)
    opt = pixel_options()
    uv, flag = UO.points(ocam, np.stack([x, y], axis=1))
    assert flag.sum() == 0
    a = uv + np.array([opt.off_x, opt.off_y])
    sure = (np.abs(np.abs(a - UO.round_half_away(a)) - 0.5) > 1e-6).all(axis=1)
    print("fisheye PIXEL case: %d of %d events left out" % (n - int(sure.sum()), n))
    assert sure.sum() >= 0.99 * n
    rec = records(5.0 + np.arange(n) * 1e-6, x, y, rng.choice([0, 1, 7], n)).reshape(-1, 25)[sure].ravel()
    tot = check_events(ctx, cam, ocam, opt, rec)
    print("fisheye PIXEL case: %.1f %% inside the canvas" % (100.0 * tot["n_kept"] / tot["n_events"]))
    assert 0.7 * n < tot["n_kept"] < 0.9 * n and tot["n_invalid"] == 0
    check_events(ctx, cam, ocam, capi.undistort_options(), rec, exact=False)


def test_unaligned_input_and_an_output_of_exactly_the_kept_size(ctx):
    import torch
    from eventcalib_amd import capi
    rng = np.random.default_rng(12)
    n = 2 * BLOCK + 1
    rec = random_records(rng, n, lo=(-300, -300), hi=(650, 560), nan_every=13)
    cam, ocam = cams(RADIAL_INTR, capi.CAMERA_RADIAL)
    st = torch.cuda.current_stream().cuda_stream
    for opt in (capi.undistort_options(), pixel_options()):
        want, want_tot = UO.events(ocam, opt.as_dict(), rec)
        assert 0 < want.size < rec.size
        for shift in (1, 7, 15):
            # one allocation: the output in front — the kept records, then guard bytes —, the events at its end, both unaligned
            off_e = (shift + n * 25 + 15) // 16 * 16 + shift
            arena = torch.full((off_e + n * 25,), 0xEE, dtype=torch.uint8, device="cuda")
            arena[off_e:] = torch.from_numpy(rec.copy()).cuda()
            view, out = arena[off_e:], arena[shift:]
            assert view.data_ptr() % 16 == shift == out.data_ptr() % 16
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            tot = torch.zeros(4, dtype=torch.int64, device="cuda")
            ctx.undistort_events_dev(cam, opt, view.data_ptr(), n, out.data_ptr(), cnt.data_ptr(), tot.data_ptr(), st)
            torch.cuda.synchronize()
            assert int(cnt.item()) == want.size // 25 == int(tot[3].item())
            assert [int(v) for v in tot.cpu()] == [want_tot[k] for k in ("n_events", "n_invalid", "n_outside", "n_kept")]
            assert out[: want.size].cpu().numpy().tobytes() == want.tobytes()
            assert (arena[:shift] == 0xEE).all() and (arena[shift + want.size: off_e] == 0xEE).all()   # nothing behind the kept records
            assert torch.equal(view.cpu(), torch.from_numpy(rec.copy()))
    # a null options pointer is SUBPIXEL; null totals are allowed
    ev = torch.from_numpy(rec.copy()).cuda()
    out = torch.empty(n * 25, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.undistort_events_dev(cam, None, ev.data_ptr(), n, out.data_ptr(), cnt.data_ptr(), None, st)
    torch.cuda.synchronize()
    want, _ = UO.events(ocam, capi.undistort_options().as_dict(), rec)
    assert out[: int(cnt.item()) * 25].cpu().numpy().tobytes() == want.tobytes()


def test_stream_call_gives_the_dev_result(ctx):
    from eventcalib_amd import capi
    rng = np.random.default_rng(13)
    rec = random_records(rng, 3 * BLOCK + 5, lo=(-300, -300), hi=(650, 560), nan_every=29)
    cam, ocam = cams(RADIAL_INTR, capi.CAMERA_RADIAL)
    for opt in (capi.undistort_options(), pixel_options()):
        a, ta = ctx.undistort_events(cam, rec, opt)
        b, tb = ctx.undistort_stream(cam, rec, opt)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and tb == {k: int(ta[k]) for k in ta.dtype.names}
        assert 0 < tb["n_kept"] < tb["n_events"]
    out, tot = ctx.undistort_stream(cam, np.zeros(0, np.uint8))
    assert out.numel() == 0 and tot == dict(n_events=0, n_invalid=0, n_outside=0, n_kept=0)


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def frame_stream(rng, W, H, n_per_window):
    """Three windows: [0, 0.3] both polarities, [0.4, 0.5] empty, [0.6, 0.9] positive events only; constructed events in the first:
    a pixel with both polarities (the slicer erases it), the same pixel twice with one polarity."""
    t, x, y, p = [], [], [], []
    for lo, hi, pols in ((0.0, 0.3, (0, 1)), (0.6, 0.9, (1,))):
        n = n_per_window
        t.append(np.sort(rng.uniform(lo + 0.01, hi - 0.01, n)))
        x.append(rng.integers(0, W, n))
        y.append(rng.integers(0, H, n))
        p.append(rng.choice(pols, n))
    t, x, y, p = (np.concatenate(v).astype(np.float64) for v in (t, x, y, p))
    x[:4], y[:4], p[:4] = [W // 2, W // 2, 1, 1], [H // 2, H // 2, 1, 1], [1, 0, 1, 1]
    return records(t, x, y, p), np.array([0.0, 0.4, 0.6]), np.array([0.3, 0.5, 0.9])


def slicer_oracle(rec, t0, t1):
    """EventFrame's constructor: per window the unique positive and negative pixels, minus those present in both"""
    r = np.frombuffer(rec.tobytes(), UO.RECORD)
    out = []
    for a, b in zip(t0, t1):
        w = r[(r["t"] >= a) & (r["t"] <= b)]
        pos = {(float(e["x"]), float(e["y"])) for e in w if e["p"] != 0}
        neg = {(float(e["x"]), float(e["y"])) for e in w if e["p"] == 0}
        both = pos & neg
        out.append((np.array(sorted(pos - both)).reshape(-1, 2), np.array(sorted(neg - both)).reshape(-1, 2), len(both)))
    return out


FRAME_CASES = {
    # sensor, intrinsics (k1 strong enough for invalid corners), the ideal camera (half the focal length: neighbours round together;
    # a principal point left of the canvas: points outside), events per window
    "346x260": ((346, 260), [250.0, 250.0, 173.0, 130.0, -3.0, 0.0, 0.0, 0.0, 0.0], [125.0, 125.0, -40.0, 130.0], 3000),
    "640x480": ((640, 480), [400.0, 400.0, 320.0, 240.0, -2.5, 0.0, 0.0, 0.0, 0.0], [200.0, 200.0, -80.0, 240.0], 3000),
    "5x3": ((5, 3), [4.0, 4.0, 2.0, 1.0, -5.0, 0.0, 0.0, 0.0, 0.0], [2.0, 2.0, -0.8, 1.0], 12),
}


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("case", sorted(FRAME_CASES))
def test_frames_against_the_numpy_rule(ctx, case, S):
    import torch
    from eventcalib_amd import capi
    from eventcalib_amd.pipeline import DetectPipeline
    (W, H), intr, out_k, n_per = FRAME_CASES[case]
    rng = np.random.default_rng(W + S)
    rec, t0, t1 = frame_stream(rng, W, H, n_per)
    t0, t1 = t0[:S], t1[:S]
    cam, ocam = cams(intr, capi.CAMERA_RADIAL, out_k=out_k)
    opt = pixel_options(W, H)
    cw, ch = UO.reference_canvas(W, H)[:2]
    assert (opt.out_width, opt.out_height) == (cw, ch)
    # the numpy rule on the numpy slicer
    want_rgb = np.zeros((S, ch, cw, 3), np.uint8)
    want_tot = []
    windows = slicer_oracle(rec, t0, t1)
    for s, (pos, neg, n_both) in enumerate(windows):
        want_rgb[s], tot = UO.frame(ocam, opt.as_dict(), pos, neg)
        want_tot.append(tot)
    pos, neg, n_both = windows[0]
    assert n_both >= 1 and want_tot[0][2] > 0 and (want_tot[0][3] > 0 or case == "5x3")   # an erased pixel, invalid points, points outside
    red, green = (want_rgb[0] == (255, 0, 0)).all(axis=2).sum(), (want_rgb[0] == (0, 255, 0)).all(axis=2).sum()
    assert 0 < green < want_tot[0][1] or case == "5x3"                             # negatives that round together
    assert 0 < red < want_tot[0][0] or case == "5x3"                                             # positives that round together, or under a green
    pxy, pwhat = UO.classify(ocam, opt.as_dict(), pos)
    nxy, nwhat = UO.classify(ocam, opt.as_dict(), neg)
    on_pos = {tuple(v) for v in pxy[pwhat == 0]}
    assert on_pos & {tuple(v) for v in nxy[nwhat == 0]} or case == "5x3"         # a positive and a negative on one pixel: green
    if S == 3:
        assert want_tot[1] == (0, 0, 0, 0) and not want_rgb[1].any()                # the empty window
        assert want_tot[2][1] == 0 and want_tot[2][0] > 0 and not (want_rgb[2][:, :, 1]).any()   # one polarity only
    # staged: window bounds and the slicer (packed and doubles), then the frames
    ev = torch.from_numpy(rec.copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    got = {}
    for packed in (True, False):
        pipe = DetectPipeline(ctx, packed=packed, want_event_point=False)
        pipe.set_windows(t0, t1)
        pipe.run(ev, slice_only=True)
        assert not pipe.overflowed()
        if packed:
            fmt = pipe.seg_fmt[: 2 * S].cpu().numpy()
            print("%s, S = %d: segment formats %s" % (case, S, fmt.tolist()))
        rgb = torch.full((S * ch * cw * 3 + 64,), 0x77, dtype=torch.uint8, device="cuda")
        tot = torch.full((S + 1, 4), -1, dtype=torch.int32, device="cuda")
        ctx.undistorted_frames_dev(cam, opt, pipe._xy.data_ptr(), pipe._pk() if packed else None, pipe.seg_off.data_ptr(), pipe.seg_cnt.data_ptr(),
                                   S, rgb.data_ptr(), tot.data_ptr(), st)
        torch.cuda.synchronize()
        assert (rgb[S * ch * cw * 3:] == 0x77).all() and (tot[S] == -1).all()
        got[packed] = (rgb[: S * ch * cw * 3].cpu().numpy().reshape(S, ch, cw, 3), [tuple(int(v) for v in row) for row in tot[:S].cpu().numpy()])
        assert got[packed][1] == want_tot
        assert (got[packed][0] == want_rgb).all()
        # an unaligned picture, no totals
        ctx.undistorted_frames_dev(cam, opt, pipe._xy.data_ptr(), pipe._pk() if packed else None, pipe.seg_off.data_ptr(), pipe.seg_cnt.data_ptr(),
                                   S, rgb.data_ptr() + 1, None, st)
        torch.cuda.synchronize()
        assert (rgb[1: 1 + S * ch * cw * 3].cpu().numpy().reshape(S, ch, cw, 3) == want_rgb).all() and int(rgb[0]) == want_rgb.ravel()[0]
    assert (got[True][0] == got[False][0]).all()
    # the composite call
    rgb, tot = ctx.undistorted_frames(cam, rec, t0, t1, opt)
    assert (rgb == want_rgb).all() and [tuple(int(v) for v in row) for row in tot] == want_tot


def test_refusals(ctx):
    import torch
    from eventcalib_amd import capi
    rec = torch.zeros(50, dtype=torch.uint8, device="cuda")
    out = torch.zeros(50, dtype=torch.uint8, device="cuda")
    uv = torch.zeros(4, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    good = capi.undistort_camera(RADIAL_INTR)
    calls = lambda c, o: (lambda: ctx.undistort_points_dev(c, rec.data_ptr(), 2, uv.data_ptr(), out.data_ptr()),   # noqa: E731
                          lambda: ctx.undistort_events_dev(c, o, rec.data_ptr(), 2, out.data_ptr(), cnt.data_ptr()),
                          lambda: ctx.undistort_stream(c, np.zeros(50, np.uint8), o),
                          lambda: ctx.undistorted_frames(c, np.zeros(50, np.uint8), [0.0], [1.0], pixel_options() if o.mode == 0 else o))
    bad_cameras = []
    for idx, word in ((0, "fx "), (1, "fy "), (4, "k1"), (8, "k5")):
        c = capi.undistort_camera(RADIAL_INTR)
        c.intr[idx] = float("nan")
        bad_cameras.append((c, word))
    c = capi.undistort_camera(RADIAL_INTR, out_k=[0.0, 1.0, 0.0, 0.0])
    bad_cameras.append((c, "fx'"))
    bad_cameras.append((capi.undistort_camera(RADIAL_INTR, reserved=1), "reserved"))
    bad_cameras.append((capi.undistort_camera(RADIAL_INTR, model=5), "model"))
    for c, word in bad_cameras:
        for call in calls(c, capi.undistort_options()):
            with pytest.raises(capi.EcalError) as e:
                call()
            assert e.value.status == -1 and word in str(e.value), (word, str(e.value))
    for change, word in ((dict(mode=2), "mode"), (dict(out_width=0), "out_width"), (dict(out_height=8193), "out_height"), (dict(reserved=1), "reserved"),
                         (dict(off_x=float("nan")), "off_x")):
        o = pixel_options(**change)
        for call in calls(good, o)[1:]:
            with pytest.raises(capi.EcalError) as e:
                call()
            assert e.value.status == -1 and word in str(e.value), (change, str(e.value))
    with pytest.raises(capi.EcalError) as e:   # the frames want PIXEL
        ctx.undistorted_frames(good, np.zeros(50, np.uint8), [0.0], [1.0], capi.undistort_options())
    assert e.value.status == -1 and "mode" in str(e.value)
    for call in (lambda: ctx.undistort_points_dev(good, rec.data_ptr(), 1 << 32, uv.data_ptr(), out.data_ptr()),
                 lambda: ctx.undistort_events_dev(good, None, rec.data_ptr(), 1 << 32, out.data_ptr(), cnt.data_ptr())):
        with pytest.raises(capi.EcalError) as e:
            call()
        assert e.value.status == -6
    for overlapping in (rec.data_ptr(), rec.data_ptr() + 25, rec.data_ptr() + 49):
        with pytest.raises(capi.EcalError) as e:
            ctx.undistort_events_dev(good, None, rec.data_ptr(), 2, overlapping, cnt.data_ptr())
        assert e.value.status == -1 and "overlaps" in str(e.value)
    torch.cuda.synchronize()
