"""GPU: the detection chain (slice -> pixel DBSCAN -> extraction -> grid -> keyframe search -> calibrate_stream) on sensors other
than 346 x 260: the synthetic scene scaled to 640 x 480 and 1280 x 720 (synth_sensor.sensor), every array of every window against
the CPU oracle with the sensor's own circle radius threshold, bit for bit, and the tiers the windows take stated by assertions:

  * slicer: a window of <= 2047 events is a hash pass's on both sensors (x <= 2047); one of 2048 .. 4095 events is the second
    hash pass's on 640 x 480 (x <= 1023) and the general tiers' on 1280 x 720; longer ones are the general tiers' on both;
  * pixel DBSCAN: the board fills the image and the noise the whole sensor, so every segment's box is the sensor's — 488 rows on
    640 x 480, 728 on 1280 x 720, beyond the bitmap's 472: every segment is listed by the first pass, left by the second and
    labelled by the general tiers (Context.debug_px_todo_counts);
  * the driver: calibrate_stream(width=, height=) derives the radius threshold of both its detection passes from the sensor's
    size; with the 346 x 260 value the hover streams end in "no keyframe found" and the orbit stream keeps 13 keyframes of 130."""
import numpy as np
import pytest

import oracle_lib as O
import synth_sensor as SN
import synth_stream as SS

pytestmark = pytest.mark.gpu
THR_346 = 15.511363636363637
S_EACH = 20
# sensor -> event rate, the two window lengths of the comparison (S_EACH tiled windows each) and a short length whose windows
# hold <= 2047 events (the first hash pass's; too sparse for 36 circles on these sensors: compared, not counted below)
SCENES = {(640, 480): (4.0e6, (0.75e-3, 1.5e-3), 0.5e-3), (1280, 720): (6.0e6, (0.5e-3, 1.5e-3), 0.33e-3)}


def _threshold(W, H):
    return O.circle_radius_threshold(float(W), float(H), 9, 4, 1, 5.5, 1.75)


def _admitted(pts, cap, cmask, rd=4):
    """px_segment's admission (dbscan_pixel.hpp) of a segment of integer pixels, as far as size and box decide it."""
    if len(pts) == 0:
        return True
    W, H = int(np.ptp(pts[:, 0])) + 1 + 2 * rd, int(np.ptp(pts[:, 1])) + 1 + 2 * rd
    rw = (W + 31) // 32
    return len(pts) <= cap and H <= 472 and H * rw <= 3232 and W <= cmask and H <= cmask and H * ((rw + 3) // 4) <= 1032


@pytest.fixture(scope="module", params=sorted(SCENES), ids=lambda p: "%dx%d" % p)
def scene(request):
    """The stream, its windows and the oracle's results (computed once), with a context and a pipeline."""
    import torch
    import eventcalib_amd
    from eventcalib_amd.pipeline import DetectPipeline
    W, H = request.param
    rate, lengths, short = SCENES[request.param]
    n = int(round(rate * max(lengths) * S_EACH))
    with SN.sensor(W, H) as s:
        buf = SS.make_stream(n, rate=rate, device="cpu", seed=31)
    t0, t1 = [], []
    for ln in lengths + (short,):
        a, b = SS.tiled_windows(5.0, 5.0 + (n - 1) / rate, ln)
        t0.append(a[:S_EACH])
        t1.append(b[:S_EACH])
    t0, t1 = np.concatenate(t0), np.concatenate(t1)
    rec = buf.numpy()
    thr = _threshold(W, H)
    bounds = [O.window_bounds(rec, a, b) for a, b in zip(t0, t1)]
    wb = np.concatenate([[0], np.cumsum([hi - lo for lo, hi in bounds])]).astype(np.uint64)
    ref = O.detect_windows_full(rec, t0, t1, wb, int(wb[-1]), 4.0, 2, 5, 36, thr)
    ctx = eventcalib_amd.Context(0)
    yield dict(W=W, H=H, s=s, thr=thr, rec=rec, ev=buf.cuda(), t0=t0, t1=t1, wb=wb, ref=ref, ctx=ctx, pipe=DetectPipeline(ctx), torch=torch)
    ctx.close()


def test_the_scaled_scenes_reach_the_grid_stage(scene):
    """Condition on the inputs, from the oracle alone: of the 2 x 20 windows of the comparison >= 90 % reach the pairing stage and
    >= 50 % have >= 36 candidates with the sensor's own threshold — and with the 346 x 260 value next to none of the 1.5 ms windows
    has (a circle of a shorter window is a thinner arc, and some pass the smaller radius test)."""
    info = scene["ref"]["win_info"][:2 * S_EACH]
    assert int((info[:, 3] == 0).sum()) >= 0.9 * len(info)
    assert int(((info[:, 3] == 0) & (info[:, 0] >= 36)).sum()) >= 0.5 * len(info)
    sc = scene
    low = O.detect_windows_full(sc["rec"], sc["t0"], sc["t1"], sc["wb"], int(sc["wb"][-1]), 4.0, 2, 5, 36, THR_346)["win_info"][S_EACH:2 * S_EACH]
    assert int(((low[:, 3] == 0) & (low[:, 0] >= 36)).sum()) <= 1


def _prime_semi(sc):
    """Leaves the stages' records of their last call as a 346 x 260 stream of 2 Mev/s leaves them — first lists filled, second lists
    empty —, so that the next call under "auto" takes the two pixel passes and one tail launch ("semi", ecal_ctx.hpp)."""
    from eventcalib_amd.pipeline import DetectPipeline
    buf = SS.make_stream(30000, rate=2.0e6, device="cpu", seed=5)
    t0, t1 = SS.tiled_windows(5.0, 5.0 + (30000 - 1) / 2.0e6)
    p = DetectPipeline(sc["ctx"])
    p.set_windows(t0, t1)
    for _ in range(2):
        p.run(buf.cuda())
        sc["torch"].cuda.synchronize()
    # what the next call of the two stages that plan their tails will do, by what these calls left
    assert sc["ctx"].debug_tail_plans() == {"slice": "semi", "dbscan": "semi"}


def _tiers(sc, pipe, listed, lean):
    """The tiers the windows took, by their sizes and the sensor's width, against seg_fmt and the pixel passes' counters."""
    S = len(sc["t0"])
    sizes = np.diff(sc["wb"].astype(np.int64))
    xmax = sc["W"] - 1
    hash_pass = (sizes <= 2047) | ((sizes <= 4095) & (xmax <= 1023)) | ((sizes <= 5119) & (xmax <= 511))
    if lean:
        hash_pass = sizes <= 2047           # one general launch behind the first pass: no second or third hash pass
    assert hash_pass.any() and (~hash_pass).any() and int(sc["ref"]["xy"][:, 0].max()) == xmax
    fmt = pipe.seg_fmt[:2 * S].cpu().numpy() != 0
    assert np.array_equal(fmt[0::2], hash_pass) and np.array_equal(fmt[1::2], hash_pass)
    # pixel DBSCAN: what size and box leave to the lists (a segment the kernel gives up for another reason would add to them)
    f, cnt = sc["ref"], sc["ref"]["seg_cnt"].astype(np.int64)
    off = np.repeat(sc["wb"][:-1].astype(np.int64), 2)
    off[1::2] += cnt[0::2]
    segs = [f["xy"][o:o + c] for o, c in zip(off, cnt)]
    first = sum(not _admitted(p, 768, 2047) for p in segs)
    second = sum(not _admitted(p, 768, 2047) and not _admitted(p, 2048, 1023) for p in segs)
    assert first == second == 2 * S and int(cnt.min()) > 0 and int(cnt.max()) > 768      # every segment's box is the sensor's
    assert listed == ((first, None) if lean else (first, second))


@pytest.mark.parametrize("mode", ["tiered", "lean", "semi"])
def test_every_window_equals_the_oracle(scene, mode):
    import full_compare as FC
    import test_gpu_fused as TF
    sc = scene
    ctx, pipe, torch, t0, t1 = sc["ctx"], sc["pipe"], sc["torch"], sc["t0"], sc["t1"]
    S = len(t0)
    try:
        if mode == "semi":
            ctx.set_tail_mode("auto")
            _prime_semi(sc)
        else:
            ctx.set_tail_mode(mode)
        pipe.set_windows(t0, t1)
        pipe.set_detect_params(5, 36, sc["thr"])
        pipe._ensure(S, int(sc["wb"][-1]))
        TF._poison(pipe)
        pipe.run(sc["ev"], slots=int(sc["wb"][-1]))
        torch.cuda.synchronize()
        assert not pipe.overflowed()
        listed = ctx.debug_px_todo_counts(torch.cuda.current_stream().cuda_stream)
        st = FC.compare_all_windows(pipe, sc["rec"], t0, t1, torch, det=(5, 36, sc["thr"]), oracle=sc["ref"])
        assert st["windows"] == S and st["paired"] >= 0.9 * 2 * S_EACH
        _tiers(sc, pipe, listed, mode == "lean")
    finally:
        ctx.set_tail_mode("auto")


def test_fused_call_equals_the_stage_calls(scene):
    """ecal_detect_fused_dev (the three stage calls on doubles, the smaller-pid tie rule) against the packed stage calls with that
    tie rule, which differ from the run pinned to the oracle above in nothing but the rule: every defined slot, bit for bit."""
    import test_gpu_fused as TF
    sc = scene
    ctx, pipe, torch, t0, t1 = sc["ctx"], sc["pipe"], sc["torch"], sc["t0"], sc["t1"]
    S, slots = len(t0), int(sc["wb"][-1])
    pipe.set_windows(t0, t1)
    pipe.set_detect_params(5, 36, sc["thr"])
    snaps = []
    for fused in (False, True):
        pipe._ensure(S, slots)
        TF._poison(pipe)
        pipe.run(sc["ev"], slots=slots, fused=fused, exact_ties=False)
        torch.cuda.synchronize()
        assert not pipe.overflowed()
        snaps.append(TF._snapshot(pipe, S, torch))
    a, b = snaps
    assert int((a["win_info"][:2 * S_EACH, 3] == 0).sum()) >= 0.9 * 2 * S_EACH
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape, k
        assert torch.equal(x.view(torch.int64) if x.dtype.is_floating_point else x, y.view(torch.int64) if y.dtype.is_floating_point else y), k
    assert np.array_equal(a["labels"].cpu().numpy(), sc["ref"]["labels"][sc["ref"]["def_pts"] != 0])


# window length and count of the grid stage's test (1.5 ms windows rarely hold exactly 36 candidates on these sensors)
GRID_WINDOWS = {(640, 480): (2.5e-3, 60), (1280, 720): (4.0e-3, 100)}


def _walk_triples(rows=9, cols=4):
    """(a, b, c): model points that follow each other along a diagonal of the pattern's centred-square lattice — the walk's steps
    (ecal_grid.hip): standing on b, reached from a, it predicts c at b + (b - a).  Grid index i * cols + j is ((2j + i % 2) s, i s)."""
    at = {(2 * j + i % 2, i): i * cols + j for i in range(rows) for j in range(cols)}
    out = []
    for (x, y), a in at.items():
        for dx, dy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            b, c = at.get((x + dx, y + dy)), at.get((x + 2 * dx, y + 2 * dy))
            if b is not None and c is not None:
                out.append((a, b, c))
    return np.array(out)


def test_grid_order_against_the_generating_camera(scene):
    """The grid stage on GRID_WINDOWS (60 windows of 2.5 ms at 640 x 480, 100 of 4 ms at 1280 x 720), on those where the oracle
    has exactly the 36 candidates and every circle has its own within 14 s px of the generating camera's centre
    (test_gpu_oracle_chain.py::test_grid_order_against_ground_truth, the distance scaled with the sensor).

    The walk takes the nearest candidate within 20 px of its prediction as the hole (the reference's rule, a constant of OpenCV's
    finder in pixels: circlesgrid.cpp:528,812-840).  The midpoint circles of these scenes lie up to 19 px off their centres
    (14 px at 640 x 480), a prediction from two of them further.  Which windows are inside that tolerance is decided from the
    oracle's candidates in the truth's order alone, whatever the product does with them: for every three circles in a row along
    a lattice diagonal the prediction b + (b - a) lies within 20 px of c's candidate (_walk_triples: 84 predictions a window).
    Measured: 21 of the 54 windows at 640 x 480 and 8 of the 21 at 1280 x 720 are inside, and the product finds and orders as the
    truth 21 of 21 and 8 of 8 of them; of ALL the windows 53 of 54 and 21 of 21 (later starts and the homography pass recover
    most windows with a prediction beyond 20 px; on 60 windows of 2.5 ms at 1280 x 720 it was 16 of 19); with the tolerance scaled
    like the scene (ECAL_GRID_TOL_PX = 20 s) 54 of 54 and 21 of 21.  The reference's constant is kept.
    Asserted: the project's 99 % bar over the windows inside the tolerance, with 20 px; the same bar over all of them with
    20 s px; a window found is never ordered otherwise than the truth.  The share of ALL windows with 20 px is a measurement,
    printed here and written into design/14_other_sensors.md: no bar of the project's applies to windows that the reference's own
    rule does not reach."""
    import os
    import eventcalib_amd
    import oracle_chain as OC
    from eventcalib_amd.pipeline import DetectPipeline
    sc = scene
    torch = sc["torch"]
    W, H, s = sc["W"], sc["H"], sc["s"]
    rate, (length, S) = SCENES[(W, H)][0], GRID_WINDOWS[(W, H)]
    n = int(round(rate * length * S))
    with SN.sensor(W, H):
        buf = SS.make_stream(n, rate=rate, device="cpu", seed=32)
        t0, t1 = SS.tiled_windows(5.0, 5.0 + (n - 1) / rate, length)
        gt = SN.project_centres((t0 + t1) / 2)
    assert len(t0) == S
    rec = buf.numpy()
    bounds = [O.window_bounds(rec, a, b) for a, b in zip(t0, t1)]
    wb = np.concatenate([[0], np.cumsum([hi - lo for lo, hi in bounds])]).astype(np.uint64)
    ref = O.detect_windows_full(rec, t0, t1, wb, int(wb[-1]), 4.0, 2, 5, 36, sc["thr"])
    picks, inside, tri = {}, set(), _walk_triples()
    assert len(tri) == 84
    for k in range(S):
        if ref["win_info"][k, 3] == 0 and ref["win_info"][k, 0] == 36:
            pick = OC.grid_by_ground_truth(ref["cand_xyr"][int(wb[k]):int(wb[k]) + 36, :2], gt[k], OC.GT_TOL_PX * s)
            if pick is not None:
                picks[k] = pick
                p = ref["cand_xyr"][int(wb[k]):int(wb[k]) + 36, :2][pick]
                err = np.linalg.norm(p[tri[:, 2]] - (2 * p[tri[:, 1]] - p[tri[:, 0]]), axis=1)
                if err.max() <= 20.0:
                    inside.add(k)
    ev = buf.cuda()
    right = {}
    for tol in (20.0, 20.0 * s):
        os.environ["ECAL_GRID_TOL_PX"] = repr(tol)       # (read when a context is made)
        try:
            ctx = eventcalib_amd.Context(0)
        finally:
            del os.environ["ECAL_GRID_TOL_PX"]
        try:
            pipe = DetectPipeline(ctx)
            pipe.set_windows(t0, t1)
            pipe.set_detect_params(5, 36, sc["thr"])
            pipe.run(ev)
            order, found = pipe.order_grid(9, 4)
            torch.cuda.synchronize()
            order, found = order.cpu().numpy(), found.cpu().numpy()
            assert np.array_equal(pipe.win_info[:S].cpu().numpy().astype(np.uint32), ref["win_info"])
            off, xyr = pipe.seg_off[:2 * S].cpu().numpy(), pipe.cand_xyr.cpu().numpy()
            for k, pick in picks.items():
                assert np.array_equal(xyr[off[2 * k]:off[2 * k] + 36], ref["cand_xyr"][int(wb[k]):int(wb[k]) + 36])
                assert not found[k] or np.array_equal(order[k], pick), "window %d ordered otherwise than the truth (tolerance %.1f px)" % (k, tol)
            right[tol] = {k for k in picks if found[k]}
        finally:
            ctx.close()
    fixed, scaled = right[20.0], right[20.0 * s]
    clean = len(picks)
    print("\n[%dx%d] grid stage vs the generating camera, %d windows of exactly 36 candidates: %d as the truth with the reference's 20 px, "
          "%d with %.1f px; %d have every walk prediction within 20 px, %d of them as the truth" % (
              W, H, clean, len(fixed), len(scaled), 20.0 * s, len(inside), len(fixed & inside)))
    assert clean >= 10 and len(inside) >= 5
    assert len(fixed & inside) >= 0.99 * len(inside)
    assert len(scaled) >= 0.99 * clean


# ---- the keyframe search and the driver with the sensor's own threshold ----
# frame_event_num_threshold (the events a window may hold before it slides instead of growing) is scaled with the sensor by the
# caller: about 4000 s^2, s = the scale of synth_sensor
SEARCH = {(640, 480): (4.0e6, 16000), (1280, 720): (6.0e6, 30000)}


@pytest.fixture(scope="module", params=sorted(SEARCH), ids=lambda p: "%dx%d" % p)
def search(request):
    """0.2 s of the scaled hover stream on the device, and the cache of the oracle's window callback: capi.detect_pass on one
    window with the sensor's own threshold (those stages have their oracles above: what is checked here is the search)."""
    import torch
    import eventcalib_amd
    import eventcalib_amd.capi as capi
    W, H = request.param
    rate, fent = SEARCH[request.param]
    n = int(round(rate * 0.2))
    with SN.sensor(W, H):
        ev = SS.make_stream(n, rate=rate, device="cpu", seed=21).cuda()
    ctx = eventcalib_amd.Context(0)
    thr = ctx.circle_radius_threshold(W, H, 9, 4, True, 5.5, 1.75)
    assert thr == _threshold(W, H)
    cache = {}

    def detect(t0, t1):
        if (t0, t1) not in cache:
            packed = capi.detect_pass(ctx, ev.data_ptr(), n, np.array([t0]), np.array([t1]), 1 << 17, 4.0, 2, 5, 9, 4, thr)
            found = (int(packed[0, 0]) & 0xFF) == 0 and packed[0, 1] != 0
            cache[(t0, t1)] = (found, int(packed[0, 2]), packed[0, 3:].reshape(36, 3).copy() if found else None)
        return cache[(t0, t1)]
    yield dict(ctx=ctx, ev=ev, n=n, thr=thr, fent=fent, detect=detect, t_first=5.0, t_last=5.0 + (n - 1) / rate, torch=torch)
    ctx.close()


@pytest.mark.parametrize("pieces", [1, 6])
@pytest.mark.parametrize("gate", ["own_piece", "shared_map"])
def test_keyframe_search_with_the_sensor_s_threshold(search, gate, pieces):
    """detect_keyframes_device(radius_threshold = the sensor's) against oracle/policy_oracle.cpp in both gate modes: keyframes,
    windows, counts and features identical; and the search with the 346 x 260 value — what calibrate_stream ran before it
    carried the sensor's size — finds fewer keyframes on the same stream."""
    import eventcalib_amd.capi as capi
    from eventcalib_amd.adaptive import detect_keyframes_device
    se = search
    mode = {"own_piece": capi.GATE_OWN_PIECE, "shared_map": capi.GATE_SHARED_MAP}[gate]
    ref = O.policy_run(se["detect"], se["t_first"], se["t_last"], pieces, 5e-4, se["fent"], 9, 4, mode=mode)
    dev = detect_keyframes_device(se["ctx"], se["ev"], 5e-4, se["fent"], pieces, se["t_first"], se["t_last"], gate_mode=mode,
                                  radius_threshold=se["thr"])
    assert len(ref["time"]) >= 8
    assert dev["windows"] == ref["windows"]
    for k in ("time", "duration", "events_num", "features"):
        assert np.array_equal(dev[k], ref[k]), k
    low = detect_keyframes_device(se["ctx"], se["ev"], 5e-4, se["fent"], pieces, se["t_first"], se["t_last"], gate_mode=mode)
    print("\nkeyframes: %d with the sensor's threshold %.2f, %d with %.2f" % (len(dev["time"]), se["thr"], len(low["time"]), THR_346))
    assert len(low["time"]) < len(dev["time"])


ORBIT_EVENTS, ORBIT_RATE = 2_400_000, 4.0e6


@pytest.fixture(scope="module")
def orbit_640():
    import eventcalib_amd
    import eventcalib_amd.capi as capi
    from eventcalib_amd.adaptive import detect_keyframes_device
    from eventcalib_amd.calibrate import calibrate_stream
    W, H = 640, 480
    with SN.sensor(W, H, "orbit") as s:
        ev = SS.make_stream(ORBIT_EVENTS, rate=ORBIT_RATE, t_start=5.0, device="cuda", seed=21)
        truth = (SS.FX, SS.CX, SS.CY)
    t_last = 5.0 + (ORBIT_EVENTS - 1) / ORBIT_RATE
    with eventcalib_amd.Context(0) as ctx:
        out = calibrate_stream(ctx, ev, 5.0, t_last, frame_event_num_threshold=16000, width=float(W), height=float(H))
        low = detect_keyframes_device(ctx, ev, 5e-4, 16000, 30, 5.0, t_last, gate_mode=capi.GATE_SHARED_MAP)      # the search as it ran before: 346 x 260's threshold
    return out, truth, s, len(low["time"])


def test_calibrate_stream_on_a_640x480_sensor(orbit_640):
    """calibrate_stream(width=640, height=480) on the scaled orbit stream completes: keyframes, init calibration, rectify, splines
    and the solve; the refined focal length within 2e-3 relative of the generating camera's and the principal point within 0.3 s px
    of (CX - 0.5, CY - 0.5) (the bars of the 346 x 260 chain tests, the second as the same share of the sensor).  Measured: 130
    keyframes, fx 2.2e-4 relative, principal point 0.04 and 0.07 px off (bar 0.55).  The keyframe search with the 346 x 260
    threshold — what the driver ran before it carried the sensor's size — finds 13 keyframes in this stream instead of 130 (none
    at all in the hover streams above): short of the 100 this test asks for."""
    out, (fx_t, cx_t, cy_t), s, low = orbit_640
    fx, fy, cx, cy = out["intrinsics"][:4]
    print("\n[640x480 orbit] %d keyframes (%d with the 346x260 threshold); fx %.3f (truth %.3f, relative %.2e), cx %.3f cy %.3f (truth - 0.5: %.1f %.1f; "
          "errors %.3f %.3f px, bar %.3f)" % (out["keyframes"], low, fx, fx_t, abs(fx / fx_t - 1), cx, cy, cx_t - 0.5, cy_t - 0.5,
                                            abs(cx - (cx_t - 0.5)), abs(cy - (cy_t - 0.5)), 0.3 * s))
    assert out["keyframes"] >= 100 > low
    assert out["spline"]["final_cost"] < out["spline"]["initial_cost"]
    assert abs(fx / fx_t - 1) < 2e-3
    assert abs(cx - (cx_t - 0.5)) < 0.3 * s and abs(cy - (cy_t - 0.5)) < 0.3 * s
