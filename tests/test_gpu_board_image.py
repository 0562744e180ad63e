"""GPU: the board-frame event image (ecal_solver_board_image[_dev] / ecal_solver_board_points[_dev], include/ecal.h: every event
of a packed stream carried through the intrinsics and the spline pose at its own time stamp onto the board plane, binned into
an image per polarity and a ring profile per circle) against a numpy float64 reference, `_board_points`, built from
synth_solver.find_span / basis / quat_rotate / so3_spline_pose.

Tolerances.  TOL_X = 1e-9 board units caps the deviation of a board point: coordinates stay below ~100 units, ~200 operations
at 1.1e-16 relative error each and a ray / plane conditioning of ~4 at the generator's tilts make ~1e-11 the expected figure,
so the cap has a 100x margin (test_points_match_numpy prints the measured maximum).  Counts are integer atomics and must
be EXACT except where a reference point lies within TOL_X of a decision: an image bin edge (the image's border is one), |d| =
ring_range, a ring-histogram edge, or equal distance to two landmarks.  Such an event is "slack"; a count may differ from the
reference by the slack events attributed to it (an image pixel: those of its 3 x 3 neighbourhood), and the slack must stay below
0.1 % of the events for the test to say anything (with bin = radius / 8 and continuous random inputs the expectation is 0).
sum_d / sum_d2 follow the report's rule (tests/test_gpu_report.py) with TOL_X in the place of its residual tolerance:
1e-11 relative + n * TOL_X.

The image cases put 1 % of the pixels 10 000 px off the sensor with the pinhole camera (both rotation splines).  There the
fisheye model evaluates tan() of ~1e10 rad and the SIGN of the ray depends on the last bits of the argument — nothing a
tolerance-based reference can pin —, so the fisheye image cases run on the same stream WITHOUT the far pixels."""
import functools

import numpy as np
import pytest

import synth_solver as SV

pytestmark = pytest.mark.gpu

TOL_X = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    c = eventcalib_amd.Context(0)
    yield c
    c.close()


def _pack(t, xy, pol):
    rec = np.zeros((len(t), 25), np.uint8)
    rec[:, 0:8] = np.ascontiguousarray(t, np.float64).view(np.uint8).reshape(-1, 8)
    rec[:, 8:16] = np.ascontiguousarray(xy[:, 0], np.float64).view(np.uint8).reshape(-1, 8)
    rec[:, 16:24] = np.ascontiguousarray(xy[:, 1], np.float64).view(np.uint8).reshape(-1, 8)
    rec[:, 24] = pol
    return rec.ravel()


def _segments(prob):
    cp_off = np.asarray(prob["seg_cp_off"], np.int64)
    out = []
    for g in range(len(cp_off) - 1):
        ncp = int(cp_off[g + 1] - cp_off[g])
        k0 = int(cp_off[g] + 4 * g)
        out.append((prob["knots"][k0: k0 + ncp + 4], ncp, int(cp_off[g])))
    return out


def _board_points(prob, x, t, xy):
    """numpy float64 reference: (xw [n, 2], flag [n]: 0 ok, 1 outside every segment's time range, 2 behind), (0, 0) where flag != 0"""
    segs = _segments(prob)
    n_cp = int(prob["seg_cp_off"][-1])
    intr = x[:9]
    q_all, t_all = x[9: 9 + 4 * n_cp].reshape(n_cp, 4), x[9 + 4 * n_cp:].reshape(n_cp, 3)
    fisheye, so3 = bool(prob.get("fisheye", False)), bool(prob.get("use_so3", False))
    xw, flag = np.zeros((len(t), 2)), np.zeros(len(t), np.uint8)
    for i in range(len(t)):
        seg = None
        for kn, ncp, c0 in segs:          # (where two segments touch at one time, the earlier one: include/ecal.h)
            if kn[3] <= t[i] <= kn[ncp]:
                seg = (kn, ncp, c0)
                break
        if seg is None:
            flag[i] = 1
            continue
        kn, ncp, c0 = seg
        sp = SV.find_span(kn, ncp, t[i])
        b = SV.basis(kn, sp, t[i])
        q4, t4 = q_all[c0 + sp - 3: c0 + sp + 1], t_all[c0 + sp - 3: c0 + sp + 1]
        if so3:
            qn = SV.so3_spline_pose(q4, b)
        else:
            qv = b @ q4
            qn = qv / np.linalg.norm(qv)
        T = b @ t4
        px, py = (xy[i, 0] - intr[2]) / intr[0], (xy[i, 1] - intr[3]) / intr[1]
        r2 = px * px + py * py
        c = 1 + intr[4] * r2 + intr[5] * r2 ** 2 + intr[6] * r2 ** 3 + intr[7] * r2 ** 4 + intr[8] * r2 ** 5
        if fisheye and r2 > 1e-16:
            r = np.sqrt(r2)
            c = np.tan(r * c) / r
        Y = SV.quat_rotate(qn, np.array([px * c, py * c, 1.0]))
        with np.errstate(divide="ignore", invalid="ignore"):
            s = -T[2] / Y[2]
        if not (np.isfinite(s) and s > 0):
            flag[i] = 2
            continue
        xw[i] = T[:2] + s * Y[:2]
    return xw, flag


def _block_modes(prob, t):
    """what the kernel's workgroups do with their blocks of BOARD_IMAGE_BLOCK events (include/ecal.h): 'none' (no segment between
    the block's first and last time), 'staged' (one segment, at most BOARD_IMAGE_CP_LDS control points) or 'global'"""
    from eventcalib_amd import capi
    segs = _segments(prob)
    modes = []
    for a in range(0, len(t), capi.BOARD_IMAGE_BLOCK):
        t0, t1 = t[a], t[min(a + capi.BOARD_IMAGE_BLOCK, len(t)) - 1]
        hit = [g for g, (kn, ncp, _) in enumerate(segs) if kn[ncp] >= t0 and kn[3] <= t1]
        if not hit:
            modes.append("none")
        elif len(hit) > 1:
            modes.append("global")
        else:
            kn, ncp, _ = segs[hit[0]]
            s0, s1 = SV.find_span(kn, ncp, min(max(t0, kn[3]), kn[ncp])), SV.find_span(kn, ncp, min(max(t1, kn[3]), kn[ncp]))
            modes.append("staged" if s1 - s0 + 4 <= capi.BOARD_IMAGE_CP_LDS else "global")
    return modes


def _box3(a):
    """sum over the 3 x 3 neighbourhood, per plane"""
    p = np.pad(a, ((0, 0), (1, 1), (1, 1)))
    H, W = a.shape[1:]
    return sum(p[:, 1 + dy: 1 + dy + H, 1 + dx: 1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def _reference_image(prob, xw, flag, pol, o, n_lm_used=None):
    """numpy floor / bincount / argmin on the reference points, and the slack attributed to every count"""
    n = len(flag)
    ok = flag == 0
    H, W, B = int(o.height), int(o.width), int(o.ring_bins)
    ref = {"n_events": n, "n_outside_time": int((flag == 1).sum()), "n_behind": int((flag == 2).sum())}
    X, P = xw[ok], pol[ok].astype(np.int64)
    gx, gy = (X[:, 0] - o.x0) / o.bin, (X[:, 1] - o.y0) / o.bin
    ix, iy = np.floor(gx), np.floor(gy)
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    ref["n_outside_image"] = int((~inside).sum())
    ref["n_image"] = np.bincount(P[inside], minlength=2)
    flat = (P[inside] * H + iy[inside].astype(np.int64)) * W + ix[inside].astype(np.int64)
    ref["image"] = np.bincount(flat, minlength=2 * H * W).reshape(2, H, W)
    # slack: within TOL_X of a bin edge (x or y), attributed to the reference pixel clipped into the image
    near = (np.abs(gx - np.round(gx)) * o.bin <= TOL_X) | (np.abs(gy - np.round(gy)) * o.bin <= TOL_X)
    near &= (ix >= -1) & (ix <= W) & (iy >= -1) & (iy <= H)
    cx, cy = np.clip(ix[near], 0, W - 1).astype(np.int64), np.clip(iy[near], 0, H - 1).astype(np.int64)
    ref["slack_image"] = np.bincount((P[near] * H + cy) * W + cx, minlength=2 * H * W).reshape(2, H, W) if H * W else np.zeros((2, H, W), np.int64)
    ref["slack_image_total"] = int(near.sum())
    slack_total = int(near.sum())
    if B:
        lms = prob["landmarks"][:, :2]
        L = len(lms)
        dist = np.sqrt(((X[:, None, :] - lms[None, :, :]) ** 2).sum(axis=2))          # [n_ok, L]
        order = np.argsort(dist, axis=1, kind="stable")                              # ties to the lower index
        near_lm = np.argmin(((X[:, None, :] - lms[None, :, :]) ** 2).sum(axis=2), axis=1)
        rows = np.arange(len(X))
        d = dist[rows, near_lm] - prob["circle_radius"]
        rr = o.ring_range
        in_ring = np.abs(d) < rr
        pos = (d + rr) * B / (2 * rr)
        hb = np.clip(np.floor(pos), 0, B - 1).astype(np.int64)
        ref["n_ring"] = int(in_ring.sum())
        ref["ring_hist"] = np.bincount(near_lm[in_ring] * B + hb[in_ring], minlength=L * B).reshape(L, B)
        key = near_lm[in_ring] * 2 + P[in_ring]
        ref["ring_n"] = np.bincount(key, minlength=2 * L).reshape(L, 2)
        ref["ring_sum_d"] = np.bincount(key, weights=d[in_ring], minlength=2 * L).reshape(L, 2)
        ref["ring_sum_abs"] = np.bincount(key, weights=np.abs(d[in_ring]), minlength=2 * L).reshape(L, 2)
        ref["ring_sum_d2"] = np.bincount(key, weights=d[in_ring] ** 2, minlength=2 * L).reshape(L, 2)
        # slack: |d| = ring_range, or two landmarks at equal distance -> per landmark (both of a tie); a histogram edge -> the two
        # bins beside it
        second = order[:, 1] if L > 1 else near_lm
        tie = (np.abs(dist[rows, second] - dist[rows, near_lm]) <= 2 * TOL_X) & (L > 1) & (np.minimum(np.abs(d), np.abs(dist[rows, second] - prob["circle_radius"])) < rr + TOL_X)
        at_range = np.abs(np.abs(d) - rr) <= TOL_X
        lm_slack = np.bincount(near_lm[tie | at_range], minlength=L) + np.bincount(second[tie], minlength=L)
        edge = in_ring & (np.abs(pos - np.round(pos)) * (2 * rr / B) <= TOL_X)
        e = np.round(pos[edge]).astype(np.int64)                                        # edge e borders bins e - 1 and e
        bin_slack = np.zeros((L, B + 2), np.int64)
        np.add.at(bin_slack, (near_lm[edge], np.clip(e, 0, B) + 1), 1)
        np.add.at(bin_slack, (near_lm[edge], np.clip(e - 1, -1, B - 1) + 1), 1)
        ref["slack_lm"] = lm_slack
        ref["slack_bin"] = bin_slack[:, 1: B + 1] + lm_slack[:, None]
        slack_total += int((tie | at_range | edge).sum())
    ref["slack_total"] = slack_total
    return ref


def _check_image(s, prob, x, t, xy, pol, **options):
    """one board image with everything on against the numpy reference; returns (result, reference)"""
    events = _pack(t, xy, pol)
    got = s.board_image(x, events, **options)
    o = got["options"]
    xw, flag = _board_points(prob, x, t, xy)
    ref = _reference_image(prob, xw, flag, pol, o)
    tot = got["totals"]
    n = len(t)
    print("events %d: outside time %d, behind %d, outside image %d, image %s, ring %d; slack %d" % (
        n, int(tot["n_outside_time"]), int(tot["n_behind"]), int(tot["n_outside_image"]), tot["n_image"].tolist(), int(tot["n_ring"]),
        ref["slack_total"]))
    assert 1000 * ref["slack_total"] <= n                      # (the test's own validity, see the module's docstring)
    assert int(tot["n_events"]) == n and int(tot["n_outside_time"]) == ref["n_outside_time"]
    assert int(tot["n_behind"]) == ref["n_behind"]             # (no slack is attributed to the depth's sign)
    assert abs(int(tot["n_outside_image"]) - ref["n_outside_image"]) <= ref["slack_image_total"]
    assert (np.abs(tot["n_image"].astype(np.int64) - ref["n_image"]) <= ref["slack_image_total"]).all()
    assert int(tot["n_outside_time"] + tot["n_behind"] + tot["n_outside_image"] + tot["n_image"].sum()) == n
    img = got["image"].astype(np.int64)
    assert img.shape == ref["image"].shape
    assert (np.abs(img - ref["image"]) <= _box3(ref["slack_image"])).all()
    assert (img.sum(axis=(1, 2)) == tot["n_image"].astype(np.int64)).all()
    if o.ring_bins:
        assert abs(int(tot["n_ring"]) - ref["n_ring"]) <= int(ref["slack_lm"].sum())
        assert (np.abs(got["ring_hist"].astype(np.int64) - ref["ring_hist"]) <= ref["slack_bin"]).all()
        st = got["ring_stats"]
        sl = ref["slack_lm"][:, None].astype(np.float64)
        nn = ref["ring_n"].astype(np.float64)
        assert (np.abs(st["n"].astype(np.int64) - ref["ring_n"]) <= sl).all()
        assert int(st["n"].sum()) == int(tot["n_ring"]) == int(got["ring_hist"].sum())
        rr = o.ring_range
        print("ring: max |d sum_d| %.3g, max |d sum_d2| %.3g" % (np.abs(st["sum_d"] - ref["ring_sum_d"]).max(initial=0.0),
                                                                np.abs(st["sum_d2"] - ref["ring_sum_d2"]).max(initial=0.0)))
        assert (np.abs(st["sum_d"] - ref["ring_sum_d"]) <= 1e-11 * ref["ring_sum_abs"] + nn * TOL_X + sl * rr).all()
        assert (np.abs(st["sum_d2"] - ref["ring_sum_d2"]) <= 1e-11 * ref["ring_sum_d2"] + 2 * TOL_X * ref["ring_sum_abs"] + sl * rr * rr).all()
        # the derived figures of the Python layer
        n_lm = st["n"].sum(axis=1).astype(np.float64)
        has = n_lm > 0
        mean = st["sum_d"].sum(axis=1)[has] / n_lm[has]
        assert np.array_equal(got["ring_n"], st["n"].sum(axis=1)) and np.allclose(got["ring_mean"][has], mean, rtol=0, atol=1e-15)
        var = np.maximum(st["sum_d2"].sum(axis=1)[has] / n_lm[has] - mean * mean, 0.0)
        assert np.allclose(got["ring_std"][has], np.sqrt(var), rtol=0, atol=1e-15) and np.isnan(got["ring_mean"][~has]).all()
    assert got["extent"] == (o.x0, o.x0 + o.width * o.bin, o.y0, o.y0 + o.height * o.bin)
    return got, ref, events


# ---- 1. points -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _points_problem(use_so3, fisheye):
    prob, x = SV.make_problem(5000, n_cp=8, seed=11 + 2 * use_so3 + fisheye, pixel_noise=0.5, use_so3=use_so3, fisheye=fisheye)
    y = SV.perturb(x, 8, np.random.default_rng(5), intr_rel=0.01, rot=0.005, trans=0.2)
    rng = np.random.default_rng(6)
    # 40 events before and 40 after the segment's time range, and one exactly on either end (both ends are inclusive)
    t = np.concatenate([np.sort(rng.uniform(4.9, 5.0, 40)), prob["time"], np.sort(rng.uniform(5.5, 5.6, 40))])
    t[40], t[-41] = 5.0, 5.5
    t[39], t[-40] = np.nextafter(5.0, 0.0), np.nextafter(5.5, 6.0)
    xy = np.concatenate([rng.uniform(0, 260, (40, 2)), prob["obs"], rng.uniform(0, 260, (40, 2))])
    return prob, y, t, xy


@pytest.mark.parametrize("use_so3,fisheye", [(False, False), (False, True), (True, False), (True, True)])
def test_points_match_numpy(ctx, use_so3, fisheye):
    """Prints the measured max |xw - numpy| over 5 080 events (board units) per variant before it asserts the cap."""
    from eventcalib_amd.capi import Solver
    prob, y, t, xy = _points_problem(use_so3, fisheye)
    assert len(t) == 5080 and (np.diff(t) >= 0).all()
    s = Solver(ctx, prob)
    xw, flag = s.board_points(y, _pack(t, xy, np.zeros(len(t), np.uint8)))
    ref_xw, ref_flag = _board_points(prob, y, t, xy)
    dev = np.abs(xw - ref_xw).max()
    print("so3 %d fisheye %d: max |xw - numpy| %.3g board units, flags %s" % (use_so3, fisheye, dev, np.bincount(flag, minlength=3).tolist()))
    assert np.array_equal(flag, ref_flag)
    assert (ref_flag[:40] == 1).all() and (ref_flag[-40:] == 1).all() and (ref_flag[40:-40] == 0).all()
    assert dev <= TOL_X
    assert (xw[flag != 0] == 0).all()
    s.close()


# ---- 2. image, ring profile, totals ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gap_stream(use_so3, fisheye=False):
    """3 segments with gaps, n_cp = 12 each, 3 * 4096 + 17 events: 3 x 4000 on the circles' rims (0.5 px noise) and 305 outside
    every segment (before the first, in both gaps, behind the last); both polarities; 1 % of the pixels 10 000 px off the sensor
    (pinhole only: the module's docstring)"""
    prob, x = SV.make_problem(12000, n_cp=12, seed=31 + use_so3 + 2 * fisheye, pixel_noise=0.5, n_segments=3, use_so3=use_so3, fisheye=fisheye)
    y = SV.perturb(x, 36, np.random.default_rng(8), intr_rel=0.002, rot=0.001, trans=0.05)
    rng = np.random.default_rng(9)
    segs = _segments(prob)
    ends = [(kn[3], kn[ncp]) for kn, ncp, _ in segs]
    extra_t = np.concatenate([rng.uniform(ends[0][0] - 0.05, ends[0][0], 100), rng.uniform(ends[0][1], ends[1][0], 50),
                              rng.uniform(ends[1][1], ends[2][0], 50), rng.uniform(ends[2][1], ends[2][1] + 0.05, 105)])
    extra_t = extra_t[(np.array([[a < v < b for a, b in ends] for v in extra_t]).sum(axis=1) == 0)]
    assert len(extra_t) == 305
    t = np.concatenate([prob["time"], extra_t])
    xy = np.concatenate([prob["obs"], rng.uniform(0, 260, (305, 2))])
    # events exactly on a segment's first and last knot and on an interior knot
    kn1, ncp1, _ = segs[1]
    idx = np.flatnonzero((prob["time"] > kn1[5]))[:1]
    t[idx] = kn1[5]
    first1 = np.flatnonzero(prob["seg_id"] == 1)
    t[first1[0]], t[first1[-1]] = kn1[3], kn1[ncp1]
    order = np.argsort(t, kind="stable")
    t, xy = t[order], xy[order]
    far = rng.choice(len(t), len(t) // 100, replace=False)
    if not fisheye:
        xy[far] += 10000.0 * rng.choice([-1.0, 1.0], (len(far), 2))
    pol = rng.integers(0, 2, len(t)).astype(np.uint8)
    return prob, y, t, xy, pol


@pytest.mark.parametrize("use_so3,fisheye", [(False, False), (True, False), (False, True), (True, True)])
def test_image_ring_profile_and_totals(ctx, use_so3, fisheye):
    from eventcalib_amd.capi import Solver
    prob, y, t, xy, pol = _gap_stream(use_so3, fisheye)
    assert len(t) == 3 * 4096 + 17
    modes = _block_modes(prob, t)
    assert len(modes) == 4 and {"none", "staged", "global"} <= set(modes), modes     # every path of the kernel, a partial last block
    s = Solver(ctx, prob)
    # an image of 120 x 120 bins from the default corner: 26 board units of the board's 49 x 55
    got, ref, events = _check_image(s, prob, y, t, xy, pol, width=120, height=120)
    tot = got["totals"]
    assert tot["n_outside_time"] == 305 and (fisheye or tot["n_behind"] + tot["n_outside_image"] >= len(t) // 100)
    assert tot["n_outside_image"] > 1000 and (tot["n_image"] > 1000).all() and tot["n_ring"] > 10000
    # the per-event form on the same stream: the flags (the depth's sign among them) exactly, the points to TOL_X where the pixel
    # is on the sensor
    xw, flag = s.board_points(y, events)
    ref_xw, ref_flag = _board_points(prob, y, t, xy)
    on = (np.abs(xy) < 1000).all(axis=1)
    assert np.array_equal(flag, ref_flag) and np.abs(xw[on] - ref_xw[on]).max() <= TOL_X
    # the default image holds every in-time event whose pixel is on the sensor's side of the board
    _check_image(s, prob, y, t, xy, pol)
    s.close()


# ---- 3. many spans per block -----------------------------------------------------------------------------------------------

def test_many_spans_per_block_take_the_global_path(ctx):
    from eventcalib_amd import capi
    prob, x = SV.make_problem(5000, n_cp=64, seed=41, pixel_noise=0.5)
    y = SV.perturb(x, 64, np.random.default_rng(12), intr_rel=0.002, rot=0.001, trans=0.05)
    t, xy = prob["time"], prob["obs"]
    modes = _block_modes(prob, t)
    assert modes[0] == "global", modes               # 61 spans of ~82 events: a block of 4096 meets ~50, the staging holds 13
    assert capi.BOARD_IMAGE_CP_LDS == 16 and capi.BOARD_IMAGE_BLOCK == 4096
    pol = (np.arange(len(t)) % 3 == 0).astype(np.uint8)
    s = capi.Solver(ctx, prob)
    _check_image(s, prob, y, t, xy, pol)
    # the same spline met by short blocks: 300 events meet ~4 spans, staged
    assert _block_modes(prob, t[:300]) == ["staged"]
    _check_image(s, prob, y, t[:300], xy[:300], pol[:300])
    s.close()


# ---- 4. degenerate sizes ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _small():
    prob, x = SV.make_problem(600, n_cp=6, seed=51, pixel_noise=0.5)
    return prob, SV.perturb(x, 6, np.random.default_rng(13), intr_rel=0.002, rot=0.001, trans=0.05)


def test_degenerate_sizes(ctx):
    from eventcalib_amd.capi import Solver
    prob, y = _small()
    s = Solver(ctx, prob)
    got = s.board_image(y, np.zeros(0, np.uint8))                                   # no event: zeros, ECAL_OK
    assert not any(int(np.sum(got["totals"][k])) for k in got["totals"].dtype.names)
    assert not got["image"].any() and not got["ring_hist"].any() and not got["ring_stats"]["n"].any()
    assert got["image"].shape == (2, got["options"].height, got["options"].width) and got["ring_hist"].shape == (36, 64)
    xw, flag = s.board_points(y, np.zeros(0, np.uint8))
    assert xw.shape == (0, 2) and flag.shape == (0,)
    t, xy = prob["time"], prob["obs"]
    _check_image(s, prob, y, t[:1], xy[:1], np.ones(1, np.uint8))                 # one event
    got, _, _ = _check_image(s, prob, y, t + 10.0, xy, np.zeros(600, np.uint8))   # every event outside the segment
    assert got["totals"]["n_outside_time"] == 600 and not got["image"].any()
    got, _, _ = _check_image(s, prob, y, t, xy, np.zeros(600, np.uint8), ring_bins=0)
    assert "ring_hist" not in got and "ring_stats" not in got and got["totals"]["n_ring"] == 0 and got["image"].sum() > 0
    _check_image(s, prob, y, t, xy, np.zeros(600, np.uint8), ring_bins=1)
    _check_image(s, prob, y, t, xy, np.zeros(600, np.uint8), ring_bins=256, ring_range=0.3, width=1, height=1, x0=19.0, y0=22.0, bin=5.0)
    s.close()


def test_null_outputs_touch_no_memory(ctx):
    """board_image_dev with outputs left out, in every combination: one arena filled with a canary, the outputs carved out of it
    side by side — only what was asked for is written, and the totals do not depend on it"""
    import torch
    from eventcalib_amd import capi
    prob, y = _small()
    s = capi.Solver(ctx, prob)
    events = _pack(prob["time"], prob["obs"], (np.arange(600) % 2).astype(np.uint8))
    full = s.board_image(y, events, width=40, height=30)
    o = full["options"]
    sizes = dict(totals=7, img=40 * 30, stats=36 * 2 * 3, hist=36 * 64)             # in 8-byte words
    off, at = {}, 3
    for name, w in sizes.items():
        off[name] = at
        at += w + 3
    canary = -7.25e77
    d_y = torch.as_tensor(y, device="cuda")
    d_ev = torch.from_numpy(events).cuda()
    for mask in range(8):
        asked = tuple(n for k, n in enumerate(("img", "stats", "hist")) if mask >> k & 1)
        arena = torch.full((at,), canary, dtype=torch.float64, device="cuda")

        def p(name):
            return arena.data_ptr() + 8 * off[name] if name in asked or name == "totals" else None
        s.board_image_dev(d_y.data_ptr(), d_ev.data_ptr(), 600, o, p("img"), p("totals"), p("stats"), p("hist"),
                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        host = arena.cpu().numpy()
        written = np.zeros(at, bool)
        for name in asked + ("totals",):
            written[off[name]: off[name] + sizes[name]] = True
        assert (host[~written] == canary).all(), asked
        assert not (host[written] == canary).any(), asked
        tot = host[off["totals"]: off["totals"] + 7].view(capi.BOARD_IMAGE_TOTALS)[0]
        assert tot.tobytes() == full["totals"].tobytes(), asked
        if "img" in asked:
            assert np.array_equal(host[off["img"]: off["img"] + 1200].view(np.uint32).reshape(2, 30, 40), full["image"])
        if "stats" in asked:
            assert np.array_equal(host[off["stats"]: off["stats"] + 216].view(capi.RING_STATS).reshape(36, 2)["n"], full["ring_stats"]["n"])
        if "hist" in asked:
            assert np.array_equal(host[off["hist"]: off["hist"] + 2304].view(np.uint64).reshape(36, 64), full["ring_hist"])
    s.close()


def test_invalid_options_are_refused_with_a_message(ctx):
    import torch
    from eventcalib_amd.capi import EcalError, Solver
    prob, y = _small()
    s = Solver(ctx, prob)
    events = _pack(prob["time"], prob["obs"], np.zeros(600, np.uint8))
    for bad, status in ((dict(bin=0.0), -1), (dict(bin=-1.0), -1), (dict(bin=float("nan")), -1), (dict(x0=float("inf")), -1),
                        (dict(width=4097, height=4096), -6), (dict(ring_bins=257), -1), (dict(ring_range=0.0), -1),
                        (dict(ring_range=float("nan")), -1)):
        with pytest.raises(EcalError) as e:
            s.board_image(y, events, **bad)
        assert e.value.status == status and "ecal_solver_board_image" in str(e.value), bad
    # refused before anything is launched or zeroed: the outputs keep their canary
    arena = torch.full((7,), -7.25e77, dtype=torch.float64, device="cuda")
    d_y = torch.as_tensor(y, device="cuda")
    with pytest.raises(EcalError):
        s.board_image_dev(d_y.data_ptr(), torch.from_numpy(events).cuda().data_ptr(), 600, s.board_image_options(bin=0.0), None,
                          arena.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (arena.cpu().numpy() == -7.25e77).all()
    assert s.board_image(y, events, width=4096, height=4096, outputs=())["totals"]["n_events"] == 600      # 2^24 bins: the limit itself
    s.close()
    # a ring profile for more than 128 landmarks: ECAL_ERR_RANGE; without the profile the same board is fine
    many = dict(prob, landmarks=np.concatenate([prob["landmarks"]] * 4)[:129])
    s = Solver(ctx, many)
    with pytest.raises(EcalError) as e:
        s.board_image(y, events)
    assert e.value.status == -6 and "128 landmarks" in str(e.value)
    assert s.board_image(y, events, ring_bins=0)["totals"]["n_events"] == 600
    s.close()
    s = Solver(ctx, dict(prob, landmarks=np.concatenate([prob["landmarks"]] * 4)[:128]))
    assert s.board_image(y, events, ring_bins=256, outputs=("ring_hist",))["ring_hist"].shape == (128, 256)   # the largest LDS layout
    s.close()


# ---- 5. forms --------------------------------------------------------------------------------------------------------------

def test_dev_form_equals_host_form_and_calls_repeat(ctx):
    from eventcalib_amd.capi import Solver
    prob, y, t, xy, pol = _gap_stream(False)
    s = Solver(ctx, prob)
    events = _pack(t, xy, pol)
    a = s.board_image(y, events, width=120, height=120)
    b = s.board_image(y, events, width=120, height=120)
    img, tot, rs, rh = s.board_image_host(y, events, width=120, height=120)
    for other_img, other_tot, other_n, other_hist in ((b["image"], b["totals"], b["ring_stats"]["n"], b["ring_hist"]), (img, tot, rs["n"], rh)):
        assert np.array_equal(a["image"], other_img) and a["totals"].tobytes() == other_tot.tobytes()
        assert np.array_equal(a["ring_stats"]["n"], other_n) and np.array_equal(a["ring_hist"], other_hist)
    # the FP64 sums depend on the order of arrival in their last bits: the rule of the image test between any two calls
    for other in (b["ring_stats"], rs):
        nn = a["ring_stats"]["n"].astype(np.float64)
        bound = 1e-11 * nn * a["options"].ring_range + nn * TOL_X
        assert (np.abs(a["ring_stats"]["sum_d"] - other["sum_d"]) <= bound).all()
        assert (np.abs(a["ring_stats"]["sum_d2"] - other["sum_d2"]) <= bound * 2 * a["options"].ring_range).all()
    xw, flag = s.board_points(y, events)
    h_xw, h_flag = s.board_points_host(y, events)
    assert np.array_equal(xw, h_xw) and np.array_equal(flag, h_flag)
    # the host form with outputs left out
    img2, tot2, rs2, rh2 = s.board_image_host(y, events, outputs=("ring_hist",), width=120, height=120)
    assert img2 is None and rs2 is None and tot2.tobytes() == tot.tobytes() and np.array_equal(rh2, rh)
    s.close()


# ---- 6. meaning ------------------------------------------------------------------------------------------------------------

def test_rings_are_sharp_at_the_truth_and_smear_off_it(ctx):
    """events generated ON the circles' rims (zero pixel noise): at the ground truth every circle's ring has |mean d| and std d
    below 1e-6 radius; after perturb(intr_rel=0.01, rot=0.005, trans=0.2) the mean ring_std is at least 100 x larger"""
    from eventcalib_amd.capi import Solver
    prob, x = SV.make_problem(3000, n_cp=8, seed=61)
    events = _pack(prob["time"], prob["obs"], (np.arange(3000) % 2).astype(np.uint8))
    s = Solver(ctx, prob)
    good = s.board_image(x, events)
    R = prob["circle_radius"]
    assert (good["ring_n"] > 0).all() and int(good["ring_n"].sum()) == 3000 == int(good["totals"]["n_ring"])
    print("truth: max ring_std %.3g, max |ring_mean| %.3g" % (good["ring_std"].max(), np.abs(good["ring_mean"]).max()))
    assert (good["ring_std"] < 1e-6 * R).all() and (np.abs(good["ring_mean"]) < 1e-6).all()
    # ... and the image shows them: every event in the ring of pixels around its circle's rim
    assert int(good["image"].sum()) == 3000
    y = SV.perturb(x, 8, np.random.default_rng(14), intr_rel=0.01, rot=0.005, trans=0.2)
    bad = s.board_image(y, events)
    has = bad["ring_n"] > 0
    print("perturbed: mean ring_std %.3g over %d circles" % (bad["ring_std"][has].mean(), int(has.sum())))
    assert has.sum() >= 30
    assert bad["ring_std"][has].mean() >= 100 * max(good["ring_std"].mean(), 1e-12)
    assert bad["ring_std"][has].mean() >= 100 * 1e-6 * R
    s.close()
