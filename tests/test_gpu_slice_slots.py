"""GPU: the first hash pass's two forms — six event slots per thread for windows of up to 1535 events, eight for 1536 .. 2047
(slice_hash.hpp, slice_hash_window) — against the oracle's EventFrame (real std::unordered_set order, or first occurrence):
every slot boundary, the hand-over between the forms inside one call in every tail mode and in the latency form, the votes and
limits that must not depend on the empty last slots, and sets that fill the reference-order layout's overlaid arrays."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SIX = 6 * 256 - 1        # the last window size of the six-slot form


@pytest.fixture(scope="module")
def env():
    import torch
    import eventcalib_amd
    from eventcalib_amd.pipeline import DetectPipeline
    ctx = eventcalib_amd.Context(0)
    yield ctx, DetectPipeline, torch
    ctx.set_point_order("reference")
    ctx.set_tail_mode("auto")
    ctx.close()


class _Windows:
    """Windows laid one behind the other on the time axis, 1 us between events, 1 ms between windows."""

    def __init__(self):
        self.recs, self.t0, self.t1, self.t_at = [], [], [], 1.0

    def add(self, x, y, p):
        n = len(x)
        t = self.t_at + 1e-6 * (1 + np.arange(n))
        self.recs.append(O.pack_events(t, np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(p, np.uint8)))
        self.t0.append(t[0])
        self.t1.append(t[-1] + 5e-7)
        self.t_at = t[-1] + 1e-3

    def rec(self):
        return np.concatenate(self.recs)


def _patch_window(rng, n, w=40, h=30):
    """n events on a w x h patch, both polarities: repeated pixels and +/- cancellations are common."""
    return rng.integers(100, 100 + w, n), rng.integers(50, 50 + h, n), rng.integers(0, 2, n)


def _distinct(rng, n_pos, n_neg):
    """n_pos + n_neg events on as many distinct sensor pixels (346 x 260), the polarities interleaved at random."""
    n = n_pos + n_neg
    pix = rng.choice(346 * 260, n, replace=False)
    p = np.zeros(n, np.uint8)
    p[rng.permutation(n)[:n_pos]] = 1
    return pix // 260, pix % 260, p


def _run(env, rec, t0, t1, packed=True, want_ep=True, passes=1):
    ctx, DetectPipeline, torch = env
    pipe = DetectPipeline(ctx, packed=packed, want_event_point=want_ep)
    pipe.set_windows(t0, t1)
    ev = torch.from_numpy(rec).cuda()
    for _ in range(passes):
        pipe._ensure(len(t0), rec.size // 25 + 64)
        pipe.event_point.fill_(-77)
        pipe.run(ev, slots=rec.size // 25 + 64, slice_only=True)
        torch.cuda.synchronize()
    assert not pipe.overflowed()
    return pipe


def _check(env, pipe, rec, t0, t1, want_ep=True):
    """Window bounds, segment offsets and counts, the points (bit for bit) and the event -> point map against the oracle."""
    ctx = env[0]
    S = len(t0)
    order = {"reference": "reference", "first": "canonical"}[ctx.point_order()]
    lo = pipe.win_lo[:S].cpu().numpy().astype(np.int64)
    hi = pipe.win_hi[:S].cpu().numpy().astype(np.int64)
    base = pipe.win_base[:S + 1].cpu().numpy().astype(np.int64)
    seg_off = pipe.seg_off[:2 * S].cpu().numpy().astype(np.int64)
    seg_cnt = pipe.seg_cnt[:2 * S].cpu().numpy().astype(np.int64)
    xy = pipe.xy.cpu().numpy()
    ep = pipe.event_point.cpu().numpy()
    run = 0
    for s in range(S):
        olo, ohi = O.window_bounds(rec, t0[s], t1[s])
        assert (lo[s], hi[s]) == (olo, ohi), "window %d bounds" % s
        assert base[s] == run
        run += ohi - olo
        pos, neg, oep = O.event_frame(rec, olo, ohi, order)
        assert seg_cnt[2 * s] == pos.shape[0] and seg_cnt[2 * s + 1] == neg.shape[0], "window %d (%d events) counts" % (s, ohi - olo)
        assert seg_off[2 * s] == base[s] and seg_off[2 * s + 1] == base[s] + pos.shape[0], "window %d offsets" % s
        gp = xy[seg_off[2 * s]:seg_off[2 * s] + seg_cnt[2 * s]]
        gn = xy[seg_off[2 * s + 1]:seg_off[2 * s + 1] + seg_cnt[2 * s + 1]]
        assert np.array_equal(gp.view(np.uint64), pos.view(np.uint64)), "window %d (%d events) + points" % (s, ohi - olo)
        assert np.array_equal(gn.view(np.uint64), neg.view(np.uint64)), "window %d (%d events) - points" % (s, ohi - olo)
        if want_ep:
            assert np.array_equal(ep[base[s]:base[s] + (ohi - olo)], oep), "window %d (%d events) event_point" % (s, ohi - olo)
    assert base[S] == run
    if not want_ep:
        assert bool((pipe.event_point == -77).all()), "the event -> point map was not asked for"
    return hi - lo


def _hash_pass_took(pipe, S):
    """Per window: its points went out packed, i.e. a hash pass (first, second or third) took it, not a general tier."""
    return pipe.seg_fmt[:2 * S].cpu().numpy()[0::2] != 0


BOUNDARY_SIZES = (1, 63, 64, 255, 256, 257, 1279, 1280, 1281, 1535, 1536, 1537, 1791, 1793, 2047, 2048)


@pytest.fixture(scope="module")
def boundary_windows():
    rng = np.random.default_rng(611)
    w = _Windows()
    for n in BOUNDARY_SIZES:
        w.add(*_patch_window(rng, n))
    return w.rec(), w.t0, w.t1


@pytest.mark.parametrize("order", ["reference", "first"])
@pytest.mark.parametrize("want_ep", [True, False])
@pytest.mark.parametrize("packed", [True, False])
def test_single_windows_at_every_slot_boundary(env, boundary_windows, packed, want_ep, order):
    ctx = env[0]
    rec, t0, t1 = boundary_windows
    ctx.set_point_order(order)
    try:
        pipe = _run(env, rec, t0, t1, packed=packed, want_ep=want_ep)
        sizes = _check(env, pipe, rec, t0, t1, want_ep=want_ep)
        assert tuple(int(v) for v in sizes) == BOUNDARY_SIZES
        if packed:   # every one of them is a hash pass's window: 2048 events are the second pass's (the first holds 2047)
            assert _hash_pass_took(pipe, len(t0)).all()
    finally:
        ctx.set_point_order("reference")


@pytest.fixture(scope="module")
def mixed_windows():
    rng = np.random.default_rng(612)
    sizes = np.concatenate([np.arange(SIX - 7, SIX + 9), [SIX, SIX + 1] * 8, rng.integers(1400, 1700, 24), [1, 256, 2047, 2048, 700, 1280, 1792, 3000]])
    assert len(sizes) == 64
    sizes = sizes[rng.permutation(64)]
    w = _Windows()
    for n in sizes:
        w.add(*_patch_window(rng, int(n), 60, 50))
    return w.rec(), w.t0, w.t1, sizes


@pytest.mark.parametrize("mode", ["tiered", "lean", "auto", "latency_forms"])
def test_one_call_over_windows_on_both_sides_of_the_hand_over(env, mixed_windows, mode):
    """64 windows, sizes on both sides of 1535 / 1536 in mixed order, in one call: the workgroups choose their form one by one."""
    import eventcalib_amd.capi as capi
    ctx = env[0]
    rec, t0, t1, sizes = mixed_windows
    try:
        if mode == "latency_forms":
            os.environ["ECAL_FORCE"] = mode
            capi.sync_env()
            ctx.set_tail_mode("tiered")   # (a lean plan would launch the staged first pass + the general tail instead)
        else:
            ctx.set_tail_mode(mode)
        pipe = _run(env, rec, t0, t1, passes=2)   # (auto: the second call is scheduled from what the first one saw)
        got = _check(env, pipe, rec, t0, t1)
        assert np.array_equal(got, sizes)
        if mode != "lean":   # (lean: what the first pass lists goes to the general tail)
            assert _hash_pass_took(pipe, len(t0)).all()
        else:
            assert _hash_pass_took(pipe, len(t0))[sizes <= 2047].all()
    finally:
        os.environ.pop("ECAL_FORCE", None)
        capi.sync_env()
        ctx.set_tail_mode("auto")


def test_odd_last_event_takes_the_window_off_the_pixel_path(env):
    """A non-pixel coordinate (10.5) or -0.0 as the LAST event of a 1535-event and of a 1536-event window: the slots behind it are
    empty, the vote must still see it.  The window goes to the general slicer (doubles, not packed) and equals the oracle."""
    rng = np.random.default_rng(613)
    w = _Windows()
    for n in (SIX, SIX + 1):
        for odd in (10.5, -0.0):
            for axis in (0, 1):
                x, y, p = _patch_window(rng, n)
                xy = [x.astype(np.float64), y.astype(np.float64)]
                xy[axis][-1] = odd
                w.add(xy[0], xy[1], p)
    rec = w.rec()
    pipe = _run(env, rec, w.t0, w.t1)
    sizes = _check(env, pipe, rec, w.t0, w.t1)
    assert sorted(set(int(v) for v in sizes)) == [SIX, SIX + 1]
    assert not _hash_pass_took(pipe, len(w.t0)).any()


def test_key_limits_on_the_six_slot_form(env):
    """More keys than the first pass holds, met on the six-slot form: 1535 events of one polarity on 1535 distinct pixels (the wave
    pair's registers hold 1152 keys), and 1300 events with 1110 and 1200 keys of one polarity (past the 1109-bucket epoch).  The
    windows go on to the next tier — a hash pass still — and equal the oracle."""
    rng = np.random.default_rng(614)
    w = _Windows()
    for pol in (1, 0):
        w.add(*_distinct(rng, SIX if pol else 0, 0 if pol else SIX))
    for keys in (1109, 1110, 1200):
        for pol in (1, 0):
            x, y, p = _distinct(rng, keys if pol else 1300 - keys, 1300 - keys if pol else keys)
            w.add(x, y, p)
    for keys in (1110, 1152, 1153):   # ... and with repeats of the set's own pixels behind the keys
        x, y, p = _distinct(rng, keys, 0)
        idx = np.concatenate([np.arange(keys), rng.integers(0, keys, 1300 - keys)])
        w.add(x[idx], y[idx], p[idx])
    rec = w.rec()
    pipe = _run(env, rec, w.t0, w.t1)
    _check(env, pipe, rec, w.t0, w.t1)
    assert _hash_pass_took(pipe, len(w.t0)).all()


@pytest.mark.parametrize("want_ep", [True, False])
def test_full_sets_use_every_byte_of_the_overlaid_arrays(env, want_ep):
    """Windows without a repeated pixel whose larger set has 1100 keys: seven full epochs (1109 buckets), the final indices of the
    keys fill the array that shares its bytes with the epochs' position words.  (A window holds fewer than 2200 events, so the
    1100 keys are given to each polarity in turn: 1100 + 435 and 435 + 1100 in 1535 events on the six-slot form, 1100 + 947 and
    947 + 1100 in 2047 events on the eight-slot form, 1100 + 1 and 1152 + 383.)  Points, segment counts and the event -> point
    map against the oracle."""
    rng = np.random.default_rng(615)
    w = _Windows()
    for a, b in ((1100, SIX - 1100), (SIX - 1100, 1100), (1100, 2047 - 1100), (2047 - 1100, 1100), (1100, 1), (1109, 0), (383, 1152 - 43)):
        w.add(*_distinct(rng, a, b))
    rec = w.rec()
    pipe = _run(env, rec, w.t0, w.t1, want_ep=want_ep)
    _check(env, pipe, rec, w.t0, w.t1, want_ep=want_ep)
    assert _hash_pass_took(pipe, len(w.t0)).all()
    cnt = pipe.seg_cnt[:4].cpu().numpy()
    assert [int(v) for v in cnt] == [1100, SIX - 1100, SIX - 1100, 1100]
