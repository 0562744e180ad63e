"""GPU: the first hash pass at every event count at which a thread's event slot changes from empty to partial to full, in both of its
forms (six slots for windows of up to 1535 events, eight for 1536 .. 2047; slice_hash.hpp): the default path against the general
slicer (ECAL_FORCE=slice_general) and against the oracle's EventFrame — segment offsets and counts, the points bit for bit, the
event -> point map, the overflow flag — with the map and without it, one window per launch and many windows of different counts
in one launch, and with a non-pixel coordinate in a full slot and in the partial one."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

T = 256                  # threads per window: event k sits in slot k // T of thread k % T
# every slot boundary of the six-slot form (1280 = five full slots, 1535 its last size) and of the eight-slot form; 2048 is the
# second pass's
SIZES = (0, 1, 63, 64, 255, 256, 257, 511, 512, 513, 1279, 1280, 1281, 1535, 1536, 1537, 1791, 1792, 2047, 2048)
W, H = 346, 260


@pytest.fixture(scope="module")
def env():
    import torch
    import eventcalib_amd
    from eventcalib_amd.pipeline import DetectPipeline
    ctx = eventcalib_amd.Context(0)
    assert ctx.point_order() == "reference"
    ctx.set_tail_mode("tiered")   # what the first pass lists goes to the second pass in every call (auto plans from the calls before)
    yield ctx, DetectPipeline, torch
    ctx.set_tail_mode("auto")
    ctx.close()


class _Windows:
    """Windows one behind the other on the time axis: 1 us between events, 1 ms between windows; a window may be empty."""

    def __init__(self):
        self.recs, self.t0, self.t1, self.t_at = [], [], [], 1.0

    def add(self, x, y, p):
        n = len(x)
        if n == 0:
            self.t0.append(self.t_at + 1e-4)
            self.t1.append(self.t_at + 2e-4)
            self.t_at += 1e-3
            return
        t = self.t_at + 1e-6 * (1 + np.arange(n))
        self.recs.append(O.pack_events(t, np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(p, np.uint8)))
        self.t0.append(t[0])
        self.t1.append(t[-1] + 5e-7)
        self.t_at = t[-1] + 1e-3

    def rec(self):
        return np.concatenate(self.recs)


def _events(rng, n):
    """n events on sensor pixels of 346 x 260, both polarities: two thirds on a 36 x 28 patch (repeated pixels, +/- cancellations),
    the rest anywhere on the sensor, its corners included."""
    x0, y0 = int(rng.integers(0, W - 36)), int(rng.integers(0, H - 28))
    x, y = rng.integers(x0, x0 + 36, n), rng.integers(y0, y0 + 28, n)
    far = rng.random(n) < 1.0 / 3.0
    x[far], y[far] = rng.integers(0, W, int(far.sum())), rng.integers(0, H, int(far.sum()))
    if n >= 4:
        at = rng.choice(n, 4, replace=False)
        x[at], y[at] = [0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1]
    return x, y, rng.integers(0, 2, n)


def _slice(env, rec, t0, t1, want_ep, general):
    """One slicing call in a pipeline of its own; what it left, as numpy arrays."""
    import eventcalib_amd.capi as capi
    ctx, DetectPipeline, torch = env
    n, S = rec.size // 25, len(t0)
    if general:
        os.environ["ECAL_FORCE"] = "slice_general"
        capi.sync_env()   # (the switches are read once per context)
    try:
        pipe = DetectPipeline(ctx, want_event_point=want_ep)
        pipe.set_windows(t0, t1)
        pipe._ensure(S, n + 64)
        pipe.event_point.fill_(-77)
        pipe.run(torch.from_numpy(rec).cuda(), slots=n + 64, slice_only=True)
        torch.cuda.synchronize()
        assert not pipe.overflowed(), "overflow flag"
        return {"lo": pipe.win_lo[:S].cpu().numpy().astype(np.int64), "hi": pipe.win_hi[:S].cpu().numpy().astype(np.int64),
                "base": pipe.win_base[:S + 1].cpu().numpy().astype(np.int64),
                "seg_off": pipe.seg_off[:2 * S].cpu().numpy().astype(np.int64),
                "seg_cnt": pipe.seg_cnt[:2 * S].cpu().numpy().astype(np.int64),
                "packed": pipe.seg_fmt[:2 * S].cpu().numpy()[0::2] != 0,   # a hash pass took the window, not a general tier
                "xy": pipe.xy.cpu().numpy().copy(), "ep": pipe.event_point.cpu().numpy().copy()}
    finally:
        if general:
            os.environ.pop("ECAL_FORCE", None)
            capi.sync_env()


def _points(out):
    used = np.zeros(out["xy"].shape[0], bool)
    for o, c in zip(out["seg_off"], out["seg_cnt"]):
        used[o:o + c] = True
    return out["xy"][used].view(np.uint64)


def _same(a, b, want_ep):
    assert np.array_equal(a["lo"], b["lo"]) and np.array_equal(a["hi"], b["hi"]) and np.array_equal(a["base"], b["base"])
    assert np.array_equal(a["seg_off"], b["seg_off"]), "seg_off: default path against the general slicer"
    assert np.array_equal(a["seg_cnt"], b["seg_cnt"]), "seg_cnt: default path against the general slicer"
    assert np.array_equal(_points(a), _points(b)), "points: default path against the general slicer"
    if want_ep:
        assert np.array_equal(a["ep"], b["ep"]), "event -> point map: default path against the general slicer"
    else:
        assert (a["ep"] == -77).all() and (b["ep"] == -77).all(), "the event -> point map was not asked for"


def _oracle(out, rec, t0, t1, want_ep):
    run = 0
    for s in range(len(t0)):
        olo, ohi = O.window_bounds(rec, t0[s], t1[s])
        n = ohi - olo
        assert (out["lo"][s], out["hi"][s]) == (olo, ohi) or (n == 0 and out["hi"][s] == out["lo"][s]), "window %d bounds" % s
        assert out["base"][s] == run
        run += n
        pos, neg, oep = O.event_frame(rec, olo, ohi, "reference")
        so, sc = out["seg_off"], out["seg_cnt"]
        assert sc[2 * s] == pos.shape[0] and sc[2 * s + 1] == neg.shape[0], "window %d (%d events) counts" % (s, n)
        if n:
            assert so[2 * s] == out["base"][s] and so[2 * s + 1] == out["base"][s] + pos.shape[0], "window %d offsets" % s
        gp, gn = out["xy"][so[2 * s]:so[2 * s] + sc[2 * s]], out["xy"][so[2 * s + 1]:so[2 * s + 1] + sc[2 * s + 1]]
        assert np.array_equal(gp.view(np.uint64), pos.view(np.uint64)), "window %d (%d events) + points" % (s, n)
        assert np.array_equal(gn.view(np.uint64), neg.view(np.uint64)), "window %d (%d events) - points" % (s, n)
        if want_ep:
            assert np.array_equal(out["ep"][out["base"][s]:out["base"][s] + n], oep), "window %d (%d events) event_point" % (s, n)
    assert out["base"][len(t0)] == run


def _both_ways(env, w, want_ep):
    rec = w.rec()
    a = _slice(env, rec, w.t0, w.t1, want_ep, general=False)
    b = _slice(env, rec, w.t0, w.t1, want_ep, general=True)
    assert not b["packed"].any(), "ECAL_FORCE=slice_general: no hash pass"
    _same(a, b, want_ep)
    _oracle(a, rec, w.t0, w.t1, want_ep)
    return a


@pytest.mark.parametrize("want_ep", [True, False])
def test_one_window_per_launch_at_every_slot_boundary(env, want_ep):
    """Each count alone in its launch, behind an anchor window of three events (the stream is never empty)."""
    rng = np.random.default_rng(711)
    for n in SIZES:
        w = _Windows()
        w.add(*_events(rng, 3))
        w.add(*_events(rng, n))
        a = _both_ways(env, w, want_ep)
        assert int(a["hi"][1] - a["lo"][1]) == n
        assert bool(a["packed"][1]) == (n > 0), "%d events: a hash pass's window (2048: listed for the second pass)" % n


@pytest.mark.parametrize("want_ep", [True, False])
def test_windows_of_different_counts_in_one_launch(env, want_ep):
    """Every boundary count twice and counts between them, shuffled, in one launch: neighbouring workgroups take different forms and
    different full / partial / empty slots."""
    rng = np.random.default_rng(712)
    sizes = np.concatenate([SIZES, SIZES, rng.integers(2, 2047, 24)])
    sizes = sizes[rng.permutation(len(sizes))]
    w = _Windows()
    for n in sizes:
        w.add(*_events(rng, int(n)))
    a = _both_ways(env, w, want_ep)
    assert np.array_equal(a["hi"] - a["lo"], sizes)
    assert np.array_equal(a["packed"], sizes > 0)


@pytest.mark.parametrize("want_ep", [True, False])
def test_non_pixel_coordinate_in_a_full_slot_and_in_the_partial_slot(env, want_ep):
    """One coordinate of 10.5 in a window of the six-slot form (1500 events: slots 0 - 4 full, slot 5 partial) and of the eight-slot
    form (1900 events: slots 0 - 6 full, slot 7 partial), in a full slot or as an event of the partial one — its first, its last.
    The window leaves the pixel path whole (doubles, not packed words) and still equals the general slicer and the oracle; its
    neighbours stay on the hash pass."""
    rng = np.random.default_rng(713)
    w = _Windows()
    odd_window = []
    for n in (1500, 1900, 1281, 1537):
        full_to = (n // T) * T   # events [0, full_to) sit in full slots, [full_to, n) in the partial one
        for k in (int(rng.integers(0, full_to)), T + 7, full_to - 1, full_to, n - 1):
            for axis in (0, 1):
                x, y, p = _events(rng, n)
                xy = [x.astype(np.float64), y.astype(np.float64)]
                xy[axis][k] = 10.5
                w.add(xy[0], xy[1], p)
                odd_window.append(True)
                w.add(*_events(rng, n))
                odd_window.append(False)
    a = _both_ways(env, w, want_ep)
    assert np.array_equal(a["packed"], ~np.array(odd_window))
