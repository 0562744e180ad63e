"""GPU: the noise filter's kernels (eventcalib_amd/csrc/ecal_noise.hip) through capi.Context.  Every case compares
Context.noise_verdict with ecal_noise_verdict_host (the sequential walk, on the host) byte for byte, and Context.denoise_events with
the host compaction by those verdicts byte for byte, totals included.

Sizes around the compaction's block of 4096 events on a 16 x 12 grid (long lists, dense neighbourhoods) and one stream of 4.3 M events
(the block scan's second round); six sensors and a 4096 x 4096 one (the start table); tied stamps, a shuffled stream, dt = +inf, NaN
stamps, every off-grid kind of coordinate; a pixel with a million events beside one with ten; 64 adjacent pixels that each take a
whole wave's events; every radius, both include_self values, min_support in {1, 2, 8, 9}; an unaligned input with nothing behind it
and an output of exactly the kept size; the chain behind the hot-pixel filter against the oracle chain; what is refused."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hot_pixel_oracle as HP  # noqa: E402
import noise_filter_oracle as NF  # noqa: E402
from test_noise_filter_host import random_stream, records  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCK = 4096


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    with eventcalib_amd.Context(0) as c:
        yield c


def check(ctx, rec, W, H, events=None, **opts):
    """the device verdicts and the device compaction against the host walk; returns (host verdicts, totals dict)"""
    import torch
    from eventcalib_amd import capi
    want, want_tot = capi.noise_verdict_host(rec, width=W, height=H, **opts)
    want_tot = {k: int(want_tot[k]) for k in want_tot.dtype.names}
    ev = torch.from_numpy(rec).cuda() if events is None else events
    v, tot = ctx.noise_verdict(ev, width=W, height=H, **opts)
    assert v.numel() == want.size and torch.equal(v.cpu(), torch.from_numpy(want))
    assert {k: int(tot[k]) for k in tot.dtype.names} == want_tot
    out, tot = ctx.denoise_events(ev, width=W, height=H, **opts)
    kept = NF.compact(rec, want)
    assert {k: int(tot[k]) for k in tot.dtype.names} == want_tot
    assert out.numel() == kept.size == want_tot["n_kept"] * 25
    assert torch.equal(out.cpu(), torch.from_numpy(kept))
    return want, want_tot


@pytest.mark.parametrize("n", [0, 1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5])
def test_sizes_around_the_block_on_a_small_grid(ctx, n):
    rng = np.random.default_rng(200 + n)
    rec = random_stream(rng, n, 16, 12)
    _, tot = check(ctx, rec, 16, 12, dt=2e-4)
    if n > 2:
        assert 0 < tot["n_removed"] and tot["n_off_grid"] < tot["n_kept"] < n
    check(ctx, rec, 16, 12, dt=1e-4, min_support=2)    # (few stay)


def test_the_scan_goes_into_its_second_round(ctx):
    """4.3 M events on 346 x 260: 1050 blocks of 4096"""
    n = 4_300_000
    rng = np.random.default_rng(9)
    rec = random_stream(rng, n, 346, 260, off_frac=0.01, nan_frac=0.001)
    _, tot = check(ctx, rec, 346, 260, dt=0.8)    # (about 8000 events back: half of the events find a neighbour)
    assert (n + BLOCK - 1) // BLOCK > 1024 and n // 4 < tot["n_kept"] < 3 * n // 4


@pytest.mark.parametrize("W,H", [(346, 260), (640, 480), (1280, 720), (1, 1), (347, 3), (1, 64)])
def test_sensors(ctx, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    rec = random_stream(rng, 3 * BLOCK + 5, W, H)
    _, tot = check(ctx, rec, W, H, dt=float("inf") if W * H > 50000 else 1e-3, include_self=1 if W * H == 1 else 0)
    assert 0 < tot["n_removed"] and tot["n_kept"] > tot["n_off_grid"]
    check(ctx, rec, W, H, radius=3, min_support=2, dt=float("inf"))


def test_the_largest_sensor(ctx):
    """4096 x 4096 with 10 k events: a start table of 16.7 M words, nearly all lists empty"""
    rng = np.random.default_rng(77)
    n = 10_000
    rec = random_stream(rng, n, 4096, 4096)
    x = rng.integers(4000, 4096, n // 2).astype(np.float64)   # half of them crowd a corner, so that some are supported
    y = rng.integers(4040, 4096, n // 2).astype(np.float64)
    r = rec.reshape(-1, 25)
    r[: n // 2, 8:24] = np.stack([x, y], axis=1).astype("<f8").view(np.uint8).reshape(-1, 16)
    _, tot = check(ctx, rec, 4096, 4096, dt=float("inf"), radius=2)
    assert 500 < tot["n_kept"] - tot["n_off_grid"] and 3000 < tot["n_removed"]


def test_tied_stamps(ctx):
    rng = np.random.default_rng(5)
    n = 2 * BLOCK + 77
    i = np.arange(n)
    rec = records(np.full(n, 5.0), rng.integers(0, 40, n), rng.integers(0, 30, n), i & 1)
    v, tot = check(ctx, rec, 40, 30, dt=0.0)        # all stamps equal: everything behind the first few events is supported
    assert v[0] == 0 and tot["n_kept"] > n - 600
    rec = random_stream(rng, n, 40, 30, values=8)   # eight distinct stamps, 1 ms apart
    for dt in (0.0, 1e-3, 1.5e-3):
        check(ctx, rec, 40, 30, dt=dt)
    a = check(ctx, rec, 40, 30, dt=0.0)[1]["n_kept"]
    b = check(ctx, rec, 40, 30, dt=1e-3)[1]["n_kept"]
    assert a < b


def test_a_shuffled_stream(ctx):
    """the stamps are not monotone: the most recent earlier event BY INDEX counts, and its stamp may lie in the future"""
    rng = np.random.default_rng(6)
    n = 3 * BLOCK + 5
    rec = random_stream(rng, n, 60, 40, shuffle=True)
    t = HP.fields(rec)[0]
    assert (np.diff(t[~np.isnan(t)]) < 0).any()
    for dt in (0.0, 1e-3, float("inf")):
        _, tot = check(ctx, rec, 60, 40, dt=dt)
        assert 0 < tot["n_removed"] < n


def test_infinite_dt_nan_stamps_and_off_grid_events(ctx):
    rng = np.random.default_rng(7)
    n = 2 * BLOCK + 9
    W, H = 50, 40
    rec = random_stream(rng, n, W, H, off_frac=0.3, nan_frac=0.2)
    on, _ = HP.pixels(rec, W, H)
    t = HP.fields(rec)[0]
    v, tot = check(ctx, rec, W, H, dt=float("inf"))
    assert tot["n_off_grid"] == n - on.sum() > 1000 and v[~on].all()          # off the grid: kept, all of them
    assert not v[on & np.isnan(t)].any() and (on & np.isnan(t)).sum() > 500    # a NaN stamp is never supported
    # off-grid events support nothing: without them the on-grid verdicts are the same
    from eventcalib_amd import capi
    v_on, _ = capi.noise_verdict_host(rec.reshape(-1, 25)[on].ravel(), width=W, height=H, dt=float("inf"))
    assert (v_on == v[on]).all()
    check(ctx, rec, W, H, dt=1e-3, radius=2, min_support=2)
    # only off-grid events
    check(ctx, rec.reshape(-1, 25)[~on].ravel(), W, H)


def test_one_pixel_takes_a_million_events_beside_one_that_takes_ten(ctx):
    n = 1_000_000
    W, H = 346, 260
    i = np.arange(n)
    x = np.full(n, 123.0)
    few = np.arange(50_000, n, 100_000)      # ten events of the neighbour pixel
    x[few] = 124.0
    rec = records(5.0 + i * 1e-6, x, np.full(n, 45.0), i & 1)
    v, tot = check(ctx, rec, W, H)           # the hot pixel is supported for 5 ms behind each of the neighbour's events
    assert v[few].all() and 10 * 4990 < tot["n_kept"] < 10 * 5010
    v, tot = check(ctx, rec, W, H, include_self=1)
    assert tot["n_removed"] == 1 and v[0] == 0
    check(ctx, rec, W, H, include_self=1, min_support=2, dt=1e-4)


def test_pixels_that_each_take_a_whole_wave(ctx):
    """64 adjacent pixels of one row, every run of 64 events on one of them"""
    n = 64 * 64 * 4 + 13
    i = np.arange(n)
    p = (i // 64) % 64
    rec = records(5.0 + i * 1e-6, 10 + p, np.full(n, 200.0), (i // 3) & 1)
    _, tot = check(ctx, rec, 346, 260, dt=100e-6)
    assert 0 < tot["n_removed"] < n
    _, tot = check(ctx, rec, 346, 260, dt=130e-6, min_support=2, radius=2)    # the two pixels in front of the run's support it
    assert 0 < tot["n_removed"] < n // 4
    check(ctx, rec, 346, 260, dt=float("inf"), include_self=1)


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("include_self", [0, 1])
def test_every_radius_self_and_support(ctx, radius, include_self):
    rng = np.random.default_rng(31 * radius + include_self)
    dense = random_stream(rng, BLOCK + 100, 16, 12)
    sparse = random_stream(rng, 2 * BLOCK + 3, 100, 80)
    kept = []
    for min_support in (1, 2, 8, 9):
        _, tot = check(ctx, dense, 16, 12, radius=radius, include_self=include_self, min_support=min_support, dt=2e-2)
        kept.append(tot["n_kept"])
        check(ctx, sparse, 100, 80, radius=radius, include_self=include_self, min_support=min_support, dt=float("inf"))
    assert kept == sorted(kept, reverse=True) and kept[0] > kept[-1]


def test_an_unaligned_input_with_nothing_behind_it_and_an_exact_output(ctx):
    import torch
    from eventcalib_amd import capi
    rng = np.random.default_rng(12)
    W, H = 60, 40
    n = 2 * BLOCK + 1
    rec = random_stream(rng, n, W, H)
    want, want_tot = capi.noise_verdict_host(rec, width=W, height=H, dt=1e-3)
    kept = NF.compact(rec, want)
    assert 0 < kept.size < rec.size
    o = capi.noise_options(width=W, height=H, dt=1e-3)
    st = torch.cuda.current_stream().cuda_stream
    for shift in (1, 3, 8):
        # One allocation: the output in front — exactly the kept records, then guard bytes up to the events —, the events at its end
        # with nothing behind them, both unaligned.  The call wants the n * 25 bytes from d_out on not to overlap the events (its
        # contract speaks of room for n_events records), so the events start behind them; whatever lies there must stay untouched.
        off_e = (shift + n * 25 + 15) // 16 * 16 + shift
        arena = torch.full((off_e + n * 25,), 0xEE, dtype=torch.uint8, device="cuda")
        arena[off_e:] = torch.from_numpy(rec).cuda()
        view, out = arena[off_e:], arena[shift:]
        assert view.data_ptr() % 16 == shift == out.data_ptr() % 16 and view.is_contiguous()
        check(ctx, rec, W, H, events=view, dt=1e-3)
        ver = torch.full((shift + n + 64,), 0xEE, dtype=torch.uint8, device="cuda")   # a verdict array of exactly n bytes, unaligned
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        tot = torch.zeros(4, dtype=torch.int64, device="cuda")
        ctx.denoise_events_dev(view.data_ptr(), n, o, out.data_ptr(), cnt.data_ptr(), tot.data_ptr(), st)
        ctx.noise_verdict_dev(view.data_ptr(), n, o, ver[shift:].data_ptr(), None, st)
        torch.cuda.synchronize()
        assert int(cnt.item()) == kept.size // 25 == int(tot[3].item())
        assert torch.equal(out[: kept.size].cpu(), torch.from_numpy(kept))
        assert (arena[:shift] == 0xEE).all() and (arena[shift + kept.size: off_e] == 0xEE).all()   # nothing behind the kept records is stored
        assert torch.equal(view.cpu(), torch.from_numpy(rec))
        assert torch.equal(ver[shift: shift + n].cpu(), torch.from_numpy(want))
        assert (ver[:shift] == 0xEE).all() and (ver[shift + n:] == 0xEE).all()
    # the options pointer may be null: the defaults
    rec = random_stream(rng, 1000, 346, 260)
    ev = torch.from_numpy(rec).cuda()
    ver = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    ctx.noise_verdict_dev(ev.data_ptr(), 1000, None, ver.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert torch.equal(ver.cpu(), torch.from_numpy(capi.noise_verdict_host(rec)[0]))


@pytest.fixture(scope="module")
def dirty_hover():
    import synth_stream as SS
    clean = SS.make_stream(60000, device="cpu", seed=3).numpy()
    dirty, where, _ = HP.inject_hot_pixels(clean, 346, 260, n_pixels=5, per_pixel=2000)
    return clean, dirty, where


def test_two_calls_give_the_same_bytes_and_a_sorted_stream_stays_sorted(ctx, dirty_hover):
    import torch
    _, dirty, _ = dirty_hover
    ev = torch.from_numpy(dirty).cuda()
    a, ta = ctx.denoise_events(ev)
    b, tb = ctx.denoise_events(ev)
    assert torch.equal(a, b) and ta == tb
    va, _ = ctx.noise_verdict(ev)
    vb, _ = ctx.noise_verdict(ev)
    assert torch.equal(va, vb)
    n = a.numel() // 25
    assert 0 < n < dirty.size // 25
    t = HP.fields(a.cpu().numpy())[0]
    assert (np.diff(t) >= 0).all() and (np.diff(t) == 0).any()
    check(ctx, dirty, 346, 260)


def test_hot_pixels_then_noise_equals_the_oracle_chain(ctx, dirty_hover):
    import torch
    from eventcalib_amd.calibrate import remove_hot_pixels, remove_noise
    clean, dirty, where = dirty_hover
    want_hot, hot_info = HP.remove_hot_pixels(dirty, 346, 260)
    assert want_hot.tobytes() == clean.tobytes() and hot_info["n_hot_pixels"] == 5
    want, want_tot = NF.denoise(want_hot, 346, 260)
    assert 0.8 * 60000 < want_tot["n_kept"] < 60000
    mid, info = remove_hot_pixels(ctx, torch.from_numpy(dirty).cuda())
    assert info["n_removed"] == 10000
    out, info = remove_noise(ctx, mid)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert {k: info[k] for k in want_tot} == want_tot
    assert {k: info[k] for k in ("width", "height", "radius", "min_support", "include_self", "dt")} == dict(width=346, height=260, **NF.DEFAULTS)
    # the library-owned stream's way, and other options
    out, tot = ctx.stream_remove_noise(want_hot)
    assert out.cpu().numpy().tobytes() == want.tobytes() and tot == want_tot
    opts = dict(radius=2, min_support=3, include_self=1, dt=2e-3)
    want2, want2_tot = NF.denoise(want_hot, 346, 260, **opts)
    out, tot = ctx.stream_remove_noise(want_hot, **opts)
    assert out.cpu().numpy().tobytes() == want2.tobytes() and tot == want2_tot and tot["n_kept"] != want_tot["n_kept"]
    out, tot = ctx.stream_remove_noise(np.zeros(0, np.uint8))
    assert out.numel() == 0 and tot == dict(n_events=0, n_off_grid=0, n_removed=0, n_kept=0)


def test_refusals(ctx):
    import torch
    from eventcalib_amd import capi
    rec = torch.zeros(50, dtype=torch.uint8, device="cuda")
    out = torch.zeros(50, dtype=torch.uint8, device="cuda")
    ver = torch.zeros(16, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    bad_options = ((dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(min_support=0), "min_support"), (dict(dt=-1.0), "dt"),
                   (dict(dt=float("nan")), "dt"), (dict(reserved=1), "reserved"), (dict(width=4097), "width"), (dict(height=4097), "height"),
                   (dict(include_self=2), "include_self"))
    for bad, word in bad_options:
        o = capi.noise_options(**bad)
        for call in (lambda: ctx.noise_verdict_dev(rec.data_ptr(), 2, o, ver.data_ptr()),
                     lambda: ctx.denoise_events_dev(rec.data_ptr(), 2, o, out.data_ptr(), cnt.data_ptr())):
            with pytest.raises(capi.EcalError) as e:
                call()
            assert e.value.status == -1 and word in str(e.value), (bad, str(e.value))
        with pytest.raises(capi.EcalError) as e:
            ctx.stream_remove_noise(np.zeros(50, np.uint8), **bad)
        assert e.value.status == -1 and word in str(e.value)
    o = capi.noise_options()
    for call in (lambda: ctx.noise_verdict_dev(rec.data_ptr(), 1 << 32, o, ver.data_ptr()),
                 lambda: ctx.denoise_events_dev(rec.data_ptr(), 1 << 32, o, out.data_ptr(), cnt.data_ptr())):
        with pytest.raises(capi.EcalError) as e:
            call()
        assert e.value.status == -6
    for overlapping in (rec.data_ptr(), rec.data_ptr() + 25, rec.data_ptr() + 49):   # the output may not overlap the events
        with pytest.raises(capi.EcalError) as e:
            ctx.denoise_events_dev(rec.data_ptr(), 2, o, overlapping, cnt.data_ptr())
        assert e.value.status == -1 and "overlaps" in str(e.value)
    torch.cuda.synchronize()
