"""GPU: the hot-pixel filter's kernels (eventcalib_amd/csrc/ecal_activity.hip) through capi.Context — the per-pixel count map
(pixel_activity), the order-preserving filter (filter_events) and their chain (remove_hot_pixels, and the C chain
ecal_stream_remove_hot_pixels) — exactly against the numpy oracle of tests/hot_pixel_oracle.py: counts, totals and the kept bytes.

Sizes around the kernels' block of 4096 events and one stream of 1024 * 4096 + 1 events (the block scan's second round); five
sensors; every off-grid kind of coordinate; the contention the feature is about (a million events on one pixel, 64 pixels that each
take a whole wave's events); masks of all zeros and all ones; an input tensor that is not 16-byte aligned and has nothing behind it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hot_pixel_oracle as HP  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCK = 4096


def records(t, x, y, pol):
    n = len(t)
    r = np.zeros((n, 25), np.uint8)
    r[:, :24] = np.stack([np.asarray(t, np.float64), np.asarray(x, np.float64), np.asarray(y, np.float64)], axis=1).astype("<f8").view(np.uint8).reshape(n, 24)
    r[:, 24] = np.asarray(pol, np.uint8)
    return r.ravel()


OFF_GRID = (np.nan, np.inf, -np.inf, -1.0, 0.5, -0.5, 2.0 ** 53, -4.9e-324, 1e-300)


def random_stream(rng, n, W, H, off_frac=0.1):
    """time-sorted (equal stamps too), whole pixels with some off-grid coordinates of every kind, polarity bytes beyond 0 and 1"""
    t = 5.0 + np.cumsum(rng.integers(0, 3, n)) * 1e-6
    x = rng.integers(0, W, n).astype(np.float64)
    y = rng.integers(0, H, n).astype(np.float64)
    x[rng.random(n) < 0.02] = -0.0
    kinds = np.array(OFF_GRID + (float(W), float(W) - 0.5))
    bad = rng.random(n) < off_frac
    x[bad] = rng.choice(kinds, int(bad.sum()))
    kinds = np.array(OFF_GRID + (float(H), 1e9))
    bad = rng.random(n) < off_frac
    y[bad] = rng.choice(kinds, int(bad.sum()))
    pol = np.where(rng.random(n) < 0.1, rng.integers(0, 256, n), rng.integers(0, 2, n))
    return records(t, x, y, pol)


@pytest.fixture(scope="module")
def ctx():
    import eventcalib_amd
    with eventcalib_amd.Context(0) as c:
        yield c


def check_activity(ctx, rec, W, H):
    import torch
    counts, tot = ctx.pixel_activity(torch.from_numpy(rec), W, H)
    want, want_tot = HP.count_events(rec, W, H)
    assert counts.shape == (2, H, W)
    assert (counts.cpu().numpy() == want).all()
    assert {k: int(tot[k]) for k in tot.dtype.names} == want_tot
    return want


def check_filter(ctx, rec, mask, events=None):
    import torch
    out, tot = ctx.filter_events(torch.from_numpy(rec) if events is None else events, mask)
    want, want_tot = HP.filter_events(rec, mask)
    assert {k: int(tot[k]) for k in tot.dtype.names} == want_tot
    assert out.numel() == want.size
    assert torch.equal(out, torch.from_numpy(want).to(out.device))
    return out


@pytest.mark.parametrize("n", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5])
def test_sizes_around_the_block(ctx, n):
    rng = np.random.default_rng(100 + n)
    W, H = 346, 260
    rec = random_stream(rng, n, W, H)
    check_activity(ctx, rec, W, H)
    check_filter(ctx, rec, rng.random((H, W)) < 0.3)
    check_filter(ctx, rec, rng.random((H, W)) < 0.97)    # (few stay: chunks of the writing pass that hold nothing)


def test_the_scan_goes_into_its_second_round(ctx):
    """1024 * 4096 + 1 events: 1025 blocks, 105 MB; the last block holds one event"""
    import torch
    n = 1024 * BLOCK + 1
    W, H = 346, 260
    i = np.arange(n)
    rec = records(5.0 + i * 1e-6, (i * 7) % W, (i // 5) % H, i & 1)
    rng = np.random.default_rng(9)
    mask = rng.random((H, W)) < 0.5
    mask[(n - 1) // 5 % H, (n - 1) * 7 % W] = False   # the last event stays
    check_activity(ctx, rec, W, H)
    out = check_filter(ctx, rec, mask)
    assert torch.equal(out[-25:].cpu(), torch.from_numpy(rec[-25:]))


@pytest.mark.parametrize("W,H", [(346, 260), (640, 480), (1280, 720), (1, 1), (347, 3)])
def test_sensors(ctx, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    rec = random_stream(rng, 3 * BLOCK + 5, W, H)
    counts = check_activity(ctx, rec, W, H)
    assert counts.sum() > 0
    check_filter(ctx, rec, rng.random((H, W)) < 0.4)


def test_off_grid_events_are_kept_and_counted(ctx):
    rng = np.random.default_rng(4)
    W, H = 346, 260
    n = 2 * BLOCK + 77
    rec = random_stream(rng, n, W, H, off_frac=0.5)
    on, _ = HP.pixels(rec, W, H)
    assert 0 < on.sum() < n
    import torch
    counts, tot = ctx.pixel_activity(torch.from_numpy(rec), W, H)
    assert int(tot["n_off_grid"]) == n - on.sum() and int(counts.sum()) == on.sum() == int(tot["n_on_grid"])
    out, ftot = ctx.filter_events(torch.from_numpy(rec), np.ones((H, W), bool))     # every pixel masked: the off-grid events stay, all of them
    assert int(ftot["n_off_grid"]) == n - on.sum() == int(ftot["n_kept"]) and int(ftot["n_removed"]) == on.sum()
    assert out.cpu().numpy().tobytes() == rec.reshape(-1, 25)[~on].tobytes()
    check_activity(ctx, rec, W, H)
    check_filter(ctx, rec, rng.random((H, W)) < 0.5)


def test_one_pixel_takes_a_million_events(ctx):
    import torch
    n = 1_000_000
    W, H = 346, 260
    i = np.arange(n)
    rec = records(5.0 + i * 1e-6, np.full(n, 123.0), np.full(n, 45.0), i & 1)
    counts, tot = ctx.pixel_activity(torch.from_numpy(rec), W, H)
    assert int(counts[0, 45, 123]) == 500000 == int(counts[1, 45, 123]) and int(counts.sum()) == n == int(tot["n_on_grid"])
    mask = np.zeros((H, W), bool)
    mask[45, 123] = True
    out, ftot = ctx.filter_events(torch.from_numpy(rec), mask)
    assert out.numel() == 0 and int(ftot["n_removed"]) == n and int(ftot["n_kept"]) == 0
    mask[:] = True
    mask[45, 123] = False
    check_filter(ctx, rec, mask)


def test_pixels_that_each_take_a_whole_wave(ctx):
    """a wave of the kernels handles 64 consecutive events at a time: 64 pixels, every run of 64 events on one of them"""
    n = 64 * 64 * 4 + 13
    W, H = 346, 260
    i = np.arange(n)
    p = (i // 64) % 64
    rec = records(5.0 + i * 1e-6, 10 + p, 200 - p, (i // 3) & 1)
    counts = check_activity(ctx, rec, W, H)
    assert np.count_nonzero(counts[0] + counts[1]) == 64
    mask = np.zeros((H, W), bool)
    mask[200 - np.arange(0, 64, 2), 10 + np.arange(0, 64, 2)] = True
    check_filter(ctx, rec, mask)


def test_mask_extremes_and_an_unaligned_input_with_nothing_behind_it(ctx):
    import torch
    rng = np.random.default_rng(12)
    W, H = 346, 260
    n = 2 * BLOCK + 1
    rec = random_stream(rng, n, W, H, off_frac=0.0)
    out = check_filter(ctx, rec, np.zeros((H, W), bool))
    assert out.cpu().numpy().tobytes() == rec.tobytes()
    out = check_filter(ctx, rec, np.ones((H, W), bool))
    assert out.numel() == 0
    for shift in (1, 3, 8):
        big = torch.zeros(shift + n * 25, dtype=torch.uint8, device="cuda")
        big[shift:] = torch.from_numpy(rec).cuda()
        view = big[shift:]
        assert view.data_ptr() % 16 == shift and view.is_contiguous()
        counts, _ = ctx.pixel_activity(view, W, H)
        assert (counts.cpu().numpy() == HP.count_events(rec, W, H)[0]).all()
        check_filter(ctx, rec, rng.random((H, W)) < 0.3, events=view)


def test_refusals(ctx):
    import torch
    from eventcalib_amd import capi
    rec = torch.zeros(25, dtype=torch.uint8, device="cuda")
    out = torch.zeros(25, dtype=torch.uint8, device="cuda")
    mask = torch.zeros(16, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    for W, H in ((0, 4), (4, 0), (4097, 1), (1, 4097)):
        with pytest.raises(capi.EcalError) as e:
            ctx.pixel_activity_dev(rec.data_ptr(), 1, W, H, cnt.data_ptr())
        assert e.value.status == -1
        with pytest.raises(capi.EcalError) as e:
            ctx.filter_events_dev(rec.data_ptr(), 1, mask.data_ptr(), W, H, out.data_ptr(), cnt.data_ptr())
        assert e.value.status == -1
    for call in (lambda: ctx.pixel_activity_dev(rec.data_ptr(), 1 << 32, 4, 4, cnt.data_ptr()),
                 lambda: ctx.filter_events_dev(rec.data_ptr(), 1 << 32, mask.data_ptr(), 4, 4, out.data_ptr(), cnt.data_ptr())):
        with pytest.raises(capi.EcalError) as e:
            call()
        assert e.value.status == -6
    with pytest.raises(capi.EcalError) as e:   # the output may not overlap the events
        ctx.filter_events_dev(rec.data_ptr(), 1, mask.data_ptr(), 4, 4, rec.data_ptr(), cnt.data_ptr())
    assert e.value.status == -1
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def dirty_hover():
    import synth_stream as SS
    clean = SS.make_stream(60000, device="cpu", seed=3).numpy()
    dirty, where, _ = HP.inject_hot_pixels(clean, 346, 260, n_pixels=5, per_pixel=2000)
    return clean, dirty, where


def test_remove_hot_pixels_equals_the_oracle_chain(ctx, dirty_hover):
    import torch
    clean, dirty, where = dirty_hover
    want, want_info = HP.remove_hot_pixels(dirty, 346, 260)
    assert want.tobytes() == clean.tobytes() and want_info["n_hot_pixels"] == 5
    for chain in (lambda **kw: ctx.remove_hot_pixels(torch.from_numpy(dirty), **kw), lambda **kw: ctx.stream_remove_hot_pixels(dirty, **kw)):
        out, info = chain()
        assert out.cpu().numpy().tobytes() == want.tobytes()
        assert (info["mask"] == want_info["mask"]).all() and (info["counts"] == want_info["counts"]).all()
        assert {k: v for k, v in info.items() if k not in ("mask", "counts")} == {k: v for k, v in want_info.items() if k not in ("mask", "counts")}
        ys, xs = np.nonzero(info["mask"])
        assert sorted(zip(xs.tolist(), ys.tolist())) == sorted(where)
        # other options and an extra mask: still the oracle's chain
        extra = np.zeros((260, 346), bool)
        extra[100:140, 150:200] = True
        opts = dict(quantile_permille=500, min_count=10, factor=3.0)
        out, info = chain(extra_mask=extra, **opts)
        want2, want2_info = HP.remove_hot_pixels(dirty, 346, 260, extra_mask=extra, **opts)
        assert out.cpu().numpy().tobytes() == want2.tobytes() and (info["mask"] == want2_info["mask"]).all()
        assert info["n_removed"] == want2_info["n_removed"] > want_info["n_removed"] and info["n_masked_pixels"] == want2_info["n_masked_pixels"]


def test_a_sorted_stream_stays_sorted(ctx, dirty_hover):
    import torch
    _, dirty, _ = dirty_hover
    rng = np.random.default_rng(2)
    out, _ = ctx.filter_events(torch.from_numpy(dirty), rng.random((260, 346)) < 0.5)
    n = out.numel() // 25
    assert 0 < n < dirty.size // 25
    t = HP.fields(out.cpu().numpy())[0]
    assert (np.diff(t) >= 0).all() and (np.diff(t) == 0).any()
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    own = out.clone()   # (a tensor of its own: the check may read the spare bytes a library-owned stream has)
    own = torch.cat([own, torch.zeros(16, dtype=torch.uint8, device="cuda")])
    ctx.check_sorted_dev(own.data_ptr(), n, flag.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
