"""The numpy oracle of the hot-pixel filter (include/ecal.h, "pixel activity / hot pixels"): the pixel of a record, the count map,
the rule restated bit for bit, the order-preserving filter, their chain — and the injection of hot pixels into a clean stream that
the tests of the filter share.  Records are numpy uint8 arrays of packed 25-byte events (f64 t, f64 x, f64 y, u8 polarity)."""
import numpy as np

RECORD = 25
DEFAULTS = dict(quantile_permille=990, min_count=64, factor=8.0)


def _records(rec):
    a = np.ascontiguousarray(np.asarray(rec, np.uint8).ravel())
    assert a.size % RECORD == 0
    return a.reshape(-1, RECORD)


def fields(rec):
    """(t, x, y float64 [n], polarity byte uint8 [n])"""
    a = _records(rec)
    f = np.ascontiguousarray(a[:, :24]).view("<f8").reshape(-1, 3)
    return f[:, 0].copy(), f[:, 1].copy(), f[:, 2].copy(), a[:, 24].copy()


def pixels(rec, width, height):
    """(on_grid bool [n], pixel index int64 [n], -1 where off the grid): v is on the grid iff v >= 0 and v < n and v == floor(v)"""
    _, x, y, _ = fields(rec)
    with np.errstate(invalid="ignore"):
        on = (x >= 0) & (x < width) & (x == np.floor(x)) & (y >= 0) & (y < height) & (y == np.floor(y))
    idx = np.full(x.shape, -1, np.int64)
    idx[on] = y[on].astype(np.int64) * width + x[on].astype(np.int64)
    return on, idx


def count_events(rec, width, height):
    """(counts [2, H, W] uint32 — plane 1: polarity byte != 0 —, totals dict)"""
    on, idx = pixels(rec, width, height)
    plane = width * height
    pol = (_records(rec)[:, 24] != 0).astype(np.int64)
    counts = np.bincount(pol[on] * plane + idx[on], minlength=2 * plane).astype(np.uint32).reshape(2, height, width)
    return counts, dict(n_events=int(on.size), n_on_grid=int(on.sum()), n_off_grid=int(on.size - on.sum()))


def hot_mask(counts, extra_mask=None, quantile_permille=990, min_count=64, factor=8.0):
    """the rule: c = counts[0] + counts[1]; A = sorted non-zero c; Q = A[((len(A) - 1) * quantile_permille) // 1000] (0 when A is
    empty: nothing is hot); hot iff c >= min_count and float64(c) > factor * float64(Q); mask = hot | extra_mask.
    -> (mask [H, W] bool, info dict; its event fields speak of the counted events alone)"""
    c = counts[0].astype(np.uint64) + counts[1].astype(np.uint64)
    A = np.sort(c[c > 0], kind="stable")
    Q = int(A[((len(A) - 1) * int(quantile_permille)) // 1000]) if len(A) else 0
    hot = (c >= np.uint64(min_count)) & (c.astype(np.float64) > np.float64(factor) * np.float64(Q)) if len(A) else np.zeros(c.shape, bool)
    mask = hot | (np.asarray(extra_mask) != 0) if extra_mask is not None else hot.copy()
    sat = lambda v: min(int(v), 0xFFFFFFFF)   # noqa: E731
    removed = int(c[mask].sum())
    info = dict(n_events=int(c.sum()), n_off_grid=0, n_removed=removed, n_kept=int(c.sum()) - removed, n_active_pixels=sat(len(A)),
                n_hot_pixels=sat(hot.sum()), n_masked_pixels=sat(mask.sum()), quantile_count=sat(Q), max_count=sat(c.max() if c.size else 0),
                max_kept_count=sat(c[~mask].max() if (~mask).any() else 0))
    return mask, info


def filter_events(rec, mask):
    """(kept records uint8 [n_kept * 25] in input order, totals dict): removed iff on the grid and the pixel is masked"""
    mask = np.asarray(mask) != 0
    height, width = mask.shape
    on, idx = pixels(rec, width, height)
    remove = np.zeros(on.shape, bool)
    remove[on] = mask.ravel()[idx[on]]
    a = _records(rec)
    out = np.ascontiguousarray(a[~remove]).ravel()
    return out, dict(n_events=int(on.size), n_off_grid=int(on.size - on.sum()), n_removed=int(remove.sum()), n_kept=int(on.size - remove.sum()))


def remove_hot_pixels(rec, width=346, height=260, extra_mask=None, **options):
    """the chain: (kept records, info dict with `mask` and `counts`; the event fields are the filter's totals)"""
    counts, _ = count_events(rec, width, height)
    mask, info = hot_mask(counts, extra_mask=extra_mask, **options)
    out, tot = filter_events(rec, mask)
    info.update(tot)
    info["mask"], info["counts"] = mask, counts
    return out, info


def ratio_max_to_quantile(counts, quantile_permille=990):
    """the largest per-pixel count over the quantile of the non-zero counts (where the default factor comes from)"""
    c = counts[0].astype(np.uint64) + counts[1].astype(np.uint64)
    A = np.sort(c[c > 0])
    return float(A[-1]) / float(A[((len(A) - 1) * quantile_permille) // 1000])


def inject_hot_pixels(clean, width, height, n_pixels=5, per_pixel=10000):
    """Hot pixels at the first n_pixels pixels in row-major order that the clean stream never touches, each firing per_pixel events at
    even spacing from the stream's first to its last stamp with alternating polarity, merged by a stable sort on time with the clean
    event first on ties.  -> (dirty records uint8, the pixels as [(x, y)], per-pixel counts [(negative, positive)])"""
    a = _records(clean)
    t, _, _, _ = fields(clean)
    counts, _ = count_events(clean, width, height)
    free = np.flatnonzero((counts[0].astype(np.uint64) + counts[1]).ravel() == 0)[:n_pixels]
    assert len(free) == n_pixels, "the clean stream touches every pixel"
    where = [(int(p % width), int(p // width)) for p in free]
    ts = np.linspace(t[0], t[-1], per_pixel)
    pol = (np.arange(per_pixel) % 2).astype(np.uint8)
    parts = [a]
    for x, y in where:
        r = np.zeros((per_pixel, RECORD), np.uint8)
        r[:, :24] = np.stack([ts, np.full(per_pixel, float(x)), np.full(per_pixel, float(y))], axis=1).astype("<f8").view(np.uint8).reshape(per_pixel, 24)
        r[:, 24] = pol
        parts.append(r)
    both = np.concatenate(parts)
    order = np.argsort(np.concatenate([t] + [ts] * n_pixels), kind="stable")   # (clean first, then the pixels in their order, on ties)
    per = (int((pol == 0).sum()), int((pol != 0).sum()))
    return np.ascontiguousarray(both[order]).ravel(), where, [per] * n_pixels
