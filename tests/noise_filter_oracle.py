"""The numpy oracle of the noise filter (include/ecal.h, "noise filter"): the sequential rule restated as a plain loop — for streams
up to a few hundred thousand events —, the compaction by its verdicts, and the labelling of a synthetic stream's noise by its
`noise_frac=0.0` twin that the tests of the filter share.  Records are numpy uint8 arrays of packed 25-byte events (f64 t, f64 x,
f64 y, u8 polarity); the pixel of a record is tests/hot_pixel_oracle.py's."""
import numpy as np

import hot_pixel_oracle as HP

RECORD = 25
DEFAULTS = dict(radius=1, min_support=1, include_self=0, dt=0.005)


def verdict(rec, width=346, height=260, radius=1, min_support=1, include_self=0, dt=0.005):
    """The walk over the records in stream order with a per-pixel `last` stamp and a `seen` flag, both empty at the start.  An
    off-grid event is kept, updates nothing and supports nothing.  For an on-grid event at (X, Y) with stamp t: support = the number
    of pixels q of the square |dx| <= radius, |dy| <= radius around (X, Y), clipped to the sensor, the own pixel only with
    include_self, with seen[q] and (t - last[q]) <= dt in float64 (a NaN on either side: false); kept iff support >= min_support;
    then last[(X, Y)] = t, seen[(X, Y)] = 1, kept or not.
    -> (verdict uint8 [n]: 1 keep, 0 remove; totals dict)"""
    t = HP.fields(rec)[0].tolist()           # (python floats: IEEE f64, inf - inf = nan, comparisons with nan are false)
    on, idx = HP.pixels(rec, width, height)
    idx = idx.tolist()
    n = len(t)
    out = bytearray(n)
    last = [0.0] * (width * height)
    seen = bytearray(width * height)
    radius, min_support, dt = int(radius), int(min_support), float(dt)
    for i in range(n):
        p = idx[i]
        if p < 0:
            out[i] = 1
            continue
        ti = t[i]
        X, Y = p % width, p // width
        support = 0
        for qy in range(max(Y - radius, 0), min(Y + radius, height - 1) + 1):
            row = qy * width
            for qx in range(max(X - radius, 0), min(X + radius, width - 1) + 1):
                q = row + qx
                if q == p and not include_self:
                    continue
                if seen[q] and (ti - last[q]) <= dt:
                    support += 1
        out[i] = 1 if support >= min_support else 0
        last[p] = ti
        seen[p] = 1
    v = np.frombuffer(bytes(out), np.uint8).copy()
    kept = int(v.sum())
    return v, dict(n_events=n, n_off_grid=int(n - on.sum()), n_removed=n - kept, n_kept=kept)


def compact(rec, v):
    """the records whose verdict is non-zero, in input order: uint8 [n_kept * 25]"""
    a = np.ascontiguousarray(np.asarray(rec, np.uint8).ravel()).reshape(-1, RECORD)
    return np.ascontiguousarray(a[np.asarray(v) != 0]).ravel()


def denoise(rec, width=346, height=260, **options):
    """the chain: (kept records, totals dict)"""
    v, tot = verdict(rec, width, height, **options)
    return compact(rec, v), tot


def labelled_stream(n_events, trajectory="hover", rate=1.0e6, seed=3, t_start=5.0, noise_frac=0.1):
    """A synthetic stream (tests/synth_stream.py) with its noise labelled: noise is every record that differs from the same call
    with noise_frac=0.0 — the generator draws the same random numbers either way.  -> (records uint8, is_noise bool [n])"""
    import synth_stream as SS
    saved = SS.TRAJECTORY
    SS.TRAJECTORY = trajectory
    try:
        dirty = SS.make_stream(n_events, rate=rate, t_start=t_start, device="cpu", seed=seed, noise_frac=noise_frac).numpy()
        twin = SS.make_stream(n_events, rate=rate, t_start=t_start, device="cpu", seed=seed, noise_frac=0.0).numpy()
    finally:
        SS.TRAJECTORY = saved
    is_noise = (dirty.reshape(-1, RECORD) != twin.reshape(-1, RECORD)).any(axis=1)
    return dirty, is_noise


def quality(rec, is_noise, v, dt):
    """(signal kept, noise removed) as ratios over the events behind the first dt of the stream"""
    t = HP.fields(rec)[0]
    late = t > t[0] + dt
    v = np.asarray(v) != 0
    signal, noise = late & ~is_noise, late & is_noise
    return float(v[signal].sum()) / float(signal.sum()), float((~v[noise]).sum()) / float(noise.sum())
