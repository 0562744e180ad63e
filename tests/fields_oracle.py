"""The array ingest's rule (include/ecal.h, "array ingest") in numpy: columns -> packed 25-byte records with the filter's counters, and
records -> columns with the count of what an output type cannot hold.  numpy multiplies and converts one operation at a time (no
contraction), rounds float -> float32 to nearest and np.rint ties to even: the operations the contract names.  Written from the
contract alone; the tests hold ecal_events_from_fields_host, ecal_events_to_fields_host and the kernels to it byte for byte."""
import numpy as np

RECORD = np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")])
assert RECORD.itemsize == 25

STAMP_DTYPES = (np.uint32, np.int32, np.int64, np.float32, np.float64)
ALL_DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.int64, np.float32, np.float64)
COUNTERS = ("n_raw_events", "n_events", "n_outside", "n_negative", "n_before_start", "n_after_end")


def _is_float(a):
    return a.dtype.kind == "f"


def stamps_seconds(t, time_magnitude, time_base=0):
    t = np.asarray(t)
    if _is_float(t):
        assert time_base == 0
        return t.astype(np.float64) * np.float64(time_magnitude)
    with np.errstate(over="ignore"):
        d = t.astype(np.int64) - np.int64(time_base)       # (wraps like the C subtraction)
    return d.astype(np.float64) * np.float64(time_magnitude)


def from_fields(t, x, y, p, time_magnitude=1e-6, time_base=0, width=0, height=0, flip_x=False, flip_y=False, start_time=0.0, end_time=None):
    """-> (records as a uint8 array [n_events * 25], counters dict)"""
    t, x, y, p = (np.asarray(a) for a in (t, x, y, p))
    if t.dtype == np.bool_:
        raise ValueError("t")
    n = t.size
    xs, ys = x.astype(np.float64), y.astype(np.float64)
    outside = np.zeros(n, bool)
    if width:
        outside |= ~((xs >= 0) & (xs < float(width)))
    if height:
        outside |= ~((ys >= 0) & (ys < float(height)))
    if flip_x:
        assert width
        xs = np.float64(width - 1) - xs
    if flip_y:
        assert height
        ys = np.float64(height - 1) - ys
    ts = stamps_seconds(t, time_magnitude, time_base)
    with np.errstate(invalid="ignore"):
        negative = ~outside & ~(ts >= 0)
        reaches = ~outside & ~negative & (ts >= end_time) if end_time is not None else np.zeros(n, bool)
        first = int(np.argmax(reaches)) if reaches.any() else n
        live = np.arange(n) < first
        before = ~outside & ~negative & ~(ts >= start_time)
        keep = live & ~outside & ~negative & ~before
        pol = (p > 0) if p.dtype != np.bool_ else p
    rec = np.zeros(int(keep.sum()), RECORD)
    rec["t"], rec["x"], rec["y"], rec["p"] = ts[keep], xs[keep], ys[keep], pol[keep].astype(np.uint8)
    counts = {"n_raw_events": n, "n_events": int(keep.sum()), "n_outside": int((live & outside).sum()), "n_negative": int((live & negative).sum()),
              "n_before_start": int((live & before).sum()), "n_after_end": n - first}
    assert sum(counts[k] for k in COUNTERS[1:]) == n
    return rec.view(np.uint8).reshape(-1), counts


def records(events):
    return np.frombuffer(np.ascontiguousarray(events, np.uint8).tobytes(), RECORD)


def _int_range(dt):
    info = np.iinfo(dt)
    return int(info.min), int(info.max)


def _round_to_int64(v):
    """-> (ok, int64 values where ok): finite, within int64, rounded ties to even"""
    with np.errstate(invalid="ignore"):
        ok = (v >= -9223372036854775808.0) & (v < 9223372036854775808.0)
    r = np.zeros(v.shape, np.int64)
    r[ok] = np.rint(v[ok]).astype(np.int64)
    return ok, r


def to_fields(events, t=np.float64, xy=np.float64, p=np.uint8, ticks_per_second=1e6, time_base=0, polarity_signed=False):
    """-> ({"t", "x", "y", "p"} arrays, mask of the events that are not representable); the elements of those events are zero"""
    rec = records(events)
    n = rec.size
    bad = np.zeros(n, bool)
    out = {}
    dt = np.dtype(t)
    if dt.kind == "f":
        with np.errstate(over="ignore", invalid="ignore"):
            out["t"] = rec["t"].astype(dt)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            ok, r = _round_to_int64(rec["t"] * np.float64(ticks_per_second))
        s = np.array([int(v) + int(time_base) for v in r], dtype=object) if n else np.zeros(0, object)
        lo, hi = _int_range(dt)
        fits = np.array([lo <= v <= hi for v in s], bool) if n else np.zeros(0, bool)
        bad |= ~(ok & fits)
        out["t"] = np.array([v if g else 0 for v, g in zip(s, ok & fits)], dtype=dt) if n else np.zeros(0, dt)
    for name in ("x", "y"):
        dt = np.dtype(xy)
        v = rec[name]
        if dt.kind == "f":
            with np.errstate(over="ignore", invalid="ignore"):
                out[name] = v.astype(dt)
        else:
            ok, r = _round_to_int64(v)
            ok &= r.astype(np.float64) == v
            lo, hi = _int_range(dt)
            ok &= (r >= lo) & (r <= hi)
            bad |= ~ok
            out[name] = np.where(ok, r, 0).astype(dt)
    dt = np.dtype(p)
    pol = rec["p"] != 0
    if polarity_signed:
        assert dt.kind in "if", "a signed polarity needs a signed type"
        out["p"] = np.where(pol, 1, -1).astype(dt)
    else:
        out["p"] = pol.astype(dt)
    for name in out:
        if bad.any():
            out[name] = np.where(bad, np.zeros(1, out[name].dtype), out[name])
    return out, bad


def random_columns(rng, n, t=np.int64, x=np.uint16, y=np.uint16, p=np.uint8, width=346, height=260, t_span=4_000_000, sorted_time=True):
    """n events whose values fit every one of the nine types' common range where the type is narrow: x, y within the sensor (or the
    type's range), stamps rising from 1 000 000 ticks (seconds for a float stamp), polarity 0 / 1 (-1 / +1 in every third event of a
    signed type)"""
    def column(values, dt):
        dt = np.dtype(dt)
        if dt.kind in "iu":
            lo, hi = _int_range(dt)
            values = np.clip(values, max(lo, -2 ** 62), min(hi, 2 ** 62))
        return np.asarray(values).astype(dt)
    ticks = 1_000_000 + np.sort(rng.integers(0, t_span, n)) if sorted_time else 1_000_000 + rng.integers(0, t_span, n)
    tt = column(ticks * 1e-6, t) if np.dtype(t).kind == "f" else column(ticks, t)
    xx = column(rng.integers(0, width, n) + (rng.random(n) * 0.75 if np.dtype(x).kind == "f" else 0), x)
    yy = column(rng.integers(0, height, n) + (rng.random(n) * 0.75 if np.dtype(y).kind == "f" else 0), y)
    pol = rng.integers(0, 2, n)
    if np.dtype(p).kind in "if":
        pol = np.where((np.arange(n) % 3 == 0) & (pol == 0), -1, pol)
    return tt, xx, yy, column(pol, p)


def default_magnitude(t):
    return 1.0 if np.asarray(t).dtype.kind == "f" else 1e-6
