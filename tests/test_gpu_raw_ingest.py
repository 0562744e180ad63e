"""GPU: the raw ingest (include/ecal.h "raw ingest"; eventcalib_amd/csrc/ecal_raw.hip) — Prophesee EVT3 / EVT2 payloads decoded in
HBM into packed 25-byte records — against `oracle` below: a sequential Python decoder that restates the contract with its state in
plain variables (nothing of raw_events.hpp's summaries), byte for byte, the info fields included.  No tolerance anywhere.
The encoders of this file build the cases; B = ecal_raw_block_words(format) places them on the decode blocks' boundaries."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import eventcalib_amd
from eventcalib_amd import calibrate

pytestmark = pytest.mark.gpu

INF = float("inf")
REC = np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")])     # packed: 25 bytes
assert REC.itemsize == 25


# ---- EVT3 words ---------------------------------------------------------------------------------------------------------------------
def Y(y, bit11=0): return (0x0 << 12) | (bit11 << 11) | y
def X(x, p): return (0x2 << 12) | (p << 11) | x
def BASE(x, p): return (0x3 << 12) | (p << 11) | x
def V12(mask): return (0x4 << 12) | mask
def V8(mask, high_bits=0): return (0x5 << 12) | (high_bits << 8) | mask
def TL(v): return (0x6 << 12) | v
def TH(v): return (0x8 << 12) | v
def OTHER3(k=0): return ((0x7, 0xA, 0xE, 0xF, 0x1, 0x9, 0xB, 0xC, 0xD)[k % 9] << 12) | (k * 37 & 0xFFF)


# ---- EVT2 words ---------------------------------------------------------------------------------------------------------------------
def CD(p, low6, x, y): return (p << 28) | (low6 << 22) | (x << 11) | y
def TH2(v): return (0x8 << 28) | v
def OTHER2(k=0): return ((0xA, 0xE, 0xF, 0x2, 0x7)[k % 5] << 28) | (k * 4099 & 0x0FFFFFFF)


def payload_of(words, fmt, trailing=b""):
    return np.asarray(words, dtype="<u2" if fmt == "EVT3" else "<u4").tobytes() + trailing


def oracle(payload, fmt, time_base=0, width=0, height=0, start_time=-INF, end_time=None):
    """The contract of include/ecal.h, restated -> (the records' bytes, the info fields, the events emitted before any drop)."""
    wb = 2 if fmt == "EVT3" else 4
    n_words = len(payload) // wb
    words = np.frombuffer(payload[: n_words * wb], "<u2" if fmt == "EVT3" else "<u4").tolist()
    info = dict(n_words=n_words, n_events=0, n_no_state=0, n_outside=0, n_negative=0, n_before_start=0, n_after_end=0, n_other_words=0,
                n_trailing_bytes=len(payload) - n_words * wb, n_time_wraps=0, format=3 if fmt == "EVT3" else 2)
    kept, state = [], dict(stopped=False, raw=0)

    def event(has_state, t_us, x, y, p):
        state["raw"] += 1
        if state["stopped"]:
            info["n_after_end"] += 1
        elif not has_state:
            info["n_no_state"] += 1
        elif (width and x >= width) or (height and y >= height):
            info["n_outside"] += 1
        else:
            t = float(t_us - time_base) * 1e-6
            if t < 0:
                info["n_negative"] += 1
            elif end_time is not None and t >= end_time:
                state["stopped"] = True
                info["n_after_end"] += 1
            elif t >= start_time:
                kept.append((t, float(x), float(y), p))
            else:
                info["n_before_start"] += 1

    if fmt == "EVT3":
        y = high = base_x = None
        low = vpol = wraps = 0
        for w in words:
            typ = w >> 12
            t_us = (wraps << 24) | ((high or 0) << 12) | low
            timed = high is not None and y is not None
            if typ == 0x0:
                y = w & 0x7FF
            elif typ == 0x2:
                event(timed, t_us, w & 0x7FF, y, (w >> 11) & 1)
            elif typ == 0x3:
                base_x, vpol = w & 0x7FF, (w >> 11) & 1
            elif typ in (0x4, 0x5):
                n = 12 if typ == 0x4 else 8
                for i in range(n):
                    if w >> i & 1:
                        event(timed and base_x is not None, t_us, (base_x or 0) + i, y, vpol)
                if base_x is not None:
                    base_x += n
            elif typ == 0x6:
                low = w & 0xFFF
            elif typ == 0x8:
                q = w & 0xFFF
                if high is not None and q < high and high - q > 2048:
                    wraps += 1
                high = q
            else:
                info["n_other_words"] += 1
        info["n_time_wraps"] = wraps
    else:
        high = None
        for w in words:
            typ = w >> 28
            if typ <= 1:
                event(high is not None, ((high or 0) << 6) | ((w >> 22) & 0x3F), (w >> 11) & 0x7FF, w & 0x7FF, typ)
            elif typ == 0x8:
                high = w & 0x0FFFFFFF
            else:
                info["n_other_words"] += 1
    info["n_events"] = len(kept)
    return np.array(kept, dtype=REC).tobytes(), info, state["raw"]


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def B(ctx):
    b = {"EVT3": ctx.raw_block_words("EVT3"), "EVT2": ctx.raw_block_words("EVT2")}
    assert b["EVT3"] >= 64 and b["EVT2"] >= 64 and ctx.raw_block_words(7) == 0
    return b


def check(ctx, payload, fmt, **opts):
    """decode on the device, compare everything with the oracle -> (records, info)"""
    want, want_info, n_raw = oracle(payload, fmt, **opts)
    got, info = ctx.events_from_raw(payload, fmt, **opts)
    torch.cuda.synchronize()
    data = got.cpu().numpy().tobytes()
    assert {k: info[k] for k in want_info} == want_info
    assert data == want
    assert info["header_bytes"] == 0
    assert ctx.raw_count_events(payload, fmt) == n_raw
    assert sum(info[k] for k in ("n_events", "n_no_state", "n_outside", "n_negative", "n_before_start", "n_after_end")) == n_raw
    return data, info


def random_words(fmt, n, seed, many_highs=False):
    """n seeded random words: all types, the skipped ones among them; TIME_HIGH steps forward with wraps, jumps and backward steps"""
    rng = np.random.default_rng(seed)
    if fmt == "EVT3":
        types = np.array([0x0, 0x2, 0x3, 0x4, 0x5, 0x6, 0x8, 0x7, 0xA, 0xE, 0xF, 0x1, 0x9])
        p = np.array([8, 30, 6, 12, 10, 10, 30 if many_highs else 4, 1, 1, 1, 1, 1, 1], float)
        typ = rng.choice(types, size=n, p=p / p.sum())
        val = rng.integers(0, 4096, size=n)
        th = np.flatnonzero(typ == 0x8)
        step = rng.integers(0, 60, size=len(th))
        kind = rng.integers(0, 20, size=len(th))
        step = np.where(kind == 0, rng.integers(0, 4096, size=len(th)), step)        # a jump
        step = np.where(kind == 1, 4096 - 2048, step)                                 # back by exactly 2048 (mod 4096: also forward)
        step = np.where(kind == 2, 4096 - 30, step)                                   # a small backward step
        val[th] = (1000 + np.cumsum(step)) % 4096
        return ((typ << 12) | val).astype("<u2").tolist()
    types = np.array([0x0, 0x1, 0x8, 0xA, 0xE, 0xF, 0x2, 0x7])
    p = np.array([40, 40, 30 if many_highs else 5, 1, 1, 1, 1, 1], float)
    typ = rng.choice(types, size=n, p=p / p.sum()).astype(np.uint64)
    val = rng.integers(0, 1 << 28, size=n).astype(np.uint64)
    th = np.flatnonzero(typ == 0x8)
    val[th] = (5000 + np.cumsum(rng.integers(0, 3, size=len(th)))).astype(np.uint64)
    return ((typ << np.uint64(28)) | val).astype("<u4").tolist()


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["EVT3", "EVT2"])
def test_sizes_around_the_block_and_trailing_bytes(ctx, B, fmt):
    b = B[fmt]
    head = [Y(5), TH(7), TL(9), BASE(100, 1)] if fmt == "EVT3" else [TH2(77)]
    for n in (0, 1, b - 1, b, b + 1, 3 * b + 5):
        words = (head + random_words(fmt, n, 100 + n))[:n]
        tails = (b"", b"\x21") if fmt == "EVT3" else (b"", b"\x21", b"\x21\x43", b"\x21\x43\x65")
        for tail in tails:
            _, info = check(ctx, payload_of(words, fmt, tail), fmt)
            assert info["n_words"] == n and info["n_trailing_bytes"] == len(tail)
    # a device tensor whose bytes sit in front of other words: nothing behind n_bytes is read (it would show as records)
    words = head + [X(3, 1) if fmt == "EVT3" else CD(1, 2, 3, 4)] * 10
    poison = [X(9, 0) if fmt == "EVT3" else CD(0, 1, 9, 9)] * 64
    whole = torch.from_numpy(np.frombuffer(payload_of(words + poison, fmt), np.uint8).copy()).cuda()
    view = whole[: len(payload_of(words, fmt))]
    got, info = ctx.events_from_raw(view, fmt)
    assert info["n_events"] == 10 and got.cpu().numpy().tobytes() == oracle(payload_of(words, fmt), fmt)[0]


# ---- state across blocks ----------------------------------------------------------------------------------------------------------
def test_state_is_carried_through_a_block_with_an_empty_summary(ctx, B):
    b = B["EVT3"]
    block0 = [Y(123), TH(17), TL(1234), BASE(600, 1)] + [OTHER3(k) for k in range(b - 4)]
    block1 = [OTHER3(k) for k in range(b)]
    block2 = [X(10, 1), V12(0b101000000101), X(11, 0), V8(0b10000001, high_bits=0xF), V12(0xFFF), X(345, 1)]
    data, info = check(ctx, payload_of(block0 + block1 + block2, "EVT3"), "EVT3")
    assert info["n_events"] == 1 + 4 + 1 + 2 + 12 + 1 and info["n_no_state"] == 0 and info["n_other_words"] == 2 * b - 4
    rec = np.frombuffer(data, REC)
    assert (rec["t"] == float((17 << 12) | 1234) * 1e-6).all() and (rec["y"] == 123.0).all()
    assert rec["x"][1:5].tolist() == [600.0, 602.0, 609.0, 611.0] and rec["x"][6:8].tolist() == [612.0, 619.0] and rec["x"][8] == 620.0
    # the same for EVT2: the TIME_HIGH in block 0, a block of other words, the events in block 2
    b = B["EVT2"]
    words = [TH2(123456)] + [OTHER2(k) for k in range(2 * b - 1)] + [CD(1, 63, 1279, 719), CD(0, 0, 0, 0)]
    data, info = check(ctx, payload_of(words, "EVT2"), "EVT2")
    assert info["n_events"] == 2 and np.frombuffer(data, REC)["t"].tolist() == [float((123456 << 6) | 63) * 1e-6, float(123456 << 6) * 1e-6]


def test_a_vector_run_advances_its_base_across_blocks(ctx, B):
    b = B["EVT3"]
    rng = np.random.default_rng(5)
    n_vec = 2 * b + 300
    vec = [V12(int(m)) if k else V8(int(m) & 0xFF, high_bits=int(m) >> 8) for m, k in zip(rng.integers(0, 4096, n_vec), rng.integers(0, 2, n_vec))]
    words = [Y(9), TH(3), BASE(7, 0)] + vec
    words[b - 1] = V12(0xFFF)          # all ones as the last word of a block
    words[2 * b - 1] = V12(0xFFF)
    words.append(V12(0xFFF))           # ... and as the last word of the file
    data, info = check(ctx, payload_of(words, "EVT3"), "EVT3")
    rec = np.frombuffer(data, REC)
    assert info["n_no_state"] == 0 and len(rec) > 8 * b
    advance = sum(12 if (w >> 12) == 0x4 else 8 for w in words[3:-1])
    assert rec["x"][-12:].tolist() == [float(7 + advance + i) for i in range(12)] and 7 + advance > 2047


# ---- time wraps ----------------------------------------------------------------------------------------------------------------------
def test_time_wraps(ctx, B):
    b = B["EVT3"]
    pre = [Y(1), TL(5)]

    def fill(words, n):
        return words + [OTHER3(k) for k in range(n - len(words))]
    cases = {
        # p at the last word of block 0, q at the first word of block 1
        "split_across_blocks": (fill(pre + [TH(100), X(1, 1)], b - 1) + [TH(4000), TH(10), X(2, 1), TH(11), X(3, 0)], 1),
        "inside_a_block": (pre + [TH(3000), X(1, 1), TH(100), X(2, 1)], 1),
        "two_in_one_block": (fill(pre, b) + [TH(4095), X(1, 1), TH(0), X(2, 1), TH(3000), TH(5), X(3, 1)], 2),
        "back_by_2048_is_no_wrap": (pre + [TH(3000), X(1, 1), TH(952), X(2, 1)], 0),
        "back_by_2049_is_a_wrap": (pre + [TH(3000), X(1, 1), TH(951), X(2, 1)], 1),
        "repeated_value": (pre + [TH(3000), TH(3000), X(1, 1), TH(3000), X(2, 1)], 0),
        # the carry of `last` through a block without TIME_HIGH, and wraps of two blocks adding up
        "through_an_empty_block": (fill(pre + [TH(4000), X(1, 1)], b) + fill([], b) + [TH(1), X(2, 1)] + fill([], b - 2) + [TH(4090), TH(3), X(3, 1)], 2),
    }
    for name, (words, wraps) in cases.items():
        data, info = check(ctx, payload_of(words, "EVT3"), "EVT3")
        print(name, info)
        assert info["n_time_wraps"] == wraps, name
        t = np.frombuffer(data, REC)["t"]
        if name == "back_by_2048_is_no_wrap":
            assert t[1] < t[0]                     # time runs backwards and is taken as is
        if wraps and name != "two_in_one_block":
            assert t[-1] >= float(1 << 24) * 1e-6


# ---- no state ------------------------------------------------------------------------------------------------------------------------
def test_events_without_state_are_dropped_and_counted(ctx, B):
    b = B["EVT3"]
    # ADDR_Y and the base in block 0, the first TIME_HIGH only in block 1: everything emitted before it is dropped
    block0 = [X(1, 1), V12(0b11), Y(4), X(2, 1), BASE(50, 1), V8(0b111)] + [OTHER3(k) for k in range(b - 6)]
    block1 = [X(3, 0), V12(0b1), TH(9), X(4, 1), V12(0b1001)]
    data, info = check(ctx, payload_of(block0 + block1, "EVT3"), "EVT3")
    assert info["n_no_state"] == 1 + 2 + 1 + 3 + 1 + 1 and info["n_events"] == 3
    assert np.frombuffer(data, REC)["x"].tolist() == [4.0, 50.0 + 8 + 12, 50.0 + 8 + 12 + 3]   # the dropped vectors advanced the base
    # time known, no ADDR_Y yet; then vectors without a base (they advance nothing: the first base stands as it is set)
    words = [TH(1), X(1, 1), V12(0xF), Y(2), X(5, 0), V12(0xF), V8(0x3), BASE(10, 0), V12(0b1)]
    data, info = check(ctx, payload_of(words, "EVT3"), "EVT3")
    assert info["n_no_state"] == 1 + 4 + 4 + 2 and np.frombuffer(data, REC)["x"].tolist() == [5.0, 10.0]
    # EVT2: events before the first TIME_HIGH, which sits in block 1
    b = B["EVT2"]
    words = [CD(1, 1, 2, 3)] * 5 + [OTHER2(k) for k in range(b)] + [CD(0, 1, 2, 3), TH2(4), CD(1, 1, 2, 3)]
    _, info = check(ctx, payload_of(words, "EVT2"), "EVT2")
    assert info["n_no_state"] == 6 and info["n_events"] == 1


# ---- filters -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["EVT3", "EVT2"])
def test_filters(ctx, B, fmt):
    b = B[fmt]
    words = random_words(fmt, 3 * b + 17, 31)
    if fmt == "EVT3":
        words[:4] = [Y(100), TH(1000), TL(0), BASE(300, 1)]
        t0 = 1000 << 12
    else:
        words[0] = TH2(5000)
        t0 = 5000 << 6
    payload = payload_of(words, fmt)
    _, base_info = check(ctx, payload, fmt)
    _, info = check(ctx, payload, fmt, width=640, height=480)
    assert 0 < info["n_outside"] < base_info["n_events"]
    _, info = check(ctx, payload, fmt, time_base=t0 + (200 if fmt == "EVT2" else 200000))
    assert info["n_negative"] > 0 and info["n_events"] > 0
    _, info = check(ctx, payload, fmt, time_base=t0, start_time=1e-4 if fmt == "EVT2" else 0.1)
    assert info["n_before_start"] > 0 and info["n_events"] > 0
    # the end time is first reached in a later block than the first; time runs backwards behind it (the random TIME_HIGH steps), and
    # nothing behind the offender may appear
    recs = np.frombuffer(oracle(payload, fmt, time_base=t0)[0], REC)
    half = len(recs) // 2
    t_end = float(np.nextafter(recs["t"][:half].max(), INF))                 # not reached by the first half of the records
    data, info = check(ctx, payload, fmt, time_base=t0, end_time=t_end)
    first = int(np.flatnonzero(recs["t"] >= t_end)[0])
    assert info["n_events"] == first >= half and info["n_after_end"] > 0
    assert first > oracle(payload[: b * (2 if fmt == "EVT3" else 4)], fmt)[2]  # more than block 0 emits: the offender sits in a later block
    check(ctx, payload, fmt, time_base=t0, start_time=t_end / 2, end_time=t_end, width=1000, height=1500)
    _, info = check(ctx, payload, fmt, time_base=t0, end_time=0.0)       # the very first timed event ends the stream
    assert info["n_events"] == 0
    # time runs backwards behind the offender: block 0 at time high 10, in block 1 the steps 20, 30 (the offender) and back to 15
    th, ev = (TH, lambda k: X(k % 640, k & 1)) if fmt == "EVT3" else (TH2, lambda k: CD(k & 1, 0, k % 640, 7))
    words = ([Y(7), TL(0)] if fmt == "EVT3" else []) + [th(10)]
    words += [ev(k) for k in range(b - len(words))] + [th(20)] + [ev(k) for k in range(50)] + [th(30)] + [ev(k) for k in range(5)] + [th(15)]
    words += [ev(k) for k in range(3 * b - len(words))]
    unit = 1 << (12 if fmt == "EVT3" else 6)
    data, info = check(ctx, payload_of(words, fmt), fmt, end_time=25 * unit * 1e-6)
    n_before = b - (3 if fmt == "EVT3" else 1) + 50
    assert info["n_events"] == n_before and info["n_after_end"] == 3 * b - (6 if fmt == "EVT3" else 4) - n_before
    assert np.frombuffer(data, REC)["t"].max() == 20 * unit * 1e-6


def test_capacity(ctx, B):
    for fmt in ("EVT3", "EVT2"):
        payload = payload_of(random_words(fmt, 2 * B[fmt] + 9, 8), fmt)
        want, want_info, n_raw = oracle(payload, fmt)
        n = want_info["n_events"]
        assert 0 < n < n_raw                     # (events without state at the start: the kept count is below the emitted one)
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.events_from_raw(payload, fmt, capacity=n - 1)
        assert e.value.status == -6 and e.value.info["n_events"] == n
        got, info = ctx.events_from_raw(payload, fmt, capacity=n)
        assert got.cpu().numpy().tobytes() == want and info["n_events"] == n
        assert ctx.raw_count_events(payload, fmt) == n_raw
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.events_from_raw(payload, fmt, capacity=0)
        assert e.value.status == -6
    with pytest.raises(eventcalib_amd.EcalError) as e:      # the _dev form wants an explicit format
        ctx.events_from_raw(payload, None, capacity=10)
    assert e.value.status == -1


# ---- random streams --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["EVT3", "EVT2"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_streams_of_300k_words(ctx, fmt, seed):
    words = random_words(fmt, 300000 + 1111 * seed, seed, many_highs=seed == 3)
    opts = [{}, {"width": 1280, "height": 720, "time_base": 3000}, {"time_base": 0, "start_time": 0.002, "end_time": 10000.0 if fmt == "EVT3" else 4.0}][seed - 1]
    _, info = check(ctx, payload_of(words, fmt, b"\x07" if seed == 2 else b""), fmt, **opts)
    print(fmt, seed, info)
    assert info["n_events"] > 50000 and info["n_other_words"] > 1000 and (seed != 3 or info["n_after_end"] > 1000)
    assert fmt == "EVT2" or info["n_time_wraps"] > 10


# ---- files -----------------------------------------------------------------------------------------------------------------------------
def encode(fmt, t_us, x, y, p):
    """events (int64 microseconds, integer x / y, polarity) as payload bytes: a state word wherever a piece of state changes"""
    t_us, x, y, p = (np.asarray(a, np.int64) for a in (t_us, x, y, p))
    n = len(t_us)

    def changed(v):
        return np.concatenate([[True], v[1:] != v[:-1]]) if n else np.zeros(0, bool)
    if fmt == "EVT3":
        parts = [(changed((t_us >> 12) & 0xFFF), (0x8 << 12) | ((t_us >> 12) & 0xFFF)), (changed(t_us & 0xFFF), (0x6 << 12) | (t_us & 0xFFF)),
                 (changed(y), y), (np.ones(n, bool), (0x2 << 12) | (p << 11) | x)]
        dt = "<u2"
    else:
        parts = [(changed(t_us >> 6), (0x8 << 28) | (t_us >> 6)), (np.ones(n, bool), (p << 28) | ((t_us & 0x3F) << 22) | (x << 11) | y)]
        dt = "<u4"
    count = sum(m.astype(np.int64) for m, _ in parts) if n else np.zeros(0, np.int64)
    at = np.cumsum(count) - count
    out = np.zeros(int(count.sum()), np.int64)
    for m, w in parts:
        out[at[m]] = w[m]
        at = at + m
    return out.astype(dt).tobytes()


@pytest.fixture(scope="module")
def synthetic():
    """200 000 events of the synthetic calibration stream, times quantised to integer microseconds -> (t_us, x, y, p, .bin bytes)"""
    import synth_stream as SS
    t, xy, pol = SS.unpack_records(SS.make_stream(200000, device="cpu", seed=3))
    t_us = torch.round(t * 1e6).to(torch.int64)
    records = SS.pack_records(t_us.to(torch.float64) * 1e-6, xy, pol).numpy().tobytes()      # t = (double)(t_us - 0) * 1e-6
    return t_us.numpy(), xy[:, 0].to(torch.int64).numpy(), xy[:, 1].to(torch.int64).numpy(), pol.to(torch.int64).numpy(), records


def load_bin(ctx, path):
    L = ctx._L
    vp = ctypes.c_void_p
    h = vp()
    assert L.ecal_stream_create_from_file(ctx._h, os.fsencode(path), -INF, 0, 0.0, ctypes.byref(h)) == 0
    return ctx._stream_records(h)


@pytest.mark.parametrize("fmt,header", [("EVT3", b"% date 2024-01-01\n% evt 3.0\n% geometry 640x480\n% end\n"),
                                        ("EVT2", b"% format EVT2;height=480;width=640\n% end\n")])
def test_round_trip_through_a_file(ctx, tmp_path, synthetic, fmt, header):
    t_us, x, y, p, records = synthetic
    payload = encode(fmt, t_us, x, y, p)
    raw, binf = str(tmp_path / "events.raw"), str(tmp_path / "events.bin")
    open(raw, "wb").write(header + payload)
    open(binf, "wb").write(records)
    ev, info, t_first, t_last = ctx.stream_from_raw_file(raw)
    assert ev.cpu().numpy().tobytes() == records
    assert info["n_events"] == 200000 and info["header_bytes"] == len(header) and info["format"] == int(fmt[-1])
    assert info["n_words"] == len(payload) // (2 if fmt == "EVT3" else 4) and info["n_no_state"] == 0
    assert struct.pack("<dd", t_first, t_last) == records[:8] + records[-25:-17]
    info2 = ctx.raw_to_bin(raw, str(tmp_path / "by_library.bin"))
    assert open(str(tmp_path / "by_library.bin"), "rb").read() == records and info2 == info
    events, t0, t1 = calibrate.load_events_raw(ctx, raw)
    want, w0, w1 = load_bin(ctx, binf)
    assert torch.equal(events, want) and (t0, t1) == (w0, w1)
    # blocks of time shuffled: the file forms' difference — raw_to_bin keeps the file order, the stream sorts (stable)
    cuts = [0, 30000, 71000, 90001, 140000, 200000]
    order = [3, 0, 4, 2, 1]
    idx = np.concatenate([np.arange(cuts[k], cuts[k + 1]) for k in order])
    open(raw, "wb").write(header + encode(fmt, t_us[idx], x[idx], y[idx], p[idx]))
    shuffled = np.frombuffer(records, REC)[idx]
    ev, info, _, _ = ctx.stream_from_raw_file(raw)
    assert info["n_events"] == 200000 and info["n_time_wraps"] == 0
    assert ev.cpu().numpy().tobytes() == shuffled[np.argsort(shuffled["t"], kind="stable")].tobytes()
    ctx.raw_to_bin(raw, str(tmp_path / "shuffled.bin"))
    assert open(str(tmp_path / "shuffled.bin"), "rb").read() == shuffled.tobytes()


def test_headers(ctx, tmp_path):
    words3 = [Y(1), TH(2), TL(3), X(4, 1), X(5, 0)]
    p3, p2 = payload_of(words3, "EVT3"), payload_of([TH2(9), CD(1, 2, 3, 4)], "EVT2")
    want3, want2 = oracle(p3, "EVT3")[0], oracle(p2, "EVT2")[0]
    path = str(tmp_path / "h.raw")

    def load(data, **opts):
        open(path, "wb").write(data)
        ev, info, _, _ = ctx.stream_from_raw_file(path, **opts)
        return ev.cpu().numpy().tobytes(), info
    for header, payload, want, fmt in [(b"% evt 3.0\n", p3, want3, 3), (b"% evt 2.0\n", p2, want2, 2), (b"% format EVT3\n", p3, want3, 3),
                                       (b"% format EVT2\n", p2, want2, 2), (b"% format EVT3;height=720;width=1280\n% end\n", p3, want3, 3),
                                       (b"% camera_integrator_name Prophesee\n% format EVT2;x=1\n% plugin_name p\n", p2, want2, 2),
                                       (b"% evt 3.0", b"", b"", 3)]:
        got, info = load(header + payload)
        assert got == want and info["format"] == fmt and info["header_bytes"] == len(header), header
    # "% end" closes the header: payload bytes that begin with '%' stay payload ('%' = 0x25: the low byte of an ADDR_Y word)
    pct = payload_of([Y(0x25), TH(2), X(4, 1), (0x0 << 12) | 0x425, X(6, 1)], "EVT3")
    assert pct[:1] == b"%"
    got, info = load(b"% evt 3.0\n% end\n" + pct)
    assert got == oracle(pct, "EVT3")[0] and info["n_events"] == 2 and info["header_bytes"] == 16
    # an explicit format beats the header; without a header it is all there is
    got, info = load(b"% evt 2.0\n" + p3, format="EVT3")
    assert got == want3 and info["format"] == 3
    got, info = load(p2, format="EVT2")
    assert got == want2 and info["header_bytes"] == 0
    # no format anywhere
    for data in (b"% date 2024\n% end\n" + p3, p3, b""):
        open(path, "wb").write(data)
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.stream_from_raw_file(path)
        assert e.value.status == -1
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.raw_to_bin(path, str(tmp_path / "none.bin"))
        assert e.value.status == -1
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.stream_from_raw_file(str(tmp_path / "missing.raw"))
    assert e.value.status == -1
    got, info = load(b"% evt 3.0\n% end\n" + p3)      # the context is usable afterwards
    assert got == want3
