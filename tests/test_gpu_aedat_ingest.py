"""GPU: the AEDAT ingest (include/ecal.h "aedat ingest"; eventcalib_amd/csrc/ecal_aedat.hip) — iniVation AEDAT 3.1 / 2.0 payloads
decoded in HBM into packed 25-byte records — against `oracle` below: a sequential Python decoder that restates the contract with its
state in plain variables (nothing of aedat_events.hpp), byte for byte, the info fields and the packet table included.  No tolerance
anywhere.  The encoders of this file build the cases; B = ecal_aedat_block_events(format) places them on the decode blocks'
boundaries.  No AEDAT file of a real camera was at hand: the known answer below is assembled by hand from the contract."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import eventcalib_amd
from eventcalib_amd import calibrate, capi

pytestmark = pytest.mark.gpu

INF = float("inf")
REC = np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")])     # packed: 25 bytes
assert REC.itemsize == 25
COUNTERS = ("n_events", "n_invalid", "n_outside", "n_negative", "n_before_start", "n_after_end")


# ---- AEDAT 3.1 packets --------------------------------------------------------------------------------------------------------------
def header31(etype, source, size, ts_offset, overflow, capacity, number, valid=None):
    return struct.pack("<hhiiiiii", etype, source, size, ts_offset, overflow, capacity, number, number if valid is None else valid)


def ev(x, y, p, ts, valid=1):
    """one polarity event: (data word, stamp)"""
    return ((x << 17) | (y << 2) | (p << 1) | valid, ts)


def polarity(events, overflow=0, source=1, spare=0):
    """a polarity packet of these events; `spare` slots of capacity behind eventNumber, filled with events that must not appear"""
    body = b"".join(struct.pack("<II", d, t & 0xFFFFFFFF) for d, t in list(events) + [ev(300, 200, 1, 1)] * spare)
    return header31(1, source, 8, 4, overflow, len(events) + spare, len(events)) + body


def foreign(size, capacity, etype=2, source=1, number=None, fill=0xA5):
    """a packet of another type (frame 2, IMU 3, special 0, ...): size x capacity body bytes"""
    return header31(etype, source, size, 0, 0, capacity, capacity if number is None else number) + bytes([fill]) * (size * capacity)


def ramp(n, t0=1000, dt=3, seed=0):
    """n events on the sensor with stamps t0, t0 + dt, ..."""
    rng = np.random.default_rng(seed)
    x, y, p = rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n)
    return [ev(int(x[k]), int(y[k]), int(p[k]), t0 + dt * k) for k in range(n)]


# ---- AEDAT 2.0 records --------------------------------------------------------------------------------------------------------------
def dvs(x, y, p, ts, low=0):
    """(address, stamp) of a DVS event; `low`: bits 9..0, which mean nothing"""
    return ((y << 22) | (x << 12) | (p << 11) | (low & 0x3FF), ts & 0xFFFFFFFF)


def aps(ts, k=0): return (0x80000000 | (k * 2654435761 & 0x7FFFFFFF), ts & 0xFFFFFFFF)
def ext(ts, k=0): return ((1 << 10) | ((k * 40503 & 0x1FFFFF) << 11 & 0x7FFFF800) | (k & 0x3FF), ts & 0xFFFFFFFF)


def payload20(records, trailing=b""):
    return np.asarray(records, dtype=np.uint32).astype(">u4").tobytes() + trailing


def oracle(payload, fmt, source=-1, time_base=0, width=0, height=0, flip_x=False, flip_y=False, start_time=-INF, end_time=None):
    """The contract of include/ecal.h, restated -> (the records' bytes, the info fields, the packet table)."""
    info = dict(n_raw_events=0, n_events=0, n_invalid=0, n_outside=0, n_negative=0, n_before_start=0, n_after_end=0, n_packets=0,
                n_other_packets=0, n_records=0, n_other_records=0, n_trailing_bytes=0, n_time_wraps=0, format=31 if fmt == "3.1" else 20)
    kept, state, table = [], dict(stopped=False), []

    def event(valid, t_us, x, y, p):
        info["n_raw_events"] += 1
        if state["stopped"]:
            info["n_after_end"] += 1
        elif not valid:
            info["n_invalid"] += 1
        elif (width and x >= width) or (height and y >= height):
            info["n_outside"] += 1
        else:
            if flip_x:
                x = width - 1 - x
            if flip_y:
                y = height - 1 - y
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

    n = len(payload)
    if fmt == "3.1":
        pos = number = 0
        while pos < n:
            if n - pos < 28:
                info["n_trailing_bytes"] = n - pos
                break
            etype, src, size, ts_offset, overflow, capacity, count, valid = struct.unpack_from("<hhiiiiii", payload, pos)
            carries = etype == 1 and (source < 0 or src == source)
            if min(size, capacity, count, valid) < 0 or count > capacity or (carries and (size != 8 or ts_offset != 4)):
                raise ValueError("packet %d at byte %d" % (number, pos))
            body, length, decode = pos + 28, capacity * size, count
            cut = body + length > n
            if cut:
                whole = (n - body) // size
                decode = min(count, whole)
                info["n_trailing_bytes"] = (n - body) - whole * size
            if carries:
                info["n_packets"] += 1
                table.append((body, decode, overflow))
                for k in range(decode):
                    data, ts = struct.unpack_from("<Ii", payload, body + 8 * k)
                    event(data & 1, (overflow << 31) + (ts & 0x7FFFFFFF), data >> 17, (data >> 2) & 0x7FFF, (data >> 1) & 1)
            else:
                info["n_other_packets"] += 1
            if cut:
                break
            pos = body + length
            number += 1
    else:
        n_rec = n // 8
        info["n_records"], info["n_trailing_bytes"] = n_rec, n - 8 * n_rec
        wraps, prev = 0, None
        for r in range(n_rec):
            address, ts = struct.unpack_from(">II", payload, 8 * r)
            if prev is not None and ts < prev and prev - ts > 2 ** 31:
                wraps += 1
            prev = ts
            if address >> 31 == 0 and (address >> 10) & 1 == 0:
                event(1, (wraps << 32) | ts, (address >> 12) & 0x3FF, (address >> 22) & 0x1FF, (address >> 11) & 1)
            else:
                info["n_other_records"] += 1
        info["n_time_wraps"] = wraps
    info["n_events"] = len(kept)
    return np.array(kept, dtype=REC).tobytes(), info, np.array(table, dtype=capi.AEDAT_PACKET_DTYPE)


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def B(ctx):
    b = ctx.aedat_block_events("3.1")
    assert b >= 64 and ctx.aedat_block_events("2.0") == b and ctx.aedat_block_events(7) == 0
    return b


def test_structures_have_the_library_sizes(ctx):
    """ecal_aedat_default_options writes the whole structure: a ctypes mirror that is too short would lose its guard bytes"""
    class Guarded(ctypes.Structure):
        _fields_ = [("o", capi.AedatOptions), ("guard", ctypes.c_uint8 * 64)]
    g = Guarded()
    ctypes.memset(ctypes.byref(g), 0x5A, ctypes.sizeof(g))
    raw = ctypes.CDLL(capi.lib_path())      # (a handle of the test's own: the shared one keeps its struct-pointer prototype)
    raw.ecal_aedat_default_options.argtypes, raw.ecal_aedat_default_options.restype = [ctypes.c_void_p], None
    raw.ecal_aedat_default_options(ctypes.byref(g))
    assert bytes(g.guard) == b"\x5A" * 64 and g.o.source == -1 and g.o.format == 0 and g.o.start_time == -INF and g.o.flip_x == 0
    assert ctypes.sizeof(capi.AedatPacket) == 16 == capi.AEDAT_PACKET_DTYPE.itemsize and ctypes.sizeof(capi.AedatInfo) == 15 * 8


def check(ctx, payload, fmt, **opts):
    """index and decode on the device, compare everything with the oracle -> (records, info)"""
    want, want_info, want_table = oracle(payload, fmt, **opts)
    table = None
    dev_fields = ["n_raw_events", "n_packets", "format"] + list(COUNTERS)
    if fmt == "3.1":
        table, tinfo = ctx.aedat_index_packets(payload, source=opts.get("source", -1))
        assert table.tobytes() == want_table.tobytes()
        assert {k: tinfo[k] for k in ("n_packets", "n_other_packets", "n_raw_events", "n_trailing_bytes")} == \
               {k: want_info[k] for k in ("n_packets", "n_other_packets", "n_raw_events", "n_trailing_bytes")}
    else:
        dev_fields += ["n_records", "n_other_records", "n_trailing_bytes", "n_time_wraps"]
    got, info = ctx.events_from_aedat(payload, fmt, packets=table, **opts)
    torch.cuda.synchronize()
    data = got.cpu().numpy().tobytes()
    assert {k: info[k] for k in dev_fields} == {k: want_info[k] for k in dev_fields}
    assert data == want
    assert info["header_bytes"] == 0
    assert ctx.aedat_count_events(payload, fmt, table) == want_info["n_raw_events"] == sum(info[k] for k in COUNTERS)
    return data, info


# ---- 3.1: packet sizes and boundaries ---------------------------------------------------------------------------------------------------
def test_packet_sizes_around_the_block(ctx, B):
    sizes = (0, 1, B - 1, B, B + 1, 3 * B + 5)
    for n in sizes:                                     # each alone, with spare capacity behind eventNumber
        _, info = check(ctx, polarity(ramp(n, seed=n), spare=2), "3.1")
        assert info["n_events"] == n and info["n_packets"] == 1
    chain = b"".join(polarity(ramp(n, t0=1000 + 7 * k, seed=k), spare=k % 3) for k, n in enumerate(sizes + sizes[::-1]))
    _, info = check(ctx, chain, "3.1")
    assert info["n_events"] == 2 * sum(sizes) and info["n_packets"] == 12


def test_runs_of_one_event_packets_and_of_empty_packets_cross_a_block(ctx, B):
    ones = b"".join(polarity([ev(k % 346, k % 260, k & 1, 5000 + k)], overflow=k // 700) for k in range(B + 300))
    data, info = check(ctx, ones, "3.1")
    assert info["n_events"] == B + 300 == info["n_packets"]
    t = np.frombuffer(data, REC)["t"]
    assert t[B - 1] == float((((B - 1) // 700) << 31) + 5000 + B - 1) * 1e-6 and t[B] == float(((B // 700) << 31) + 5000 + B) * 1e-6
    # empty packets in the table exactly where the slot space crosses the block boundary, and at both ends of the chain
    empties = b"".join(polarity([], overflow=9, spare=k % 2) for k in range(70))
    chain = empties + polarity(ramp(B - 1, seed=1), overflow=1) + empties + polarity(ramp(1, seed=2), overflow=2) + empties + \
        polarity(ramp(1, seed=3), overflow=3) + empties + polarity(ramp(B + 2, seed=4), overflow=4) + empties
    data, info = check(ctx, chain, "3.1")
    assert info["n_events"] == 2 * B + 3 and info["n_packets"] == 4 + 5 * 70
    t = np.frombuffer(data, REC)["t"]
    assert [int(v * 1e6) >> 31 for v in t[[B - 2, B - 1, B, B + 1]]] == [1, 2, 3, 4]
    # nothing but empty packets
    _, info = check(ctx, empties, "3.1")
    assert info["n_events"] == 0 and info["n_packets"] == 70


def test_foreign_packets_of_odd_sizes_put_events_at_every_residue(ctx, B):
    chain = b""
    for k in range(40):
        chain += polarity(ramp(3 + k % 4, t0=100 * k, seed=k)) + foreign(7, k % 3 + 1 if k % 7 else 0, etype=(0, 2, 3, 4)[k % 4])
    chain += polarity(ramp(B + 9, t0=9000, seed=99))       # ... and a long one at an odd offset, across a block boundary
    table = oracle(chain, "3.1")[2]
    assert set((table["offset_of_first_event"] % 16).tolist()) == set(range(16))
    assert int(table["offset_of_first_event"][-1]) % 4 != 0
    _, info = check(ctx, chain, "3.1")
    assert info["n_events"] == sum(3 + k % 4 for k in range(40)) + B + 9
    # a frame-sized foreign packet between two polarity packets: 346 x 260 x 2 bytes and a few
    chain = polarity(ramp(5, seed=1)) + foreign(36 + 346 * 260 * 2 + 1, 1, fill=0x01) + polarity(ramp(B + 1, seed=2), overflow=1)
    assert len(chain) > 150000
    _, info = check(ctx, chain, "3.1")
    assert info["n_events"] == B + 6
    # the device tensor sits in front of other bytes: nothing behind n_bytes is read (the last event ends at the last byte, off
    # every alignment)
    for pad in (1, 2, 3, 5):
        part = foreign(pad, 1) + polarity(ramp(10, seed=pad))
        poison = polarity([ev(9, 9, 1, 77)] * 16)[28:]
        whole = torch.from_numpy(np.frombuffer(part + poison, np.uint8).copy()).cuda()
        table, _ = ctx.aedat_index_packets(part)
        got, info = ctx.events_from_aedat(whole[: len(part)], "3.1", packets=table)
        assert info["n_events"] == 10 and got.cpu().numpy().tobytes() == oracle(part, "3.1")[0]


# ---- 3.1: fields and counters ---------------------------------------------------------------------------------------------------------
def test_overflow_invalid_outside_flips_and_times(ctx, B):
    rng = np.random.default_rng(11)
    packets = []
    for k in range(12):
        n = int(rng.integers(1, 500))
        x, y = rng.integers(0, 400, n), rng.integers(0, 300, n)            # some outside 346 x 260
        valid = (rng.integers(0, 4, n) > 0).astype(int) if k != 5 else np.zeros(n, int)    # packet 5: none valid
        ts = np.sort(rng.integers(0, 1 << 20, n)) | (0x80000000 if k == 7 else 0)          # (bit 31 of a stamp is masked off)
        events = [ev(int(x[i]), int(y[i]), int(i & 1), int(ts[i]), int(valid[i])) for i in range(n)]
        packets.append(polarity(events, overflow=k // 4 - (1 if k == 11 else 0)))          # the overflow steps mid-file (and back)
    chain = b"".join(packets)
    data, info = check(ctx, chain, "3.1")
    assert info["n_invalid"] > 100 and info["n_outside"] == 0
    assert np.frombuffer(data, REC)["t"].max() >= float(2 << 31) * 1e-6
    _, info = check(ctx, chain, "3.1", width=346, height=260)
    assert info["n_outside"] > 100 and info["n_invalid"] > 100
    plain, _ = check(ctx, chain, "3.1", width=400, height=300)
    for fx, fy in ((True, False), (False, True), (True, True)):
        flipped, info = check(ctx, chain, "3.1", width=400, height=300, flip_x=fx, flip_y=fy)
        a, b = np.frombuffer(plain, REC), np.frombuffer(flipped, REC)
        assert (b["x"] == (399 - a["x"] if fx else a["x"])).all() and (b["y"] == (299 - a["y"] if fy else a["y"])).all()
    check(ctx, chain, "3.1", width=346, height=260, flip_x=True, flip_y=True)      # outside first, then the flip
    _, info = check(ctx, chain, "3.1", time_base=(1 << 31) + 500000)
    assert info["n_negative"] > 100 and info["n_events"] > 100
    _, info = check(ctx, chain, "3.1", time_base=1 << 31, start_time=0.5)
    assert info["n_before_start"] > 100 and info["n_negative"] > 100 and info["n_events"] > 100
    _, info = check(ctx, chain, "3.1", time_base=-(1 << 40), start_time=1.0)       # a negative base: every time far above zero
    assert info["n_negative"] == 0
    # a flip without the sensor's size is refused
    table, _ = ctx.aedat_index_packets(chain)
    for opts in (dict(flip_x=True), dict(flip_y=True, width=346), dict(flip_x=True, height=260)):
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.events_from_aedat(chain, "3.1", packets=table, **opts)
        assert e.value.status == -1


def test_source_filter(ctx):
    chain = polarity(ramp(5, seed=1), source=1) + polarity(ramp(7, seed=2), source=2) + foreign(12, 3, etype=3, source=2) + \
        header31(1, 3, 12, 8, 0, 2, 2) + b"\0" * 24 + polarity(ramp(3, seed=3), source=2)
    _, info = check(ctx, chain, "3.1", source=2)          # the odd polarity packet of source 3 is stepped over
    assert info["n_events"] == 10 and info["n_packets"] == 2
    _, info = check(ctx, chain, "3.1", source=1)
    assert info["n_events"] == 5
    with pytest.raises(eventcalib_amd.EcalError) as e:    # ... and refused when it is to carry events
        ctx.aedat_index_packets(chain)
    assert e.value.status == -1 and "packet 3 at byte %d" % (28 + 40 + 28 + 56 + 28 + 36) in str(e.value)


# ---- 3.1: the end of the stream ---------------------------------------------------------------------------------------------------------
def test_end_of_stream(ctx, B):
    # packets of 600 events, stamps k microseconds: block boundaries fall inside packets, packet boundaries inside blocks
    n, per = 3 * B + 40, 600
    x = np.arange(n) % 346

    def chain_of(ts):
        return b"".join(polarity([ev(int(x[k]), 7, k & 1, int(ts[k])) for k in range(a, min(a + per, n))]) for a in range(0, n, per))
    ts = np.arange(n) + 10
    chain = chain_of(ts)
    # the offender in the first, a middle and the last block; at a packet's first and last slot; at the first and last slot of all
    for k in (0, 5, B - 1, B, B + 3, per - 1, per, 2 * per, 3 * per - 1, 2 * B + 17, 3 * B, n - 1):
        data, info = check(ctx, chain, "3.1", end_time=float(10 + k) * 1e-6)
        assert info["n_events"] == k and info["n_after_end"] == n - k
    _, info = check(ctx, chain, "3.1", end_time=float(10 + n) * 1e-6)          # not reached
    assert info["n_events"] == n and info["n_after_end"] == 0
    # time runs backwards behind the offender: nothing behind it may appear, whatever its time
    for k in (B - 1, B + 3, 2 * per):
        back = ts.copy()
        back[k + 1:] = np.arange(n - k - 1) % 50 + 10
        data, info = check(ctx, chain_of(back), "3.1", end_time=float(10 + k) * 1e-6, start_time=19.5e-6)
        assert info["n_events"] == k - 10 and info["n_after_end"] == n - k and info["n_before_start"] == 10
    # an invalid or outside event that reaches the end time does not end the stream
    events = [ev(1, 1, 1, 10), ev(2, 2, 1, 99, valid=0), ev(400, 2, 1, 99), ev(3, 3, 0, 20), ev(4, 4, 1, 50), ev(5, 5, 1, 20)]
    data, info = check(ctx, polarity(events), "3.1", width=346, height=260, end_time=float(50) * 1e-6)
    assert (info["n_events"], info["n_invalid"], info["n_outside"], info["n_after_end"]) == (2, 1, 1, 2)


# ---- 3.1: sizes and capacity ------------------------------------------------------------------------------------------------------------
def test_capacity_and_empty_inputs(ctx, B):
    events = ramp(2 * B + 9, seed=5)
    events[3] = ev(1, 1, 1, 1012, valid=0)
    chain = polarity(events[:B + 3]) + foreign(5, 1) + polarity(events[B + 3:])
    want, want_info, table = oracle(chain, "3.1")
    n = want_info["n_events"]
    assert n == 2 * B + 8
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat(chain, "3.1", packets=table, capacity=n - 1)
    assert e.value.status == -6 and e.value.info["n_events"] == n
    got, info = ctx.events_from_aedat(chain, "3.1", packets=table, capacity=n)
    assert got.cpu().numpy().tobytes() == want and info["n_events"] == n
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat(chain, "3.1", packets=table, capacity=0)
    assert e.value.status == -6
    with pytest.raises(eventcalib_amd.EcalError) as e:      # the _dev form wants an explicit format
        ctx.events_from_aedat(chain, None, packets=table, capacity=10)
    assert e.value.status == -1
    # the indexer's capacity: the count comes back with ECAL_ERR_RANGE
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.aedat_index_packets(chain, capacity=1)
    assert e.value.status == -6 and e.value.info["n_packets"] == 2
    # zero packets (a payload of foreign packets only), zero bytes
    _, info = check(ctx, foreign(7, 3) + foreign(0, 0), "3.1")
    assert info["n_events"] == 0 and info["n_packets"] == 0
    for fmt in ("3.1", "2.0"):
        data, info = check(ctx, b"", fmt)
        assert data == b"" and info["n_events"] == 0
    # a table that does not fit the payload is refused, and nothing outside the payload is read
    bad = table.copy()
    bad["offset_of_first_event"][1] = len(chain) - 8
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat(chain, "3.1", packets=bad)
    assert e.value.status == -1
    got, info = ctx.events_from_aedat(chain, "3.1", packets=table)       # the context is usable afterwards
    assert got.cpu().numpy().tobytes() == want


def test_truncated_chains(ctx, B):
    chain = polarity(ramp(B + 5, seed=1)) + foreign(7, 3) + polarity(ramp(20, seed=2), spare=3)
    for cut in (1, 3, 8, 8 * 3 + 1, 8 * 3 + 8 * 5 + 4, 8 * 23 + 11, 8 * 23 + 28 + 9, 8 * 23 + 28 + 21 + 5):
        part = chain[: len(chain) - cut]
        _, info = check(ctx, part, "3.1")
        print(cut, info)
    assert info["n_events"] == B + 5 and info["n_packets"] == 1


# ---- a known answer ---------------------------------------------------------------------------------------------------------------------
def test_a_hand_assembled_file(ctx, tmp_path):
    """A dozen events written out as bytes, the expected records computed by hand from the contract: no code shared with the encoders."""
    data = (
        b"#!AER-DAT3.1\r\n#Format: RAW\r\n#Source 1: DAVIS346\r\n#Start-Time: 2024-01-01 00:00:00 (TZ+0000)\r\n#!END-HEADER\r\n"
        # packet 0: special events (type 0, source 1), eventSize 8, one event: stepped over
        b"\x00\x00\x01\x00" b"\x08\x00\x00\x00" b"\x04\x00\x00\x00" b"\x00\x00\x00\x00" b"\x01\x00\x00\x00" b"\x01\x00\x00\x00" b"\x01\x00\x00\x00"
        b"\x07\x00\x00\x00\x10\x00\x00\x00"
        # packet 1: polarity (type 1), overflow 0, capacity 5, number 4
        b"\x01\x00\x01\x00" b"\x08\x00\x00\x00" b"\x04\x00\x00\x00" b"\x00\x00\x00\x00" b"\x05\x00\x00\x00" b"\x04\x00\x00\x00" b"\x03\x00\x00\x00"
        b"\x0B\x00\x14\x00" b"\xE8\x03\x00\x00"      # data 0x0014000B: x 10, y 2, polarity 1, valid; ts 1000
        b"\x99\x03\xB2\x02" b"\xE9\x03\x00\x00"      # data 0x02B20399: x 345, y 230, polarity 0, valid; ts 1001
        b"\x06\x00\x02\x00" b"\xEA\x03\x00\x00"      # data 0x00020006: x 1, y 1, polarity 1, NOT valid; ts 1002
        b"\x01\x00\x00\x00" b"\x00\x00\x00\x80"      # data 0x00000001: x 0, y 0, polarity 0, valid; ts 0x80000000 -> 0
        b"\xFF\xFF\xFF\xFF" b"\xFF\xFF\xFF\x7F"      # behind eventNumber: not decoded
        # packet 2: a frame (type 2) of 3 x 7 bytes: the packets behind it are off every alignment
        b"\x02\x00\x01\x00" b"\x07\x00\x00\x00" b"\x00\x00\x00\x00" b"\x00\x00\x00\x00" b"\x03\x00\x00\x00" b"\x03\x00\x00\x00" b"\x03\x00\x00\x00"
        + b"\xEE" * 21 +
        # packet 3: polarity, overflow 1, capacity 2, number 2
        b"\x01\x00\x01\x00" b"\x08\x00\x00\x00" b"\x04\x00\x00\x00" b"\x01\x00\x00\x00" b"\x02\x00\x00\x00" b"\x02\x00\x00\x00" b"\x02\x00\x00\x00"
        b"\x03\x00\x90\x02" b"\x05\x00\x00\x00"      # data 0x02900003: x 328, y 0, polarity 1, valid; ts 5
        b"\x0D\x04\x00\x80" b"\x40\x42\x0F\x00"      # data 0x8000040D: x 16384, y 259, polarity 0, valid; ts 1 000 000
        # packet 4: polarity of source 2, overflow 1, one event
        b"\x01\x00\x02\x00" b"\x08\x00\x00\x00" b"\x04\x00\x00\x00" b"\x01\x00\x00\x00" b"\x01\x00\x00\x00" b"\x01\x00\x00\x00" b"\x01\x00\x00\x00"
        b"\x0B\x00\x14\x00" b"\x41\x42\x0F\x00"      # x 10, y 2, polarity 1, valid; ts 1 000 001
        # a header cut short: 5 trailing bytes
        b"\x01\x00\x01\x00\x08"
    )
    header_bytes = data.index(b"#!END-HEADER\r\n") + 14
    path = str(tmp_path / "hand.aedat")
    open(path, "wb").write(data)
    o = 2147483648   # one overflow, in microseconds
    every = [(1000e-6, 10.0, 2.0, 1), (1001e-6, 345.0, 230.0, 0), (0.0, 0.0, 0.0, 0), (float(o + 5) * 1e-6, 328.0, 0.0, 1),
             (float(o + 1000000) * 1e-6, 16384.0, 259.0, 0), (float(o + 1000001) * 1e-6, 10.0, 2.0, 1)]
    ev_, info, t_first, t_last = ctx.stream_from_aedat_file(path)
    # (the stream sorts by time: the event of stamp 0 comes first)
    assert ev_.cpu().numpy().tobytes() == np.array([every[2], every[0], every[1]] + every[3:], dtype=REC).tobytes()
    assert info == dict(n_raw_events=7, n_events=6, n_invalid=1, n_outside=0, n_negative=0, n_before_start=0, n_after_end=0, n_packets=3,
                        n_other_packets=2, n_records=0, n_other_records=0, n_trailing_bytes=5, n_time_wraps=0, header_bytes=header_bytes,
                        format=31)
    assert (t_first, t_last) == (0.0, float(o + 1000001) * 1e-6)
    # file order, the sensor's bounds, source 1 only, both flips, a time base, a start and an end
    info = ctx.aedat_to_bin(path, str(tmp_path / "hand.bin"), width=346, height=260, source=1, flip_x=True, flip_y=True, time_base=1000,
                            start_time=0.0, end_time=2147.0)
    want = [(0.0, 335.0, 257.0, 1), (1e-6, 0.0, 29.0, 0)]           # ts 0 is negative; x 16384 is outside; overflow 1 is behind the end
    assert open(str(tmp_path / "hand.bin"), "rb").read() == np.array(want, dtype=REC).tobytes()
    assert info == dict(n_raw_events=6, n_events=2, n_invalid=1, n_outside=0, n_negative=1, n_before_start=0, n_after_end=2, n_packets=2,
                        n_other_packets=3, n_records=0, n_other_records=0, n_trailing_bytes=5, n_time_wraps=0, header_bytes=header_bytes,
                        format=31)
    fmt, hb = ctx.aedat_parse_header(data[:200])
    assert (fmt, hb) == (31, header_bytes)
    # the same dozen bytes of events as an AEDAT 2.0 file: big-endian, y 2 x 10 polarity 1 / an APS word / a wrap
    data20 = (b"#!AER-DAT2.0\r\n# This is a raw AE data file\r\n"
              b"\x00\x80\xA8\x00" b"\xFF\xFF\xFF\xF0"    # address 0x0080A800: y 2, x 10, polarity 1; ts 4294967280
              b"\x80\x00\x00\x01" b"\xFF\xFF\xFF\xF8"    # bit 31: APS
              b"\x00\x80\xA4\x00" b"\x00\x00\x00\x02"    # bit 10: external input — and the stamp has wrapped
              b"\x23\x15\x90\x23" b"\x00\x00\x00\x03"    # address 0x23159023: y 140, x 345, polarity 0 (low bits mean nothing); ts 3 + 2^32
              b"\x01\x02\x03")
    path20 = str(tmp_path / "hand20.aedat")
    open(path20, "wb").write(data20)
    ev_, info, _, _ = ctx.stream_from_aedat_file(path20)
    want = [(4294967280e-6, 10.0, 2.0, 1), (float(4294967296 + 3) * 1e-6, 345.0, 140.0, 0)]
    assert ev_.cpu().numpy().tobytes() == np.array(want, dtype=REC).tobytes()
    assert info == dict(n_raw_events=2, n_events=2, n_invalid=0, n_outside=0, n_negative=0, n_before_start=0, n_after_end=0, n_packets=0,
                        n_other_packets=0, n_records=4, n_other_records=2, n_trailing_bytes=3, n_time_wraps=1, header_bytes=44, format=20)


# ---- 2.0 --------------------------------------------------------------------------------------------------------------------------------
def test_aedat2_sizes_and_trailing_bytes(ctx, B):
    rng = np.random.default_rng(3)
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 5):
        recs = [dvs(int(rng.integers(0, 346)), int(rng.integers(0, 260)), k & 1, 100 + 2 * k, low=k) if k % 7 else aps(100 + 2 * k, k) for k in range(n)]
        for tail in (b"", b"\x21", b"\x00\x00\x00", b"\x00\x00\x00\x00\x00\x00\x07"):
            _, info = check(ctx, payload20(recs, tail), "2.0")
            assert info["n_records"] == n and info["n_trailing_bytes"] == len(tail) and info["n_other_records"] == (n + 6) // 7
    for extra in range(1, 8):
        _, info = check(ctx, payload20([dvs(1, 2, 1, 5)], b"\x00" * extra), "2.0")
        assert info["n_trailing_bytes"] == extra and info["n_events"] == 1
    # nothing behind n_bytes is read
    recs = [dvs(3, 4, 1, 10 + k) for k in range(10)]
    whole = torch.from_numpy(np.frombuffer(payload20(recs + [dvs(9, 9, 0, 99)] * 64), np.uint8).copy()).cuda()
    got, info = ctx.events_from_aedat(whole[: 80 + 5], "2.0")
    assert info["n_events"] == 10 and info["n_trailing_bytes"] == 5 and got.cpu().numpy().tobytes() == oracle(payload20(recs), "2.0")[0]


def test_aedat2_time_wraps(ctx, B):
    top = 0xFFFFFF00

    def run_of(n, ts, k0=0):
        return [dvs((k0 + k) % 346, (k0 + k) % 260, k & 1, ts + (k % 3)) for k in range(n)]
    cases = {
        # the first record of block 1 is the one behind the wrap
        "at_a_blocks_first_record": (run_of(B, top) + run_of(B, 5), 1),
        # the last record of block 0 is
        "at_a_blocks_last_record": (run_of(B - 1, top) + run_of(B + 1, 5), 1),
        "two_in_one_block": (run_of(B + 10, 7) + run_of(20, top) + run_of(20, 9) + run_of(20, top + 3) + run_of(20, 1), 2),
        "back_by_2_to_31_is_no_wrap": ([dvs(1, 1, 1, 0x80000005), dvs(2, 2, 1, 5), dvs(3, 3, 1, 6)], 0),
        "back_by_2_to_31_and_one_is_a_wrap": ([dvs(1, 1, 1, 0x80000006), dvs(2, 2, 1, 5), dvs(3, 3, 1, 6)], 1),
        # wraps are counted over all records: the stamps of APS and external-input records take part
        "other_records_carry_the_wrap": ([dvs(1, 1, 1, top)] + [aps(top + 1, k) for k in range(B)] + [ext(3), aps(4), dvs(2, 2, 0, 5)], 1),
        "a_first_record_that_is_no_event": ([aps(top), ext(2), dvs(4, 4, 1, 3)] + run_of(B, 9), 1),
        "wraps_of_three_blocks_add_up": (run_of(B - 5, top) + run_of(B, 5) + run_of(10, top) + run_of(B, 3) + run_of(7, top) + run_of(9, 0), 3),
    }
    for name, (recs, wraps) in cases.items():
        data, info = check(ctx, payload20(recs), "2.0")
        print(name, info)
        assert info["n_time_wraps"] == wraps, name
        t = np.frombuffer(data, REC)["t"]
        if name == "back_by_2_to_31_is_no_wrap":
            assert t[1] < t[0]
        elif wraps:
            assert t[-1] >= float(wraps << 32) * 1e-6 and (t[0] < 4294.967296 or name == "a_first_record_that_is_no_event")
    # the filters on a wrapped stream, the end of the stream behind the wrap
    recs, _ = cases["wraps_of_three_blocks_add_up"]
    check(ctx, payload20(recs), "2.0", time_base=top, width=300, height=200, flip_x=True)
    data, info = check(ctx, payload20(recs), "2.0", time_base=top, end_time=float((1 << 32) - top + 5) * 1e-6, start_time=1e-6)
    assert info["n_after_end"] > 2 * B and info["n_before_start"] > 0 and info["n_events"] > 0
    _, info = check(ctx, payload20(recs), "2.0", end_time=0.0)
    assert info["n_events"] == 0 and info["n_after_end"] == info["n_raw_events"]


def test_aedat2_end_of_stream_and_capacity(ctx, B):
    n = 3 * B + 40
    recs = [dvs(k % 346, 7, k & 1, 10 + k) if k % 5 else ext(10 + k, k) for k in range(n)]
    events_before = lambda k: k - (k + 4) // 5      # DVS records in front of record k
    for k in (1, B - 1, B + 2, 2 * B + 18, 3 * B + 1, n - 1):
        assert k % 5
        _, info = check(ctx, payload20(recs), "2.0", end_time=float(10 + k) * 1e-6)
        assert info["n_events"] == events_before(k) and info["n_after_end"] == events_before(n) - events_before(k)
    back = list(recs)
    for k in range(B + 3, n):
        back[k] = dvs(k % 346, 7, 1, 10 + k % 40)
    _, info = check(ctx, payload20(back), "2.0", end_time=float(10 + B + 2) * 1e-6)
    assert info["n_events"] == events_before(B + 2)
    want, want_info, _ = oracle(payload20(recs), "2.0")
    m = want_info["n_events"]
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat(payload20(recs), "2.0", capacity=m - 1)
    assert e.value.status == -6 and e.value.info["n_events"] == m
    got, info = ctx.events_from_aedat(payload20(recs), "2.0", capacity=m)
    assert got.cpu().numpy().tobytes() == want


# ---- random payloads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_random_chains(ctx, seed):
    rng = np.random.default_rng(seed)
    parts, ts, overflow = [], 1000, 0
    for k in range(160):
        kind = int(rng.integers(0, 10))
        if kind < 6:
            n = int(rng.integers(0, 900))
            x, y = rng.integers(0, 360, n), rng.integers(0, 270, n)
            stamps = ts + np.cumsum(rng.integers(0, 30, n)) - (rng.integers(0, 40, n) == 0) * 500
            ts = int(stamps[-1]) if n else ts
            if int(rng.integers(0, 30)) == 0:
                overflow += 1
            events = [ev(int(x[i]), int(y[i]), int(i & 1), max(int(stamps[i]), 0), int(rng.integers(0, 9) > 0)) for i in range(n)]
            parts.append(polarity(events, overflow=overflow, source=int(rng.integers(1, 3)), spare=int(rng.integers(0, 3))))
        else:
            parts.append(foreign(int(rng.integers(0, 50)), int(rng.integers(0, 9)), etype=int(rng.integers(2, 6)), source=int(rng.integers(1, 3))))
    chain = b"".join(parts)
    opts = [dict(width=346, height=260, flip_y=True, time_base=500), dict(source=1, start_time=0.01, end_time=float((overflow << 31) + ts // 2) * 1e-6)][seed - 1]
    _, info = check(ctx, chain, "3.1", **opts)
    print(seed, info)
    assert info["n_events"] > 10000 and info["n_invalid"] > 1000
    _, info = check(ctx, chain[: len(chain) * 2 // 3], "3.1", **opts)       # cut short somewhere


@pytest.mark.parametrize("seed", [1, 2])
def test_random_aedat2_records(ctx, seed):
    rng = np.random.default_rng(seed)
    n = 60000 + 77 * seed
    step = rng.integers(0, 40, n).astype(np.int64)
    step[rng.integers(0, n, 8)] = 0x80000000 + rng.integers(-2, 3, 8)          # jumps of about half the range: wraps, or not
    step[rng.integers(0, n, 300)] = -rng.integers(0, 300, 300)                  # small backward steps
    ts = (0xFFFF0000 + np.cumsum(step)) & 0xFFFFFFFF
    kind = rng.integers(0, 10, n)
    addr = (rng.integers(0, 300, n) << 22) | (rng.integers(0, 400, n) << 12) | (rng.integers(0, 2, n) << 11) | rng.integers(0, 1024, n)
    addr = np.where(kind == 0, addr | 0x80000000, np.where(kind == 1, addr | 0x400, addr & ~0x400))
    payload = payload20(np.stack([addr, ts], axis=1).ravel().tolist(), b"\x01\x02\x03" if seed == 2 else b"")
    opts = [dict(width=346, height=260, flip_x=True), dict(time_base=0xFFFF0000, start_time=0.05, end_time=float(1 << 33) * 1e-6)][seed - 1]
    _, info = check(ctx, payload, "2.0", **opts)
    print(seed, info)
    assert info["n_events"] > 10000 and info["n_other_records"] > 5000 and info["n_time_wraps"] >= 1


# ---- files --------------------------------------------------------------------------------------------------------------------------------
def encode31(t_us, x, y, p, per=4096, source=1, order=None, between=None):
    """events (int64 microseconds, integer x / y, polarity) as a chain of polarity packets of up to `per` events (a packet ends where
    the overflow steps); order: a permutation of the packets; between(k): foreign bytes behind packet k"""
    t_us, x, y, p = (np.asarray(a, np.int64) for a in (t_us, x, y, p))
    n = len(t_us)
    ov = t_us >> 31
    steps = set((np.flatnonzero(ov[1:] != ov[:-1]) + 1).tolist())
    cuts, a = [0], 0
    while a < n:
        b = min([a + per, n] + [s for s in steps if a < s < a + per])
        cuts.append(b)
        a = b
    packets = []
    for k in range(len(cuts) - 1):
        a, b = cuts[k], cuts[k + 1]
        body = np.empty((b - a, 2), "<u4")
        body[:, 0] = (x[a:b] << 17) | (y[a:b] << 2) | (p[a:b] << 1) | 1
        body[:, 1] = t_us[a:b] & 0x7FFFFFFF
        packets.append(header31(1, source, 8, 4, int(ov[a]), b - a, b - a) + body.tobytes() + (between(k) if between else b""))
    return b"".join(packets[k] for k in (order if order is not None else range(len(packets)))), len(packets)


def encode20(t_us, x, y, p):
    t_us, x, y, p = (np.asarray(a, np.int64) for a in (t_us, x, y, p))
    body = np.empty((len(t_us), 2), ">u4")
    body[:, 0] = (y << 22) | (x << 12) | (p << 11)
    body[:, 1] = t_us & 0xFFFFFFFF
    return body.tobytes()


@pytest.fixture(scope="module")
def synthetic():
    """200 000 events of the synthetic 346 x 260 calibration stream, times quantised to integer microseconds and moved up to an overflow
    step of the 3.1 stamp -> (t_us, x, y, p, .bin bytes with t = (t_us - base) * 1e-6, base)"""
    import synth_stream as SS
    t, xy, pol = SS.unpack_records(SS.make_stream(200000, device="cpu", seed=3))
    t_us = torch.round(t * 1e6).to(torch.int64)
    records = SS.pack_records(t_us.to(torch.float64) * 1e-6, xy, pol).numpy().tobytes()      # t = (double)(t_us + base - base) * 1e-6
    base = (1 << 31) - int(t_us[70000])                                                      # event 70 000 is the first of overflow 1
    assert base > 0
    return t_us.numpy() + base, xy[:, 0].to(torch.int64).numpy(), xy[:, 1].to(torch.int64).numpy(), pol.to(torch.int64).numpy(), records, base


def load_bin(ctx, path):
    L = ctx._L
    vp = ctypes.c_void_p
    h = vp()
    assert L.ecal_stream_create_from_file(ctx._h, os.fsencode(path), -INF, 0, 0.0, ctypes.byref(h)) == 0
    return ctx._stream_records(h)


HEADER31 = b"#!AER-DAT3.1\r\n#Format: RAW\r\n#Source 1: DAVIS346\r\n#Start-Time: 2024-01-01 00:00:00 (TZ+0000)\r\n#!END-HEADER\r\n"
HEADER20 = b"#!AER-DAT2.0\r\n# This is a raw AE data file - do not edit\r\n# Data format is int32 address, int32 timestamp\r\n"


@pytest.mark.parametrize("fmt", ["3.1", "2.0"])
def test_round_trip_through_a_file(ctx, tmp_path, synthetic, fmt):
    t_us, x, y, p, records, base = synthetic
    header = HEADER31 if fmt == "3.1" else HEADER20
    if fmt == "3.1":
        # a frame of the sensor's size behind every fourth packet, an IMU packet of odd size behind every other
        between = lambda k: foreign(36 + 346 * 260 * 2, 1) if k % 4 == 0 else foreign(51, 1 + k % 3, etype=3) if k % 4 == 2 else b""
        payload, n_packets = encode31(t_us, x, y, p, between=between)
    else:
        payload, n_packets = encode20(t_us, x, y, p) + b"\x00\x01", 0
    path, binf = str(tmp_path / "events.aedat"), str(tmp_path / "events.bin")
    open(path, "wb").write(header + payload)
    open(binf, "wb").write(records)
    ev_, info, t_first, t_last = ctx.stream_from_aedat_file(path, time_base=base)
    assert ev_.cpu().numpy().tobytes() == records
    assert info["n_events"] == 200000 == info["n_raw_events"] and info["header_bytes"] == len(header) and info["format"] == int(fmt.replace(".", ""))
    if fmt == "3.1":
        assert info["n_packets"] == n_packets == 50 and info["n_other_packets"] == 13 + 12 and info["n_trailing_bytes"] == 0
    else:
        assert info["n_records"] == 200000 and info["n_trailing_bytes"] == 2 and info["n_time_wraps"] == 0
    assert struct.pack("<dd", t_first, t_last) == records[:8] + records[-25:-17]
    info2 = ctx.aedat_to_bin(path, str(tmp_path / "by_library.bin"), time_base=base)
    assert open(str(tmp_path / "by_library.bin"), "rb").read() == records and info2 == info
    events, t0, t1 = calibrate.load_events_aedat(ctx, path, time_base=base)
    want, w0, w1 = load_bin(ctx, binf)
    assert torch.equal(events, want) and (t0, t1) == (w0, w1)
    # the fast path's sensor: the bounds drop nothing of this stream
    _, info3, _, _ = ctx.stream_from_aedat_file(path, time_base=base, width=346, height=260)
    assert info3["n_events"] == 200000 and info3["n_outside"] == 0
    # packets shuffled: the file forms' difference — aedat_to_bin keeps the file order, the stream sorts (stable)
    if fmt == "3.1":
        order = np.random.default_rng(4).permutation(n_packets).tolist()
        shuffled_payload, _ = encode31(t_us, x, y, p, order=order, between=between)
        # (the packets' cuts: every 4096 events from each overflow's first event on)
        cuts = list(range(0, 70000, 4096)) + list(range(70000, 200000, 4096)) + [200000]
        idx = np.concatenate([np.arange(cuts[k], cuts[k + 1]) for k in order])
    else:
        cuts = [0, 30000, 71000, 90001, 140000, 200000]
        order = [3, 0, 4, 2, 1]
        idx = np.concatenate([np.arange(cuts[k], cuts[k + 1]) for k in order])
        shuffled_payload = encode20(t_us[idx], x[idx], y[idx], p[idx])
    open(path, "wb").write(header + shuffled_payload)
    shuffled = np.frombuffer(records, REC)[idx]
    ev_, info, _, _ = ctx.stream_from_aedat_file(path, time_base=base)
    assert info["n_events"] == 200000 and info["n_time_wraps"] == 0
    assert ev_.cpu().numpy().tobytes() == shuffled[np.argsort(shuffled["t"], kind="stable")].tobytes()
    ctx.aedat_to_bin(path, str(tmp_path / "shuffled.bin"), time_base=base)
    assert open(str(tmp_path / "shuffled.bin"), "rb").read() == shuffled.tobytes()


def test_headers(ctx, tmp_path):
    p31 = polarity([ev(1, 2, 1, 10), ev(3, 4, 0, 11)])
    p20 = payload20([dvs(1, 2, 1, 10), dvs(3, 4, 0, 11)])
    hash20 = payload20([dvs(0x15A, 0x8C, 0, 10, low=0x23), dvs(3, 4, 0, 11)])     # a 2.0 record whose first byte is '#'
    assert hash20[:1] == b"#"
    want31, want20, want_hash = oracle(p31, "3.1")[0], oracle(p20, "2.0")[0], oracle(hash20, "2.0")[0]
    path = str(tmp_path / "h.aedat")

    def load(data, **opts):
        open(path, "wb").write(data)
        ev_, info, _, _ = ctx.stream_from_aedat_file(path, **opts)
        return ev_.cpu().numpy().tobytes(), info
    for header, payload, want, fmt in [(HEADER31, p31, want31, 31), (b"#!AER-DAT3.1\r\n#!END-HEADER\r\n", p31, want31, 31), (HEADER20, p20, want20, 20),
                                       (b"#!AER-DAT2.0\r\n", p20, want20, 20), (HEADER20, hash20, want_hash, 20), (HEADER20, b"", b"", 20),
                                       (HEADER31, b"", b"", 31)]:
        got, info = load(header + payload)
        assert got == want and info["format"] == fmt and info["header_bytes"] == len(header), header
    # an explicit format beats the version line; without a header it is all there is
    got, info = load(b"#!AER-DAT4.0\r\n# x\r\n" + p20, format="2.0")
    assert got == want20 and info["format"] == 20 and info["header_bytes"] == 19
    got, info = load(p20, format="2.0")
    assert got == want20 and info["header_bytes"] == 0
    # refused, with the version named
    for data, word in [(b"#!AER-DAT4.0\r\n" + p31, "4.0"), (b"#!AER-DAT1.0\r\n" + p20, "1.0"), (b"#!AER-DAT3.0\r\n#!END-HEADER\r\n" + p31, "3.0"),
                       (b"#!AER-DAT3.1\r\n#Format: RAW\r\n" + p31, "END-HEADER"), (b"#!AER-DAT3.1\r\n#Format: Compressed\r\n#!END-HEADER\r\n" + p31, "Compressed"),
                       (p31, "version"), (b"", "version"),
                       (HEADER31 + header31(1, 1, 8, 4, 0, 2, 3), "packet 0 at byte 0"),
                       (HEADER31 + p31 + header31(1, 1, 16, 4, 0, 0, 0), "packet 1 at byte %d" % len(p31))]:
        open(path, "wb").write(data)
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.stream_from_aedat_file(path)
        assert e.value.status == -1 and word in str(e.value), (data[:40], str(e.value))
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.aedat_to_bin(path, str(tmp_path / "none.bin"))
        assert e.value.status == -1
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.stream_from_aedat_file(str(tmp_path / "missing.aedat"))
    assert e.value.status == -1
    open(path, "wb").write(HEADER31 + p31)
    with pytest.raises(eventcalib_amd.EcalError) as e:       # a flip without the sensor's size
        ctx.stream_from_aedat_file(path, flip_x=True)
    assert e.value.status == -1
    got, info = load(HEADER31 + p31)      # the context is usable afterwards
    assert got == want31
