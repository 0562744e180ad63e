"""GPU: the bag ingest (include/ecal.h "bag ingest"; eventcalib_amd/csrc/ecal_bag.hip) — ROS 1 bags of dvs_msgs/EventArray messages
decoded in HBM into packed 25-byte records — against the oracle of tests/bag_writer.py: a plain Python decoder that restates the
contract (nothing of bag_events.hpp), byte for byte, the info fields and the message table included.  No tolerance anywhere.
bag_writer builds the cases; B = ecal_bag_block_events() places them on the decode blocks' boundaries.  No bag of a real camera was
at hand: the known answer below is assembled by hand from the contract."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import bag_writer as bw
import eventcalib_amd
from eventcalib_amd import calibrate, capi

pytestmark = pytest.mark.gpu

INF = float("inf")
REC = bw.REC
S0 = 1600000000                       # the second the test stamps start in
BASE = S0 * 10 ** 9
COUNTERS = ("n_events", "n_outside", "n_negative", "n_before_start", "n_after_end")
INDEX_FIELDS = ("n_raw_events", "n_messages", "n_other_messages", "n_chunks", "n_connections", "n_trailing_bytes", "first_stamp_ns", "msg_width",
                "msg_height")
CONNS = [(0, "/dvs/events", bw.DVS), (1, "/dvs/image_raw", "sensor_msgs/Image"), (2, "/dvs/imu", "sensor_msgs/Imu")]


def ramp(n, t0=1000, dt=3000, seed=0, secs=S0):
    """n events on the sensor with stamps secs s + t0 ns, + dt, ..."""
    rng = np.random.default_rng(seed)
    t = t0 + dt * np.arange(n, dtype=np.int64)
    return bw.events_array(rng.integers(0, 346, n), rng.integers(0, 260, n), secs + t // 10 ** 9, t % 10 ** 9, rng.integers(0, 2, n))


def msg(events, frame_id=b"", **kw):
    return (0, bw.event_array_message(events, frame_id=frame_id, **kw))


def image(size, conn=1, fill=0xA5):
    return (conn, bytes([fill]) * size)


def bag(messages, **kw):
    return bw.write_bag(CONNS, messages, **kw)


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def B(ctx):
    b = ctx.bag_block_events()
    assert b >= 64
    return b


def test_structures_have_the_library_sizes(ctx):
    """ecal_bag_default_options writes the whole structure: a ctypes mirror that is too short would lose its guard bytes"""
    class Guarded(ctypes.Structure):
        _fields_ = [("o", capi.BagOptions), ("guard", ctypes.c_uint8 * 64)]
    g = Guarded()
    ctypes.memset(ctypes.byref(g), 0x5A, ctypes.sizeof(g))
    raw = ctypes.CDLL(capi.lib_path())      # (a handle of the test's own: the shared one keeps its struct-pointer prototype)
    raw.ecal_bag_default_options.argtypes, raw.ecal_bag_default_options.restype = [ctypes.c_void_p], None
    raw.ecal_bag_default_options(ctypes.byref(g))
    assert bytes(g.guard) == b"\x5A" * 64 and g.o.auto_time_base == 1 and g.o.time_base == 0 and g.o.start_time == -INF and g.o.flip_x == 0
    assert not g.o.topic and not g.o.type and g.o.has_end_time == 0 and g.o.width == 0
    assert ctypes.sizeof(capi.BagMessage) == 16 == capi.BAG_MESSAGE_DTYPE.itemsize and ctypes.sizeof(capi.BagInfo) == 14 * 8
    assert ctypes.sizeof(capi.BagOptions) == 72


def check(ctx, data, time_base=BASE, topic=None, type=None, **flt):
    """index on the host, decode on the device, compare everything with the oracle -> (records, info)"""
    want, want_info, want_table = bw.decode(data, topic=topic, type=type, time_base=time_base, **flt)
    table, tinfo = ctx.bag_index_messages(data, topic=topic, type=type)
    assert table.tobytes() == want_table.tobytes()
    assert {k: tinfo[k] for k in INDEX_FIELDS} == {k: want_info[k] for k in INDEX_FIELDS}
    got, info = ctx.events_from_bag(data, table, time_base=want_info["time_base"], **flt)
    torch.cuda.synchronize()
    records = got.cpu().numpy().tobytes()
    dev_fields = ("n_raw_events", "n_messages", "time_base") + COUNTERS
    assert {k: info[k] for k in dev_fields} == {k: want_info[k] for k in dev_fields}
    assert records == want
    assert ctx.bag_count_events(data, table) == want_info["n_raw_events"] == sum(info[k] for k in COUNTERS)
    return records, info


# ---- message sizes and boundaries -------------------------------------------------------------------------------------------------------
def test_message_sizes_around_the_block(ctx, B):
    sizes = (B - 1, B, B + 1, 2 * B + 1)
    for n in sizes:                                     # each alone
        _, info = check(ctx, bag([msg(ramp(n, seed=n), frame_id=b"ab")]))
        assert info["n_events"] == n and info["n_messages"] == 1
    messages = [msg(ramp(n, t0=1000 + 7 * k, seed=k), frame_id=b"x" * (k % 4)) for k, n in enumerate(sizes + (0, 1) + sizes[::-1])]
    _, info = check(ctx, bag(messages, per_chunk=[3, 1, 2]))
    assert info["n_events"] == 2 * sum(sizes) + 1 and info["n_messages"] == 10


def test_runs_of_one_event_messages_and_of_empty_messages_cross_a_block(ctx, B):
    n = B + 300
    ones = [msg(bw.events_array([k % 346], [k % 260], [S0 + k // 700], [5000 + k], [k & 1]), frame_id=b"abc"[: k % 4]) for k in range(n)]
    records, info = check(ctx, bag(ones, per_chunk=[7, 1, 64]))
    assert info["n_events"] == n == info["n_messages"]
    t = np.frombuffer(records, REC)["t"]
    assert t[B - 1] == float(((B - 1) // 700) * 10 ** 9 + 5000 + B - 1) * 1e-9 and t[B] == float((B // 700) * 10 ** 9 + 5000 + B) * 1e-9
    # empty messages in the table exactly where the slot space crosses the block boundary, and at both ends of the chain
    empties = [msg(ramp(0), frame_id=b"e" * (k % 3)) for k in range(70)]
    messages = empties + [msg(ramp(B - 1, seed=1, secs=S0 + 1))] + empties + [msg(ramp(1, seed=2, secs=S0 + 2))] + empties + \
        [msg(ramp(1, seed=3, secs=S0 + 3))] + empties + [msg(ramp(B + 2, seed=4, secs=S0 + 4))] + empties
    records, info = check(ctx, bag(messages, per_chunk=9))
    assert info["n_events"] == 2 * B + 3 and info["n_messages"] == 4 + 5 * 70
    t = np.frombuffer(records, REC)["t"]
    assert [int(v) for v in t[[B - 2, B - 1, B, B + 1]]] == [1, 2, 3, 4]
    # nothing but empty messages
    _, info = check(ctx, bag(empties))
    assert info["n_events"] == 0 and info["n_messages"] == 70 and info["time_base"] == BASE


def test_frame_ids_and_foreign_messages_put_events_at_every_residue(ctx, B):
    messages = []
    for k in range(48):
        messages += [msg(ramp(3 + k % 5, t0=100000 * k, seed=k), frame_id=b"davis346"[: k % 8]), image((5 * k) % 13 + (k % 3) * 16, conn=1 + k % 2)]
    messages.append(msg(ramp(B + 9, t0=9000000, seed=99), frame_id=b"cam"))     # ... and a long one at an odd offset, across a block boundary
    data = bag(messages, per_chunk=[5, 2])
    table = bw.index_messages(data)[0]
    assert set((table["offset_of_first_event"] % 16).tolist()) == set(range(16))
    assert int(table["offset_of_first_event"][-1]) % 4 != 0
    _, info = check(ctx, data)
    assert info["n_events"] == sum(3 + k % 5 for k in range(48)) + B + 9
    # an image of the sensor's size between two event messages
    data = bag([msg(ramp(5, seed=1)), image(346 * 260 + 1, fill=0x01), msg(ramp(B + 1, t0=50000, seed=2))], per_chunk=3)
    _, info = check(ctx, data)
    assert info["n_events"] == B + 6
    # an event whose last byte is the file's last byte, off every alignment: the message stands at top level of a bag that was never
    # closed, and the device tensor sits in front of other bytes — nothing behind n_bytes is read (the clipped fourth word)
    seen = set()
    for pad in range(8):
        part = bag([image(pad), msg(ramp(10, seed=pad), frame_id=b"q" * (pad % 3))], per_chunk=0, closed=False)
        table, _ = ctx.bag_index_messages(part)
        assert int(table["offset_of_first_event"][0]) + 130 == len(part)
        seen.add((len(part) - 13) % 4)
        poison = bw.events_array([9] * 16, [9] * 16, [S0] * 16, [77] * 16, [1] * 16).tobytes()
        whole = torch.from_numpy(np.frombuffer(part + poison, np.uint8).copy()).cuda()
        got, info = ctx.events_from_bag(whole[: len(part)], table, time_base=BASE)
        assert info["n_events"] == 10 and got.cpu().numpy().tobytes() == bw.decode(part, time_base=BASE)[0]
    assert seen == {0, 1, 2, 3}


# ---- fields and counters ----------------------------------------------------------------------------------------------------------------
def test_outside_flips_negative_and_start(ctx, B):
    rng = np.random.default_rng(11)
    messages = []
    for k in range(12):
        n = int(rng.integers(1, 500))
        t = np.sort(rng.integers(0, 3 * 10 ** 9, n))
        ev = bw.events_array(rng.integers(0, 400, n), rng.integers(0, 300, n), S0 - 1 + t // 10 ** 9, t % 10 ** 9, rng.integers(0, 2, n))    # some outside 346 x 260
        messages.append(msg(ev, frame_id=b"f" * (k % 5)))
    data = bag(messages)
    records, info = check(ctx, data)
    assert info["n_negative"] > 100 and info["n_outside"] == 0
    records, info = check(ctx, data, width=346, height=260)
    assert info["n_outside"] > 100 and info["n_negative"] > 100
    for fx, fy in ((True, False), (False, True), (True, True)):
        flipped, info2 = check(ctx, data, width=346, height=260, flip_x=fx, flip_y=fy)
        a, b = np.frombuffer(records, REC), np.frombuffer(flipped, REC)
        assert np.array_equal(b["x"], 345 - a["x"] if fx else a["x"]) and np.array_equal(b["y"], 259 - a["y"] if fy else a["y"])
        assert info2 == info
    _, info = check(ctx, data, width=346, height=260, start_time=0.75)
    assert info["n_before_start"] > 100
    _, info = check(ctx, data, width=100, height=0, flip_x=True, time_base=BASE - 10 ** 9)     # one bound alone; nothing negative
    assert info["n_negative"] == 0 and info["n_outside"] > 1000
    with pytest.raises(eventcalib_amd.EcalError) as e:       # a flip needs its bound
        ctx.events_from_bag(data, bw.index_messages(data)[0], time_base=BASE, flip_x=True)
    assert e.value.status == -1


def test_nsecs_beyond_a_second_and_polarity_bytes(ctx):
    ev = bw.events_array([1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1], [S0, S0, S0 + 1, S0, S0, 0xFFFFFFFF],
                         [999999999, 1000000000, 0, 4294967295, 1500000000, 4294967295], [0, 1, 255, 2, 128, 1])
    records, info = check(ctx, bag([msg(ev)]))
    r = np.frombuffer(records, REC)
    assert r["p"].tolist() == [0, 1, 1, 1, 1, 1]
    assert r["t"].tolist() == [float(999999999) * 1e-9, float(1000000000) * 1e-9, float(1000000000) * 1e-9, float(4294967295) * 1e-9,
                               float(1500000000) * 1e-9, float((0xFFFFFFFF - S0) * 10 ** 9 + 4294967295) * 1e-9]
    assert r["t"][1] == r["t"][2] == 1.0                    # nsecs is taken as it is: no carry, no refusal
    # epoch time against base 0: the doubles are the conversion of the whole count of nanoseconds
    records, info = check(ctx, bag([msg(ev)]), time_base=0)
    assert np.frombuffer(records, REC)["t"][0] == float(S0 * 10 ** 9 + 999999999) * 1e-9


def test_end_of_stream(ctx, B):
    # messages of 600 events, stamps k microseconds: block boundaries fall inside messages, message boundaries inside blocks
    n, per = 3 * B + 40, 600
    x = np.arange(n) % 346

    def bag_of(ts):
        return bag([msg(bw.events_array(x[a: a + per], [7] * len(x[a: a + per]), [S0] * len(x[a: a + per]), ts[a: a + per], x[a: a + per] & 1),
                        frame_id=b"e" * (a // per % 4)) for a in range(0, n, per)])
    ts = 1000 * (np.arange(n) + 10)
    data = bag_of(ts)
    # the offender in the first, a middle and the last block; at a block's first slot; at a message's first and last slot (a later
    # message); at the first and last slot of all
    for k in (0, 5, B - 1, B, B + 3, per - 1, per, 2 * per, 3 * per - 1, 2 * B, 2 * B + 17, 3 * B, n - 1):
        records, info = check(ctx, data, end_time=float(1000 * (10 + k)) * 1e-9)
        assert info["n_events"] == k and info["n_after_end"] == n - k
    _, info = check(ctx, data, end_time=float(1000 * (10 + n)) * 1e-9)          # not reached
    assert info["n_events"] == n and info["n_after_end"] == 0
    # time runs backwards behind the offender: nothing behind it may appear, whatever its time
    for k in (B - 1, B + 3, 2 * per):
        back = ts.copy()
        back[k + 1:] = 1000 * (np.arange(n - k - 1) % 50 + 10)
        _, info = check(ctx, bag_of(back), end_time=float(1000 * (10 + k)) * 1e-9, start_time=19.5e-6)
        assert info["n_events"] == k - 10 and info["n_after_end"] == n - k and info["n_before_start"] == 10
    # an outside or negative event that reaches the end time does not end the stream
    ev = bw.events_array([1, 400, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6], [S0, S0, S0 - 1, S0, S0, S0], [10, 99, 99, 20, 50, 20], [1, 1, 1, 0, 1, 1])
    _, info = check(ctx, bag([msg(ev)]), width=346, height=260, end_time=float(50) * 1e-9)
    assert (info["n_events"], info["n_outside"], info["n_negative"], info["n_after_end"]) == (2, 1, 1, 2)


# ---- time base, capacity, empty inputs, a bad table ---------------------------------------------------------------------------------------
def test_time_base_explicit_and_automatic(ctx, tmp_path):
    ev1 = ramp(50, t0=700000000, dt=20000000, seed=1, secs=S0 + 3)      # the first event: second S0 + 3, 0.7 s into it
    ev2 = ramp(50, t0=0, dt=20000000, seed=2, secs=S0 + 2)              # a message behind it that starts a second EARLIER
    data = bag([image(33), msg(ramp(0)), msg(ev1, frame_id=b"dvs"), msg(ev2)])
    path = str(tmp_path / "base.bag")
    open(path, "wb").write(data)
    want, want_info, table = bw.decode(data)                                # automatic
    assert want_info["time_base"] == (S0 + 3) * 10 ** 9 == want_info["first_stamp_ns"] and want_info["n_negative"] == 50
    info = ctx.bag_to_bin(path, str(tmp_path / "auto.bin"))
    assert open(str(tmp_path / "auto.bin"), "rb").read() == want and info == want_info
    assert np.frombuffer(want, REC)["t"][0] == float(700000000) * 1e-9
    want, want_info, _ = bw.decode(data, time_base=(S0 + 2) * 10 ** 9 + 5)  # explicit: nothing negative but the first event of ev2
    info = ctx.bag_to_bin(path, str(tmp_path / "explicit.bin"), time_base=(S0 + 2) * 10 ** 9 + 5)
    assert open(str(tmp_path / "explicit.bin"), "rb").read() == want and info == want_info
    assert info["time_base"] == (S0 + 2) * 10 ** 9 + 5 and info["first_stamp_ns"] == (S0 + 3) * 10 ** 9 and info["n_negative"] == 1
    check(ctx, data, time_base=None)                                        # the device form with the indexer's base
    check(ctx, data, time_base=12345)
    with pytest.raises(eventcalib_amd.EcalError) as e:                      # ... which it must be given
        ctx.events_from_bag(data, table)
    assert e.value.status == -1 and "time base" in str(e.value)


def test_capacity_and_empty_inputs(ctx, B):
    ev = ramp(2 * B + 9, seed=5)
    ev["x"][3] = 400
    data = bag([msg(ev[: B + 3]), image(5), msg(ev[B + 3:], frame_id=b"z")])
    want, want_info, table = bw.decode(data, time_base=BASE, width=346)
    n = want_info["n_events"]
    assert n == 2 * B + 8
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_bag(data, table, capacity=n - 1, time_base=BASE, width=346)
    assert e.value.status == -6 and e.value.info["n_events"] == n
    got, info = ctx.events_from_bag(data, table, capacity=n, time_base=BASE, width=346)
    assert got.cpu().numpy().tobytes() == want and info["n_events"] == n
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_bag(data, table, capacity=0, time_base=BASE)
    assert e.value.status == -6 and e.value.info["n_events"] == n + 1
    # the indexer's capacity: the count comes back with ECAL_ERR_RANGE
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.bag_index_messages(data, capacity=1)
    assert e.value.status == -6 and e.value.info["n_messages"] == 2
    # an empty table (with the file, and with no byte at all)
    for d in (data, b""):
        got, info = ctx.events_from_bag(d, None, time_base=BASE)
        assert got.numel() == 0 and info["n_events"] == 0 == info["n_raw_events"] and ctx.bag_count_events(d, None) == 0
    # a table entry that reaches past n_bytes is refused, and nothing outside the file is read
    for field, value in (("offset_of_first_event", len(data) - 12), ("offset_of_first_event", len(data) + 1), ("offset_of_first_event", 2 ** 63),
                         ("n_events", (len(data) - int(table["offset_of_first_event"][1])) // 13 + 1)):
        bad = table.copy()
        bad[field][1] = value
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.events_from_bag(data, bad, time_base=BASE, capacity=4 * B)
        assert e.value.status == -1
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.bag_count_events(data, bad)
        assert e.value.status == -1
    got, info = ctx.events_from_bag(data, table, time_base=BASE, width=346)       # the context is usable afterwards
    assert got.cpu().numpy().tobytes() == want


def test_truncated_bags(ctx, B):
    data = bag([msg(ramp(B + 5, seed=1)), image(21), msg(ramp(20, t0=10 ** 7, seed=2), frame_id=b"abc"), image(9)], per_chunk=[1, 3], closed=False)
    table = bw.index_messages(data)[0]
    first, second = int(table["offset_of_first_event"][0]), int(table["offset_of_first_event"][1])
    # in the last index record; in the image behind the second message (its chunk is cut short); in the second message's events, in
    # its front, in its record header; in the first message's events
    for size, messages, events in ((len(data) - 1, 2, B + 25), (second + 13 * 20 + 5, 2, B + 25), (second + 13 * 20 - 1, 1, B + 5), (second - 9, 1, B + 5),
                                   (second - 60, 1, B + 5), (first + 100, 0, 0)):
        _, info = check(ctx, data[:size])
        assert (info["n_messages"], info["n_events"]) == (messages, events)
    with pytest.raises(eventcalib_amd.EcalError) as e:      # cut in front of the first connection: nothing to choose from
        ctx.bag_index_messages(data[:4200])
    assert e.value.status == -1 and "no connection" in str(e.value)


# ---- a file written out byte by byte ------------------------------------------------------------------------------------------------------
HAND = b"".join([
    b"#ROSBAG V2.0\n",
    # bag header record: header of 69 bytes (op, index_pos = 0: never closed, conn_count, chunk_count), 3 bytes of padding
    b"\x45\x00\x00\x00", b"\x04\x00\x00\x00op=\x03", b"\x12\x00\x00\x00index_pos=\x00\x00\x00\x00\x00\x00\x00\x00",
    b"\x0f\x00\x00\x00conn_count=\x01\x00\x00\x00", b"\x10\x00\x00\x00chunk_count=\x01\x00\x00\x00", b"\x03\x00\x00\x00   ",
    # chunk record: header of 41 bytes, 406 bytes of data
    b"\x29\x00\x00\x00", b"\x04\x00\x00\x00op=\x05", b"\x10\x00\x00\x00compression=none", b"\x09\x00\x00\x00size=\x96\x01\x00\x00", b"\x96\x01\x00\x00",
    #   connection 0: /dvs/events, dvs_msgs/EventArray (header 42 bytes, data 49 bytes)
    b"\x2a\x00\x00\x00", b"\x04\x00\x00\x00op=\x07", b"\x09\x00\x00\x00conn=\x00\x00\x00\x00", b"\x11\x00\x00\x00topic=/dvs/events",
    b"\x31\x00\x00\x00", b"\x11\x00\x00\x00topic=/dvs/events", b"\x18\x00\x00\x00type=dvs_msgs/EventArray",
    #   message of connection 0 (header 38 bytes): seq 1, stamp, frame_id "cam", 260 x 346, 7 events: 28 + 3 + 91 = 122 bytes
    b"\x26\x00\x00\x00", b"\x04\x00\x00\x00op=\x02", b"\x09\x00\x00\x00conn=\x00\x00\x00\x00", b"\x0d\x00\x00\x00time=\x00\x10\x5e\x5f\x00\x00\x00\x00",
    b"\x7a\x00\x00\x00", b"\x01\x00\x00\x00", b"\x00\x10\x5e\x5f", b"\x00\x00\x00\x00", b"\x03\x00\x00\x00cam", b"\x04\x01\x00\x00", b"\x5a\x01\x00\x00",
    b"\x07\x00\x00\x00",
    bytes.fromhex("0a00 1400 00105e5f e8030000 01"),      # x 10, y 20, 1600000000 s + 1000 ns, on
    bytes.fromhex("5901 0301 00105e5f d0070000 00"),      # x 345, y 259, + 2000 ns, off
    bytes.fromhex("0000 0000 00105e5f 00ca9a3b 01"),      # x 0, y 0, nsecs = 1 000 000 000 taken as it is
    bytes.fromhex("5a01 0500 00105e5f b80b0000 01"),      # x 346: outside 346 x 260
    bytes.fromhex("0700 0401 00105e5f a00f0000 01"),      # y 260: outside
    bytes.fromhex("0100 0200 ff0f5e5f ffc99a3b 01"),      # 1599999999 s + 999 999 999 ns: one nanosecond before the base
    bytes.fromhex("0300 0400 01105e5f 05000000 ff"),      # 1600000001 s + 5 ns, polarity byte 255
    #   message of connection 0: seq 2, no frame_id, 5 events: 28 + 65 = 93 bytes
    b"\x26\x00\x00\x00", b"\x04\x00\x00\x00op=\x02", b"\x09\x00\x00\x00conn=\x00\x00\x00\x00", b"\x0d\x00\x00\x00time=\x01\x10\x5e\x5f\x00\x00\x00\x00",
    b"\x5d\x00\x00\x00", b"\x02\x00\x00\x00", b"\x01\x10\x5e\x5f", b"\x00\x00\x00\x00", b"\x00\x00\x00\x00", b"\x04\x01\x00\x00", b"\x5a\x01\x00\x00",
    b"\x05\x00\x00\x00",
    bytes.fromhex("6400 c800 01105e5f 00e1f505 00"),      # x 100, y 200, 1600000001 s + 100 000 000 ns
    bytes.fromhex("6500 c900 01105e5f 0065cd1d 01"),      # + 500 000 000 ns
    bytes.fromhex("6600 ca00 02105e5f 00000000 02"),      # 1600000002 s: reaches end_time 2.0 in the second run below
    bytes.fromhex("6700 cb00 00105e5f 01000000 01"),      # earlier again (behind the end: never seen in the second run)
    bytes.fromhex("6800 cc00 02105e5f 01000000 00"),
])
HAND_ALL = [(float(1000) * 1e-9, 10.0, 20.0, 1), (float(2000) * 1e-9, 345.0, 259.0, 0), (1.0, 0.0, 0.0, 1), (float(1000000005) * 1e-9, 3.0, 4.0, 1),
            (float(1100000000) * 1e-9, 100.0, 200.0, 0), (1.5, 101.0, 201.0, 1), (2.0, 102.0, 202.0, 1), (float(1) * 1e-9, 103.0, 203.0, 1),
            (float(2000000001) * 1e-9, 104.0, 204.0, 0)]


def test_a_hand_assembled_file(ctx, tmp_path):
    assert len(HAND) == 548
    path = str(tmp_path / "hand.bag")
    open(path, "wb").write(HAND)
    out = str(tmp_path / "hand.bin")
    info = ctx.bag_to_bin(path, out, width=346, height=260)
    assert open(out, "rb").read() == np.array(HAND_ALL, dtype=REC).tobytes()
    assert info == dict(n_raw_events=12, n_events=9, n_outside=2, n_negative=1, n_before_start=0, n_after_end=0, n_messages=2, n_other_messages=0,
                        n_chunks=1, n_connections=1, n_trailing_bytes=0, first_stamp_ns=BASE, time_base=BASE, msg_width=346, msg_height=260)
    info = ctx.bag_to_bin(path, out, width=346, height=260, flip_x=True, flip_y=True, start_time=1.0, end_time=2.0)
    want = [(t, 345.0 - x, 259.0 - y, p) for t, x, y, p in HAND_ALL[2:6]]
    assert open(out, "rb").read() == np.array(want, dtype=REC).tobytes()
    assert (info["n_events"], info["n_outside"], info["n_negative"], info["n_before_start"], info["n_after_end"]) == (4, 2, 1, 2, 3)
    table, tinfo = ctx.bag_index_messages(HAND)
    assert table.tolist() == [(93 + 49 + 99 + 46 + 31, 7, 0), (93 + 49 + 99 + 168 + 46 + 28, 5, 0)] and tinfo["n_raw_events"] == 12
    check(ctx, HAND, width=346, height=260)
    ev_, info, t_first, t_last = ctx.stream_from_bag_file(path, width=346, height=260)      # the stream sorts (stable)
    rec = np.array(HAND_ALL, dtype=REC)
    assert ev_.cpu().numpy().tobytes() == rec[np.argsort(rec["t"], kind="stable")].tobytes()
    assert (t_first, t_last) == (float(1) * 1e-9, float(2000000001) * 1e-9) and info["n_events"] == 9


# ---- random bags ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_random_bags(ctx, seed):
    rng = np.random.default_rng(seed)
    messages, total = [], 0
    while total < 20000:
        kind = int(rng.integers(0, 10))
        if kind < 3:
            messages.append(image(int(rng.integers(0, 3000)), conn=1 + kind % 2, fill=kind))
            continue
        n = 0 if kind == 3 else int(rng.integers(1, 40)) if kind < 6 else int(rng.integers(40, 1500))
        t = 4 * 10 ** 9 * total // 22000 + rng.integers(0, 2 * 10 ** 8, n)     # time advances over the file: 3.6 s from S0 - 1 on
        t = np.sort(t) if kind != 9 else t
        ev = bw.events_array(rng.integers(0, 360, n), rng.integers(0, 270, n), S0 - 1 + t // 10 ** 9, t % 10 ** 9 + (10 ** 9 if kind == 8 else 0),
                             np.where(rng.integers(0, 8, n) == 0, rng.integers(0, 256, n), rng.integers(0, 2, n)))
        messages.append(msg(ev, frame_id=bytes(rng.integers(97, 123, int(rng.integers(0, 12)), dtype=np.uint8)), seq=len(messages)))
        total += n
    data = bag(messages, per_chunk=[int(v) for v in rng.integers(0, 9, 5)], closed=bool(seed & 1))
    _, info = check(ctx, data)
    assert info["n_events"] > 10000
    _, info = check(ctx, data, width=346, height=260, flip_y=True, start_time=0.5, end_time=2.5)
    assert min(info[k] for k in COUNTERS) > 0
    check(ctx, data, time_base=None, width=346, height=260)
    check(ctx, data[: len(data) * 2 // 3], time_base=BASE - 10 ** 9)


# ---- the file forms -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    """200 000 events of the synthetic 346 x 260 calibration stream, times quantised to integer nanoseconds of epoch time -> (t_ns, x, y, p,
    .bin bytes with t = (t_ns - base) * 1e-9, base = the whole second of the first event)"""
    import synth_stream as SS
    t, xy, pol = SS.unpack_records(SS.make_stream(200000, device="cpu", seed=3))
    t_ns = torch.round(t * 1e9).to(torch.int64) + BASE + 250000000
    base = int(t_ns[0]) // 10 ** 9 * 10 ** 9
    records = SS.pack_records((t_ns - base).to(torch.float64) * 1e-9, xy, pol).numpy().tobytes()
    return t_ns.numpy(), xy[:, 0].to(torch.int64).numpy(), xy[:, 1].to(torch.int64).numpy(), pol.to(torch.int64).numpy(), records, base


def load_bin(ctx, path):
    L = ctx._L
    vp = ctypes.c_void_p
    h = vp()
    assert L.ecal_stream_create_from_file(ctx._h, os.fsencode(path), -INF, 0, 0.0, ctypes.byref(h)) == 0
    return ctx._stream_records(h)


def test_round_trip_through_a_file(ctx, tmp_path, synthetic):
    t_ns, x, y, p, records, base = synthetic
    per = 4096
    cuts = list(range(0, 200000, per)) + [200000]

    def bag_of(order):
        messages = []
        for i, k in enumerate(order):
            s = slice(cuts[k], cuts[k + 1])
            messages.append(msg(bw.events_array(x[s], y[s], t_ns[s] // 10 ** 9, t_ns[s] % 10 ** 9, p[s]), frame_id=b"davis"[: i % 6], seq=i))
            if i % 4 == 0:
                messages.append(image(346 * 260 + 3))                # an image of the sensor's size behind every fourth message
            elif i % 4 == 2:
                messages.append(image(320 + i % 3, conn=2))          # an IMU sample of odd size behind every other
        return bag(messages, per_chunk=[3, 5, 2])
    path, binf = str(tmp_path / "events.bag"), str(tmp_path / "events.bin")
    open(path, "wb").write(bag_of(range(len(cuts) - 1)))
    open(binf, "wb").write(records)
    ev_, info, t_first, t_last = ctx.stream_from_bag_file(path)                  # the automatic base
    assert ev_.cpu().numpy().tobytes() == records
    assert info["n_events"] == 200000 == info["n_raw_events"] and info["time_base"] == base == info["first_stamp_ns"]
    assert info["n_messages"] == 49 and info["n_other_messages"] == 13 + 12 and info["n_trailing_bytes"] == 0 and info["n_connections"] == 3
    assert (info["msg_width"], info["msg_height"]) == (346, 260)
    assert struct.pack("<dd", t_first, t_last) == records[:8] + records[-25:-17]
    info2 = ctx.bag_to_bin(path, str(tmp_path / "by_library.bin"))
    assert open(str(tmp_path / "by_library.bin"), "rb").read() == records and info2 == info
    events, t0, t1 = calibrate.load_events_bag(ctx, path)
    want, w0, w1 = load_bin(ctx, binf)
    assert torch.equal(events, want) and (t0, t1) == (w0, w1)
    # the fast path's sensor: the bounds drop nothing of this stream
    _, info3, _, _ = ctx.stream_from_bag_file(path, width=346, height=260)
    assert info3["n_events"] == 200000 and info3["n_outside"] == 0
    # messages shuffled: the file forms' difference — bag_to_bin keeps the file order, the stream finish must sort (stable); the
    # base is given, since the first event of the file is no longer the earliest
    order = np.random.default_rng(4).permutation(len(cuts) - 1).tolist()
    open(path, "wb").write(bag_of(order))
    idx = np.concatenate([np.arange(cuts[k], cuts[k + 1]) for k in order])
    shuffled = np.frombuffer(records, REC)[idx]
    ev_, info, _, _ = ctx.stream_from_bag_file(path, time_base=base)
    assert info["n_events"] == 200000 and info["time_base"] == base
    assert ev_.cpu().numpy().tobytes() == shuffled[np.argsort(shuffled["t"], kind="stable")].tobytes()
    events, t0, t1 = calibrate.load_events_bag(ctx, path, time_base=base)
    assert torch.equal(events, ev_)
    ctx.bag_to_bin(path, str(tmp_path / "shuffled.bin"), time_base=base)
    assert open(str(tmp_path / "shuffled.bin"), "rb").read() == shuffled.tobytes()


def test_topic_and_type_choice_and_refusals_through_the_file(ctx, tmp_path):
    ev_l, ev_r = ramp(300, seed=1), ramp(200, t0=500, seed=2)
    stereo_conns = [(4, "/davis/left/events", bw.DVS), (5, "/davis/right/events", bw.DVS), (6, "/davis/left/image_raw", "sensor_msgs/Image"),
                    (9, "/other/events", "my_msgs/EventArray")]
    messages = [(4, bw.event_array_message(ev_l[:100])), (5, bw.event_array_message(ev_r[:150], frame_id=b"r")), (6, b"\x07" * 333),
                (9, bw.event_array_message(ev_r[:7])), (4, bw.event_array_message(ev_l[100:], frame_id=b"left")), (5, bw.event_array_message(ev_r[150:]))]
    path = str(tmp_path / "stereo.bag")

    def refused(data, *words, **options):
        open(path, "wb").write(data)
        for call in (lambda: ctx.stream_from_bag_file(path, **options), lambda: ctx.bag_to_bin(path, str(tmp_path / "never.bin"), **options)):
            with pytest.raises(eventcalib_amd.EcalError) as e:
                call()
            assert e.value.status == -1
            for w in words:
                assert w in str(e.value), (w, str(e.value))
        with pytest.raises(bw.BagError):
            bw.decode(data, topic=options.get("topic"), type=options.get("type"))

    stereo = bw.write_bag(stereo_conns, messages, per_chunk=4)
    refused(stereo, "/davis/left/events", "/davis/right/events")
    refused(stereo, "/davis/middle", topic="/davis/middle")
    refused(stereo, "sensor_msgs/Imu", type="sensor_msgs/Imu")
    for options, n, other in ((dict(topic="/davis/left/events"), 300, 4), (dict(topic="/davis/right/events"), 200, 4),
                              (dict(type="my_msgs/EventArray"), 7, 5), (dict(type="my_msgs/EventArray", topic="/other/events"), 7, 5)):
        open(path, "wb").write(stereo)
        want, want_info, _ = bw.decode(stereo, **options)
        info = ctx.bag_to_bin(path, str(tmp_path / "one.bin"), **options)
        assert open(str(tmp_path / "one.bin"), "rb").read() == want and info == want_info
        assert info["n_events"] == n and info["n_other_messages"] == other and info["n_connections"] == 4
        check(ctx, stereo, **options)
    one = [(0, "/dvs/events", bw.DVS)]
    m = [(0, bw.event_array_message(ev_l))]
    refused(bw.write_bag(one, m, magic=b"#ROSBAG V1.2\n"), "1.2")
    refused(b"SQLite format 3\0" + bytes(4096), "ROS 2", "SQLite")
    refused(b"\x89MCAP0\r\n" + bytes(4096), "ROS 2", "MCAP")
    refused(b"\x00" * 100, "not a ROS 1 bag")
    refused(b"", "not a ROS 1 bag")
    refused(bw.write_bag(one, m, compression="bz2"), "bz2", "rosbag decompress", "record 1 at byte 4109")
    refused(bw.write_bag(one, m, compression="lz4"), "lz4", "rosbag decompress")
    refused(bw.write_bag([(1, "/dvs/image_raw", "sensor_msgs/Image")], [(1, b"abc")]), "/dvs/image_raw", "sensor_msgs/Image")
    refused(bw.write_bag(one, [(0, bw.event_array_message(ev_l) + b"\x00")]), "28 + L + 13 n", "record 3")
    good = bw.write_bag(one, m)
    refused(good[:4109] + bw.record(bw.op(9), b"") + good[4109:], "0x09", "record 1 at byte 4109")
    refused(good[:4109] + bw.record(bw.field("conn", b"\0\0\0\0"), b"") + good[4109:], "op field")
    refused(good[:4109] + bw.record(bw.op(4) + b"\x40\x00\x00\x00ab=", b"") + good[4109:], "runs past its header")
    refused(good[:4109] + bw.chunk_record(bw.connection_record(*one[0]) + bw.message_record(0, m[0][1]), size=7) + good[4109:], "size field")
    refused(good[:4109] + bw.chunk_record(bw.record(bw.op(6), b"")) + good[4109:], "0x06 inside a chunk")
    refused(good + bw.connection_record(0, "/dvs/events", "sensor_msgs/Image"), "connection 0", "defined again")
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.stream_from_bag_file(str(tmp_path / "missing.bag"))
    assert e.value.status == -1
    with pytest.raises(eventcalib_amd.EcalError) as e:          # a flip needs its bound
        open(path, "wb").write(good)
        ctx.stream_from_bag_file(path, flip_y=True)
    assert e.value.status == -1
    open(path, "wb").write(good)                                 # and the context is usable afterwards
    assert ctx.stream_from_bag_file(path)[1]["n_events"] == 300
