"""GPU: the mcap ingest (include/ecal_mcap.h; eventcalib_amd/csrc/ecal_mcap.hip) — ROS 2 MCAP recordings of event messages decoded in
HBM into packed 25-byte records — against the reader of tests/mcap_writer.py: a plain Python decoder that restates the contract
(nothing of mcap_events.hpp), byte for byte, the info fields and the message table included.  No tolerance anywhere.  mcap_writer
builds the cases; B = ecal_mcap_block_events() places them on the decode blocks' boundaries.  EVT3 packets are compared with
Context.events_from_raw over the concatenated payload: the raw ingest's decoder is the reference there.  No recording of a real
camera was at hand."""
import numpy as np
import pytest
import torch

import mcap_writer as mw
import test_gpu_raw_ingest as RAW
import eventcalib_amd
from eventcalib_amd import calibrate, mcap

pytestmark = pytest.mark.gpu

REC = mw.REC
S0 = 1600000000                       # the second the test stamps start in
BASE = S0 * 10 ** 9
COUNTERS = ("n_events", "n_outside", "n_negative", "n_before_start", "n_after_end")
INDEX_FIELDS = ("n_raw_events", "n_messages", "n_other_messages", "n_chunks", "n_schemas", "n_channels", "n_trailing_bytes", "first_stamp_ns",
                "msg_width", "msg_height", "n_payload_bytes", "kind", "layout")
SCHEMAS = [mw.DVS_SCHEMA, mw.PACKET_SCHEMA, mw.IMAGE_SCHEMA]
KINDS = [mw.STRUCT, mw.MONO]


def channels(kind):
    return [(0, 1 if kind == mw.STRUCT else 2, "/dvs/events"), (1, 3, "/dvs/image_raw"), (2, 0, "/rosout", "json")]


def ramp(n, t0=1000, dt=3000, seed=0):
    """n events on the sensor, t0 + dt k nanoseconds behind BASE -> (x, y, t_ns, p)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 346, n), rng.integers(0, 260, n), BASE + t0 + dt * np.arange(n, dtype=np.int64), rng.integers(0, 2, n)


def msg(kind, ev, frame_id=b""):
    """one message of the kind with the events (x, y, t_ns, p): an EventArray, or a mono packet whose time_base is the first stamp"""
    x, y, t, p = (np.asarray(v) for v in ev)
    if kind == mw.STRUCT:
        return (0, mw.event_array_message(mw.events_array(x, y, t // 10 ** 9, t % 10 ** 9, p), frame_id=frame_id))
    tb = int(t[0]) - 7 if len(t) else BASE
    return (0, mw.event_packet_message(mw.mono_words(x, y, t - tb, p), encoding=b"mono", time_base=tb, frame_id=frame_id))


def image(size, channel=1, fill=0xA5):
    return (channel, bytes([fill]) * size)


def cut(ev, a, b):
    return tuple(np.asarray(v)[a:b] for v in ev)


def file_of(kind, messages, **kw):
    return mw.write_mcap(SCHEMAS, channels(kind), messages, **kw)


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def B():
    b = mcap.mcap_block_events()
    assert b >= 64
    return b


def check(ctx, data, time_base=BASE, topic=None, **flt):
    """index on the host, decode on the device, compare everything with the reader -> (records, info)"""
    want, want_info, want_table = mw.decode(data, topic=topic, time_base=time_base, **flt)
    table, tinfo = ctx.mcap_index_messages(data, topic=topic)
    assert table.tobytes() == want_table.tobytes()
    assert {k: tinfo[k] for k in INDEX_FIELDS} == {k: want_info[k] for k in INDEX_FIELDS}
    got, info = ctx.events_from_mcap(data, table, tinfo["layout"], time_base=want_info["time_base"], **flt)
    torch.cuda.synchronize()
    records = got.cpu().numpy().tobytes()
    dev_fields = ("n_raw_events", "n_messages", "time_base") + COUNTERS
    assert {k: info[k] for k in dev_fields} == {k: want_info[k] for k in dev_fields}
    assert records == want
    assert ctx.mcap_count_events(data, table, tinfo["layout"]) == want_info["n_raw_events"] == sum(info[k] for k in COUNTERS)
    return records, info


# ---- message sizes and boundaries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_small_messages_where_lead_and_stride_meet(ctx, kind):
    for n in (0, 1, 2, 3):
        _, info = check(ctx, file_of(kind, [msg(kind, ramp(n, seed=n), frame_id=b"ab")]))
        assert info["n_events"] == n
    messages = [msg(kind, ramp(k % 4, t0=1000 + 50000 * k, seed=k), frame_id=b"x" * (k % 5)) for k in range(40)]
    _, info = check(ctx, file_of(kind, messages, per_chunk=[3, 1, 0, 2]))
    assert info["n_events"] == 60 and info["n_messages"] == 40


@pytest.mark.parametrize("kind", KINDS)
def test_totals_around_the_block(ctx, B, kind):
    for n in (B - 1, B, B + 1, 3 * B + 5):
        ev = ramp(n, seed=n)
        _, info = check(ctx, file_of(kind, [msg(kind, ev, frame_id=b"ab")]))                     # one message
        assert info["n_events"] == n
        cuts = [0, 1, 3, 6, B // 2, B - 2, min(n, B + 1), n]                                       # ... and cut into several: one straddles the block boundary
        parts = [msg(kind, cut(ev, a, b), frame_id=b"f" * (i % 4)) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
        _, info = check(ctx, file_of(kind, parts + [image(33)], per_chunk=3))
        assert info["n_events"] == n


@pytest.mark.parametrize("kind", KINDS)
def test_more_than_1024_blocks(ctx, B, kind):
    """the block scan's second round"""
    n = 1024 * B + B + 7
    ev = ramp(n, dt=700, seed=1)
    per = 65536 + 3
    messages = [msg(kind, cut(ev, a, min(a + per, n)), frame_id=b"cam"[: (a // per) % 4]) for a in range(0, n, per)]
    data = file_of(kind, messages, per_chunk=5)
    records, info = check(ctx, data, width=346, height=260, start_time=1e-4, end_time=float(700 * (n - 10)) * 1e-9)
    assert info["n_after_end"] == 11 and info["n_before_start"] == 142 and info["n_events"] == n - 153 > 1024 * B


@pytest.mark.parametrize("kind", KINDS)
def test_sixteen_start_alignments_and_the_file_end(ctx, B, kind):
    seen = set()
    for pad in range(16):
        part = file_of(kind, [image(pad), msg(kind, ramp(B + 9, seed=pad), frame_id=b"q")], per_chunk=0, closed=False)
        table, tinfo = ctx.mcap_index_messages(part)
        seen.add(int(table["offset"][0]) % 16)
        # the last event's last byte is the file's last byte (up to the CDR's end), and the device tensor sits in front of other bytes
        assert int(table["offset"][0]) + (14 + 16 * (B + 7) + 15 if kind == mw.STRUCT else 8 * (B + 9)) == len(part)
        whole = torch.from_numpy(np.frombuffer(part + b"\xFF" * 64, np.uint8).copy()).cuda()
        got, info = ctx.events_from_mcap(whole[: len(part)], table, tinfo["layout"], time_base=BASE)
        assert info["n_events"] == B + 9 and got.cpu().numpy().tobytes() == mw.decode(part, time_base=BASE)[0]
    assert seen == set(range(16))


# ---- fields and counters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_outside_flips_negative_start_and_end_inside_a_message(ctx, B, kind):
    rng = np.random.default_rng(11)
    messages, t0 = [], -10 ** 9
    for k in range(12):
        n = int(rng.integers(1, 500))
        t = t0 + np.sort(rng.integers(0, 25 * 10 ** 7, n))
        t0 += 25 * 10 ** 7
        messages.append(msg(kind, (rng.integers(0, 400, n), rng.integers(0, 300, n), BASE + t, rng.integers(0, 2, n)), frame_id=b"f" * (k % 5)))    # some outside 346 x 260
    data = file_of(kind, messages)
    records, info = check(ctx, data)
    assert info["n_negative"] > 100 and info["n_outside"] == 0
    records, info = check(ctx, data, width=346, height=260)
    assert info["n_outside"] > 100 and info["n_negative"] > 100
    for fx, fy in ((True, False), (False, True), (True, True)):
        flipped, info2 = check(ctx, data, width=346, height=260, flip_x=fx, flip_y=fy)
        a, b = np.frombuffer(records, REC), np.frombuffer(flipped, REC)
        assert np.array_equal(b["x"], 345 - a["x"] if fx else a["x"]) and np.array_equal(b["y"], 259 - a["y"] if fy else a["y"])
        assert {k: info2[k] for k in COUNTERS} == {k: info[k] for k in COUNTERS}
    _, info = check(ctx, data, width=346, height=260, start_time=0.6, end_time=1.4)       # both fall inside messages
    assert min(info[k] for k in COUNTERS) > 0
    _, info = check(ctx, data, width=100, height=0, flip_x=True, time_base=BASE - 10 ** 9)     # one bound alone; nothing negative
    assert info["n_negative"] == 0 and info["n_outside"] > 1000
    check(ctx, data, time_base=None)                                                            # the indexer's automatic base
    table, tinfo = ctx.mcap_index_messages(data)
    with pytest.raises(eventcalib_amd.EcalError) as e:       # a flip needs its bound
        ctx.events_from_mcap(data, table, tinfo["layout"], time_base=BASE, flip_x=True)
    assert e.value.status == -1
    with pytest.raises(eventcalib_amd.EcalError) as e:       # the device form must be given its base
        ctx.events_from_mcap(data, table, tinfo["layout"])
    assert e.value.status == -1 and "time base" in str(e.value)


def test_signed_seconds_nanoseconds_beyond_a_second_and_polarity_bytes(ctx):
    ev = mw.events_array([1, 2, 3, 4, 5, 65535], [6, 5, 4, 3, 2, 65535], [S0, S0, S0 + 1, -1, -2 ** 31, 2 ** 31 - 1],
                         [999999999, 1000000000, 0, 4294967295, 5, 4294967295], [0, 1, 255, 2, 128, 1])
    data = file_of(mw.STRUCT, [(0, mw.event_array_message(ev))])
    records, info = check(ctx, data)
    r = np.frombuffer(records, REC)
    assert r["p"].tolist() == [0, 1, 1, 1] and r["x"].tolist() == [1.0, 2.0, 3.0, 65535.0] and info["n_negative"] == 2
    assert r["t"].tolist() == [float(999999999) * 1e-9, 1.0, 1.0, float((2 ** 31 - 1 - S0) * 10 ** 9 + 4294967295) * 1e-9]
    records, info = check(ctx, data, time_base=-2 ** 31 * 10 ** 9)        # sec is signed: the earliest second there is
    assert info["n_negative"] == 0 and np.frombuffer(records, REC)["t"][4] == float(5) * 1e-9


def test_mono_words_and_time_bases(ctx):
    words = mw.mono_words([0, 65535, 7], [0, 32767, 9], [0, 2 ** 32 - 1, 5], [0, 1, 1])
    data = file_of(mw.MONO, [(0, mw.event_packet_message(words, time_base=BASE + 999999999, frame_id=b"abc")),
                             (0, mw.event_packet_message(words[:8], time_base=2 ** 64 - 5)), (0, mw.event_packet_message(b""))])
    records, info = check(ctx, data, time_base=None)
    r = np.frombuffer(records, REC)
    assert info["time_base"] == BASE and info["n_negative"] == 1 and r["x"].tolist() == [0.0, 65535.0, 7.0] and r["y"].tolist() == [0.0, 32767.0, 9.0]
    assert r["t"].tolist() == [float(999999999) * 1e-9, float(999999999 + 2 ** 32 - 1) * 1e-9, float(1000000004) * 1e-9] and r["p"].tolist() == [0, 1, 1]


# ---- capacity, the output buffer, a bad table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_capacity_output_alignment_and_a_bad_table(ctx, B, kind):
    ev = ramp(2 * B + 9, seed=5)
    ev[0][3] = 400
    data = file_of(kind, [msg(kind, cut(ev, 0, B + 3)), image(5), msg(kind, cut(ev, B + 3, 2 * B + 9), frame_id=b"z")])
    want, want_info, table = mw.decode(data, time_base=BASE, width=346)
    layout, n = want_info["layout"], want_info["n_events"]
    assert n == 2 * B + 8
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_mcap(data, table, layout, capacity=n - 1, time_base=BASE, width=346)
    assert e.value.status == -6 and e.value.info["n_events"] == n
    got, info = ctx.events_from_mcap(data, table, layout, capacity=n, time_base=BASE, width=346)
    assert got.cpu().numpy().tobytes() == want and info["n_events"] == n
    # an output of exactly the kept size at every alignment, guard bytes on both sides
    for shift in (1, 2, 3, 5, 8, 13):
        buf = torch.full((shift + n * 25 + 32,), 0x5A, dtype=torch.uint8, device="cuda")
        got, info = ctx.events_from_mcap(data, table, layout, capacity=n, out=buf[shift:], time_base=BASE, width=346)
        host = buf.cpu().numpy().tobytes()
        assert host[shift: shift + n * 25] == want and host[:shift] == b"\x5A" * shift and host[shift + n * 25:] == b"\x5A" * 32
    # an empty table (with the file, and with no byte at all)
    for d in (data, b""):
        got, info = ctx.events_from_mcap(d, None, layout, time_base=BASE)
        assert got.numel() == 0 and info["n_events"] == 0 == info["n_raw_events"] and ctx.mcap_count_events(d, None, layout) == 0
    # a table entry that reaches past n_bytes is refused, and nothing outside the file is read
    step = 16 if kind == mw.STRUCT else 8
    for field, value in (("offset", len(data) - 7), ("offset", len(data) + 1), ("offset", 2 ** 63), ("offset", 2 ** 64 - 4),
                         ("n", (len(data) - int(table["offset"][1])) // step + 2)):
        bad = table.copy()
        bad[field][1] = value
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.events_from_mcap(data, bad, layout, time_base=BASE, capacity=4 * B)
        assert e.value.status == -1
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.mcap_count_events(data, bad, layout)
        assert e.value.status == -1
    for bad_layout in (dict(layout, kind=0), dict(layout, kind=9), dict(layout, stride=7), dict(layout, span=[200, 15])):
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.events_from_mcap(data, table, bad_layout, time_base=BASE)
        assert e.value.status == -1 and "layout" in str(e.value)
    got, info = ctx.events_from_mcap(data, table, layout, time_base=BASE, width=346)       # the context is usable afterwards
    assert got.cpu().numpy().tobytes() == want


# ---- evt3 packets ---------------------------------------------------------------------------------------------------------------------------
def evt3_file(payload, rng, per_chunk=3, max_packet=4000):
    """the payload cut into packets at random even offsets (some empty), other messages between them"""
    cuts = sorted(set([0, len(payload)] + (2 * rng.integers(0, len(payload) // 2 + 1, max(1, len(payload) // max_packet))).tolist()))
    messages = []
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        messages.append((0, mw.event_packet_message(payload[a:b], encoding=b"evt3", frame_id=b"pk"[: i % 3], seq=i)))
        if i % 5 == 0:
            messages += [(0, mw.event_packet_message(b"", encoding=b"evt3")), image(int(rng.integers(0, 40)))]
    return mw.write_mcap(SCHEMAS, channels(mw.EVT3), messages, per_chunk=per_chunk), sum(1 for m in messages if m[0] == 0)


@pytest.mark.parametrize("seed,n_words,max_packet", [(1, 60000, 4000), (2, 9000, 30), (3, 2049, 8)])
def test_evt3_packets_equal_the_raw_ingest_on_the_concatenation(ctx, seed, n_words, max_packet):
    """vector runs and time words split across packets: the decoder's state runs across the message boundaries"""
    rng = np.random.default_rng(seed)
    payload = RAW.payload_of(RAW.random_words("EVT3", n_words, seed, many_highs=seed == 2), "EVT3")
    data, n_messages = evt3_file(payload, rng, max_packet=max_packet)
    want_table, want_info = mw.index_messages(data)
    assert want_info["kind"] == mw.EVT3 and mw.payload_of(data, want_table) == payload
    table, tinfo = ctx.mcap_index_messages(data)
    assert table.tobytes() == want_table.tobytes() and {k: tinfo[k] for k in INDEX_FIELDS} == {k: want_info[k] for k in INDEX_FIELDS}
    assert len(set((table["offset"] % 4).tolist())) == 4 or len(table) < 100
    for opts in (dict(time_base=0), dict(time_base=2000, width=1000, height=700, start_time=0.01, end_time=0.5)):
        want, raw_info = ctx.events_from_raw(payload, "EVT3", **opts)
        got, info = ctx.events_from_mcap(data, table, tinfo["layout"], **opts)
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() and (want.numel() > 25 * 100 or "width" in opts)
        for k in COUNTERS + ("n_no_state", "n_other_words", "n_time_wraps"):
            assert info[k] == raw_info[k], k
        assert info["n_payload_bytes"] == len(payload) and info["n_messages"] == len(table) == n_messages
        assert info["n_raw_events"] == sum(info[k] for k in COUNTERS) + info["n_no_state"]
    assert ctx.mcap_count_events(data, table, tinfo["layout"]) == ctx.raw_count_events(payload, "EVT3")
    n = int(ctx.events_from_raw(payload, "EVT3", time_base=0)[1]["n_events"])
    assert n > 100
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_mcap(data, table, tinfo["layout"], capacity=n - 1, time_base=0)
    assert e.value.status == -6 and e.value.info["n_events"] == n
    with pytest.raises(eventcalib_amd.EcalError) as e:       # no flips for evt3
        ctx.events_from_mcap(data, table, tinfo["layout"], time_base=0, width=1280, flip_x=True)
    assert e.value.status == -1 and "evt3" in str(e.value)
    bad = table.copy()
    bad["n"][len(bad) // 2] += 1                               # an odd byte count
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_mcap(data, bad, tinfo["layout"], time_base=0)
    assert e.value.status == -1


# ---- the file forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + [mw.EVT3])
def test_stream_and_bin_from_a_file(ctx, tmp_path, kind):
    path, out = str(tmp_path / "events.mcap"), str(tmp_path / "events.bin")
    rng = np.random.default_rng(4)
    if kind == mw.EVT3:
        payload = RAW.payload_of(RAW.random_words("EVT3", 30000, 5), "EVT3")
        data, _ = evt3_file(payload, rng)
        open(path, "wb").write(data)
        want, raw_info = ctx.events_from_raw(payload, "EVT3", time_base=0, width=1280, height=720)
        info = ctx.mcap_to_bin(path, out, width=1280, height=720)
        assert open(out, "rb").read() == want.cpu().numpy().tobytes() and info["kind"] == mw.EVT3 and info["time_base"] == 0
        assert info["n_events"] == raw_info["n_events"] and info["n_trailing_bytes"] == 0 and info["n_chunks"] > 1
        ev_, info2, t_first, t_last = ctx.stream_from_mcap_file(path, width=1280, height=720)
        rec = np.frombuffer(want.cpu().numpy().tobytes(), REC)
        assert ev_.cpu().numpy().tobytes() == rec[np.argsort(rec["t"], kind="stable")].tobytes() and info2 == info
        return
    n = 5000
    ev = ramp(n, t0=250000000, dt=40000, seed=3)
    order = rng.permutation(10)                                              # messages shuffled: the stream must sort, the .bin keeps the file order
    messages = []
    for i in order:
        messages += [msg(kind, cut(ev, 500 * i, 500 * i + 500), frame_id=b"davis"[: i % 6]), image(7 * i)]
    data = file_of(kind, messages, per_chunk=[3, 5, 2])
    open(path, "wb").write(data)
    want, want_info, _ = mw.decode(data)                                     # automatic base: the first event's whole second
    assert want_info["time_base"] == BASE
    info = ctx.mcap_to_bin(path, out)
    assert open(out, "rb").read() == want
    assert {k: info[k] for k in INDEX_FIELDS + COUNTERS + ("time_base",)} == {k: want_info[k] for k in INDEX_FIELDS + COUNTERS + ("time_base",)}
    ev_, info2, t_first, t_last = ctx.stream_from_mcap_file(path)
    rec = np.frombuffer(want, REC)
    assert ev_.cpu().numpy().tobytes() == rec[np.argsort(rec["t"], kind="stable")].tobytes() and info2 == info
    assert (t_first, t_last) == (rec["t"].min(), rec["t"].max())
    events, t0, t1 = calibrate.load_events_mcap(ctx, path, width=346, height=260, time_base=BASE - 5)
    want2, _, _ = mw.decode(data, time_base=BASE - 5, width=346, height=260)
    rec2 = np.frombuffer(want2, REC)
    assert events.cpu().numpy().tobytes() == rec2[np.argsort(rec2["t"], kind="stable")].tobytes()


def test_refusals_through_the_file(ctx, tmp_path):
    path = str(tmp_path / "refused.mcap")
    good = msg(mw.STRUCT, ramp(30))

    def refused(data, *words, **options):
        open(path, "wb").write(data)
        for call in (lambda: ctx.stream_from_mcap_file(path, **options), lambda: ctx.mcap_to_bin(path, str(tmp_path / "never.bin"), **options)):
            with pytest.raises(eventcalib_amd.EcalError) as e:
                call()
            assert e.value.status == -1
            for w in words:
                assert w in str(e.value), (w, str(e.value))
        if data[:8] == mw.MAGIC:
            with pytest.raises(mw.McapError):
                mw.decode(data, topic=options.get("topic"))

    stereo = [(4, 1, "/left/events"), (5, 1, "/right/events"), (1, 3, "/left/image")]
    messages = [(4, good[1]), (5, good[1]), (1, b"abc"), (4, good[1])]
    data = mw.write_mcap(SCHEMAS, stereo, messages)
    refused(data, "/left/events", "/right/events", "more than one topic")
    refused(data, "/middle", topic="/middle")
    open(path, "wb").write(data)
    info = ctx.mcap_to_bin(path, str(tmp_path / "left.bin"), topic="/left/events")
    assert info["n_events"] == 60 and info["n_other_messages"] == 2 and info["n_channels"] == 3
    refused(file_of(mw.STRUCT, [good], compression="lz4"), "lz4", "uncompressed", "record 1 at byte")
    refused(file_of(mw.STRUCT, [good], compression="zstd"), "zstd")
    refused(b"#ROSBAG V2.0\n" + bytes(4096), "ROS 1 bag")
    refused(b"SQLite format 3\0" + bytes(4096), "SQLite", ".db3")
    refused(b"", "not an MCAP file")
    refused(mw.write_mcap([(1, "dvs_msgs/msg/EventArray", "ros2idl", "struct EventArray { sequence<Event> events; };")], [(0, 1, "/e")], [(0, good[1])]), "ros2idl")
    refused(mw.write_mcap(SCHEMAS, [(0, 2, "/e")], [(0, mw.event_packet_message(bytes(16), encoding=b"libcaer_cmp"))]), "libcaer_cmp")
    refused(mw.write_mcap(SCHEMAS, [(0, 2, "/e")], [(0, mw.event_packet_message(bytes(16), encoding=b"evt2"))]), "evt2")
    refused(file_of(mw.STRUCT, [(0, mw.event_array_message(mw.events_array([1], [1], [S0], [0], [1]), encapsulation=b"\x00\x00\x00\x00"))]), "big-endian")
    refused(file_of(mw.STRUCT, [(1, b"abc")]), "no channel", "/dvs/image_raw")
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.stream_from_mcap_file(str(tmp_path / "missing.mcap"))
    assert e.value.status == -1
    open(path, "wb").write(file_of(mw.STRUCT, [good]))                    # and the context is usable afterwards
    assert ctx.stream_from_mcap_file(path)[1]["n_events"] == 30
    with pytest.raises(eventcalib_amd.EcalError) as e:                   # the bag ingest keeps refusing the container by name
        ctx.stream_from_bag_file(path)
    assert e.value.status == -1 and "MCAP" in str(e.value)
