"""GPU: the AEDAT 4 ingest (include/ecal.h "aedat4 ingest"; eventcalib_amd/csrc/ecal_aedat4.hip) — iniVation DV recordings, LZ4 packets
of FlatBuffers, inflated and decoded in HBM into packed 25-byte records — against tests/aedat4_oracle.py: a sequential Python decoder
written from the contract (nothing of aedat4_events.hpp), byte for byte, the info fields and the packet table included.  No tolerance
anywhere.  tests/aedat4_writer.py builds the cases; B = ecal_aedat4_block_events() places packets on the decode blocks' boundaries.  No
AEDAT 4 file of a real camera was at hand; tests/golden/aedat4_liblz4_frames.npz holds frames that liblz4 made (LZ4F_compressFrame), so
that frames this project's own encoder did not write are decoded too."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import aedat4_oracle as AO
import aedat4_writer as AW
import eventcalib_amd
from eventcalib_amd import calibrate, capi

pytestmark = pytest.mark.gpu

INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("n_events", "n_outside", "n_negative", "n_before_start", "n_after_end")
T0 = 1_700_000_000_250_000     # epoch microseconds of the cases' first events
PREFIX = len(AW.packet_prefix(0, vector_mod=0))   # bytes in front of the first event, a multiple of 16


@pytest.fixture(scope="module")
def ctx():
    with eventcalib_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def B(ctx):
    b = ctx.aedat4_block_events()
    assert b >= 64
    return b


def ramp(n, t0=T0, dt=3, seed=0):
    rng = np.random.default_rng(seed)
    return AW.make_events(t0 + dt * np.arange(n), rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n))


def event_file(packets, compression=AW.LZ4, stream=1, compressed=True, **build):
    """packets: event arrays (or ready FlatBuffers as bytes) of stream `stream`, or (stream id, bytes) for a foreign packet"""
    chain = []
    for p in packets:
        if isinstance(p, tuple):
            chain.append((p[0], AW.wrap(p[1], compression)))
        else:
            fb = p if isinstance(p, (bytes, bytearray)) else AW.event_packet(p)
            chain.append((stream, AW.wrap(bytes(fb), compression, compressed=compressed)))
    return AW.build_file(chain, compression, **build)


def check(ctx, f, capacity=None, **opts):
    """index and decode on the device, compare everything with the oracle -> (records, info)"""
    sid = opts.pop("stream_id", -1)
    want_table, want_tinfo = AO.index(f, sid)
    table, tinfo = ctx.aedat4_index_packets(f, stream_id=sid)
    assert [(int(r["offset_of_data"]), int(r["n_bytes"]), int(r["zero"])) for r in table] == [(o, s, 0) for o, s in want_table]
    assert {k: tinfo[k] for k in want_tinfo} == want_tinfo
    opts.setdefault("time_base", want_tinfo["first_stamp_us"])      # the _dev form takes an explicit base
    want, want_info = AO.decode(f, stream_id=sid, **opts)
    comp = want_tinfo["compression"]
    got, info = ctx.events_from_aedat4(f, comp, table, capacity=capacity, **opts)
    torch.cuda.synchronize()
    data = got.cpu().numpy().tobytes()
    dev_fields = ["n_raw_events", "n_packets", "n_compressed_bytes", "n_inflated_bytes", "time_base", "compression"] + list(COUNTERS)
    assert {k: info[k] for k in dev_fields} == {k: want_info[k] for k in dev_fields}
    assert data == want.tobytes()
    assert ctx.aedat4_count_events(f, comp, table) == want_info["n_raw_events"] == sum(info[k] for k in COUNTERS)
    return data, info


def test_structures_have_the_library_sizes(ctx):
    """ecal_aedat4_default_options writes the whole structure: a ctypes mirror that is too short would lose its guard bytes"""
    class Guarded(ctypes.Structure):
        _fields_ = [("o", capi.Aedat4Options), ("guard", ctypes.c_uint8 * 64)]
    g = Guarded()
    ctypes.memset(ctypes.byref(g), 0x5A, ctypes.sizeof(g))
    raw = ctypes.CDLL(capi.lib_path())      # (a handle of the test's own: the shared one keeps its struct-pointer prototype)
    raw.ecal_aedat4_default_options.argtypes, raw.ecal_aedat4_default_options.restype = [ctypes.c_void_p], None
    raw.ecal_aedat4_default_options(ctypes.byref(g))
    assert bytes(g.guard) == b"\x5A" * 64 and g.o.stream_id == -1 and g.o.auto_time_base == 1 and g.o.start_time == -INF
    assert g.o.max_inflated_bytes == 1 << 34 and g.o.compression == capi.AEDAT4_LZ4
    assert ctypes.sizeof(capi.Aedat4Packet) == 16 == capi.AEDAT4_PACKET_DTYPE.itemsize and ctypes.sizeof(capi.Aedat4Info) == 14 * 8


# ---- LZ4 sequences -------------------------------------------------------------------------------------------------------------------
LITERALS = (0, 14, 15, 16, 269, 270, 271, 15 + 2 * 255)
MATCHES = (4, 18, 19, 20, 273, 274)
OFFSETS = (1, 2, 3, 7, 8, 13, 16, 63, 64, 65, 255, 256, 65535)


def sequence_cases():
    """(literal length, offset, match length): every listed value at least once, and offsets below, at and above the match length"""
    cases = [(ll, OFFSETS[k % len(OFFSETS)], MATCHES[k % len(MATCHES)]) for k, ll in enumerate(LITERALS)]
    cases += [(LITERALS[k % len(LITERALS)], OFFSETS[(3 * k + 1) % len(OFFSETS)], ml) for k, ml in enumerate(MATCHES)]
    cases += [(LITERALS[(k + 2) % len(LITERALS)], off, MATCHES[(k + 3) % len(MATCHES)]) for k, off in enumerate(OFFSETS)]
    cases += [(5, 20, 20), (0, 19, 20), (3, 21, 20), (0, 64, 274), (1, 65, 273), (0, 63, 274), (2, 1, 274), (0, 256, 273), (0, 255, 274),
              (0, 4, 4), (0, 3, 4), (0, 5, 4), (7, 65535, 274), (0, 65534, 19)]
    return cases


def sequence_packet(plan, rng, vector_mod=0, **frame_kw):
    """An event packet whose bytes the given blocks produce.  plan: [("stored", n) | ("lz4", [(literal length, offset, match length), ...,
    (literal length, None, 0)])]; the first block starts with at least PREFIX literal bytes.  The last literal run is lengthened so
    that the vector is whole events.  -> (the LZ4 frame, the inflated packet)"""
    def total(plan):
        return sum(b[1] if b[0] == "stored" else sum(ll + (ml if off is not None else 0) for ll, off, ml in b[1]) for b in plan)
    pad = (PREFIX - total(plan)) % 16
    plan = [list(b) for b in plan]
    if plan[-1][0] == "stored":
        plan[-1][1] += pad
    else:
        ll, off, ml = plan[-1][1][-1]
        plan[-1][1] = list(plan[-1][1][:-1]) + [(ll + pad, off, ml)]
    n_events = (total(plan) - PREFIX) // 16
    literal = AW.packet_prefix(n_events, vector_mod=0) + rng.integers(0, 256, total(plan), dtype=np.uint8).tobytes()
    assert len(AW.packet_prefix(n_events, vector_mod=0)) == PREFIX
    frame, used = AW.Lz4Frame(**frame_kw), 0
    for k, b in enumerate(plan):
        if b[0] == "stored":
            frame.stored(literal[used:used + b[1]])
            used += b[1]
        else:
            seqs = []
            for ll, off, ml in b[1]:
                seqs.append((literal[used:used + ll], off, ml))
                used += ll
            assert k or len(seqs[0][0]) >= PREFIX
            frame.block(seqs)
    data = frame.finish()
    assert len(frame.out) == PREFIX + 16 * n_events
    return data, bytes(frame.out)


def history(off):
    """literals in front of a case: the prefix and enough bytes for the offset"""
    return max(off, 300) + 37


def test_sequences_each_in_a_packet_of_its_own_and_all_in_one_frame(ctx):
    rng = np.random.default_rng(11)
    cases = sequence_cases()
    assert {c[0] for c in cases} >= set(LITERALS) and {c[1] for c in cases} >= set(OFFSETS) and {c[2] for c in cases} >= set(MATCHES)
    packets = []
    for ll, off, ml in cases:
        if history(off) + ll + ml + 21 <= 65536:
            plan = [("lz4", [(history(off), 8, 4), (ll, off, ml), (21, None, 0)])]
        else:   # the history is a block of its own: the match reaches across the block boundary into it
            plan = [("lz4", [(65536, None, 0)]), ("lz4", [(ll, off, ml), (21, None, 0)])]
        packets.append(sequence_packet(plan, rng))
    # all of them inside one frame: a stored block of history, then every case as one sequence of one block (block maximum 4 MiB)
    one = [("stored", 65536), ("lz4", [(ll, off, ml) for ll, off, ml in cases] + [(9, None, 0)])]
    packets.append(sequence_packet(one, rng, block_max=7))
    f = AW.build_file([(1, d) for d, _ in packets], AW.LZ4)
    for (d, out), (o, s) in zip(packets, AO.index(f)[0]):
        assert AO.lz4_frame(f[o:o + s]) == out        # (the oracle inflates what the writer meant)
    data, info = check(ctx, f)
    assert info["n_packets"] == len(cases) + 1 and info["n_events"] > 1000
    check(ctx, f, width=346, height=260, time_base=0)


def test_blocks_flags_and_block_maxima(ctx):
    rng = np.random.default_rng(12)
    packets = []
    # a match that ends exactly at a block's end (the block inflates to the block maximum), behind it the last sequence of no literals
    packets.append(sequence_packet([("lz4", [(65536 - 300, 100, 300), (0, None, 0)])], rng))
    # ... and the same followed by a second block that reaches back across the boundary
    packets.append(sequence_packet([("lz4", [(65536 - 20, 1, 20), (0, None, 0)]), ("lz4", [(0, 65535, 40), (24, None, 0)])], rng))
    # stored blocks between compressed ones: a frame of three blocks, and one of five
    packets.append(sequence_packet([("lz4", [(400, 16, 30), (10, None, 0)]), ("stored", 333), ("lz4", [(0, 700, 64), (12, None, 0)])], rng))
    packets.append(sequence_packet([("stored", 100), ("lz4", [(3, 50, 9), (5, None, 0)]), ("stored", 0), ("stored", 64),
                                    ("lz4", [(0, 1, 100), (8, None, 0)])], rng))
    # every combination of the four frame flags, block maxima 4 .. 7
    for flags in range(16):
        kw = dict(independent=bool(flags & 1), block_checksum=bool(flags & 2), content_size=bool(flags & 4), content_checksum=bool(flags & 8))
        packets.append(sequence_packet([("lz4", [(200 + flags, 30, 40), (6, None, 0)]), ("stored", 48), ("lz4", [(40, 7, 19), (5, None, 0)])],
                                       rng, block_max=4 + flags % 4, **kw))
    packets.append(sequence_packet([("lz4", [(70000, 65535, 300), (33, None, 0)]), ("stored", 100000)], rng, block_max=7))
    # frames whose only block is empty, and a frame of no block: packets of no events
    for blocks in ([[(b"", None, 0)]], ["stored"], []):
        fr = AW.Lz4Frame()
        for b in blocks:
            fr.stored(b"") if b == "stored" else fr.block(b)
        packets.append((fr.finish(), b""))
    packets.append(sequence_packet([("lz4", [(100, 3, 50), (11, None, 0)])], rng))
    f = AW.build_file([(1, d) for d, _ in packets], AW.LZ4)
    for (d, out), (o, s) in zip(packets, AO.index(f)[0]):
        assert AO.lz4_frame(f[o:o + s]) == out
    check(ctx, f)
    # the greedy matcher's frames of real events: three linked blocks, independent blocks
    ev = ramp(9000, seed=5)
    for kw in (dict(), dict(independent=True), dict(block_max=5, content_size=True)):
        check(ctx, AW.build_file([(1, AW.lz4_compressed_frame(AW.event_packet(ev), **kw))], AW.LZ4_HIGH), width=346, height=260)


# ---- FlatBuffers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compression", [AW.NONE, AW.LZ4])
def test_flatbuffer_layouts(ctx, compression):
    packets, t = [], T0
    for after in (False, True):
        for mod in range(16):
            packets.append(AW.event_packet(ramp(5 + mod, t0=t, seed=mod), vtable_after=after, vector_mod=mod, extra_fields=mod % 3))
            t += 100
    packets.append(AW.event_packet(ramp(0), absent=True))
    packets.append(AW.event_packet(ramp(0), absent=True, vtable_after=True, extra_fields=2))
    packets.append(AW.event_packet(ramp(0), short_vtable=True))
    packets.append(AW.event_packet(ramp(0)))                       # a count of 0
    packets.append(AW.event_packet(ramp(1, t0=t)))                 # ... and of 1
    packets.append(AW.event_packet(ramp(0), vtable_after=True))
    packets.append(AW.event_packet(ramp(1, t0=t + 9), vtable_after=True, vector_mod=13))
    data, info = check(ctx, event_file(packets, compression))
    assert info["n_events"] == sum(5 + m for m in range(16)) * 2 + 2


# ---- packets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compression", [AW.NONE, AW.LZ4])
def test_packets_around_the_decode_block(ctx, B, compression):
    sizes = [B, 1, B - 1, 2, B + 1, 0, 0, 0, B - 3, 3, 0, 2 * B, 0, 0, 0, 0, 0, 7, B // 2, B // 2, 1, 1, 1, 0, 3 * B - 5]
    packets, t = [], T0
    for k, n in enumerate(sizes):
        packets.append(ramp(n, t0=t, seed=k))
        t += 3 * n
        if k % 4 == 1:    # a foreign packet larger than any event packet
            packets.append((2 + k % 2, AW.foreign_packet(16 * 3 * B + 40 + 5 * k, seed=k)))
    f = event_file(packets, compression, compressed=False)
    data, info = check(ctx, f)
    assert info["n_events"] == sum(sizes) and AO.index(f)[1]["n_other_packets"] == 6
    check(ctx, event_file(packets, compression, compressed=False, data_table=False))     # dataTablePosition -1: never closed


def test_files_cut_short(ctx, B):
    packets = [ramp(B + 7, seed=1), (3, AW.foreign_packet(500)), ramp(300, t0=T0 + 9000, seed=2), ramp(40, t0=T0 + 9900, seed=3)]
    for compression in (AW.NONE, AW.LZ4):
        f = event_file(packets, compression, data_table=False)
        table, _ = AO.index(f)
        begin = AO.parse_header(f)[1]
        ends = [begin] + [o + s for _, o, s in AO.chain(f, begin, len(f))[0]]      # where every whole packet ends
        last = table[-1]
        # inside the last packet's data, at its first data byte, inside and at its header; inside an earlier packet; inside the first
        for cut in (last[0] + last[1] - 1, last[0] + 5, last[0], last[0] - 3, last[0] - 8, table[1][0] - 1, table[0][0] + 1):
            g = f[:cut]
            data, info = check(ctx, g)
            tinfo = ctx.aedat4_index_packets(g)[1]
            assert tinfo["n_trailing_bytes"] == cut - max(e for e in ends if e <= cut)
            assert tinfo["n_packets"] == sum(1 for o, s in table if o + s <= cut)
    # a table position that cuts the chain: what lies behind it is not read
    f = event_file(packets, AW.LZ4)
    data, info = check(ctx, f)
    assert info["n_events"] == B + 347


# ---- filter ----------------------------------------------------------------------------------------------------------------------------
def test_filter_counters_flips_and_times(ctx, B):
    rng = np.random.default_rng(21)
    n = 2 * B + 300
    t = T0 + np.cumsum(rng.integers(0, 9, n))
    x, y = rng.integers(-2, 350, n), rng.integers(-2, 263, n)
    on = rng.integers(0, 4, n) * rng.integers(0, 2, n)          # the polarity byte is on != 0
    ev = AW.make_events(t, x, y, on)
    ev["pad"] = rng.integers(0, 256, (n, 3))                     # padding means nothing
    cuts = [0, 100, B - 1, B, B + 500, n]
    packets = [ev[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    span = float(t[-1] - T0) * 1e-6
    for compression in (AW.NONE, AW.LZ4):
        f = event_file(packets, compression)
        base = T0 - 250_000
        for opts in (dict(), dict(width=346, height=260), dict(width=346, height=260, flip_x=True), dict(width=346, height=260, flip_y=True),
                     dict(width=346, height=260, flip_x=True, flip_y=True, time_base=base),
                     dict(time_base=int(t[n // 3])),                                         # a third of the events negative
                     dict(time_base=base, start_time=0.25 + span / 4),
                     dict(time_base=base, end_time=0.25 + span / 2),                          # the stream ends in the middle of a packet
                     dict(time_base=base, start_time=0.25 + span / 5, end_time=0.25 + span * 0.7, width=346, height=260),
                     dict(time_base=base, end_time=0.0), dict(time_base=base, end_time=1e9), dict(height=100), dict(width=10)):
            data, info = check(ctx, f, **opts)
        # each counter is exercised
    data, info = check(ctx, f, time_base=int(t[n // 3]), width=346, height=260, start_time=span / 2, end_time=span * 0.6)
    assert all(info[k] > 0 for k in COUNTERS)
    with pytest.raises(eventcalib_amd.EcalError) as e:       # a flip without the sensor's size
        ctx.events_from_aedat4(f, AW.LZ4, AO_table(ctx, f), flip_x=True)
    assert e.value.status == -1


def AO_table(ctx, f):
    return ctx.aedat4_index_packets(f)[0]


def test_none_and_lz4_of_the_same_events_give_the_same_records(ctx, B):
    packets = [ramp(B + 11, seed=4), ramp(0), ramp(2 * B, t0=T0 + 50_000, seed=6)]
    recs = []
    for compression, compressed in ((AW.NONE, False), (AW.LZ4, False), (AW.LZ4, True), (AW.LZ4_HIGH, True)):
        data, info = check(ctx, event_file(packets, compression, compressed=compressed), width=346, height=260)
        recs.append(data)
        assert info["n_inflated_bytes"] == sum(len(AW.event_packet(p)) for p in packets)
    assert recs[0] == recs[1] == recs[2] == recs[3] and len(recs[0]) == 25 * (3 * B + 11)


# ---- malformed -------------------------------------------------------------------------------------------------------------------------
def malformed_frames():
    """(name, the packet's data): every one is to be refused"""
    good = AW.event_packet(ramp(20))
    def fr(**kw):
        return AW.Lz4Frame(**kw)
    def lit(n):
        return good[:n]
    out = []
    f = fr(); f.raw(9, bytes([0x40]) + lit(4) + bytes([0, 0, 0x00, 0x00])); out.append(("offset 0", f.finish()))
    f = fr(); f.raw(8, bytes([0x40]) + lit(4) + bytes([5, 0, 0x00])); out.append(("an offset in front of the frame's first byte", f.finish()))
    f = fr(); f.stored(lit(12)); f.raw(4, bytes([0x00, 13, 0, 0x00])); out.append(("an offset in front of the frame, second block", f.finish()))
    f = fr(); f.raw(3, bytes([0x50]) + lit(2)); out.append(("literals past the block", f.finish()))
    f = fr(); f.raw(3, bytes([0xF0, 255, 255])); out.append(("a literal extension past the block", f.finish()))
    f = fr(); f.raw(6, bytes([0x4F]) + lit(4) + bytes([1])); out.append(("one offset byte", f.finish()))
    f = fr(); f.raw(8, bytes([0x4F]) + lit(4) + bytes([1, 0, 255])); out.append(("a match extension past the block", f.finish()))
    f = fr(); f.raw(7, bytes([0x40]) + lit(4) + bytes([1, 0])); out.append(("a block that ends on a match", f.finish()))
    f = fr(); f.stored(good); f.body += struct.pack("<I", 5000) + b"\x00" * 40; out.append(("a block that runs past the packet", f.finish(end_mark=False)))
    f = fr(); f.raw(0x80000000 | 65537, b"\x11" * 65537); out.append(("a stored block beyond the block maximum", f.finish()))
    run = bytes([0x1F, 0x22, 1, 0]) + b"\xff" * 256 + bytes([237, 0x00])
    f = fr(); f.raw(len(run), run); out.append(("a block that inflates beyond the block maximum", f.finish()))
    f = fr(); f.stored(good); out.append(("a missing end mark", f.finish(end_mark=False)))
    f = fr(); f.stored(good); out.append(("bytes behind the frame", f.finish(trailing=b"\x00")))
    f = fr(); f.stored(good); out.append(("legacy magic", f.finish(magic=0x184C2102)))
    f = fr(); f.stored(good); out.append(("skippable magic", f.finish(magic=0x184D2A50)))
    f = fr(); f.stored(good); out.append(("no magic", f.finish(magic=0x184D2205)))
    f = fr(); f.stored(good); out.append(("version 10", f.finish(version=2)))
    f = fr(); f.stored(good); out.append(("a reserved FLG bit", f.finish(flg_or=2)))
    f = fr(); f.stored(good); out.append(("a dictionary id", f.finish(flg_or=1)))
    f = fr(); f.stored(good); out.append(("a reserved BD bit", f.finish(bd_or=1)))
    f = fr(block_max=3); f.stored(good); out.append(("block maximum 3", f.finish()))
    f = fr(content_size=True); f.stored(good); out.append(("a wrong content size", f.finish(content_size_value=len(good) + 1)))
    out.append(("a frame cut short", AW.lz4_stored_frame(good)[:6]))
    out.append(("nothing", b""))
    # the FlatBuffer inside a good frame
    bad = bytearray(good); bad[len(good) - 16 * 20 - 1] = 0x40      # the count's high byte
    out.append(("a count beyond the packet", AW.lz4_stored_frame(bytes(bad))))
    out.append(("a vector cut short", AW.lz4_stored_frame(good[:-1])))
    bad = bytearray(good); bad[4:8] = struct.pack("<I", 1 << 20)
    out.append(("a root outside the packet", AW.lz4_stored_frame(bytes(bad))))
    out.append(("another identifier", AW.lz4_stored_frame(AW.event_packet(ramp(20), identifier=b"FRME"))))
    out.append(("a FlatBuffer cut short", AW.lz4_stored_frame(good[:11])))
    return out


def test_malformed_packets_are_refused_by_name_and_the_context_stays_usable(ctx):
    good = AW.lz4_compressed_frame(AW.event_packet(ramp(700, seed=9)))
    good_file = AW.build_file([(1, good), (1, good)], AW.LZ4)
    cases = malformed_frames()
    assert len(cases) == 29
    for name, data in cases:
        f = AW.build_file([(1, good), (2, AW.lz4_stored_frame(AW.foreign_packet(90))), (1, data), (1, good)], AW.LZ4)
        with pytest.raises(AO.Invalid):
            AO.decode(f)
        table, tinfo = ctx.aedat4_index_packets(f)       # (the indexer opens the first packet of each stream only)
        assert len(table) == 3
        where = "event packet 1 (data at byte %d of the file)" % int(table[1]["offset_of_data"])
        for call in (lambda: ctx.events_from_aedat4(f, AW.LZ4, table, capacity=4096), lambda: ctx.aedat4_count_events(f, AW.LZ4, table)):
            with pytest.raises(eventcalib_amd.EcalError) as e:
                call()
            assert e.value.status == -1 and where in str(e.value) and "AEDAT 4" in str(e.value), (name, str(e.value))
        got, info = ctx.events_from_aedat4(good_file, AW.LZ4, ctx.aedat4_index_packets(good_file)[0], time_base=T0)
        assert info["n_events"] == 1400, name
    # the same with no compression: the FlatBuffer cases alone
    good_fb = AW.event_packet(ramp(20))
    for data in (good_fb[:-1], good_fb[:11], AW.event_packet(ramp(20), identifier=b"IMUS")):
        f = AW.build_file([(1, good_fb), (1, data), (1, good_fb)], AW.NONE)
        table, _ = ctx.aedat4_index_packets(f, stream_id=1)
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.events_from_aedat4(f, AW.NONE, table, capacity=100)
        assert e.value.status == -1 and "event packet 1 (data at byte %d of the file)" % int(table[1]["offset_of_data"]) in str(e.value)
    # a table that points outside the file, and the lowest bad index of several
    f = AW.build_file([(1, good), (1, cases[0][1]), (1, cases[1][1])], AW.LZ4)
    table, _ = ctx.aedat4_index_packets(f)
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat4(f, AW.LZ4, table, capacity=4096)
    assert "event packet 1 " in str(e.value)
    far = table.copy()
    far["offset_of_data"][2] = len(f) - 3
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat4(good_file, AW.LZ4, far, capacity=4096)
    assert e.value.status == -1
    # the host refuses a first packet that is malformed, a negative size, and the chain's own errors, by name
    for name, data in cases[:3]:
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.aedat4_index_packets(AW.build_file([(1, data), (1, good)], AW.LZ4))
        assert e.value.status == -1 and "AEDAT 4" in str(e.value) and "packet 0" in str(e.value)
    f = bytearray(AW.build_file([(1, good), (1, good)], AW.LZ4, data_table=False))
    second = AO.index(bytes(f))[0][1][0] - 8
    f[second + 4:second + 8] = struct.pack("<i", -5)
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.aedat4_index_packets(bytes(f))
    assert e.value.status == -1 and "packet 1 at byte %d" % second in str(e.value)


def test_refusals_by_name(ctx, tmp_path):
    fb = AW.event_packet(ramp(10))
    for comp, word in ((AW.ZSTD, "ZSTD"), (AW.ZSTD_HIGH, "ZSTD_HIGH"), (9, "compression value 9")):
        f = AW.build_file([(1, fb)], comp)
        for call in (lambda: ctx.aedat4_index_packets(f), lambda: ctx.aedat4_parse_header(f)):
            with pytest.raises(eventcalib_amd.EcalError) as e:
                call()
            assert e.value.status == -1 and word in str(e.value) and "AEDAT 4" in str(e.value)
        path = str(tmp_path / "z.aedat4")
        open(path, "wb").write(f)
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.stream_from_aedat4_file(path)
        assert e.value.status == -1 and word in str(e.value) and "AEDAT 4" in str(e.value)
        assert "record with LZ4 or without compression" in str(e.value) or comp == 9     # (the ZSTD texts say what to do)
    # a stereo recording: two streams of events, refused with their ids; naming one reads it
    f = AW.build_file([(0, AW.lz4_stored_frame(fb)), (5, AW.lz4_stored_frame(AW.foreign_packet(64))), (7, AW.lz4_stored_frame(fb))], AW.LZ4)
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.aedat4_index_packets(f)
    assert e.value.status == -1 and "0, 7" in str(e.value)
    check(ctx, f, stream_id=7)
    f = AW.build_file([(4, AW.lz4_stored_frame(AW.foreign_packet(64))), (6, AW.lz4_stored_frame(AW.foreign_packet(64)))], AW.LZ4)
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.aedat4_index_packets(f)
    assert e.value.status == -1 and "4, 6" in str(e.value)
    with pytest.raises(eventcalib_amd.EcalError) as e:       # a named stream must carry EVTS
        ctx.aedat4_index_packets(f, stream_id=4)
    assert e.value.status == -1
    # headers
    for data, word in ((AW.VERSION_LINE, "AEDAT 4"), (b"#!AER-DAT3.1\r\n#!END-HEADER\r\n", "AEDAT 4"),
                       (AW.build_file([(1, fb)], AW.NONE, identifier=b"XXXX"), "IOHE")):
        with pytest.raises(eventcalib_amd.EcalError) as e:
            ctx.aedat4_parse_header(data)
        assert e.value.status == -1 and word in str(e.value)
    f = AW.build_file([(1, fb)], AW.NONE)
    comp, begin, end = ctx.aedat4_parse_header(f)
    assert (comp, begin, end) == AO.parse_header(f)
    assert ctx.aedat4_parse_header(f[:begin], file_bytes=len(f)) == (comp, begin, end)
    # the 3.1 / 2.0 entry points still refuse the version by name
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.aedat_parse_header(AW.VERSION_LINE)
    assert e.value.status == -1 and "4.0" in str(e.value)


def test_capacity_protocol_and_limits(ctx, B):
    packets = [ramp(B + 5, seed=1), ramp(700, t0=T0 + 10_000, seed=2)]
    f = event_file(packets, AW.LZ4)
    table, tinfo = ctx.aedat4_index_packets(f)
    n = B + 705
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat4(f, AW.LZ4, table, capacity=n - 1, time_base=T0)
    assert e.value.status == -6 and e.value.info["n_events"] == n
    got, info = ctx.events_from_aedat4(f, AW.LZ4, table, capacity=n, time_base=T0)
    assert info["n_events"] == n and got.numel() == 25 * n
    check(ctx, f, capacity=n + 100)
    with pytest.raises(eventcalib_amd.EcalError) as e:      # the table counted first, then too small
        ctx.aedat4_index_packets(f, capacity=1)
    assert e.value.status == -6
    inflated = info["n_inflated_bytes"]
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat4(f, AW.LZ4, table, capacity=n, time_base=T0, max_inflated_bytes=inflated - 1)
    assert e.value.status == -6 and "max_inflated_bytes" in str(e.value)
    got, info = ctx.events_from_aedat4(f, AW.LZ4, table, capacity=n, time_base=T0, max_inflated_bytes=inflated)
    assert info["n_events"] == n
    with pytest.raises(eventcalib_amd.EcalError) as e:      # the _dev form wants its compression and an explicit base
        ctx.events_from_aedat4(f, AW.ZSTD, table, capacity=n)
    assert e.value.status == -1
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.events_from_aedat4(f, AW.LZ4, table, capacity=n, time_base=None)
    assert e.value.status == -1
    # nothing to decode
    for g in (AW.build_file([], AW.LZ4), AW.build_file([(1, AW.lz4_stored_frame(AW.event_packet(ramp(0))))], AW.LZ4)):
        data, info = check(ctx, g)
        assert data == b"" and info["n_events"] == 0


def test_frames_made_by_liblz4_decode_to_their_events(ctx):
    """frames this project's encoder did not write (LZ4F_compressFrame, tests/golden/aedat4_liblz4_frames.npz)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "aedat4_liblz4_frames.npz"))
    ev = np.frombuffer(z["events"].tobytes(), AW.EVENT_DTYPE)
    assert len(ev) == 300
    frames = [z[k].tobytes() for k in sorted(z.files) if k.startswith("frame")]
    assert len(frames) >= 3 and sum(len(f) for f in frames) <= 32768
    f = AW.build_file([(1, fr) for fr in frames], AW.LZ4)
    data, info = check(ctx, f, time_base=int(ev["t"][0]))
    rec = np.frombuffer(data, np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")]))
    assert len(rec) == 300 * len(frames)
    for k in range(len(frames)):
        part = rec[300 * k:300 * (k + 1)]
        assert (part["x"] == ev["x"]).all() and (part["y"] == ev["y"]).all() and (part["p"] == ev["on"]).all()
        assert (part["t"] == (ev["t"] - ev["t"][0]).astype(np.float64) * 1e-6).all()


# ---- the file forms --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compression", [AW.NONE, AW.LZ4])
def test_round_trip_through_a_file(ctx, tmp_path, B, compression):
    rng = np.random.default_rng(31)
    n = 5 * B + 123
    t = T0 + np.cumsum(rng.integers(0, 5, n))
    ev = AW.make_events(t, rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n))
    packets, a = [], 0
    while a < n:
        b = min(n, a + int(rng.integers(1, 2 * B)))
        packets.append(ev[a:b])
        if rng.integers(0, 3) == 0:
            packets.append((int(rng.integers(2, 4)), AW.foreign_packet(int(rng.integers(20, 5000)))))
        a = b
    f = event_file(packets, compression, compressed=True)
    path, out = str(tmp_path / "r.aedat4"), str(tmp_path / "r.bin")
    open(path, "wb").write(f)
    for opts in (dict(), dict(width=346, height=260, flip_y=True, start_time=0.253), dict(time_base=T0 - 5, end_time=0.006)):
        want, want_info = AO.decode(f, **opts)
        info = ctx.aedat4_to_bin(path, out, **opts)
        assert open(out, "rb").read() == want.tobytes()
        assert info == want_info
        events, info2, t_first, t_last = ctx.stream_from_aedat4_file(path, **opts)
        assert info2 == want_info and events.cpu().numpy().tobytes() == want.tobytes()       # (the file is in time order)
        rec = np.frombuffer(want.tobytes(), np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")]))
        assert t_first == rec["t"][0] and t_last == rec["t"][-1]
    events, t_first, t_last = calibrate.load_events_aedat4(ctx, path, width=346, height=260)
    assert events.numel() == 25 * n
    # a file that is not in time order comes out sorted
    g = event_file([ev[B:2 * B], ev[:B]], compression)
    open(path, "wb").write(g)
    events, info, t_first, t_last = ctx.stream_from_aedat4_file(path, time_base=T0)
    rec = np.frombuffer(events.cpu().numpy().tobytes(), np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")]))
    assert len(rec) == 2 * B and (np.diff(rec["t"]) >= 0).all() and info["first_stamp_us"] == int(ev["t"][B]) // 1000000 * 1000000
    # cut short before its header: refused with the words AEDAT 4
    open(path, "wb").write(AW.VERSION_LINE)
    with pytest.raises(eventcalib_amd.EcalError) as e:
        ctx.stream_from_aedat4_file(path)
    assert e.value.status == -1 and "AEDAT 4" in str(e.value)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_files(ctx, seed):
    rng = np.random.default_rng(100 + seed)
    for trial in range(4):
        compression = AW.LZ4 if trial % 2 else AW.NONE
        packets, t = [], T0 + int(rng.integers(0, 10**6))
        for _ in range(int(rng.integers(1, 14))):
            if rng.integers(0, 4) == 0:
                packets.append((int(rng.integers(2, 5)), AW.foreign_packet(int(rng.integers(12, 9000)), seed=int(rng.integers(0, 99)))))
                continue
            n = int(rng.choice([0, 1, 17, 300, 1500]))
            tt = t + np.cumsum(rng.integers(-1, 12, n)) if n else np.zeros(0, np.int64)
            ev = AW.make_events(tt, rng.integers(-3, 360, n), rng.integers(-3, 270, n), rng.integers(0, 3, n))
            t = int(tt[-1]) if n else t
            packets.append(AW.event_packet(ev, vtable_after=bool(rng.integers(0, 2)), vector_mod=int(rng.integers(0, 16)), extra_fields=int(rng.integers(0, 3))))
        f = event_file(packets, compression, compressed=bool(rng.integers(0, 2)), data_table=bool(rng.integers(0, 2)))
        if not any(not isinstance(p, tuple) for p in packets):
            continue
        span = 0.02
        check(ctx, f, width=int(rng.choice([0, 346])), height=int(rng.choice([0, 260])), start_time=float(rng.choice([-INF, 0.3])),
              end_time=None if rng.integers(0, 2) else 0.25 + span * float(rng.random()))
