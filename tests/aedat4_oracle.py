"""A sequential AEDAT 4 decoder for the tests, written from the contract in include/ecal.h ("aedat4 ingest") alone: the header, the
packet chain, the LZ4 frame, the FlatBuffer, the event, the filter.  It shares nothing with eventcalib_amd/csrc/aedat4_events.hpp and
nothing with tests/aedat4_writer.py."""
import struct

import numpy as np


class Invalid(Exception):
    """what the library answers with ECAL_ERR_INVALID"""


def _u16(b, i):
    return b[i] | (b[i + 1] << 8)


def _u32(b, i):
    return struct.unpack_from("<I", b, i)[0]


def _i32(b, i):
    return struct.unpack_from("<i", b, i)[0]


def _field(b, table, fid, nbytes):
    """byte offset of a table's field, 0 when absent"""
    if table + 4 > len(b):
        raise Invalid("table")
    vt = table - _i32(b, table)
    if vt < 0 or vt + 4 > len(b):
        raise Invalid("vtable")
    if _u16(b, vt) < 6 + 2 * fid:
        return 0
    if vt + 6 + 2 * fid > len(b):
        raise Invalid("vtable")
    fo = _u16(b, vt + 4 + 2 * fid)
    if not fo:
        return 0
    if table + fo + nbytes > len(b):
        raise Invalid("field")
    return table + fo


def parse_header(f):
    """-> (compression, packets_begin, packets_end)"""
    if f[:14] != b"#!AER-DAT4.0\r\n"[: max(0, min(14, len(f)))] or len(f) < 18:
        raise Invalid("AEDAT 4 version line / cut short")
    n = _u32(f, 14)
    begin = 18 + n
    if begin > (1 << 20) or begin > len(f):
        raise Invalid("AEDAT 4 header")
    fb = f[18:begin]
    if n < 8 or fb[4:8] != b"IOHE":
        raise Invalid("AEDAT 4 identifier")
    table = _u32(fb, 0)
    compression, position = 0, -1
    a = _field(fb, table, 0, 4)
    if a:
        compression = _i32(fb, a)
    a = _field(fb, table, 1, 8)
    if a:
        position = struct.unpack_from("<q", fb, a)[0]
    if compression in (3, 4):
        raise Invalid("AEDAT 4 ZSTD")
    if compression < 0 or compression > 4:
        raise Invalid("AEDAT 4 compression %d" % compression)
    end = len(f)
    if position >= 0:
        if position < begin or position > len(f):
            raise Invalid("AEDAT 4 dataTablePosition")
        end = position
    return compression, begin, end


def chain(f, begin, end):
    """-> ([(stream_id, data offset, size)], trailing bytes)"""
    out, pos = [], begin
    while pos < end:
        if end - pos < 8:
            return out, end - pos
        sid, size = struct.unpack_from("<ii", f, pos)
        if size < 0:
            raise Invalid("AEDAT 4 packet %d at byte %d: negative size" % (len(out), pos))
        if size > end - pos - 8:
            return out, end - pos
        out.append((sid, pos + 8, size))
        pos += 8 + size
    return out, 0


def _extend(d, p, end, v):
    if v == 15:
        while True:
            if p >= end:
                raise Invalid("extension past the block")
            b = d[p]
            p += 1
            v += b
            if b != 255:
                break
    return v, p


def lz4_frame(d):
    """the bytes one LZ4 frame inflates to"""
    n = len(d)
    if n < 7:
        raise Invalid("frame cut short")
    magic = _u32(d, 0)
    if magic != 0x184D2204:
        raise Invalid("magic %08x" % magic)
    flg, bd = d[4], d[5]
    if flg >> 6 != 1 or flg & 3 or bd & 0x8F or ((bd >> 4) & 7) < 4:
        raise Invalid("frame header")
    block_max = 1 << (8 + 2 * ((bd >> 4) & 7))
    pos, size = 6, None
    if flg & 8:
        if n - pos < 8:
            raise Invalid("frame cut short")
        size = struct.unpack_from("<Q", d, pos)[0]
        pos += 8
    if n - pos < 1:
        raise Invalid("frame cut short")
    pos += 1
    out = bytearray()
    while True:
        if n - pos < 4:
            raise Invalid("no end mark")
        s = _u32(d, pos)
        pos += 4
        if s == 0:
            break
        ln = s & 0x7FFFFFFF
        if ln > n - pos:
            raise Invalid("block past the packet")
        if s >> 31:
            if ln > block_max:
                raise Invalid("block too big")
            out += d[pos:pos + ln]
        else:
            p, end, start = pos, pos + ln, len(out)
            while True:
                if p >= end:
                    raise Invalid("block ends without its last literals")
                tok = d[p]
                p += 1
                lit, p = _extend(d, p, end, tok >> 4)
                if lit > end - p:
                    raise Invalid("literals past the block")
                out += d[p:p + lit]
                p += lit
                if len(out) - start > block_max:
                    raise Invalid("block too big")
                if p == end:
                    break
                if end - p < 2:
                    raise Invalid("offset past the block")
                off = _u16(d, p)
                p += 2
                if off == 0 or off > len(out):
                    raise Invalid("offset %d" % off)
                ml, p = _extend(d, p, end, tok & 15)
                ml += 4
                if len(out) - start + ml > block_max:
                    raise Invalid("block too big")
                m = len(out) - off
                if off >= ml:
                    out += out[m:m + ml]
                else:
                    for k in range(ml):
                        out.append(out[m + k % off])
        pos += ln
        if flg & 16:
            if n - pos < 4:
                raise Invalid("no end mark")
            pos += 4
    if flg & 4:
        if n - pos < 4:
            raise Invalid("frame cut short")
        pos += 4
    if pos != n:
        raise Invalid("bytes behind the frame")
    if size is not None and size != len(out):
        raise Invalid("content size")
    return bytes(out)


def packet_events(b):
    """the EventPacket FlatBuffer -> a structured array of its events"""
    dt = np.dtype([("t", "<i8"), ("x", "<i2"), ("y", "<i2"), ("on", "u1"), ("pad", "u1", (3,))])
    if len(b) == 0:
        return np.zeros(0, dt)
    if len(b) < 12:
        raise Invalid("FlatBuffer cut short")
    if b[8:12] != b"EVTS":
        raise Invalid("identifier")
    table = 4 + _u32(b, 4)
    p = _field(b, table, 0, 4)
    if not p:
        return np.zeros(0, dt)
    vec = p + _u32(b, p)
    if vec + 4 > len(b):
        raise Invalid("vector")
    count = _u32(b, vec)
    if vec + 4 + 16 * count > len(b):
        raise Invalid("vector")
    return np.frombuffer(b, dt, count, vec + 4)


def inflate(f, compression, off, size):
    data = f[off:off + size]
    return data if compression == 0 else lz4_frame(data)


INFO_KEYS = ("n_raw_events", "n_events", "n_outside", "n_negative", "n_before_start", "n_after_end", "n_packets", "n_other_packets",
             "n_trailing_bytes", "n_compressed_bytes", "n_inflated_bytes", "first_stamp_us", "time_base", "compression", "stream_id")


def index(f, stream_id=-1):
    """-> (table [(data offset, size)], info dict of the indexer's fields)"""
    f = bytes(f)
    compression, begin, end = parse_header(f)
    packets, trailing = chain(f, begin, end)
    chosen = stream_id
    if stream_id < 0:
        seen, with_events = [], []
        for sid, off, size in packets:
            if sid in seen:
                continue
            seen.append(sid)
            b = inflate(f, compression, off, size)
            if len(b) >= 12 and b[8:12] == b"EVTS":
                with_events.append(sid)
        if len(with_events) > 1:
            raise Invalid("AEDAT 4: streams of events " + ", ".join(map(str, with_events)))
        if not with_events and packets:
            raise Invalid("AEDAT 4: no stream of events among " + ", ".join(map(str, seen)))
        chosen = with_events[0] if with_events else -1
    table = [(off, size) for sid, off, size in packets if sid == chosen]
    first = 0
    for k, (off, size) in enumerate(table):
        try:
            ev = packet_events(inflate(f, compression, off, size))
        except Invalid as e:
            raise Invalid("AEDAT 4: event packet %d (data at byte %d): %s" % (k, off, e))
        if len(ev):
            first = int(ev["t"][0]) // 1000000 * 1000000
            break
    info = dict(n_packets=len(table), n_other_packets=len(packets) - len(table), n_trailing_bytes=trailing,
                n_compressed_bytes=sum(s for _, s in table), compression=compression, stream_id=chosen, first_stamp_us=first)
    return table, info


def decode(f, stream_id=-1, time_base=None, width=0, height=0, flip_x=False, flip_y=False, start_time=None, end_time=None):
    """-> (records: uint8 [n * 25], info dict with every key of INFO_KEYS).  time_base None: automatic."""
    f = bytes(f)
    table, info = index(f, stream_id)
    parts, inflated = [], 0
    for k, (off, size) in enumerate(table):
        try:
            b = inflate(f, info["compression"], off, size)
            parts.append(packet_events(b))
        except Invalid as e:
            raise Invalid("AEDAT 4: event packet %d (data at byte %d): %s" % (k, off, e))
        inflated += len(b)
    dt = np.dtype([("t", "<i8"), ("x", "<i2"), ("y", "<i2"), ("on", "u1"), ("pad", "u1", (3,))])
    ev = np.concatenate(parts) if parts else np.zeros(0, dt)
    base = info["first_stamp_us"] if time_base is None else int(time_base)
    x, y = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
    outside = (x < 0) | (y < 0)
    if width:
        outside |= x >= width
    if height:
        outside |= y >= height
    if flip_x:
        x = width - 1 - x
    if flip_y:
        y = height - 1 - y
    t = (ev["t"] - np.int64(base)).astype(np.float64) * 1e-6
    inside = ~outside
    stop = inside & (t >= 0) & (t >= end_time) if end_time is not None else np.zeros(len(ev), bool)
    n_live = int(np.argmax(stop)) if stop.any() else len(ev)
    live = np.arange(len(ev)) < n_live
    negative = live & inside & (t < 0)
    ok = live & inside & (t >= 0)
    before = ok & (t < start_time) if start_time is not None else np.zeros(len(ev), bool)
    keep = ok & ~before
    rec = np.zeros(int(keep.sum()), np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")]))
    rec["t"], rec["x"], rec["y"], rec["p"] = t[keep], x[keep], y[keep], ev["on"][keep] != 0
    info.update(n_raw_events=len(ev), n_events=len(rec), n_outside=int((live & outside).sum()), n_negative=int(negative.sum()),
                n_before_start=int(before.sum()), n_after_end=len(ev) - n_live, n_inflated_bytes=inflated, time_base=base)
    return np.frombuffer(rec.tobytes(), np.uint8), info
