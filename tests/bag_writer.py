"""Helper of the bag ingest tests (no test in here): a writer of valid ROS 1 bags, format 2.0, and a plain decoder written from the
contract of include/ecal.h ("bag ingest") as the oracle — nothing of eventcalib_amd/csrc/bag_events.hpp.

The writer lays a bag out as `rosbag record` does: the version line, a bag header record padded to 4096 bytes, chunks (connection
records in front of the first message of each connection, then message records) each followed by its index data records, and at
index_pos the connection records and one chunk info record per chunk.  Knobs: the frame_id length of a message, foreign messages of
any size, messages per chunk, unchunked messages, the compression name, the version line."""
import struct

import numpy as np

MAGIC = b"#ROSBAG V2.0\n"
EVENT_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("secs", "<u4"), ("nsecs", "<u4"), ("p", "u1")])     # packed: 13 bytes
assert EVENT_DTYPE.itemsize == 13
REC = np.dtype([("t", "<f8"), ("x", "<f8"), ("y", "<f8"), ("p", "u1")])                                  # packed: 25 bytes
assert REC.itemsize == 25
MESSAGE_DTYPE = np.dtype([("offset_of_first_event", "<u8"), ("n_events", "<u4"), ("reserved", "<u4")])
DVS, PROPHESEE = "dvs_msgs/EventArray", "prophesee_event_msgs/EventArray"
OP_MESSAGE, OP_BAG_HEADER, OP_INDEX, OP_CHUNK, OP_CHUNK_INFO, OP_CONNECTION = 2, 3, 4, 5, 6, 7


# ---- records ------------------------------------------------------------------------------------------------------------------------
def field(name, value):
    body = name.encode() + b"=" + (value if isinstance(value, bytes) else value.encode())
    return struct.pack("<I", len(body)) + body


def record(header, data):
    return struct.pack("<I", len(header)) + header + struct.pack("<I", len(data)) + data


def op(code):
    return field("op", bytes([code]))


def events_array(x, y, secs, nsecs, p):
    """the event fields (arrays or lists of equal length) as an EVENT_DTYPE array"""
    e = np.zeros(len(x), EVENT_DTYPE)
    e["x"], e["y"], e["secs"], e["nsecs"], e["p"] = x, y, secs, nsecs, p
    return e


def event_array_message(events, seq=0, stamp=(0, 0), frame_id=b"", height=260, width=346):
    """a serialised dvs_msgs/EventArray: header (seq, stamp, frame_id), height, width, the events (an EVENT_DTYPE array)"""
    events = np.asarray(events, EVENT_DTYPE)
    return struct.pack("<IIII", seq, stamp[0], stamp[1], len(frame_id)) + frame_id + struct.pack("<III", height, width, len(events)) + events.tobytes()


def connection_record(conn, topic, type_, extra_header=b""):
    data = field("topic", topic) + field("type", type_) + field("md5sum", "5e8beee5a6c107e504c2e78903c224b8") + \
        field("message_definition", "# an array of events\nHeader header\nuint32 height\nuint32 width\nEvent[] events\n")
    return record(op(OP_CONNECTION) + field("conn", struct.pack("<I", conn)) + field("topic", topic) + extra_header, data)


def message_record(conn, data, time=(0, 0)):
    return record(op(OP_MESSAGE) + field("conn", struct.pack("<I", conn)) + field("time", struct.pack("<II", *time)), data)


def chunk_record(inner, compression="none", size=None):
    return record(op(OP_CHUNK) + field("compression", compression) + field("size", struct.pack("<I", len(inner) if size is None else size)), inner)


def bag_header_record(index_pos, conn_count, chunk_count):
    header = op(OP_BAG_HEADER) + field("index_pos", struct.pack("<Q", index_pos)) + field("conn_count", struct.pack("<I", conn_count)) + \
        field("chunk_count", struct.pack("<I", chunk_count))
    return record(header, b" " * (4096 - 8 - len(header)))     # the record is 4096 bytes in all


def write_bag(connections, messages, per_chunk=4, index=True, magic=MAGIC, compression="none", closed=True):
    """connections: [(conn id, topic, type)].  messages: [(conn id, data bytes)] in file order, or (conn id, data, (secs, nsecs)).
    per_chunk: messages per chunk (an int, or a list of ints used in turn; 0 = the messages stand at top level, unchunked).
    closed False: index_pos = 0 and nothing behind the last chunk, as a recording that was never closed.  -> the file's bytes"""
    conn_of = {c[0]: c for c in connections}
    sizes = [per_chunk] if isinstance(per_chunk, int) else list(per_chunk)
    body, chunks, seen, at, k = bytearray(), [], set(), 0, 0
    pos0 = len(magic) + 4096
    while at < len(messages):
        take = sizes[k % len(sizes)]
        k += 1
        group = messages[at: at + (take or len(messages))]
        at += len(group)
        inner, counts, index_entries = bytearray(), {}, {}
        for m in group:
            conn, data, time = (m + ((0, 0),))[:3]
            if conn not in seen:
                seen.add(conn)
                inner += connection_record(*conn_of[conn])
            index_entries.setdefault(conn, []).append((time, len(inner)))
            inner += message_record(conn, data, time)
            counts[conn] = counts.get(conn, 0) + 1
        if take == 0:
            body += inner
            continue
        chunks.append((pos0 + len(body), counts))
        body += chunk_record(bytes(inner), compression)
        if index:
            for conn, entries in index_entries.items():
                data = b"".join(struct.pack("<III", t[0], t[1], off) for t, off in entries)
                body += record(op(OP_INDEX) + field("ver", struct.pack("<I", 1)) + field("conn", struct.pack("<I", conn)) +
                               field("count", struct.pack("<I", len(entries))), data)
    index_pos = pos0 + len(body)
    tail = b""
    if closed:
        for c in connections:
            tail += connection_record(*c)
        for chunk_pos, counts in chunks:
            data = b"".join(struct.pack("<II", conn, n) for conn, n in counts.items())
            tail += record(op(OP_CHUNK_INFO) + field("ver", struct.pack("<I", 1)) + field("chunk_pos", struct.pack("<Q", chunk_pos)) +
                           field("start_time", struct.pack("<II", 0, 0)) + field("end_time", struct.pack("<II", 0, 0)) +
                           field("count", struct.pack("<I", len(counts))), data)
    return magic + bag_header_record(index_pos if closed else 0, len(connections), len(chunks)) + bytes(body) + tail


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
class BagError(ValueError):
    """what the library answers with ECAL_ERR_INVALID"""


def parse_fields(h):
    out, p = {}, 0
    while p < len(h):
        if len(h) - p < 4:
            raise BagError("a field that runs past its header")
        (fl,) = struct.unpack_from("<I", h, p)
        p += 4
        if fl > len(h) - p or b"=" not in h[p: p + fl]:
            raise BagError("a field that runs past its header, or without '='")
        name, value = h[p: p + fl].split(b"=", 1)
        out[name] = value
        p += fl
    return out


def index_messages(data, topic=None, type=None):
    """The chain of records by the contract -> (table as a MESSAGE_DTYPE array, info dict).  BagError for every refusal."""
    info = dict(n_raw_events=0, n_messages=0, n_other_messages=0, n_chunks=0, n_connections=0, n_trailing_bytes=0, first_stamp_ns=0,
                msg_width=0, msg_height=0)
    n = len(data)
    if data[:13] != MAGIC:
        if data[:9] == b"#ROSBAG V":
            raise BagError("version " + data[9:32].split(b"\n")[0].decode("latin1"))
        if data[:16] == b"SQLite format 3\0":
            raise BagError("ROS 2 bag (SQLite)")
        if data[:8] == b"\x89MCAP0\r\n":
            raise BagError("ROS 2 / MCAP")
        raise BagError("not a bag")
    accepted = (type,) if type else (DVS, PROPHESEE)
    conns, table, state = {}, [], dict(number=0, cut=False, first=True, stamp=False, event_topics=[])

    def walk(pos, end, inner):
        lim = min(end, n)
        while pos < end and not state["cut"]:
            rec = pos

            def there(at, count):
                """True: the bytes are there.  False: the file ends first (the chain ends here).  BagError: past a whole chunk"""
                if at + count <= lim:
                    return True
                if inner and end <= n:
                    raise BagError("record %d at byte %d runs past its chunk" % (state["number"], rec))
                info["n_trailing_bytes"], state["cut"] = n - rec, True
                return False
            if not there(pos, 4):
                return
            (hl,) = struct.unpack_from("<I", data, pos)
            if not there(pos + 4, hl + 4):
                return
            try:
                h = parse_fields(data[pos + 4: pos + 4 + hl])
            except BagError as e:
                raise BagError("record %d at byte %d: %s" % (state["number"], rec, e))
            (dl,) = struct.unpack_from("<I", data, pos + 4 + hl)
            body = pos + 8 + hl

            def bad(why):
                return BagError("record %d at byte %d: %s" % (state["number"], rec, why))
            if len(h.get(b"op", b"")) != 1:
                raise bad("no op")
            code = h[b"op"][0]
            if inner and code not in (OP_MESSAGE, OP_CONNECTION):
                raise bad("op 0x%02x inside a chunk" % code)
            if code == OP_CHUNK:
                if h.get(b"compression") != b"none":
                    raise bad("compression %s: rosbag decompress" % h.get(b"compression", b"?").decode("latin1"))
                if len(h.get(b"size", b"")) != 4 or struct.unpack("<I", h[b"size"])[0] != dl:
                    raise bad("size is not data_len")
                info["n_chunks"] += 1
                state["number"] += 1
                walk(body, body + dl, True)
                pos = body + dl
                continue
            if code not in (OP_MESSAGE, OP_CONNECTION, OP_BAG_HEADER, OP_INDEX, OP_CHUNK_INFO):
                raise bad("unknown op 0x%02x" % code)
            if not there(body, dl):
                return
            if code == OP_CONNECTION:
                if len(h.get(b"conn", b"")) != 4 or b"topic" not in h:
                    raise bad("connection without conn or topic")
                try:
                    d = parse_fields(data[body: body + dl])
                except BagError as e:
                    raise bad(str(e))
                if b"type" not in d:
                    raise bad("connection without type")
                cid, entry = struct.unpack("<I", h[b"conn"])[0], (h[b"topic"].decode("latin1"), d[b"type"].decode("latin1"))
                if cid in conns:
                    if conns[cid] != entry:
                        raise bad("connection %d redefined" % cid)
                else:
                    conns[cid] = entry
                    info["n_connections"] += 1
                    if entry[1] in accepted and not topic and entry[0] not in state["event_topics"]:
                        state["event_topics"].append(entry[0])
                        if len(state["event_topics"]) > 1:
                            raise bad("more than one topic of events: " + ", ".join(state["event_topics"]))
            elif code == OP_MESSAGE:
                if len(h.get(b"conn", b"")) != 4:
                    raise bad("message without conn")
                cid = struct.unpack("<I", h[b"conn"])[0]
                if cid not in conns:
                    raise bad("message of an undefined connection")
                ctopic, ctype = conns[cid]
                if ctype in accepted and (not topic or ctopic == topic):
                    if dl < 28:
                        raise bad("message length")
                    (L,) = struct.unpack_from("<I", data, body + 12)
                    if 28 + L > dl:
                        raise bad("message length")
                    height, width, count = struct.unpack_from("<III", data, body + 16 + L)
                    if 28 + L + 13 * count != dl:
                        raise bad("message length: not 28 + L + 13 n")
                    table.append((body + 28 + L, count, 0))
                    if state["first"]:
                        state["first"], info["msg_width"], info["msg_height"] = False, width, height
                    if count and not state["stamp"]:
                        state["stamp"] = True
                        info["first_stamp_ns"] = struct.unpack_from("<I", data, body + 28 + L + 4)[0] * 1000000000
                    info["n_messages"] += 1
                    info["n_raw_events"] += count
                else:
                    info["n_other_messages"] += 1
            state["number"] += 1
            pos = body + dl

    walk(13, n, False)
    if not any(t in accepted and (not topic or tp == topic) for tp, t in conns.values()):
        raise BagError("no connection of events; the bag has: " + ", ".join("%s (%s)" % c for c in conns.values()))
    return np.array(table, dtype=MESSAGE_DTYPE), info


def decode_table(data, table, time_base, width=0, height=0, flip_x=False, flip_y=False, start_time=-float("inf"), end_time=None):
    """the events of the table's messages in file order through the conversion and the filter -> (records' bytes, counters)"""
    parts = [np.frombuffer(data, EVENT_DTYPE, int(m["n_events"]), int(m["offset_of_first_event"])) for m in table if m["n_events"]]
    e = np.concatenate(parts) if parts else np.zeros(0, EVENT_DTYPE)
    x, y = e["x"].astype(np.int64), e["y"].astype(np.int64)
    t_ns = e["secs"].astype(np.int64) * 1000000000 + e["nsecs"].astype(np.int64)
    t = (t_ns - np.int64(time_base)).astype(np.float64) * 1e-9
    outside = ((x >= width) if width else np.zeros(len(e), bool)) | ((y >= height) if height else np.zeros(len(e), bool))
    negative = ~outside & (t < 0)
    live = ~outside & ~negative
    stop = live & (t >= end_time) if end_time is not None else np.zeros(len(e), bool)
    first_stop = int(np.argmax(stop)) if stop.any() else len(e)
    front = np.arange(len(e)) < first_stop
    before = live & (t < start_time)
    keep = live & ~before & front
    out = np.zeros(int(keep.sum()), REC)
    out["t"] = t[keep]
    out["x"] = (width - 1 - x[keep]) if flip_x else x[keep]
    out["y"] = (height - 1 - y[keep]) if flip_y else y[keep]
    out["p"] = e["p"][keep] != 0
    counters = dict(n_raw_events=len(e), n_events=len(out), n_outside=int((outside & front).sum()), n_negative=int((negative & front).sum()),
                    n_before_start=int((before & front).sum()), n_after_end=len(e) - first_stop)
    return out.tobytes(), counters


def decode(data, topic=None, type=None, time_base=None, **flt):
    """the whole contract: index, the base (None: automatic), conversion and filter -> (records' bytes, info dict, table)"""
    table, info = index_messages(data, topic=topic, type=type)
    base = info["first_stamp_ns"] if time_base is None else int(time_base)
    records, counters = decode_table(data, table, base, **flt)
    info.update(counters)
    info["time_base"] = base
    return records, info, table
