"""Writes AEDAT 4 files for the tests, from include/ecal.h ("aedat4 ingest") and the published formats alone: a minimal FlatBuffer
builder for IOHeader and EventPacket, foreign packets, an LZ4 frame encoder (stored blocks; explicit sequences; a plain greedy
matcher) and xxHash32 for the frame's checksums.  A test tool: it shares no code with the library."""
import struct

import numpy as np

VERSION_LINE = b"#!AER-DAT4.0\r\n"
NONE, LZ4, LZ4_HIGH, ZSTD, ZSTD_HIGH = 0, 1, 2, 3, 4
EVENT_DTYPE = np.dtype([("t", "<i8"), ("x", "<i2"), ("y", "<i2"), ("on", "u1"), ("pad", "u1", (3,))])
assert EVENT_DTYPE.itemsize == 16


def make_events(t, x, y, on):
    ev = np.zeros(len(t), EVENT_DTYPE)
    ev["t"], ev["x"], ev["y"], ev["on"] = t, x, y, on
    return ev


# ---- xxHash32 (the LZ4 frame's checksums) ----------------------------------------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5, _M = 2654435761, 2246822519, 3266489917, 668265263, 374761393, 0xFFFFFFFF


def _rotl(v, r):
    return ((v << r) | (v >> (32 - r))) & _M


def xxh32(data, seed=0):
    data = bytes(data)
    n, i = len(data), 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        while i + 16 <= n:
            for k, w in enumerate(struct.unpack_from("<4I", data, i)):
                v[k] = (_rotl((v[k] + w * _P2) & _M, 13) * _P1) & _M
            i += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, i)[0] * _P3) & _M, 17) * _P4) & _M
        i += 4
    while i < n:
        h = (_rotl((h + data[i] * _P5) & _M, 11) * _P1) & _M
        i += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    h ^= h >> 16
    return h


# ---- FlatBuffers -----------------------------------------------------------------------------------------------------------------------
def io_header(compression=LZ4, data_table_position=-1, info_node=b"<dv version=\"2.0\"></dv>", identifier=b"IOHE", omit_compression=False,
              omit_position=False):
    """the size-prefixed IOHeader: u32 N and the N bytes"""
    vt = struct.pack("<5H", 10, 20, 0 if omit_compression else 4, 0 if omit_position else 8, 16) + b"\0\0"   # at byte 8, padded to 12
    table_at = 8 + len(vt)
    table = struct.pack("<iiqI", table_at - 8, compression, data_table_position, 4)   # the string follows the offset field directly
    body = struct.pack("<I", table_at) + identifier + vt + table + struct.pack("<I", len(info_node)) + info_node + b"\0"
    body += b"\0" * (-len(body) % 8)
    return struct.pack("<I", len(body)) + body


def event_packet(events, vtable_after=False, extra_fields=0, absent=False, vector_mod=None, identifier=b"EVTS", short_vtable=False):
    """the size-prefixed EventPacket FlatBuffer.  vtable_after: the vtable lies behind the table; extra_fields: further fields behind
    field 0; absent: field 0 is 0 in the vtable; short_vtable: a vtable of 4 bytes (no field at all); vector_mod: the first event's
    byte offset in the buffer is this modulo 16."""
    events = np.ascontiguousarray(events, EVENT_DTYPE)
    nf = 0 if short_vtable else 1 + extra_fields
    table = bytearray(4 + 4 * nf)   # soffset, then one u32 a field
    vt_fields = [0 if (absent and k == 0) else 4 + 4 * k for k in range(nf)]
    vt = struct.pack("<2H", 4 + 2 * nf, len(table)) + b"".join(struct.pack("<H", f) for f in vt_fields)
    vt += b"\0" * (-len(vt) % 4)
    head = 12   # size, root offset, identifier
    if vtable_after:
        table_at, vt_at = head, head + len(table)
    else:
        vt_at, table_at = head, head + len(vt)
    vec_at = head + len(vt) + len(table)
    if vector_mod is not None:
        vec_at += (vector_mod - (vec_at + 4)) % 16
    struct.pack_into("<i", table, 0, table_at - vt_at)
    if nf:
        struct.pack_into("<I", table, 4, vec_at - (table_at + 4))
    for k in range(1, nf):
        struct.pack_into("<I", table, 4 + 4 * k, 0xA5A50000 + k)
    buf = bytearray(vec_at)
    buf[4:8] = struct.pack("<I", table_at - 4)
    buf[8:12] = identifier
    buf[table_at:table_at + len(table)] = table
    buf[vt_at:vt_at + len(vt)] = vt
    if not (absent or short_vtable):
        buf += struct.pack("<I", len(events)) + events.tobytes()
    buf[0:4] = struct.pack("<I", len(buf) - 4)
    return bytes(buf)


def packet_prefix(n_events, **knobs):
    """the bytes of event_packet in front of the first event, for a vector of n_events (the events themselves come from elsewhere)"""
    full = event_packet(np.zeros(n_events, EVENT_DTYPE), **knobs)
    return full[: len(full) - 16 * n_events]


def foreign_packet(n_bytes, identifier=b"FRME", seed=0):
    body = np.random.default_rng(seed).integers(0, 256, max(0, n_bytes - 12), dtype=np.uint8).tobytes()
    return struct.pack("<II", 8 + len(body), 4) + identifier + body


# ---- LZ4 -------------------------------------------------------------------------------------------------------------------------------
def _length_bytes(v):
    """the extension bytes of a length whose nibble is 15: v = the length - 15"""
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


def lz4_block(seqs):
    """seqs: [(literals: bytes, offset: int or None, match_length: int)]; the last one has offset None.  -> the block's bytes"""
    out = bytearray()
    for lit, off, ml in seqs:
        ll = len(lit)
        tok = (min(ll, 15) << 4) | (0 if off is None else min(ml - 4, 15))
        out.append(tok)
        if ll >= 15:
            out += _length_bytes(ll - 15)
        out += lit
        if off is not None:
            out += struct.pack("<H", off)
            if ml - 4 >= 15:
                out += _length_bytes(ml - 4 - 15)
    return bytes(out)


def greedy_sequences(data, history=b""):
    """a plain greedy matcher over `data` (matches may reach into `history`, the frame's output so far): 4-byte hash chains of depth
    one, the format's end rules kept (the last 5 bytes are literals, no match starts within the last 12)"""
    buf = bytes(history) + bytes(data)
    h0, n = len(history), len(buf)
    table = {}
    for i in range(max(0, h0 - 65535), h0 - 3):
        table[buf[i:i + 4]] = i
    seqs, anchor, i = [], h0, h0
    while i + 12 < n:
        key = buf[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is not None and i - cand <= 65535:
            ml = 4
            while i + ml < n - 5 and buf[cand + ml] == buf[i + ml]:
                ml += 1
            seqs.append((buf[anchor:i], i - cand, ml))
            i += ml
            anchor = i
        else:
            i += 1
    seqs.append((buf[anchor:], None, 0))
    return seqs


class Lz4Frame:
    """One LZ4 frame, block by block.  .out is what it inflates to."""

    def __init__(self, block_max=4, independent=False, block_checksum=False, content_size=False, content_checksum=False):
        self.block_max, self.independent = block_max, independent
        self.block_checksum, self.content_size, self.content_checksum = block_checksum, content_size, content_checksum
        self.out = bytearray()
        self.body = bytearray()

    def max_bytes(self):
        return 1 << (8 + 2 * self.block_max)

    def _append(self, word, data):
        self.body += struct.pack("<I", word) + data
        if self.block_checksum:
            self.body += struct.pack("<I", xxh32(data))

    def stored(self, data):
        self.out += data
        self._append(0x80000000 | len(data), bytes(data))

    def block(self, seqs):
        """explicit sequences [(literals, offset or None, match_length)]"""
        for lit, off, ml in seqs:
            self.out += lit
            if off is not None:
                start = len(self.out) - off
                assert start >= 0
                for k in range(ml):
                    self.out.append(self.out[start + k])
        data = lz4_block(seqs)
        self._append(len(data), data)

    def compress(self, data):
        """the greedy matcher, in blocks of the block maximum (linked unless independent)"""
        for a in range(0, len(data), self.max_bytes()):
            part = bytes(data[a:a + self.max_bytes()])
            self.block(greedy_sequences(part, b"" if self.independent else bytes(self.out[-65535:])))

    def raw(self, word, data):
        """a block word and bytes as they are (malformed cases); .out is not touched"""
        self._append(word, bytes(data))

    def header(self, flg_or=0, bd_or=0, version=1, content_size_value=None, magic=0x184D2204):
        flg = (version << 6) | (int(self.independent) << 5) | (int(self.block_checksum) << 4) | (int(self.content_size) << 3) | \
            (int(self.content_checksum) << 2) | flg_or
        desc = bytes([flg, (self.block_max << 4) | bd_or])
        if self.content_size:
            desc += struct.pack("<Q", len(self.out) if content_size_value is None else content_size_value)
        return struct.pack("<I", magic) + desc + bytes([(xxh32(desc) >> 8) & 0xFF])

    def finish(self, end_mark=True, trailing=b"", **header):
        tail = struct.pack("<I", 0) if end_mark else b""
        if self.content_checksum and end_mark:
            tail += struct.pack("<I", xxh32(self.out))
        return self.header(**header) + bytes(self.body) + tail + trailing


def lz4_stored_frame(data, block_max=4, **flags):
    """stored blocks only: fast, for large files"""
    f = Lz4Frame(block_max, **flags)
    step = f.max_bytes()
    for a in range(0, len(data), step):
        f.stored(data[a:a + step])
    return f.finish()


def lz4_compressed_frame(data, block_max=4, **flags):
    f = Lz4Frame(block_max, **flags)
    f.compress(data)
    return f.finish()


# ---- the file --------------------------------------------------------------------------------------------------------------------------
def packet(stream_id, data):
    return struct.pack("<ii", stream_id, len(data)) + data


def build_file(packets, compression=LZ4, data_table=True, header=None, **header_knobs):
    """packets: [(stream_id, data bytes as the file has them)].  data_table: a dataTablePosition and some bytes behind the packets (not
    read by anyone); False: -1, a recording that was never closed.  -> the file's bytes"""
    chain = b"".join(packet(s, d) for s, d in packets)
    if header is None:
        probe = io_header(compression, 0, **header_knobs)
        position = len(VERSION_LINE) + len(probe) + len(chain) if data_table else -1
        header = io_header(compression, position, **header_knobs)
    table = struct.pack("<II", 24, 4) + b"FTAB" + b"\x5A" * 16 if data_table else b""
    return VERSION_LINE + header + chain + table


def wrap(data, compression, compressed=False, **frame):
    """a packet's FlatBuffer as the file has it under `compression`"""
    if compression == NONE:
        return data
    return lz4_compressed_frame(data, **frame) if compressed else lz4_stored_frame(data, **frame)
