// iniVation AEDAT 4 (DV) recordings into events — one restatement of include/ecal.h, "aedat4 ingest", for the kernels
// (ecal_aedat4.hip), the host decoder (EventStream::aedat42bin, host/event.hpp) and the CPU test (tests/cpp/check_aedat4_decode.cpp):
// the file header, the packet chain, the LZ4 frame walker and inflater, the FlatBuffer locator, the 16-byte event, the filter.
//
// What crosses bytes here is the LZ4 block: a sequence is found only behind the one before it, and a match copies what earlier
// sequences of the same FRAME produced.  Packets are frames of their own: nothing crosses packets.  So
//   sequential:  packet after packet, inflate, locate, the events in order
//   block-wise:  every packet's inflated size (a walk that produces nothing), the sizes scanned into spans of one scratch, every
//                packet inflated into its span, located, the counts scanned into an event-slot space, every block on its own
// give the same events.  a4_lz4_frame is the ONE walker: the size pass, the host inflater and the wave-cooperative inflater of the
// kernels are three sinks of it.
// Nothing here is floating point but a4_classify's one conversion and one multiplication.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>
#include "event_record.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_A4_HD __host__ __device__ __forceinline__
#else
#define ECAL_A4_HD inline
#endif

namespace ecal_aedat4 {

enum : int { A4_OK = 0, A4_INVALID = -1, A4_RANGE = -6 };   // ECAL_OK / ECAL_ERR_INVALID / ECAL_ERR_RANGE
enum : int { A4_COMP_NONE = 0, A4_COMP_LZ4 = 1, A4_COMP_LZ4_HIGH = 2, A4_COMP_ZSTD = 3, A4_COMP_ZSTD_HIGH = 4 };

// a decode block of the kernels: 256 threads x 4 consecutive event slots (ecal_aedat4_block_events)
constexpr uint32_t A4_BLOCK_THREADS = 256;
constexpr uint32_t A4_THREAD_EVENTS = 4;
constexpr uint32_t A4_BLOCK_EVENTS = A4_BLOCK_THREADS * A4_THREAD_EVENTS;

constexpr uint64_t A4_VERSION_BYTES = 14;                    // "#!AER-DAT4.0\r\n"
constexpr uint64_t A4_HEADER_LIMIT = 1u << 20;               // the IOHeader lies within the first MiB
constexpr uint64_t A4_DEFAULT_MAX_INFLATED = 1ull << 34;     // options.max_inflated_bytes by default: 16 GiB
constexpr uint32_t A4_EVENT_BYTES = 16;

// why a packet's data is refused (a4_why has the words); 0 = nothing wrong
enum : int {
    A4E_NONE = 0, A4E_FRAME_SHORT, A4E_MAGIC, A4E_LEGACY, A4E_SKIPPABLE, A4E_VERSION, A4E_RESERVED, A4E_DICT, A4E_BLOCK_MAX,
    A4E_NO_END_MARK, A4E_BLOCK_PAST_PACKET, A4E_BLOCK_TOO_BIG, A4E_TOKEN_PAST, A4E_EXT_PAST, A4E_LIT_PAST, A4E_OFFSET_PAST,
    A4E_OFFSET_ZERO, A4E_OFFSET_FRONT, A4E_BYTES_BEHIND, A4E_CONTENT_SIZE, A4E_FB_SHORT, A4E_FB_IDENT, A4E_FB_TABLE, A4E_FB_VTABLE,
    A4E_FB_FIELD, A4E_FB_VECTOR, A4E_TABLE_ENTRY, A4E_COUNT
};
inline const char *a4_why(int code) {
    static const char *const text[A4E_COUNT] = {
        "nothing wrong", "the LZ4 frame is cut short", "no LZ4 frame magic", "a legacy LZ4 frame", "a skippable LZ4 frame",
        "an LZ4 frame version that is not 01", "a reserved bit of the LZ4 frame header is set", "an LZ4 frame with a dictionary id",
        "an LZ4 block maximum below 4", "the LZ4 frame has no end mark", "an LZ4 block runs past the packet",
        "an LZ4 block inflates beyond the block maximum", "an LZ4 block ends without its last literals",
        "a length extension runs past the LZ4 block", "literals run past the LZ4 block", "offset bytes run past the LZ4 block",
        "a match offset of 0", "a match offset in front of the frame's first byte", "bytes behind the LZ4 frame",
        "the LZ4 frame's content size is not what its blocks inflate to", "the packet's FlatBuffer is cut short",
        "the packet's identifier is not EVTS", "the FlatBuffer's table lies outside the packet",
        "the FlatBuffer's vtable lies outside the packet", "the FlatBuffer's field 0 lies outside the packet",
        "the event vector lies outside the packet", "the table entry does not lie within the file"};
    return code > 0 && code < A4E_COUNT ? text[code] : "unknown";
}

ECAL_A4_HD uint32_t a4_le16(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8); }
ECAL_A4_HD uint32_t a4_le32(const uint8_t *p) {
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}
ECAL_A4_HD uint64_t a4_le64(const uint8_t *p) { return (uint64_t) a4_le32(p) | ((uint64_t) a4_le32(p + 4) << 32); }

// ---- the LZ4 frame walker ---------------------------------------------------------------------------------------------------------------
// rd(i): byte i of the packet's data, 0 <= i < n (the walker asks for nothing else).  sink.literals(i, len): the next len bytes of
// the output are the packet's bytes i .. i + len; sink.match(offset, len): the next len bytes repeat the output from `offset` bytes
// back (len may exceed offset: byte k is the byte at match start + k mod offset).  Every length is checked BEFORE the sink sees it:
// literals lie inside the packet, a match starts inside what the frame has produced, a block stays within the block maximum.
// Checksums are stepped over, not verified; the independence flag is read and not enforced (a match is held against what the frame
// has produced, whichever way the blocks were made).  *inflated = the bytes the frame produces.
template <class Rd, class Sink> ECAL_A4_HD int a4_lz4_frame(const Rd &rd, uint64_t n, Sink &sink, uint64_t *inflated) {
    *inflated = 0;
    if (n < 7) return A4E_FRAME_SHORT;
    const uint32_t magic = (uint32_t) rd(0) | ((uint32_t) rd(1) << 8) | ((uint32_t) rd(2) << 16) | ((uint32_t) rd(3) << 24);
    if (magic != 0x184D2204u) return magic == 0x184C2102u ? A4E_LEGACY : (magic & 0xFFFFFFF0u) == 0x184D2A50u ? A4E_SKIPPABLE : A4E_MAGIC;
    const uint32_t flg = rd(4), bd = rd(5);
    if ((flg >> 6) != 1u) return A4E_VERSION;
    if (flg & 2u) return A4E_RESERVED;
    if (flg & 1u) return A4E_DICT;
    if (bd & 0x8Fu) return A4E_RESERVED;
    const uint32_t bm = (bd >> 4) & 7u;
    if (bm < 4u) return A4E_BLOCK_MAX;
    const uint64_t block_max = 1ull << (8u + 2u * bm);
    const bool block_sums = (flg >> 4) & 1u, has_size = (flg >> 3) & 1u, content_sum = (flg >> 2) & 1u;
    uint64_t pos = 6, content_size = 0;
    if (has_size) {
        if (n - pos < 8) return A4E_FRAME_SHORT;
        for (uint32_t b = 0; b < 8; b++) content_size |= (uint64_t) rd(pos + b) << (8u * b);
        pos += 8;
    }
    if (n - pos < 1) return A4E_FRAME_SHORT;
    pos += 1;   // the header checksum
    uint64_t produced = 0;
    for (;;) {
        if (n - pos < 4) return A4E_NO_END_MARK;
        const uint32_t s = (uint32_t) rd(pos) | ((uint32_t) rd(pos + 1) << 8) | ((uint32_t) rd(pos + 2) << 16) | ((uint32_t) rd(pos + 3) << 24);
        pos += 4;
        if (s == 0u) break;
        const uint64_t len = s & 0x7FFFFFFFu;
        if (len > n - pos) return A4E_BLOCK_PAST_PACKET;
        if (s >> 31) {   // stored
            if (len > block_max) return A4E_BLOCK_TOO_BIG;
            sink.literals(pos, len);
            produced += len;
        } else {
            uint64_t bp = pos, bout = 0;
            const uint64_t be = pos + len;
            for (;;) {
                if (bp >= be) return A4E_TOKEN_PAST;
                const uint32_t tok = rd(bp++);
                uint64_t lit = tok >> 4;
                if (lit == 15u) {
                    uint32_t b;
                    do {
                        if (bp >= be) return A4E_EXT_PAST;
                        b = rd(bp++);
                        lit += b;
                    } while (b == 255u);
                }
                if (lit > be - bp) return A4E_LIT_PAST;
                if (lit > block_max - bout) return A4E_BLOCK_TOO_BIG;
                if (lit) sink.literals(bp, lit);
                bp += lit;
                bout += lit;
                produced += lit;
                if (bp == be) break;   // a block's last sequence ends behind its literals
                if (be - bp < 2) return A4E_OFFSET_PAST;
                const uint32_t off = (uint32_t) rd(bp) | ((uint32_t) rd(bp + 1) << 8);
                bp += 2;
                if (off == 0u) return A4E_OFFSET_ZERO;
                if (off > produced) return A4E_OFFSET_FRONT;
                uint64_t ml = tok & 15u;
                if (ml == 15u) {
                    uint32_t b;
                    do {
                        if (bp >= be) return A4E_EXT_PAST;
                        b = rd(bp++);
                        ml += b;
                    } while (b == 255u);
                }
                ml += 4u;
                if (ml > block_max - bout) return A4E_BLOCK_TOO_BIG;
                sink.match(off, ml);
                bout += ml;
                produced += ml;
            }
        }
        pos += len;
        if (block_sums) {
            if (n - pos < 4) return A4E_NO_END_MARK;
            pos += 4;
        }
    }
    if (content_sum) {
        if (n - pos < 4) return A4E_FRAME_SHORT;
        pos += 4;
    }
    *inflated = produced;
    if (pos != n) return A4E_BYTES_BEHIND;
    if (has_size && content_size != produced) return A4E_CONTENT_SIZE;
    return A4E_NONE;
}

struct A4PtrReader {
    const uint8_t *p;
    ECAL_A4_HD uint8_t operator()(uint64_t i) const { return p[i]; }
};
struct A4SizeSink {   // the size pass: nothing is produced
    ECAL_A4_HD void literals(uint64_t, uint64_t) {}
    ECAL_A4_HD void match(uint32_t, uint64_t) {}
};
// the inflated size of the frame in data[0, n), or why it is refused
ECAL_A4_HD int a4_lz4_size(const uint8_t *data, uint64_t n, uint64_t *inflated) {
    A4SizeSink sink;
    return a4_lz4_frame(A4PtrReader{data}, n, sink, inflated);
}
struct A4VectorSink {
    const uint8_t *data;
    std::vector<uint8_t> &out;
    void literals(uint64_t i, uint64_t len) { out.insert(out.end(), data + i, data + i + len); }
    void match(uint32_t off, uint64_t len) {
        const size_t start = out.size() - off;
        for (uint64_t k = 0; k < len; k++) out.push_back(out[start + k]);   // (byte after byte: an overlap repeats what it just wrote)
    }
};
// the host inflater: out = what the frame produces (sized first: a refused frame appends nothing)
inline int a4_lz4_inflate(const uint8_t *data, uint64_t n, std::vector<uint8_t> &out) {
    uint64_t size = 0;
    const int why = a4_lz4_size(data, n, &size);
    out.clear();
    if (why) return why;
    out.reserve((size_t) size);
    A4VectorSink sink{data, out};
    return a4_lz4_frame(A4PtrReader{data}, n, sink, &size);
}

// ---- the FlatBuffer locator -------------------------------------------------------------------------------------------------------------
// buf[0, len): one inflated packet, a size-prefixed FlatBuffer.  *first = the byte offset in buf of the first 16-byte event,
// *count = the events.  Every read and the whole vector lie inside [0, len), else the code says which did not.  len == 0: a packet
// of no events (a frame whose blocks are all empty).
ECAL_A4_HD int a4_locate_events(const uint8_t *buf, uint64_t len, uint64_t *first, uint32_t *count) {
    *first = 0;
    *count = 0;
    if (len == 0) return A4E_NONE;
    if (len < 12) return A4E_FB_SHORT;
    if (buf[8] != 'E' || buf[9] != 'V' || buf[10] != 'T' || buf[11] != 'S') return A4E_FB_IDENT;
    const uint64_t table = 4ull + a4_le32(buf + 4);
    if (table > len || len - table < 4) return A4E_FB_TABLE;
    const int64_t vt = (int64_t) table - (int64_t) (int32_t) a4_le32(buf + table);
    if (vt < 0 || (uint64_t) vt > len || len - (uint64_t) vt < 4) return A4E_FB_VTABLE;
    const uint32_t vtable_bytes = a4_le16(buf + vt);
    if (vtable_bytes < 6) return A4E_NONE;
    if (len - (uint64_t) vt < 6) return A4E_FB_VTABLE;
    const uint32_t field0 = a4_le16(buf + vt + 4);
    if (field0 == 0) return A4E_NONE;
    const uint64_t p = table + field0;
    if (p > len || len - p < 4) return A4E_FB_FIELD;
    const uint64_t vec = p + a4_le32(buf + p);
    if (vec > len || len - vec < 4) return A4E_FB_VECTOR;
    const uint32_t c = a4_le32(buf + vec);
    if ((uint64_t) c * A4_EVENT_BYTES > len - vec - 4) return A4E_FB_VECTOR;
    *first = vec + 4;
    *count = c;
    return A4E_NONE;
}

// ---- the event, the conversion and the filter (the other ingests', with signed coordinates) ----------------------------------------------
struct A4Event {
    int64_t t_us;
    int32_t x, y;
    uint8_t on;
};
// from the 16 bytes as four little-endian words
ECAL_A4_HD A4Event a4_event(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    A4Event e;
    e.t_us = (int64_t) (((uint64_t) w1 << 32) | w0);
    e.x = (int16_t) (w2 & 0xFFFFu);
    e.y = (int16_t) (w2 >> 16);
    e.on = (uint8_t) ((w3 & 0xFFu) != 0u);
    return e;
}
ECAL_A4_HD A4Event a4_event_at(const uint8_t *r) { return a4_event(a4_le32(r), a4_le32(r + 4), a4_le32(r + 8), a4_le32(r + 12)); }

struct A4Filter {
    int64_t time_base;
    uint32_t width, height;   // 0: no bound
    double start_time;
    int has_end_time;
    double end_time;
    int flip_x, flip_y;       // need width / height
};
enum : uint8_t { A4_CLASS_KEEP = 0, A4_CLASS_OUTSIDE = 2, A4_CLASS_NEGATIVE = 3, A4_CLASS_BEFORE_START = 4, A4_CLASS_STOP = 5 };

ECAL_A4_HD uint8_t a4_classify(const A4Event &e, const A4Filter &f, double *t_out, uint32_t *x_out, uint32_t *y_out) {
    if (e.x < 0 || e.y < 0) return A4_CLASS_OUTSIDE;
    const uint32_t x = (uint32_t) e.x, y = (uint32_t) e.y;
    if ((f.width && x >= f.width) || (f.height && y >= f.height)) return A4_CLASS_OUTSIDE;
    *x_out = (f.flip_x && f.width) ? f.width - 1u - x : x;     // (behind the bounds test: no wrap below zero)
    *y_out = (f.flip_y && f.height) ? f.height - 1u - y : y;
    const int64_t d = (int64_t) ((uint64_t) e.t_us - (uint64_t) f.time_base);
    const double t = (double) d * 1e-6;   // one subtraction, one conversion, one multiplication
    *t_out = t;
    if (t < 0) return A4_CLASS_NEGATIVE;
    if (f.has_end_time && t >= f.end_time) return A4_CLASS_STOP;
    return t >= f.start_time ? A4_CLASS_KEEP : A4_CLASS_BEFORE_START;
}

// the whole second at or below a stamp: the automatic time base
inline int64_t a4_whole_second(int64_t t_us) {
    int64_t q = t_us / 1000000;
    if (t_us % 1000000 < 0) q--;
    return q * 1000000;
}

// the counters of one decode (ecal_aedat4_info's)
struct A4Counts {
    uint64_t n_raw_events, n_events, n_outside, n_negative, n_before_start, n_after_end, n_packets, n_other_packets, n_trailing_bytes,
        n_compressed_bytes, n_inflated_bytes;
    int64_t first_stamp_us, time_base;
    int compression, stream_id;
};

template <class PutRecord> struct A4Sink {
    const A4Filter &f;
    A4Counts &c;
    PutRecord &put;
    bool stopped = false;
    A4Sink(const A4Filter &f_, A4Counts &c_, PutRecord &put_) : f(f_), c(c_), put(put_) {}
    void operator()(const A4Event &e) {
        c.n_raw_events++;
        if (stopped) {
            c.n_after_end++;
            return;
        }
        double t = 0;
        uint32_t x = 0, y = 0;
        switch (a4_classify(e, f, &t, &x, &y)) {
            case A4_CLASS_OUTSIDE: c.n_outside++; break;
            case A4_CLASS_NEGATIVE: c.n_negative++; break;
            case A4_CLASS_BEFORE_START: c.n_before_start++; break;
            case A4_CLASS_STOP: stopped = true; c.n_after_end++; break;
            default: {
                uint8_t rec[25];
                ecal::pack_record(rec, t, (double) x, (double) y, e.on);
                put(rec);
                c.n_events++;
            }
        }
    }
};

// ---- the file header --------------------------------------------------------------------------------------------------------------------
struct A4Header {
    int compression;
    int64_t data_table_position;
    uint64_t packets_begin;   // 18 + N
};
// a scalar field of a FlatBuffer table in buf[0, len): the field's byte offset, 0 when it is absent, -1 when a read falls outside
inline int64_t a4_fb_field(const uint8_t *buf, uint64_t len, uint64_t table, uint32_t id, uint32_t bytes) {
    if (table > len || len - table < 4) return -1;
    const int64_t vt = (int64_t) table - (int64_t) (int32_t) a4_le32(buf + table);
    if (vt < 0 || (uint64_t) vt > len || len - (uint64_t) vt < 4) return -1;
    const uint32_t vtable_bytes = a4_le16(buf + vt);
    if (vtable_bytes < 6u + 2u * id) return 0;
    if (len - (uint64_t) vt < 6u + 2u * id) return -1;
    const uint32_t fo = a4_le16(buf + vt + 4 + 2 * id);
    if (!fo) return 0;
    if (table + fo > len || len - (table + fo) < bytes) return -1;
    return (int64_t) (table + fo);
}

// `data`: the first n bytes of the file (whole_file: these are all of it).  A4_INVALID with *err — every text has "AEDAT 4" in it.
inline int a4_parse_header(const uint8_t *data, uint64_t n, bool whole_file, A4Header *h, std::string *err) {
    static const char line[] = "#!AER-DAT4.0\r\n";
    auto fail = [&](const std::string &why) {
        if (err) *err = "AEDAT 4: " + why;
        return (int) A4_INVALID;
    };
    h->compression = 0;
    h->data_table_position = -1;
    h->packets_begin = 0;
    const uint64_t have = n < A4_VERSION_BYTES ? n : A4_VERSION_BYTES;
    if (memcmp(data, line, (size_t) have) != 0) return fail("the first line is not #!AER-DAT4.0");
    if (n < A4_VERSION_BYTES + 4) return fail("the file is cut short before its header");
    const uint64_t N = a4_le32(data + A4_VERSION_BYTES), begin = A4_VERSION_BYTES + 4 + N;
    if (begin > A4_HEADER_LIMIT) return fail("the IOHeader does not lie within the first MiB");
    if (begin > n) return fail(whole_file ? "the file is cut short inside its header" : "the IOHeader does not lie within the bytes given");
    const uint8_t *fb = data + A4_VERSION_BYTES + 4;
    if (N < 8 || memcmp(fb + 4, "IOHE", 4) != 0) return fail("the header's identifier is not IOHE");
    const uint64_t table = a4_le32(fb);
    const int64_t f0 = a4_fb_field(fb, N, table, 0, 4), f1 = a4_fb_field(fb, N, table, 1, 8);
    if (f0 < 0 || f1 < 0) return fail("the IOHeader's table lies outside it");
    if (f0) h->compression = (int32_t) a4_le32(fb + f0);
    if (f1) h->data_table_position = (int64_t) a4_le64(fb + f1);
    h->packets_begin = begin;
    if (h->compression == A4_COMP_ZSTD || h->compression == A4_COMP_ZSTD_HIGH)
        return fail(std::string(h->compression == A4_COMP_ZSTD ? "ZSTD" : "ZSTD_HIGH") + " compression is not read: record with LZ4 or without compression");
    if (h->compression < 0 || h->compression > A4_COMP_ZSTD_HIGH) return fail("compression value " + std::to_string(h->compression) + " is not known");
    return A4_OK;
}
// where the packets end in a file of file_bytes bytes
inline int a4_packets_end(const A4Header &h, uint64_t file_bytes, uint64_t *end, std::string *err) {
    *end = file_bytes;
    if (h.data_table_position < 0) return A4_OK;
    const uint64_t p = (uint64_t) h.data_table_position;
    if (p < h.packets_begin || p > file_bytes) {
        if (err) *err = "AEDAT 4: dataTablePosition " + std::to_string(h.data_table_position) + " lies in front of the first packet or behind the end of the file";
        return A4_INVALID;
    }
    *end = p;
    return A4_OK;
}

// ---- the packet chain -------------------------------------------------------------------------------------------------------------------
struct A4Packet {   // ecal_aedat4_packet of ecal.h
    uint64_t offset;   // of the packet's data, from byte 0 of the file
    uint32_t n_bytes;
    uint32_t zero;
};
struct A4ChainPacket {
    int32_t stream_id;
    uint32_t n_bytes;
    uint64_t offset;   // of the data
};
inline std::string a4_name_packet(uint64_t k, uint64_t data_offset) {
    return "AEDAT 4: event packet " + std::to_string(k) + " (data at byte " + std::to_string(data_offset) + " of the file): ";
}

// Walks the chain in [begin, end): only the 8-byte headers are read, through get_header(pos, uint8_t[8]) (false: cannot be read).
// Every whole packet goes to on_packet(const A4ChainPacket &).  *trailing: the bytes from the header of a packet cut short on.
template <class GetHeader, class OnPacket>
inline int a4_walk_chain(GetHeader &&get_header, uint64_t begin, uint64_t end, OnPacket &&on_packet, uint64_t *trailing, std::string *err) {
    *trailing = 0;
    uint64_t pos = begin, number = 0;
    while (pos < end) {
        if (end - pos < 8) {
            *trailing = end - pos;
            break;
        }
        uint8_t raw[8];
        if (!get_header(pos, raw)) {
            if (err) *err = "AEDAT 4: packet " + std::to_string(number) + " at byte " + std::to_string(pos) + " of the file: cannot be read";
            return A4_INVALID;
        }
        const int32_t size = (int32_t) a4_le32(raw + 4);
        if (size < 0) {
            if (err) *err = "AEDAT 4: packet " + std::to_string(number) + " at byte " + std::to_string(pos) + " of the file: a negative size";
            return A4_INVALID;
        }
        if ((uint64_t) size > end - pos - 8) {   // cut short: not decoded at all
            *trailing = end - pos;
            break;
        }
        on_packet(A4ChainPacket{(int32_t) a4_le32(raw), (uint32_t) size, pos + 8});
        pos += 8 + (uint64_t) size;
        number++;
    }
    return A4_OK;
}

// The identifier of a packet (its inflated bytes 8..11) through get_data(offset, n_bytes, std::vector<uint8_t> &) (the packet's data
// as the file has it; false: cannot be read); the whole inflated packet is left in `inflated`.  0 or why.
template <class GetData>
inline int a4_packet_bytes(GetData &&get_data, const A4ChainPacket &p, int compression, std::vector<uint8_t> &raw, std::vector<uint8_t> &inflated) {
    if (!get_data(p.offset, p.n_bytes, raw)) return A4E_TABLE_ENTRY;
    if (compression == A4_COMP_NONE) {
        inflated = raw;
        return A4E_NONE;
    }
    return a4_lz4_inflate(raw.data(), raw.size(), inflated);
}

// The stream of events: stream_id >= 0 names it, -1 finds it — the first packet of every stream id is inflated and its identifier
// read; exactly one stream carries EVTS.  Then `table` = its packets in file order and c.n_packets / n_other_packets / stream_id /
// first_stamp_us (the whole second of the first event in file order; 0 when there is none) / n_compressed_bytes.
template <class GetData>
inline int a4_choose_stream(const std::vector<A4ChainPacket> &chain, int compression, int stream_id, GetData &&get_data, std::vector<A4Packet> &table,
                            A4Counts &c, std::string *err) {
    std::vector<uint8_t> raw, inflated;
    int chosen = stream_id;
    if (stream_id < 0) {
        std::vector<int32_t> seen, with_events;
        for (size_t k = 0; k < chain.size(); k++) {
            const A4ChainPacket &p = chain[k];
            bool known = false;
            for (int32_t s : seen) known = known || s == p.stream_id;
            if (known) continue;
            seen.push_back(p.stream_id);
            const int why = a4_packet_bytes(get_data, p, compression, raw, inflated);
            if (why) {
                if (err) *err = "AEDAT 4: packet " + std::to_string(k) + " (data at byte " + std::to_string(p.offset) + " of the file), the first of stream " +
                                std::to_string(p.stream_id) + ": " + a4_why(why);
                return A4_INVALID;
            }
            if (inflated.size() >= 12 && memcmp(inflated.data() + 8, "EVTS", 4) == 0) with_events.push_back(p.stream_id);
        }
        std::string ids;
        for (int32_t s : (with_events.size() > 1 ? with_events : seen)) ids += (ids.empty() ? "" : ", ") + std::to_string(s);
        if (with_events.size() > 1) {
            if (err) *err = "AEDAT 4: more than one stream of events (stream ids " + ids + "): name one with stream_id";
            return A4_INVALID;
        }
        if (with_events.empty()) {
            if (chain.empty()) {
                c.stream_id = -1;
                return A4_OK;
            }
            if (err) *err = "AEDAT 4: no stream of events (EVTS) among the stream ids " + ids;
            return A4_INVALID;
        }
        chosen = with_events[0];
    }
    c.stream_id = chosen;
    bool stamped = false;
    for (const A4ChainPacket &p : chain) {
        if (p.stream_id != chosen) {
            c.n_other_packets++;
            continue;
        }
        if (!stamped) {   // the first event in file order: packets are opened until one has events (nearly always the first)
            uint64_t first = 0;
            uint32_t count = 0;
            int why = a4_packet_bytes(get_data, p, compression, raw, inflated);
            if (!why) why = a4_locate_events(inflated.data(), inflated.size(), &first, &count);
            if (why) {
                if (err) *err = a4_name_packet(c.n_packets, p.offset) + a4_why(why);
                return A4_INVALID;
            }
            if (count) {
                c.first_stamp_us = a4_whole_second(a4_event_at(inflated.data() + first).t_us);
                stamped = true;
            }
        }
        table.push_back(A4Packet{p.offset, p.n_bytes, 0u});
        c.n_packets++;
        c.n_compressed_bytes += p.n_bytes;
    }
    return A4_OK;
}

// header + chain + choice over a file in host memory
inline int a4_index_file_memory(const uint8_t *file, uint64_t n_bytes, int stream_id, std::vector<A4Packet> &table, A4Counts &c, std::string *err) {
    memset(&c, 0, sizeof(c));
    c.stream_id = -1;
    A4Header h;
    int rc = a4_parse_header(file, n_bytes, true, &h, err);
    if (rc) return rc;
    c.compression = h.compression;
    uint64_t end = 0;
    if ((rc = a4_packets_end(h, n_bytes, &end, err))) return rc;
    std::vector<A4ChainPacket> chain;
    rc = a4_walk_chain([&](uint64_t pos, uint8_t *raw) { memcpy(raw, file + pos, 8); return true; }, h.packets_begin, end,
                       [&](const A4ChainPacket &p) { chain.push_back(p); }, &c.n_trailing_bytes, err);
    if (rc) return rc;
    return a4_choose_stream(chain, h.compression, stream_id, [&](uint64_t off, uint32_t nb, std::vector<uint8_t> &out) {
        out.assign(file + off, file + off + nb);
        return true;
    }, table, c, err);
}

struct A4DecodeOptions {
    int stream_id;
    int auto_time_base;
    A4Filter filter;   // time_base: taken with auto_time_base == 0
    uint64_t max_inflated_bytes;
};

// ---- the sequential host decoder --------------------------------------------------------------------------------------------------------
template <class PutRecord>
inline int a4_decode_sequential(const uint8_t *file, uint64_t n_bytes, const A4DecodeOptions &o, A4Counts &c, PutRecord &&put, std::string *err) {
    std::vector<A4Packet> table;
    int rc = a4_index_file_memory(file, n_bytes, o.stream_id, table, c, err);
    if (rc) return rc;
    A4Filter f = o.filter;
    if (o.auto_time_base) f.time_base = c.first_stamp_us;
    c.time_base = f.time_base;
    A4Sink<PutRecord> sink(f, c, put);
    std::vector<uint8_t> inflated;
    for (size_t k = 0; k < table.size(); k++) {
        const uint8_t *buf = file + table[k].offset;
        uint64_t len = table[k].n_bytes, first = 0;
        uint32_t count = 0;
        int why = A4E_NONE;
        if (c.compression != A4_COMP_NONE) {
            why = a4_lz4_inflate(buf, len, inflated);
            buf = inflated.data();
            len = inflated.size();
        }
        if (!why) {
            c.n_inflated_bytes += len;
            if (c.n_inflated_bytes > o.max_inflated_bytes) {
                if (err) *err = "AEDAT 4: the packets inflate to more than max_inflated_bytes (" + std::to_string(o.max_inflated_bytes) + ")";
                return A4_RANGE;
            }
            why = a4_locate_events(buf, len, &first, &count);
        }
        if (why) {
            if (err) *err = a4_name_packet(k, table[k].offset) + a4_why(why);
            return A4_INVALID;
        }
        for (uint32_t e = 0; e < count; e++) sink(a4_event_at(buf + first + (uint64_t) e * A4_EVENT_BYTES));
    }
    return A4_OK;
}

// ---- the same block by block, as the kernels do it ----------------------------------------------------------------------------------------
// sizes (first bad packet = the lowest index), spans padded to 16 bytes, inflate into the spans, locate, the counts scanned into an
// event-slot space; a block owns block_events consecutive slots and finds its first packet by bisection
template <class PutRecord>
inline int a4_decode_blockwise(const uint8_t *file, uint64_t n_bytes, const A4DecodeOptions &o, uint64_t block_events, A4Counts &c, PutRecord &&put,
                               std::string *err) {
    std::vector<A4Packet> table;
    int rc = a4_index_file_memory(file, n_bytes, o.stream_id, table, c, err);
    if (rc) return rc;
    A4Filter f = o.filter;
    if (o.auto_time_base) f.time_base = c.first_stamp_us;
    c.time_base = f.time_base;
    const size_t n = table.size();
    const bool lz4 = c.compression != A4_COMP_NONE;
    std::vector<uint64_t> span(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        uint64_t size = table[k].n_bytes;
        if (lz4) {
            const int why = a4_lz4_size(file + table[k].offset, table[k].n_bytes, &size);
            if (why) {
                if (err) *err = a4_name_packet(k, table[k].offset) + a4_why(why);
                return A4_INVALID;
            }
        }
        c.n_inflated_bytes += size;
        span[k + 1] = span[k] + (lz4 ? (size + 15) / 16 * 16 : 0);
    }
    if (c.n_inflated_bytes > o.max_inflated_bytes) {
        if (err) *err = "AEDAT 4: the packets inflate to more than max_inflated_bytes (" + std::to_string(o.max_inflated_bytes) + ")";
        return A4_RANGE;
    }
    std::vector<uint8_t> scratch((size_t) span[n]), one;
    std::vector<A4Packet> located(n);
    std::vector<uint64_t> first(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        const uint8_t *buf = file + table[k].offset;
        uint64_t len = table[k].n_bytes, base = table[k].offset;
        if (lz4) {
            (void) a4_lz4_inflate(buf, len, one);
            if (!one.empty()) memcpy(scratch.data() + span[k], one.data(), one.size());
            buf = scratch.data() + span[k];
            len = one.size();
            base = span[k];
        }
        uint64_t at = 0;
        uint32_t count = 0;
        const int why = a4_locate_events(buf, len, &at, &count);
        if (why) {
            if (err) *err = a4_name_packet(k, table[k].offset) + a4_why(why);
            return A4_INVALID;
        }
        located[k] = A4Packet{base + at, count, 0u};
        first[k + 1] = first[k] + count;
    }
    const uint8_t *src = lz4 ? scratch.data() : file;
    const uint64_t S = first[n];
    A4Sink<PutRecord> sink(f, c, put);
    for (uint64_t s0 = 0; s0 < S; s0 += block_events) {
        const uint64_t s1 = s0 + block_events < S ? s0 + block_events : S;
        uint64_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (first[mid] <= s0) lo = mid; else hi = mid;
        }
        uint64_t p = lo;
        for (uint64_t s = s0; s < s1; s++) {
            while (s >= first[p + 1]) p++;
            sink(a4_event_at(src + located[p].offset + (s - first[p]) * A4_EVENT_BYTES));
        }
    }
    return A4_OK;
}

}  // namespace ecal_aedat4
