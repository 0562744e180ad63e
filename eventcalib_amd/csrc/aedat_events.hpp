// iniVation AEDAT 3.1 (packets of little-endian 8-byte polarity events) and AEDAT 2.0 (big-endian 8-byte records) payloads into
// events — one restatement of include/ecal.h, "aedat ingest", for the kernels (ecal_aedat.hip), the host decoder
// (EventStream::aedat2bin, host/event.hpp) and the CPU test (tests/cpp/check_aedat_decode.cpp).
//
// Unlike the raw encodings, an event here carries nearly all of its own state.  What crosses records:
//   3.1   the packet an event sits in (its eventTSOverflow, and where the packet lies: found only through the headers before it).
//         aedat_index_packets walks the chain ONCE, on the host, and leaves a table of the polarity packets; behind it every
//         event is "slot s of the table" and decodes on its own.
//   2.0   the count of time wraps in front of a record: a flag per record (from its stamp and its predecessor's), summed.
// So   sequential:  walk, keeping the overflow / the wrap count
//      block-wise:  the table's event counts (3.1) or the blocks' wrap counts (2.0) scanned, then every block on its own
// give the same events.
// Nothing here is floating point but aedat_classify's one conversion and one multiplication (the translation units that include this
// are built with -ffp-contract=off all the same).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <string>
#include "event_record.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_AEDAT_HD __host__ __device__ __forceinline__
#else
#define ECAL_AEDAT_HD inline
#endif

namespace ecal_aedat {

enum : int { AEDAT_FORMAT_NONE = 0, AEDAT_FORMAT_20 = 20, AEDAT_FORMAT_31 = 31 };   // ECAL_AEDAT_AUTO / _2_0 / _3_1 of ecal.h
enum : int { AEDAT_OK = 0, AEDAT_INVALID = -1, AEDAT_RANGE = -6 };                  // ECAL_OK / ECAL_ERR_INVALID / ECAL_ERR_RANGE

// a decode block of the kernels: 256 threads x 4 consecutive event slots (ecal_aedat_block_events), for both formats
constexpr uint32_t AEDAT_BLOCK_THREADS = 256;
constexpr uint32_t AEDAT_THREAD_EVENTS = 4;
constexpr uint32_t AEDAT_BLOCK_EVENTS = AEDAT_BLOCK_THREADS * AEDAT_THREAD_EVENTS;

constexpr uint32_t AEDAT31_HEADER_BYTES = 28;
constexpr int AEDAT31_POLARITY = 1;

// one decoded event in front of the filter; valid = 0: the 3.1 valid bit is clear (dropped as n_invalid)
struct AedatEvent {
    int64_t t_us;
    uint32_t x, y;
    uint8_t pol, valid;
};

// ---- field extraction ---------------------------------------------------------------------------------------------------------------
// 3.1 polarity event: the u32 data word, the i32 stamp, the packet's eventTSOverflow
ECAL_AEDAT_HD AedatEvent aedat31_event(uint32_t data, uint32_t ts, int32_t ts_overflow) {
    AedatEvent e;
    e.t_us = (int64_t) ((uint64_t) (int64_t) ts_overflow << 31) + (int64_t) (ts & 0x7FFFFFFFu);
    e.x = data >> 17;
    e.y = (data >> 2) & 0x7FFFu;
    e.pol = (uint8_t) ((data >> 1) & 1u);
    e.valid = (uint8_t) (data & 1u);
    return e;
}

// 2.0 record: is the address a DVS event (else APS, IMU, external input: n_other_records)
ECAL_AEDAT_HD bool aedat20_is_event(uint32_t address) { return (address >> 31) == 0u && ((address >> 10) & 1u) == 0u; }
// one wrap between consecutive records with stamps p then q: a backward step of more than 2^31
ECAL_AEDAT_HD uint32_t aedat20_wrap(uint32_t p, uint32_t q) { return (q < p && p - q > 0x80000000u) ? 1u : 0u; }
// `wraps`: the wraps counted up to and including this record (only its low 32 bits reach the 64-bit time)
ECAL_AEDAT_HD AedatEvent aedat20_event(uint32_t address, uint32_t ts, uint64_t wraps) {
    AedatEvent e;
    e.t_us = (int64_t) ((wraps << 32) | (uint64_t) ts);
    e.x = (address >> 12) & 0x3FFu;
    e.y = (address >> 22) & 0x1FFu;
    e.pol = (uint8_t) ((address >> 11) & 1u);
    e.valid = 1;
    return e;
}

ECAL_AEDAT_HD uint32_t aedat_le32(const uint8_t *p) {
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}
ECAL_AEDAT_HD uint32_t aedat_be32(const uint8_t *p) {
    return (uint32_t) p[3] | ((uint32_t) p[2] << 8) | ((uint32_t) p[1] << 16) | ((uint32_t) p[0] << 24);
}
ECAL_AEDAT_HD uint32_t aedat_le16(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8); }

// ---- conversion and filter (the raw ingest's, with the flips) -------------------------------------------------------------------------
struct AedatFilter {
    int64_t time_base;
    uint32_t width, height;   // 0: no bound
    double start_time;
    int has_end_time;
    double end_time;
    int flip_x, flip_y;       // need width / height
};

enum : uint8_t { AEDAT_CLASS_KEEP = 0, AEDAT_CLASS_INVALID = 1, AEDAT_CLASS_OUTSIDE = 2, AEDAT_CLASS_NEGATIVE = 3, AEDAT_CLASS_BEFORE_START = 4, AEDAT_CLASS_STOP = 5 };

// *x_out / *y_out: the coordinates behind the flips (written for every class from OUTSIDE on)
ECAL_AEDAT_HD uint8_t aedat_classify(const AedatEvent &e, const AedatFilter &f, double *t_out, uint32_t *x_out, uint32_t *y_out) {
    if (!e.valid) return AEDAT_CLASS_INVALID;
    if ((f.width && e.x >= f.width) || (f.height && e.y >= f.height)) return AEDAT_CLASS_OUTSIDE;
    *x_out = (f.flip_x && f.width) ? f.width - 1u - e.x : e.x;     // (behind the bounds test: no wrap below zero)
    *y_out = (f.flip_y && f.height) ? f.height - 1u - e.y : e.y;
    const int64_t d = (int64_t) ((uint64_t) e.t_us - (uint64_t) f.time_base);
    const double t = (double) d * 1e-6;   // one subtraction, one conversion, one multiplication
    *t_out = t;
    if (t < 0) return AEDAT_CLASS_NEGATIVE;
    if (f.has_end_time && t >= f.end_time) return AEDAT_CLASS_STOP;
    return t >= f.start_time ? AEDAT_CLASS_KEEP : AEDAT_CLASS_BEFORE_START;
}

// the counters of one decode (ecal_aedat_info's, without the header's)
struct AedatCounts {
    uint64_t n_raw_events, n_events, n_invalid, n_outside, n_negative, n_before_start, n_after_end, n_packets, n_other_packets,
        n_records, n_other_records, n_trailing_bytes, n_time_wraps;
};

// The filter in file order over a stream of events: counts into c, the kept ones to put(const uint8_t rec[25]).  The first event
// that reaches end_time ends the stream: it and every event behind it count as n_after_end and nothing else.
template <class PutRecord> struct AedatSink {
    const AedatFilter &f;
    AedatCounts &c;
    PutRecord &put;
    bool stopped = false;
    AedatSink(const AedatFilter &f_, AedatCounts &c_, PutRecord &put_) : f(f_), c(c_), put(put_) {}
    void operator()(const AedatEvent &e) {
        c.n_raw_events++;
        if (stopped) {
            c.n_after_end++;
            return;
        }
        double t = 0;
        uint32_t x = 0, y = 0;
        switch (aedat_classify(e, f, &t, &x, &y)) {
            case AEDAT_CLASS_INVALID: c.n_invalid++; break;
            case AEDAT_CLASS_OUTSIDE: c.n_outside++; break;
            case AEDAT_CLASS_NEGATIVE: c.n_negative++; break;
            case AEDAT_CLASS_BEFORE_START: c.n_before_start++; break;
            case AEDAT_CLASS_STOP: stopped = true; c.n_after_end++; break;
            default: {
                uint8_t rec[25];
                ecal::pack_record(rec, t, (double) x, (double) y, e.pol);
                put(rec);
                c.n_events++;
            }
        }
    }
};

// ---- 3.1: the packet chain ------------------------------------------------------------------------------------------------------------
struct AedatPacket {   // ecal_aedat_packet of ecal.h
    uint64_t offset;   // of the packet's first event, from the start of the payload
    uint32_t n_events; // events to decode: eventNumber, or fewer where the body is cut short
    int32_t ts_overflow;
};

struct Aedat31Header {
    int32_t type, source, size, ts_offset, ts_overflow, capacity, number, valid;
};
inline Aedat31Header aedat31_header(const uint8_t *p) {
    Aedat31Header h;
    h.type = (int16_t) aedat_le16(p);
    h.source = (int16_t) aedat_le16(p + 2);
    h.size = (int32_t) aedat_le32(p + 4);
    h.ts_offset = (int32_t) aedat_le32(p + 8);
    h.ts_overflow = (int32_t) aedat_le32(p + 12);
    h.capacity = (int32_t) aedat_le32(p + 16);
    h.number = (int32_t) aedat_le32(p + 20);
    h.valid = (int32_t) aedat_le32(p + 24);
    return h;
}

// Walks the chain: only the 28-byte headers are read, through get_header(pos, uint8_t[28]) (false: the bytes cannot be read — the
// walk ends with AEDAT_INVALID), so a file is indexed without its bodies.  Every polarity packet (of `source` when source >= 0) goes
// to on_packet(const AedatPacket &) — also one of no events; every other packet is counted.  c: n_packets, n_other_packets,
// n_raw_events, n_trailing_bytes are set.
// AEDAT_INVALID: a packet breaks a rule; *err names its number (0-based, over all packets) and byte offset.
template <class GetHeader, class OnPacket>
inline int aedat31_walk_headers(GetHeader &&get_header, uint64_t n_bytes, int source, AedatCounts &c, OnPacket &&on_packet, std::string *err) {
    c.n_packets = c.n_other_packets = c.n_raw_events = c.n_trailing_bytes = 0;
    uint64_t pos = 0, number = 0;
    while (pos < n_bytes) {
        if (n_bytes - pos < AEDAT31_HEADER_BYTES) {   // a header cut short ends the chain
            c.n_trailing_bytes = n_bytes - pos;
            break;
        }
        uint8_t raw[AEDAT31_HEADER_BYTES];
        if (!get_header(pos, raw)) {
            if (err) *err = "packet " + std::to_string(number) + " at byte " + std::to_string(pos) + " of the payload: cannot be read";
            return AEDAT_INVALID;
        }
        const Aedat31Header h = aedat31_header(raw);
        const bool polarity = h.type == AEDAT31_POLARITY && (source < 0 || h.source == source);
        const char *why = nullptr;
        if (h.size < 0 || h.capacity < 0 || h.number < 0 || h.valid < 0) why = "a negative size";
        else if (h.number > h.capacity) why = "eventNumber > eventCapacity";
        else if (polarity && h.size != 8) why = "a polarity packet whose eventSize is not 8";
        else if (polarity && h.ts_offset != 4) why = "a polarity packet whose eventTSOffset is not 4";
        if (why) {
            if (err) *err = "packet " + std::to_string(number) + " at byte " + std::to_string(pos) + " of the payload: " + why;
            return AEDAT_INVALID;
        }
        const uint64_t body = pos + AEDAT31_HEADER_BYTES, len = (uint64_t) h.capacity * (uint64_t) h.size, avail = n_bytes - body;
        const bool cut = len > avail;
        uint64_t n_ev = (uint64_t) h.number;
        if (cut) {   // a body cut short ends the chain: the records wholly present count
            const uint64_t whole = avail / (uint64_t) h.size;   // (len > 0, so size > 0)
            n_ev = n_ev < whole ? n_ev : whole;
            c.n_trailing_bytes = avail - whole * (uint64_t) h.size;
        }
        if (polarity) {
            AedatPacket p;
            p.offset = body;
            p.n_events = (uint32_t) n_ev;
            p.ts_overflow = h.ts_overflow;
            on_packet(p);
            c.n_packets++;
            c.n_raw_events += n_ev;
        } else {
            c.n_other_packets++;
        }
        if (cut) break;
        pos = body + len;
        number++;
    }
    return AEDAT_OK;
}

// the same over a payload in memory
template <class OnPacket>
inline int aedat31_walk(const uint8_t *payload, uint64_t n_bytes, int source, AedatCounts &c, OnPacket &&on_packet, std::string *err) {
    return aedat31_walk_headers([&](uint64_t pos, uint8_t *raw) { memcpy(raw, payload + pos, AEDAT31_HEADER_BYTES); return true; }, n_bytes,
                                source, c, on_packet, err);
}

// The table of the polarity packets.  out may be null with capacity 0 (a count).  AEDAT_RANGE: more than `capacity` packets —
// *n_packets is the count needed, `out` holds the first `capacity`.
inline int aedat_index_packets(const uint8_t *payload, uint64_t n_bytes, int source, AedatPacket *out, uint64_t capacity, uint64_t *n_packets,
                               AedatCounts &c, std::string *err) {
    uint64_t n = 0;
    const int rc = aedat31_walk(payload, n_bytes, source, c, [&](const AedatPacket &p) {
        if (n < capacity) out[n] = p;
        n++;
    }, err);
    *n_packets = n;
    if (rc) return rc;
    if (n > capacity) {
        if (err) *err = std::to_string(n) + " polarity packets, more than the capacity of the table";
        return AEDAT_RANGE;
    }
    return AEDAT_OK;
}

inline void aedat31_slot_event(const uint8_t *payload, const AedatPacket &p, uint64_t k, AedatEvent *e) {
    const uint8_t *r = payload + p.offset + 8u * k;
    *e = aedat31_event(aedat_le32(r), aedat_le32(r + 4), p.ts_overflow);
}

// ---- sequential host decoders -------------------------------------------------------------------------------------------------------
template <class PutRecord>
inline int aedat31_decode_sequential(const uint8_t *payload, uint64_t n_bytes, int source, const AedatFilter &f, AedatCounts &c, PutRecord &&put,
                                     std::string *err) {
    memset(&c, 0, sizeof(c));
    AedatCounts walk;
    memset(&walk, 0, sizeof(walk));
    AedatSink<PutRecord> sink(f, c, put);
    const int rc = aedat31_walk(payload, n_bytes, source, walk, [&](const AedatPacket &p) {
        for (uint64_t k = 0; k < p.n_events; k++) {
            AedatEvent e;
            aedat31_slot_event(payload, p, k, &e);
            sink(e);
        }
    }, err);
    c.n_packets = walk.n_packets;
    c.n_other_packets = walk.n_other_packets;
    c.n_trailing_bytes = walk.n_trailing_bytes;
    return rc;
}

template <class PutRecord>
inline void aedat20_decode_sequential(const uint8_t *payload, uint64_t n_bytes, const AedatFilter &f, AedatCounts &c, PutRecord &&put) {
    memset(&c, 0, sizeof(c));
    c.n_records = n_bytes / 8u;
    c.n_trailing_bytes = n_bytes % 8u;
    AedatSink<PutRecord> sink(f, c, put);
    uint64_t wraps = 0;
    uint32_t prev = 0;
    for (uint64_t r = 0; r < c.n_records; r++) {
        const uint32_t address = aedat_be32(payload + 8u * r), ts = aedat_be32(payload + 8u * r + 4u);
        if (r) wraps += aedat20_wrap(prev, ts);
        prev = ts;
        if (aedat20_is_event(address)) sink(aedat20_event(address, ts, wraps));
        else c.n_other_records++;
    }
    c.n_time_wraps = wraps;
}

// ---- the same block by block, as the kernels do it ----------------------------------------------------------------------------------
// 3.1: the table's counts scanned into an event-slot space; a block owns block_events consecutive slots, finds the packet of its
// first slot by bisection in the scanned table and walks packets from there
template <class PutRecord>
inline int aedat31_decode_blockwise(const uint8_t *payload, uint64_t n_bytes, int source, uint64_t block_events, const AedatFilter &f,
                                    AedatCounts &c, PutRecord &&put, std::string *err) {
    memset(&c, 0, sizeof(c));
    AedatCounts walk;
    memset(&walk, 0, sizeof(walk));
    uint64_t n = 0;
    int rc = aedat_index_packets(payload, n_bytes, source, nullptr, 0, &n, walk, err);
    if (rc != AEDAT_OK && rc != AEDAT_RANGE) return rc;
    AedatPacket *tab = new AedatPacket[n + 1];
    uint64_t *first = new uint64_t[n + 1];
    rc = aedat_index_packets(payload, n_bytes, source, tab, n, &n, walk, err);
    first[0] = 0;
    for (uint64_t p = 0; p < n; p++) first[p + 1] = first[p] + tab[p].n_events;
    const uint64_t S = first[n];
    AedatSink<PutRecord> sink(f, c, put);
    for (uint64_t s0 = 0; s0 < S; s0 += block_events) {
        const uint64_t s1 = s0 + block_events < S ? s0 + block_events : S;
        uint64_t lo = 0, hi = n;   // the last packet whose first slot is not behind s0: it is not empty and holds s0
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (first[mid] <= s0) lo = mid; else hi = mid;
        }
        uint64_t p = lo;
        for (uint64_t s = s0; s < s1; s++) {
            while (s >= first[p + 1]) p++;
            AedatEvent e;
            aedat31_slot_event(payload, tab[p], s - first[p], &e);
            sink(e);
        }
    }
    c.n_packets = walk.n_packets;
    c.n_other_packets = walk.n_other_packets;
    c.n_trailing_bytes = walk.n_trailing_bytes;
    delete[] tab;
    delete[] first;
    return rc;
}

// 2.0: wrap flags counted per block (a block's first record reads its predecessor), the counts scanned, every block on its own
template <class PutRecord>
inline void aedat20_decode_blockwise(const uint8_t *payload, uint64_t n_bytes, uint64_t block_events, const AedatFilter &f, AedatCounts &c,
                                     PutRecord &&put) {
    memset(&c, 0, sizeof(c));
    c.n_records = n_bytes / 8u;
    c.n_trailing_bytes = n_bytes % 8u;
    const uint64_t nb = (c.n_records + block_events - 1) / block_events;
    auto flag = [&](uint64_t r) -> uint32_t { return r ? aedat20_wrap(aedat_be32(payload + 8u * (r - 1) + 4u), aedat_be32(payload + 8u * r + 4u)) : 0u; };
    uint64_t *in = new uint64_t[nb + 1];
    uint64_t run = 0;
    for (uint64_t b = 0; b < nb; b++) {
        const uint64_t r0 = b * block_events, r1 = r0 + block_events < c.n_records ? r0 + block_events : c.n_records;
        in[b] = run;
        for (uint64_t r = r0; r < r1; r++) run += flag(r);
    }
    c.n_time_wraps = run;
    AedatSink<PutRecord> sink(f, c, put);
    for (uint64_t b = 0; b < nb; b++) {
        const uint64_t r0 = b * block_events, r1 = r0 + block_events < c.n_records ? r0 + block_events : c.n_records;
        uint64_t wraps = in[b];
        for (uint64_t r = r0; r < r1; r++) {
            wraps += flag(r);
            const uint32_t address = aedat_be32(payload + 8u * r), ts = aedat_be32(payload + 8u * r + 4u);
            if (aedat20_is_event(address)) sink(aedat20_event(address, ts, wraps));
            else c.n_other_records++;
        }
    }
    delete[] in;
}

// ---- file header --------------------------------------------------------------------------------------------------------------------
// `data`: the first n bytes of the file (whole_file: these are all of it).  The first line is "#!AER-DAT<version>\r\n".
//   3.1: the header runs up to and including the line "#!END-HEADER\r\n"; a "#Format:" line whose value is not RAW is refused.
//   2.0: the maximal run of header lines: a line that starts with '#', reaches its '\n' within 4096 bytes and holds nothing but
//        bytes 0x20..0x7E, '\t' and '\r' before it (the first byte of a 2.0 record can be '#').
// format_option other than AEDAT_FORMAT_NONE overrides the version line (which then need not be there or be a known one).
// AEDAT_INVALID with *err: no version line, another version (named), a 3.1 header without its end within the n bytes, a format
// line that is not RAW.
inline int aedat_parse_header(const uint8_t *data, size_t n, bool whole_file, int format_option, int *format, uint64_t *header_bytes,
                              std::string *err) {
    *format = format_option;
    *header_bytes = 0;
    static const char magic[] = "#!AER-DAT";
    const size_t ml = sizeof(magic) - 1;
    auto line_end = [&](size_t pos) -> size_t {   // index of the line's '\n', or n
        const void *nl = pos < n ? memchr(data + pos, '\n', n - pos) : nullptr;
        return nl ? (size_t) ((const uint8_t *) nl - data) : n;
    };
    const bool has_magic = n >= ml && memcmp(data, magic, ml) == 0;
    if (has_magic) {
        size_t e = line_end(0), ve = e < n ? e : n;
        while (ve > ml && (data[ve - 1] == '\r' || data[ve - 1] == '\n')) ve--;
        const std::string version((const char *) data + ml, ve - ml);
        if (format_option == AEDAT_FORMAT_NONE) {
            if (version == "3.1") *format = AEDAT_FORMAT_31;
            else if (version == "2.0") *format = AEDAT_FORMAT_20;
            else {
                if (err) *err = "AEDAT version " + version + " is not supported (3.1 and 2.0 are)";
                return AEDAT_INVALID;
            }
        }
    } else if (format_option == AEDAT_FORMAT_NONE) {
        if (err) *err = "no #!AER-DAT version line and no format option";
        return AEDAT_INVALID;
    }
    if (*format == AEDAT_FORMAT_31) {
        static const char end_line[] = "#!END-HEADER\r\n", fmt_line[] = "#Format:";
        const size_t el = sizeof(end_line) - 1, fl = sizeof(fmt_line) - 1;
        size_t pos = 0;
        while (pos < n) {
            const size_t e = line_end(pos);
            if (e == n) break;   // (a line without its '\n' within the bytes given)
            const size_t len = e + 1 - pos;
            if (len >= fl && memcmp(data + pos, fmt_line, fl) == 0) {
                size_t a = pos + fl, b = e;
                while (a < b && (data[a] == ' ' || data[a] == '\t')) a++;
                while (b > a && (data[b - 1] == '\r' || data[b - 1] == ' ' || data[b - 1] == '\t')) b--;
                const std::string value((const char *) data + a, b - a);
                if (value != "RAW") {
                    if (err) *err = "AEDAT 3.1 format " + value + " is not supported (RAW is)";
                    return AEDAT_INVALID;
                }
            }
            if (len == el && memcmp(data + pos, end_line, el) == 0) {
                *header_bytes = e + 1;
                return AEDAT_OK;
            }
            pos = e + 1;
        }
        if (err) *err = whole_file ? "the AEDAT 3.1 header has no #!END-HEADER line" : "the AEDAT 3.1 header does not end within the first MiB";
        return AEDAT_INVALID;
    }
    if (*format != AEDAT_FORMAT_20) {
        if (err) *err = "unknown format option";
        return AEDAT_INVALID;
    }
    size_t pos = 0;
    while (pos < n && data[pos] == '#') {
        const size_t lim = n - pos < 4096 ? n : pos + 4096;
        size_t e = pos;
        bool text = true;
        while (e < lim && data[e] != '\n') {
            const uint8_t ch = data[e];
            if (!((ch >= 0x20 && ch <= 0x7E) || ch == '\t' || ch == '\r')) {
                text = false;
                break;
            }
            e++;
        }
        if (!text || e >= lim) break;   // not a header line: the payload starts here
        pos = e + 1;
    }
    *header_bytes = pos;
    return AEDAT_OK;
}

}  // namespace ecal_aedat
