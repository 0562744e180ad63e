// ROS 1 bags (format 2.0) of dvs_msgs/EventArray messages into events — one restatement of include/ecal.h, "bag ingest", for the
// kernels (ecal_bag.hip), the host decoder (EventStream::bag2bin, host/event.hpp) and the CPU test (tests/cpp/check_bag_decode.cpp).
//
// An event is a 13-byte record that carries all of its own state.  What crosses records is where a message lies: a message is found
// only through the record header before it, inside a chunk that is found the same way.  bag_walk goes through the chain ONCE, on the
// host, and leaves a table of the chosen messages; behind it every event is "slot s of the table" and decodes on its own.
// So   sequential:  walk, decode every message where it is met
//      block-wise:  the table's event counts scanned into a slot space, then every block on its own
// give the same events.
// Nothing here is floating point but bag_classify's one conversion and one multiplication (the translation units that include this
// are built with -ffp-contract=off all the same).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "event_record.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_BAG_HD __host__ __device__ __forceinline__
#else
#define ECAL_BAG_HD inline
#endif

namespace ecal_bag {

enum : int { BAG_OK = 0, BAG_INVALID = -1, BAG_RANGE = -6 };   // ECAL_OK / ECAL_ERR_INVALID / ECAL_ERR_RANGE

// a decode block of the kernels: 256 threads x 4 consecutive event slots (ecal_bag_block_events)
constexpr uint32_t BAG_BLOCK_THREADS = 256;
constexpr uint32_t BAG_THREAD_EVENTS = 4;
constexpr uint32_t BAG_BLOCK_EVENTS = BAG_BLOCK_THREADS * BAG_THREAD_EVENTS;

constexpr uint32_t BAG_EVENT_BYTES = 13;          // u16 x, u16 y, u32 ts.secs, u32 ts.nsecs, u8 polarity
constexpr uint32_t BAG_MESSAGE_FIXED_BYTES = 28;  // seq, stamp, L, height, width, n (without the L bytes of frame_id)
constexpr int64_t BAG_NS_PER_S = 1000000000ll;

enum : int { BAG_OP_MESSAGE = 0x02, BAG_OP_BAG_HEADER = 0x03, BAG_OP_INDEX = 0x04, BAG_OP_CHUNK = 0x05, BAG_OP_CHUNK_INFO = 0x06, BAG_OP_CONNECTION = 0x07 };

// one decoded event in front of the filter
struct BagEvent {
    int64_t t_ns;
    uint32_t x, y;
    uint8_t pol;
};

// ---- field extraction ---------------------------------------------------------------------------------------------------------------
ECAL_BAG_HD uint32_t bag_le32(const uint8_t *p) {
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}

// xy: bytes 0..3 of the record (x low), secs: bytes 4..7, nsecs: bytes 8..11 (taken as it is, also >= 1e9), pol_byte: byte 12
ECAL_BAG_HD BagEvent bag_event(uint32_t xy, uint32_t secs, uint32_t nsecs, uint32_t pol_byte) {
    BagEvent e;
    e.t_ns = (int64_t) secs * BAG_NS_PER_S + (int64_t) nsecs;   // (below 2^63: 2^32 * 1e9 + 2^32)
    e.x = xy & 0xFFFFu;
    e.y = xy >> 16;
    e.pol = (uint8_t) ((pol_byte & 0xFFu) != 0u ? 1u : 0u);
    return e;
}

// The record at byte offset `off` from the four aligned little-endian words at off & ~3: r = off & 3, and r + 13 <= 16.  Bytes of
// w3 behind the record are not looked at (the caller may have clipped them at the end of the file).
ECAL_BAG_HD BagEvent bag_event_from_words(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t r) {
    const uint32_t sh = 8u * r;
    const uint32_t xy = (uint32_t) ((((uint64_t) w1 << 32) | w0) >> sh);
    const uint32_t secs = (uint32_t) ((((uint64_t) w2 << 32) | w1) >> sh);
    const uint32_t nsecs = (uint32_t) ((((uint64_t) w3 << 32) | w2) >> sh);
    return bag_event(xy, secs, nsecs, w3 >> sh);
}

inline BagEvent bag_event_at(const uint8_t *p) { return bag_event(bag_le32(p), bag_le32(p + 4), bag_le32(p + 8), p[12]); }

// ---- conversion and filter (the raw and AEDAT ingests', with nanoseconds) ---------------------------------------------------------------
struct BagFilter {
    int64_t time_base;        // nanoseconds
    uint32_t width, height;   // 0: no bound
    double start_time;
    int has_end_time;
    double end_time;
    int flip_x, flip_y;       // need width / height
};

enum : uint8_t { BAG_CLASS_KEEP = 0, BAG_CLASS_OUTSIDE = 1, BAG_CLASS_NEGATIVE = 2, BAG_CLASS_BEFORE_START = 3, BAG_CLASS_STOP = 4 };

// *x_out / *y_out: the coordinates behind the flips (written for every class but OUTSIDE)
ECAL_BAG_HD uint8_t bag_classify(const BagEvent &e, const BagFilter &f, double *t_out, uint32_t *x_out, uint32_t *y_out) {
    if ((f.width && e.x >= f.width) || (f.height && e.y >= f.height)) return BAG_CLASS_OUTSIDE;
    *x_out = (f.flip_x && f.width) ? f.width - 1u - e.x : e.x;     // (behind the bounds test: no wrap below zero)
    *y_out = (f.flip_y && f.height) ? f.height - 1u - e.y : e.y;
    const int64_t d = (int64_t) ((uint64_t) e.t_ns - (uint64_t) f.time_base);
    const double t = (double) d * 1e-9;   // one subtraction, one conversion, one multiplication
    *t_out = t;
    if (t < 0) return BAG_CLASS_NEGATIVE;
    if (f.has_end_time && t >= f.end_time) return BAG_CLASS_STOP;
    return t >= f.start_time ? BAG_CLASS_KEEP : BAG_CLASS_BEFORE_START;
}

// the counters of one decode (ecal_bag_info's)
struct BagCounts {
    uint64_t n_raw_events, n_events, n_outside, n_negative, n_before_start, n_after_end, n_messages, n_other_messages, n_chunks,
        n_connections, n_trailing_bytes;
    int64_t first_stamp_ns;   // secs x 1e9 of the first event of the first chosen message that has events (0: none has)
    uint32_t msg_width, msg_height;
};

// The filter in file order over a stream of events: counts into c, the kept ones to put(const uint8_t rec[25]).  The first event
// that reaches end_time ends the stream: it and every event behind it count as n_after_end and nothing else.
template <class PutRecord> struct BagSink {
    const BagFilter &f;
    BagCounts &c;
    PutRecord &put;
    bool stopped = false;
    BagSink(const BagFilter &f_, BagCounts &c_, PutRecord &put_) : f(f_), c(c_), put(put_) {}
    void operator()(const BagEvent &e) {
        c.n_raw_events++;
        if (stopped) {
            c.n_after_end++;
            return;
        }
        double t = 0;
        uint32_t x = 0, y = 0;
        switch (bag_classify(e, f, &t, &x, &y)) {
            case BAG_CLASS_OUTSIDE: c.n_outside++; break;
            case BAG_CLASS_NEGATIVE: c.n_negative++; break;
            case BAG_CLASS_BEFORE_START: c.n_before_start++; break;
            case BAG_CLASS_STOP: stopped = true; c.n_after_end++; break;
            default: {
                uint8_t rec[25];
                ecal::pack_record(rec, t, (double) x, (double) y, e.pol);
                put(rec);
                c.n_events++;
            }
        }
    }
};

// ---- record headers: a run of fields `u32 field_len`, then name=value ------------------------------------------------------------------
// on_field(name, name_len, value, value_len) for every field.  false: a field runs past the header, or has no '=' (*why says which)
template <class OnField> inline bool bag_parse_fields(const uint8_t *h, uint64_t len, OnField &&on_field, const char **why) {
    uint64_t p = 0;
    while (p < len) {
        if (len - p < 4) {
            *why = "a field that runs past its header";
            return false;
        }
        const uint64_t fl = bag_le32(h + p);
        p += 4;
        if (fl > len - p) {
            *why = "a field that runs past its header";
            return false;
        }
        const uint8_t *eq = fl ? (const uint8_t *) memchr(h + p, '=', (size_t) fl) : nullptr;
        if (!eq) {
            *why = "a field without '='";
            return false;
        }
        const uint64_t nl = (uint64_t) (eq - (h + p));
        on_field((const char *) (h + p), (size_t) nl, eq + 1, (size_t) (fl - nl - 1));
        p += fl;
    }
    return true;
}

struct BagHeader {
    int op = -1;   // -1: no 1-byte op field
    bool has_conn = false, has_size = false, has_topic = false, has_type = false, has_compression = false;
    uint32_t conn = 0, size = 0;
    std::string topic, type, compression;
};

inline bool bag_name_is(const char *name, size_t nl, const char *want) { return strlen(want) == nl && memcmp(name, want, nl) == 0; }

// the fields this reader looks at; every other one is ignored.  false: as bag_parse_fields
inline bool bag_parse_header(const uint8_t *h, uint64_t len, BagHeader &H, const char **why) {
    return bag_parse_fields(h, len, [&](const char *name, size_t nl, const uint8_t *v, size_t vl) {
        if (bag_name_is(name, nl, "op")) {
            if (vl == 1) H.op = v[0];
        } else if (bag_name_is(name, nl, "conn")) {
            if (vl == 4) { H.has_conn = true; H.conn = bag_le32(v); }
        } else if (bag_name_is(name, nl, "size")) {
            if (vl == 4) { H.has_size = true; H.size = bag_le32(v); }
        } else if (bag_name_is(name, nl, "topic")) {
            H.has_topic = true; H.topic.assign((const char *) v, vl);
        } else if (bag_name_is(name, nl, "type")) {
            H.has_type = true; H.type.assign((const char *) v, vl);
        } else if (bag_name_is(name, nl, "compression")) {
            H.has_compression = true; H.compression.assign((const char *) v, vl);
        }
    }, why);
}

// ---- the chain of records -------------------------------------------------------------------------------------------------------------
struct BagMessage {   // ecal_bag_message of ecal.h
    uint64_t offset;    // of the message's first event, from byte 0 of the file
    uint32_t n_events;
    uint32_t reserved;  // 0
};

struct BagChoice {
    std::string topic;  // empty: every connection of an accepted type, which must share one topic
    std::string type;   // empty: dvs_msgs/EventArray and prophesee_event_msgs/EventArray
};

struct BagConnection {
    uint32_t id;
    std::string topic, type;
    bool accepted, chosen;
};

inline bool bag_type_accepted(const std::string &type, const BagChoice &ch) {
    if (!ch.type.empty()) return type == ch.type;
    return type == "dvs_msgs/EventArray" || type == "prophesee_event_msgs/EventArray";
}

inline std::string bag_printable(const std::string &s) {
    std::string o;
    for (size_t i = 0; i < s.size() && i < 64; i++) o += (s[i] >= 0x20 && s[i] <= 0x7E) ? s[i] : '?';
    return o;
}

// the first line of the file.  BAG_INVALID with *err: another version of the format (named), a ROS 2 container (named), anything else
inline int bag_check_magic(const uint8_t *head, size_t n, std::string *err) {
    static const char v20[] = "#ROSBAG V2.0\n", any[] = "#ROSBAG V", sqlite[] = "SQLite format 3", mcap[] = "\x89MCAP0\r\n";
    if (n >= 13 && memcmp(head, v20, 13) == 0) return BAG_OK;
    std::string why;
    if (n >= 9 && memcmp(head, any, 9) == 0) {
        size_t e = 9;
        while (e < n && e < 32 && head[e] != '\n') e++;
        why = "ROS bag format version " + bag_printable(std::string((const char *) head + 9, e - 9)) + " is not read (2.0 is: `rosbag fix` rewrites an older bag)";
    } else if (n >= 16 && memcmp(head, sqlite, 16) == 0) {   // (with its closing NUL)
        why = "an SQLite file: a ROS 2 bag is not read (ROS 1 bags of format 2.0 are)";
    } else if (n >= 8 && memcmp(head, mcap, 8) == 0) {
        why = "an MCAP file: a ROS 2 / MCAP recording is not read (ROS 1 bags of format 2.0 are)";
    } else {
        why = "no #ROSBAG V2.0 line: not a ROS 1 bag";
    }
    if (err) *err = why;
    return BAG_INVALID;
}

// Walks the file: read(pos, dst, n) copies bytes [pos, pos + n) of it (always within n_bytes; false: they cannot be read — the walk
// ends with BAG_INVALID).  Only record headers, connection records and the 28 + L bytes in front of a chosen message's events (and
// the first event's stamp) are read, so a file is indexed without its events.  Every chosen message goes to
// on_message(const BagMessage &), also one of no events.  c: everything but the filter's counters is set.
// BAG_INVALID: a rule of the contract is broken; *err names the record's number (0-based, over all records, inner and outer, in file
// order) and its byte offset.
template <class Read, class OnMessage>
inline int bag_walk(Read &&read, uint64_t n_bytes, const BagChoice &choice, BagCounts &c, OnMessage &&on_message, std::string *err) {
    memset(&c, 0, sizeof(c));
    std::string scratch_err;
    if (!err) err = &scratch_err;
    {
        uint8_t head[32];
        const size_t hn = (size_t) (n_bytes < 32 ? n_bytes : 32);
        if (hn && !read(0, head, hn)) {
            *err = "the file cannot be read";
            return BAG_INVALID;
        }
        if (bag_check_magic(head, hn, err)) return BAG_INVALID;
    }
    std::vector<BagConnection> conns;
    std::vector<uint8_t> hbuf, dbuf;
    std::string event_topic;
    bool have_event_topic = false, have_first_stamp = false, have_first_message = false, truncated = false;
    uint64_t number = 0;

    auto list_connections = [&](bool accepted_only) {
        std::string s;
        for (const BagConnection &k : conns) {
            if (accepted_only && !k.accepted) continue;
            bool dup = false;
            for (const BagConnection &j : conns) {
                if (&j == &k) break;
                if (j.topic == k.topic && j.type == k.type && (!accepted_only || j.accepted)) dup = true;
            }
            if (dup) continue;
            if (!s.empty()) s += ", ";
            s += bag_printable(k.topic);
            if (!accepted_only) s += " (" + bag_printable(k.type) + ")";
        }
        return s.empty() ? std::string("none") : s;
    };

    // the records from pos up to end: the top level (end == n_bytes), or a chunk's data (inner; end may lie behind n_bytes: a
    // chunk cut short)
    auto chain = [&](auto &self, uint64_t pos, const uint64_t end, const bool inner) -> int {
        const uint64_t lim = end < n_bytes ? end : n_bytes;   // the bytes that are there
        while (pos < end && !truncated) {
            const uint64_t rec = pos;
            auto fail = [&](const std::string &why) {
                *err = "record " + std::to_string(number) + " at byte " + std::to_string(rec) + ": " + why;
                return BAG_INVALID;
            };
            // 1: the bytes are there; 0: the file ends first (the chain ends here); -1: they run past a chunk that is whole
            auto need = [&](uint64_t at, uint64_t n) -> int {
                if (at <= lim && n <= lim - at) return 1;
                if (end > lim || !inner) {
                    c.n_trailing_bytes = n_bytes - rec;
                    truncated = true;
                    return 0;
                }
                return -1;
            };
            auto get = [&](uint64_t at, uint8_t *dst, size_t n) { return n == 0 || read(at, dst, n); };
            static const char past[] = "a record that runs past the end of its chunk", unreadable[] = "cannot be read";
            int k;
            uint8_t w[16];
            if ((k = need(pos, 4)) <= 0) return k ? fail(past) : BAG_OK;
            if (!get(pos, w, 4)) return fail(unreadable);
            const uint64_t hl = bag_le32(w);
            if ((k = need(pos + 4, hl + 4)) <= 0) return k ? fail(past) : BAG_OK;
            hbuf.resize((size_t) hl + 4);
            if (!get(pos + 4, hbuf.data(), (size_t) hl + 4)) return fail(unreadable);
            const uint64_t dl = bag_le32(hbuf.data() + hl), data = pos + 8 + hl;
            BagHeader H;
            const char *why = nullptr;
            if (!bag_parse_header(hbuf.data(), hl, H, &why)) return fail(why);
            if (H.op < 0) return fail("a header without a 1-byte op field");
            char opname[16];
            snprintf(opname, sizeof(opname), "0x%02x", (unsigned) H.op);
            if (inner && H.op != BAG_OP_MESSAGE && H.op != BAG_OP_CONNECTION) return fail(std::string("op ") + opname + " inside a chunk");
            if (H.op == BAG_OP_CHUNK) {
                if (!H.has_compression) return fail("a chunk without a compression field");
                if (H.compression != "none")
                    return fail("a chunk with compression " + bag_printable(H.compression) + ": compressed chunks are not read (`rosbag decompress` rewrites the bag)");
                if (!H.has_size || H.size != dl) return fail("a chunk whose size field is not its data length");
                c.n_chunks++;
                number++;
                const int rc = self(self, data, data + dl, true);   // (of a chunk cut short: the records wholly present)
                if (rc) return rc;
                pos = data + dl;
                continue;
            }
            if (H.op != BAG_OP_MESSAGE && H.op != BAG_OP_CONNECTION && H.op != BAG_OP_BAG_HEADER && H.op != BAG_OP_INDEX && H.op != BAG_OP_CHUNK_INFO)
                return fail(std::string("unknown op ") + opname);
            if ((k = need(data, dl)) <= 0) return k ? fail(past) : BAG_OK;   // (a record cut short is not looked at)
            if (H.op == BAG_OP_CONNECTION) {
                if (!H.has_conn || !H.has_topic) return fail("a connection without conn or topic");
                dbuf.resize((size_t) dl);
                if (!get(data, dbuf.data(), (size_t) dl)) return fail(unreadable);
                BagHeader D;
                if (!bag_parse_header(dbuf.data(), dl, D, &why)) return fail(why);
                if (!D.has_type) return fail("a connection without a type");
                BagConnection *old = nullptr;
                for (BagConnection &q : conns)
                    if (q.id == H.conn) old = &q;
                if (old) {
                    if (old->topic != H.topic || old->type != D.type)
                        return fail("connection " + std::to_string(H.conn) + " defined again with another topic or type");
                } else {
                    BagConnection q;
                    q.id = H.conn;
                    q.topic = H.topic;
                    q.type = D.type;
                    q.accepted = bag_type_accepted(q.type, choice);
                    q.chosen = q.accepted && (choice.topic.empty() || q.topic == choice.topic);
                    conns.push_back(q);
                    c.n_connections++;
                    if (q.accepted && choice.topic.empty()) {
                        if (have_event_topic && q.topic != event_topic)
                            return fail("more than one topic of events and no topic chosen: " + list_connections(true));
                        have_event_topic = true;
                        event_topic = q.topic;
                    }
                }
            } else if (H.op == BAG_OP_MESSAGE) {
                if (!H.has_conn) return fail("a message without conn");
                const BagConnection *q = nullptr;
                for (const BagConnection &j : conns)
                    if (j.id == H.conn) q = &j;
                if (!q) return fail("a message of connection " + std::to_string(H.conn) + ", which is not defined in front of it");
                if (!q->chosen) {
                    c.n_other_messages++;
                } else {
                    const std::string bad = "a message of " + std::to_string(dl) + " bytes that is not 28 + L + 13 n: not the dvs_msgs/EventArray layout";
                    if (dl < BAG_MESSAGE_FIXED_BYTES) return fail(bad);
                    if (!get(data + 12, w, 4)) return fail(unreadable);
                    const uint64_t L = bag_le32(w);
                    if (L > dl - BAG_MESSAGE_FIXED_BYTES) return fail(bad);
                    if (!get(data + 16 + L, w, 12)) return fail(unreadable);
                    const uint32_t height = bag_le32(w), width = bag_le32(w + 4), n = bag_le32(w + 8);
                    if (BAG_MESSAGE_FIXED_BYTES + L + (uint64_t) BAG_EVENT_BYTES * n != dl) return fail(bad);
                    BagMessage m;
                    m.offset = data + BAG_MESSAGE_FIXED_BYTES + L;
                    m.n_events = n;
                    m.reserved = 0;
                    if (!have_first_message) {
                        have_first_message = true;
                        c.msg_width = width;
                        c.msg_height = height;
                    }
                    if (n && !have_first_stamp) {
                        if (!get(m.offset + 4, w, 4)) return fail(unreadable);
                        have_first_stamp = true;
                        c.first_stamp_ns = (int64_t) bag_le32(w) * BAG_NS_PER_S;
                    }
                    c.n_messages++;
                    c.n_raw_events += n;
                    on_message(m);
                }
            }   // (a bag header, index data, chunk info: stepped over)
            number++;
            pos = data + dl;
        }
        return BAG_OK;
    };
    const int rc = chain(chain, 13, n_bytes, false);
    if (rc) return rc;
    bool any = false;
    for (const BagConnection &q : conns) any = any || q.chosen;
    if (!any) {
        *err = std::string("no connection of ") + (choice.type.empty() ? "an event type (dvs_msgs/EventArray, prophesee_event_msgs/EventArray)" : "type " + bag_printable(choice.type)) +
               (choice.topic.empty() ? "" : " on topic " + bag_printable(choice.topic)) + "; the bag has: " + list_connections(false);
        return BAG_INVALID;
    }
    return BAG_OK;
}

// the same over a file in memory
template <class OnMessage>
inline int bag_walk_memory(const uint8_t *file, uint64_t n_bytes, const BagChoice &choice, BagCounts &c, OnMessage &&on_message, std::string *err) {
    return bag_walk([&](uint64_t pos, uint8_t *dst, size_t n) { memcpy(dst, file + pos, n); return true; }, n_bytes, choice, c, on_message, err);
}

// The table of the chosen messages.  out may be null with capacity 0 (a count).  BAG_RANGE: more than `capacity` messages —
// *n_messages is the count needed, `out` holds the first `capacity`.
inline int bag_index_messages(const uint8_t *file, uint64_t n_bytes, const BagChoice &choice, BagMessage *out, uint64_t capacity, uint64_t *n_messages,
                              BagCounts &c, std::string *err) {
    uint64_t n = 0;
    const int rc = bag_walk_memory(file, n_bytes, choice, c, [&](const BagMessage &m) {
        if (n < capacity) out[n] = m;
        n++;
    }, err);
    *n_messages = n;
    if (rc) return rc;
    if (n > capacity) {
        if (err) *err = std::to_string(n) + " messages of events, more than the capacity of the table";
        return BAG_RANGE;
    }
    return BAG_OK;
}

// the base in force: the first event's whole seconds when auto_time_base is set (0 for a bag without events)
inline int64_t bag_time_base(int auto_time_base, int64_t time_base, const BagCounts &walk) { return auto_time_base ? walk.first_stamp_ns : time_base; }

inline void bag_copy_walk_counts(BagCounts &c, const BagCounts &walk) {
    c.n_messages = walk.n_messages;
    c.n_other_messages = walk.n_other_messages;
    c.n_chunks = walk.n_chunks;
    c.n_connections = walk.n_connections;
    c.n_trailing_bytes = walk.n_trailing_bytes;
    c.first_stamp_ns = walk.first_stamp_ns;
    c.msg_width = walk.msg_width;
    c.msg_height = walk.msg_height;
}

// ---- sequential host decoder ----------------------------------------------------------------------------------------------------------
// f.time_base is ignored when auto_time_base is set: the base comes from the first event, so the walk goes first and the events
// are decoded from its table, message by message.  *base_out: the base in force.
template <class PutRecord>
inline int bag_decode_sequential(const uint8_t *file, uint64_t n_bytes, const BagChoice &choice, int auto_time_base, BagFilter f, BagCounts &c,
                                 PutRecord &&put, int64_t *base_out, std::string *err) {
    memset(&c, 0, sizeof(c));
    BagCounts walk;
    std::vector<BagMessage> tab;
    const int rc = bag_walk_memory(file, n_bytes, choice, walk, [&](const BagMessage &m) { tab.push_back(m); }, err);
    if (rc) return rc;
    f.time_base = bag_time_base(auto_time_base, f.time_base, walk);
    if (base_out) *base_out = f.time_base;
    BagSink<PutRecord> sink(f, c, put);
    for (const BagMessage &m : tab)
        for (uint64_t k = 0; k < m.n_events; k++) sink(bag_event_at(file + m.offset + BAG_EVENT_BYTES * k));
    bag_copy_walk_counts(c, walk);
    return BAG_OK;
}

// ---- the same block by block, as the kernels do it ----------------------------------------------------------------------------------
// the aligned word at a (a multiple of 4), bytes at or behind n_bytes as zeros
inline uint32_t bag_word_clipped(const uint8_t *file, uint64_t a, uint64_t n_bytes) {
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4; j++)
        if (a + j < n_bytes) v |= (uint32_t) file[a + j] << (8u * j);
    return v;
}

// the table's counts scanned into an event-slot space; a block owns block_events consecutive slots, finds the message of its first
// slot by bisection in the scanned table and steps through messages from there; every event from four aligned words
template <class PutRecord>
inline int bag_decode_blockwise(const uint8_t *file, uint64_t n_bytes, const BagChoice &choice, uint64_t block_events, int auto_time_base, BagFilter f,
                                BagCounts &c, PutRecord &&put, int64_t *base_out, std::string *err) {
    memset(&c, 0, sizeof(c));
    BagCounts walk;
    uint64_t n = 0;
    int rc = bag_index_messages(file, n_bytes, choice, nullptr, 0, &n, walk, err);
    if (rc != BAG_OK && rc != BAG_RANGE) return rc;
    std::vector<BagMessage> tab((size_t) n + 1);
    std::vector<uint64_t> first((size_t) n + 1);
    rc = bag_index_messages(file, n_bytes, choice, tab.data(), n, &n, walk, err);
    if (rc) return rc;
    f.time_base = bag_time_base(auto_time_base, f.time_base, walk);
    if (base_out) *base_out = f.time_base;
    first[0] = 0;
    for (uint64_t p = 0; p < n; p++) first[p + 1] = first[p] + tab[p].n_events;
    const uint64_t S = first[n];
    BagSink<PutRecord> sink(f, c, put);
    for (uint64_t s0 = 0; s0 < S; s0 += block_events) {
        const uint64_t s1 = s0 + block_events < S ? s0 + block_events : S;
        uint64_t lo = 0, hi = n;   // the last message whose first slot is not behind s0: it is not empty and holds s0
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (first[mid] <= s0) lo = mid; else hi = mid;
        }
        uint64_t p = lo;
        for (uint64_t s = s0; s < s1; s++) {
            while (s >= first[p + 1]) p++;
            const uint64_t off = tab[p].offset + (s - first[p]) * BAG_EVENT_BYTES, al = off & ~3ull;
            sink(bag_event_from_words(bag_word_clipped(file, al, n_bytes), bag_word_clipped(file, al + 4, n_bytes), bag_word_clipped(file, al + 8, n_bytes),
                                      bag_word_clipped(file, al + 12, n_bytes), (uint32_t) (off & 3u)));
        }
    }
    bag_copy_walk_counts(c, walk);
    return BAG_OK;
}

}  // namespace ecal_bag
