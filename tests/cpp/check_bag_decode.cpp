// CPU check of eventcalib_amd/csrc/bag_events.hpp (the bag ingest's restatement of include/ecal.h, "bag ingest").
//   1. 2 000 seeded random bags, each decoded three ways: from the generator's own book-keeping (the events it wrote, where every
//      record starts and ends, a plain filter loop — nothing of the header's walker), by the header's sequential decoder, and
//      block-wise with blocks of 1, 2, 7, 64 events and of the kernels' block.  Records and every counter must be identical.  A
//      quarter of the bags are cut short at a random byte.
//   2. the indexer's and the field parser's cases: every refusal of the contract, the choice of topic and type, every truncation
//      point, the table's capacity.
// A stand-alone program: built once with -O2 and once under -fsanitize=address,undefined by tests/test_bag_decode_host.py.
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <string>
#include <vector>
#include "bag_events.hpp"

using namespace ecal_bag;
typedef std::vector<uint8_t> Bytes;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return n ? (uint32_t) (next() % n) : 0u; }
    bool one_in(uint32_t n) { return below(n) == 0; }
};

// ---- writing records ------------------------------------------------------------------------------------------------------------------
static void put32(Bytes &b, uint32_t v) { for (int i = 0; i < 4; i++) b.push_back((uint8_t) (v >> (8 * i))); }
static void put_at(Bytes &b, size_t at, uint32_t v) { for (int i = 0; i < 4; i++) b[at + i] = (uint8_t) (v >> (8 * i)); }
static void append(Bytes &b, const Bytes &o) { b.insert(b.end(), o.begin(), o.end()); }
static Bytes str(const std::string &s) { return Bytes(s.begin(), s.end()); }
static Bytes u32(uint32_t v) { Bytes b; put32(b, v); return b; }
static Bytes field(const std::string &name, const Bytes &value) {
    Bytes b;
    put32(b, (uint32_t) (name.size() + 1 + value.size()));
    append(b, str(name + "="));
    append(b, value);
    return b;
}
static Bytes op(int code) { return field("op", Bytes(1, (uint8_t) code)); }
static Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes b;
    for (const Bytes &p : parts) append(b, p);
    return b;
}
static Bytes record(const Bytes &header, const Bytes &data) {
    Bytes b;
    put32(b, (uint32_t) header.size());
    append(b, header);
    put32(b, (uint32_t) data.size());
    append(b, data);
    return b;
}
static Bytes connection(uint32_t conn, const std::string &topic, const std::string &type) {
    return record(cat({op(BAG_OP_CONNECTION), field("conn", u32(conn)), field("topic", str(topic))}),
                  cat({field("topic", str(topic)), field("type", str(type)), field("md5sum", str("5e8beee5a6c107e504c2e78903c224b8")),
                       field("message_definition", str("Header header\nuint32 height\nuint32 width\nEvent[] events\n"))}));
}
static Bytes message(uint32_t conn, const Bytes &data) {
    return record(cat({op(BAG_OP_MESSAGE), field("conn", u32(conn)), field("time", Bytes(8, 0))}), data);
}
static Bytes chunk(const Bytes &inner, const std::string &compression = "none", int64_t size = -1) {
    return record(cat({op(BAG_OP_CHUNK), field("compression", str(compression)), field("size", u32(size < 0 ? (uint32_t) inner.size() : (uint32_t) size))}), inner);
}
static Bytes bag_header() {
    const Bytes h = cat({op(BAG_OP_BAG_HEADER), field("index_pos", Bytes(8, 0)), field("conn_count", u32(0)), field("chunk_count", u32(0))});
    return record(h, Bytes(4096 - 8 - h.size(), ' '));
}
static Bytes magic() { return str("#ROSBAG V2.0\n"); }

struct Ev {
    uint16_t x, y;
    uint32_t secs, nsecs;
    uint8_t p;
};
static Bytes event_array(const std::vector<Ev> &ev, uint32_t frame_len, uint32_t height = 260, uint32_t width = 346) {
    Bytes b;
    put32(b, 7); put32(b, 1600000000u); put32(b, 5); put32(b, frame_len);
    for (uint32_t i = 0; i < frame_len; i++) b.push_back((uint8_t) ('a' + i));
    put32(b, height); put32(b, width); put32(b, (uint32_t) ev.size());
    for (const Ev &e : ev) {
        b.push_back((uint8_t) e.x); b.push_back((uint8_t) (e.x >> 8));
        b.push_back((uint8_t) e.y); b.push_back((uint8_t) (e.y >> 8));
        put32(b, e.secs); put32(b, e.nsecs);
        b.push_back(e.p);
    }
    return b;
}

// ---- part 1 ---------------------------------------------------------------------------------------------------------------------------
struct Span {   // one record of a generated bag: where it starts, where its header (with data_len) ends, where it ends
    uint64_t start, header_end, end;
    bool is_chunk, defines_event_conn, other_message;
    int event_message;   // index into Bag::msgs, or -1
};
struct Bag {
    Bytes bytes;
    std::vector<Span> spans;              // in file order, a chunk in front of its inner records
    std::vector<std::vector<Ev>> msgs;    // the event messages
    std::vector<uint64_t> msg_offset;     // of their first event
    uint32_t first_w = 0, first_h = 0;
    uint64_t n_conn_records = 0;
};

static void add_span(Bag &g, uint64_t base, const Bytes &rec, bool is_chunk, bool defines, bool other, int em) {
    const uint64_t hl = bag_le32(rec.data());
    g.spans.push_back(Span{base, base + 8 + hl, base + rec.size(), is_chunk, defines, other, em});
}

static Bag random_bag(Rng &r, bool big) {
    Bag g;
    g.bytes = magic();
    {
        const Bytes h = bag_header();
        add_span(g, g.bytes.size(), h, false, false, false, -1);
        append(g.bytes, h);
    }
    const uint32_t n_foreign = r.below(3), n_msgs = 1 + r.below(12);
    const bool two_event_conns = r.one_in(4);   // the same topic on two connections (a recorder restarted)
    const uint32_t secs0 = 1600000000u + r.below(1000);
    std::vector<bool> seen(8, false);
    uint32_t done = 0;
    while (done < n_msgs) {
        const uint32_t in_chunk = r.one_in(6) ? 0u : 1u + r.below(4);   // 0: unchunked, at top level
        Bytes inner;
        std::vector<Span> inner_spans;
        std::vector<std::pair<size_t, uint64_t>> fix;   // (message index, offset of its first event within inner)
        const uint32_t take = in_chunk ? in_chunk : 1u;
        Bag local;
        for (uint32_t k = 0; k < take && done < n_msgs; k++, done++) {
            const bool foreign = n_foreign && r.one_in(3);
            const uint32_t conn = foreign ? 2u + r.below(n_foreign) : (two_event_conns ? r.below(2) : 0u);
            if (!seen[conn]) {
                seen[conn] = true;
                const Bytes c = connection(conn, conn < 2 ? "/dvs/events" : "/dvs/image_raw", conn < 2 ? (conn ? "prophesee_event_msgs/EventArray" : "dvs_msgs/EventArray") : "sensor_msgs/Image");
                add_span(local, inner.size(), c, false, conn < 2, false, -1);
                append(inner, c);
            }
            Bytes m;
            if (foreign) {
                m = message(conn, Bytes(r.below(60), 0xA5));
                add_span(local, inner.size(), m, false, false, true, -1);
            } else {
                const uint32_t n = r.one_in(5) ? 0u : (big && r.one_in(3) ? 1000u + r.below(1200) : 1u + r.below(40));
                std::vector<Ev> ev(n);
                for (Ev &e : ev) {
                    e.x = (uint16_t) r.below(346);
                    e.y = (uint16_t) r.below(260);
                    e.secs = secs0 + r.below(3) - (r.one_in(40) ? 1u : 0u);
                    e.nsecs = r.one_in(30) ? 1000000000u + r.below(200000000) : r.below(1000000000);
                    e.p = r.one_in(10) ? (uint8_t) r.below(256) : (uint8_t) r.below(2);
                }
                const uint32_t fl = r.below(8), w = r.one_in(4) ? 240 : 346, h = r.one_in(4) ? 180 : 260;
                const Bytes data = event_array(ev, fl, h, w);
                m = message(conn, data);
                if (g.msgs.empty() && local.msgs.empty()) { g.first_w = w; g.first_h = h; }
                add_span(local, inner.size(), m, false, false, false, (int) (g.msgs.size() + local.msgs.size()));
                local.msgs.push_back(ev);
                local.msg_offset.push_back(inner.size() + (m.size() - data.size()) + 28 + fl);
            }
            append(inner, m);
        }
        uint64_t base = g.bytes.size();
        if (in_chunk) {
            const Bytes c = chunk(inner);
            add_span(g, base, c, true, false, false, -1);
            base += c.size() - inner.size();
            append(g.bytes, c);
        } else {
            append(g.bytes, inner);
        }
        for (Span s : local.spans) {
            s.start += base; s.header_end += base; s.end += base;
            g.spans.push_back(s);
        }
        for (size_t i = 0; i < local.msgs.size(); i++) {
            g.msgs.push_back(local.msgs[i]);
            g.msg_offset.push_back(local.msg_offset[i] + base);
        }
        if (in_chunk && r.one_in(2)) {   // an index data record behind the chunk
            const Bytes x = record(cat({op(BAG_OP_INDEX), field("ver", u32(1)), field("conn", u32(0)), field("count", u32(1))}), Bytes(12, 0));
            add_span(g, g.bytes.size(), x, false, false, false, -1);
            append(g.bytes, x);
        }
    }
    if (r.one_in(2)) {   // closed: the connections again, a chunk info record
        for (uint32_t conn = 0; conn < 8; conn++) {
            if (!seen[conn]) continue;
            const Bytes c = connection(conn, conn < 2 ? "/dvs/events" : "/dvs/image_raw", conn < 2 ? (conn ? "prophesee_event_msgs/EventArray" : "dvs_msgs/EventArray") : "sensor_msgs/Image");
            add_span(g, g.bytes.size(), c, false, conn < 2, false, -1);
            append(g.bytes, c);
        }
        const Bytes x = record(cat({op(BAG_OP_CHUNK_INFO), field("ver", u32(1)), field("chunk_pos", Bytes(8, 0)), field("count", u32(0))}), Bytes());
        add_span(g, g.bytes.size(), x, false, false, false, -1);
        append(g.bytes, x);
    }
    return g;
}

struct Result {
    int rc = 0;
    Bytes records;
    BagCounts c;
    int64_t base = 0;
};

static bool same(const Result &a, const Result &b, bool walk_fields) {
    if (a.rc != b.rc) return false;
    if (a.rc) return true;
    if (a.records != b.records || a.base != b.base) return false;
    const BagCounts &p = a.c, &q = b.c;
    if (p.n_raw_events != q.n_raw_events || p.n_events != q.n_events || p.n_outside != q.n_outside || p.n_negative != q.n_negative ||
        p.n_before_start != q.n_before_start || p.n_after_end != q.n_after_end || p.n_messages != q.n_messages)
        return false;
    if (!walk_fields) return true;
    return p.n_other_messages == q.n_other_messages && p.n_chunks == q.n_chunks && p.n_trailing_bytes == q.n_trailing_bytes &&
           p.first_stamp_ns == q.first_stamp_ns && p.msg_width == q.msg_width && p.msg_height == q.msg_height;
}

// what the contract says of this bag cut at `cut` bytes, from the generator's book-keeping alone
static Result expected(const Bag &g, uint64_t cut, int auto_base, BagFilter f) {
    Result R;
    memset(&R.c, 0, sizeof(R.c));
    bool event_conn = false, have_stamp = false, have_first = false;
    std::vector<int> present;
    for (const Span &s : g.spans) {
        if (s.is_chunk ? cut < s.header_end : cut < s.end) {
            R.c.n_trailing_bytes = cut > s.start ? cut - s.start : 0;
            if (cut <= s.start) R.c.n_trailing_bytes = 0;
            break;
        }
        if (s.is_chunk) R.c.n_chunks++;
        if (s.defines_event_conn) event_conn = true;
        if (s.other_message) R.c.n_other_messages++;
        if (s.event_message >= 0) present.push_back(s.event_message);
    }
    if (!event_conn) {
        R.rc = BAG_INVALID;
        return R;
    }
    for (int m : present) {
        R.c.n_messages++;
        if (!have_first) { have_first = true; }
        if (!g.msgs[m].empty() && !have_stamp) {
            have_stamp = true;
            R.c.first_stamp_ns = (int64_t) g.msgs[m][0].secs * 1000000000ll;
        }
    }
    if (have_first) { R.c.msg_width = g.first_w; R.c.msg_height = g.first_h; }
    if (auto_base) f.time_base = R.c.first_stamp_ns;
    R.base = f.time_base;
    bool stopped = false;
    for (int m : present) {
        for (const Ev &e : g.msgs[m]) {
            R.c.n_raw_events++;
            if (stopped) { R.c.n_after_end++; continue; }
            if ((f.width && e.x >= f.width) || (f.height && e.y >= f.height)) { R.c.n_outside++; continue; }
            const int64_t t_ns = (int64_t) e.secs * 1000000000ll + (int64_t) e.nsecs;
            const double t = (double) (t_ns - f.time_base) * 1e-9;
            if (t < 0) { R.c.n_negative++; continue; }
            if (f.has_end_time && t >= f.end_time) { stopped = true; R.c.n_after_end++; continue; }
            if (!(t >= f.start_time)) { R.c.n_before_start++; continue; }
            const double x = f.flip_x ? (double) (f.width - 1 - e.x) : (double) e.x, y = f.flip_y ? (double) (f.height - 1 - e.y) : (double) e.y;
            uint8_t rec[25];
            memcpy(rec, &t, 8); memcpy(rec + 8, &x, 8); memcpy(rec + 16, &y, 8);   // (little-endian hosts only, as the rest of the suite)
            rec[24] = e.p ? 1 : 0;
            R.records.insert(R.records.end(), rec, rec + 25);
            R.c.n_events++;
        }
    }
    return R;
}

static int part1() {
    int wrong = 0;
    const uint64_t blocks[5] = {1, 2, 7, 64, BAG_BLOCK_EVENTS};
    uint64_t events = 0, cut_bags = 0, refused = 0;
    for (uint32_t seed = 0; seed < 2000; seed++) {
        Rng r(seed);
        const Bag g = random_bag(r, seed % 25 == 0);
        uint64_t cut = g.bytes.size();
        if (seed % 4 == 3) {
            // (mostly behind the 4096 bytes of the bag header, where the records of interest are)
            cut = r.one_in(8) ? 13 + r.below(4096) : 4109 + r.below((uint32_t) (g.bytes.size() - 4109));
            cut_bags++;
        }
        BagFilter f;
        memset(&f, 0, sizeof(f));
        f.start_time = -INFINITY;
        const int auto_base = r.one_in(2) ? 0 : 1;
        f.time_base = 1600000000ll * 1000000000ll + (int64_t) r.below(1000) * 1000000000ll + r.below(2000000000);
        if (r.one_in(2)) { f.width = 300; f.height = 200; f.flip_x = r.below(2); f.flip_y = r.below(2); }
        if (r.one_in(3)) f.start_time = 0.1 * r.below(20);
        if (r.one_in(3)) { f.has_end_time = 1; f.end_time = 0.1 * r.below(40); }
        const Result want = expected(g, cut, auto_base, f);
        // the file in a buffer of exactly its size: the sanitizer sees any byte read behind it
        uint8_t *file = (uint8_t *) malloc(cut ? cut : 1);
        memcpy(file, g.bytes.data(), cut);
        Result seq;
        std::string err;
        auto put_seq = [&](const uint8_t *rec) { seq.records.insert(seq.records.end(), rec, rec + 25); };
        seq.rc = bag_decode_sequential(file, cut, BagChoice(), auto_base, f, seq.c, put_seq, &seq.base, &err);
        if (!same(want, seq, true)) {
            if (wrong++ < 5) printf("seed %u: the sequential decoder differs from the generator (rc %d / %d, %s)\n", seed, want.rc, seq.rc, err.c_str());
        }
        if (want.rc) refused++;
        for (uint64_t be : blocks) {
            Result blk;
            auto put_blk = [&](const uint8_t *rec) { blk.records.insert(blk.records.end(), rec, rec + 25); };
            blk.rc = bag_decode_blockwise(file, cut, BagChoice(), be, auto_base, f, blk.c, put_blk, &blk.base, &err);
            if (!same(seq, blk, true) || (!seq.rc && seq.c.n_connections != blk.c.n_connections)) {
                if (wrong++ < 5) printf("seed %u: blocks of %llu differ from the sequential decoder\n", seed, (unsigned long long) be);
            }
        }
        if (!seq.rc) {
            events += seq.c.n_raw_events;
            if (seq.c.n_events + seq.c.n_outside + seq.c.n_negative + seq.c.n_before_start + seq.c.n_after_end != seq.c.n_raw_events) wrong++;
        }
        free(file);
    }
    printf("bags: 2000 bags %s (%llu events, %llu bags cut short, %llu refused for no connection in front of the cut)\n", wrong ? "DIFFER" : "equal",
           (unsigned long long) events, (unsigned long long) cut_bags, (unsigned long long) refused);
    return wrong;
}

// ---- part 2 ---------------------------------------------------------------------------------------------------------------------------
static int n_cases = 0, n_wrong = 0;

struct Indexed {
    int rc;
    std::string err;
    BagCounts c;
    std::vector<BagMessage> tab;
};
static Indexed index_of(const Bytes &b, const std::string &topic = "", const std::string &type = "") {
    Indexed I;
    BagChoice ch;
    ch.topic = topic;
    ch.type = type;
    uint8_t *file = (uint8_t *) malloc(b.size() ? b.size() : 1);
    if (!b.empty()) memcpy(file, b.data(), b.size());
    uint64_t n = 0;
    I.rc = bag_index_messages(file, b.size(), ch, nullptr, 0, &n, I.c, &I.err);
    if (I.rc == BAG_RANGE) {   // (the count-only form says so whenever there is a message)
        I.tab.resize((size_t) n);
        I.rc = bag_index_messages(file, b.size(), ch, I.tab.data(), n, &n, I.c, &I.err);
    }
    free(file);
    return I;
}
static void refuse(const char *name, const Bytes &b, std::initializer_list<const char *> words, const std::string &topic = "", const std::string &type = "") {
    n_cases++;
    const Indexed I = index_of(b, topic, type);
    bool ok = I.rc == BAG_INVALID;
    for (const char *w : words) ok = ok && I.err.find(w) != std::string::npos;
    if (!ok) {
        n_wrong++;
        printf("case %s: rc %d, text \"%s\"\n", name, I.rc, I.err.c_str());
    }
}
static void accept(const char *name, const Bytes &b, uint64_t messages, uint64_t raw, uint64_t other, uint64_t chunks, uint64_t trailing,
                   const std::string &topic = "", const std::string &type = "") {
    n_cases++;
    const Indexed I = index_of(b, topic, type);
    uint64_t sum = 0;
    for (const BagMessage &m : I.tab) sum += m.n_events;
    if (I.rc != BAG_OK || I.c.n_messages != messages || I.tab.size() != messages || I.c.n_raw_events != raw || sum != raw || I.c.n_other_messages != other ||
        I.c.n_chunks != chunks || I.c.n_trailing_bytes != trailing) {
        n_wrong++;
        printf("case %s: rc %d (%s), %llu messages, %llu events, %llu other, %llu chunks, %llu trailing\n", name, I.rc, I.err.c_str(),
               (unsigned long long) I.c.n_messages, (unsigned long long) I.c.n_raw_events, (unsigned long long) I.c.n_other_messages,
               (unsigned long long) I.c.n_chunks, (unsigned long long) I.c.n_trailing_bytes);
    }
}

static std::vector<Ev> some_events(uint32_t n, uint32_t secs = 1600000000u) {
    std::vector<Ev> ev(n);
    for (uint32_t i = 0; i < n; i++) ev[i] = Ev{(uint16_t) (i % 346), (uint16_t) (i % 260), secs, 1000u * i, (uint8_t) (i & 1)};
    return ev;
}

static int part2() {
    const Bytes head = cat({magic(), bag_header()});
    const Bytes c0 = connection(0, "/dvs/events", "dvs_msgs/EventArray"), c1 = connection(1, "/dvs/image_raw", "sensor_msgs/Image");
    const Bytes m3 = message(0, event_array(some_events(3), 2)), m5 = message(0, event_array(some_events(5), 0)), img = message(1, Bytes(77, 1));
    const Bytes good = cat({head, chunk(cat({c0, c1, m3, img})), chunk(cat({m5, img, img})), c0, c1});

    // the file
    accept("a plain bag", good, 2, 8, 3, 2, 0);
    {
        Bytes b = good;
        memcpy(b.data(), "#ROSBAG V1.2\n", 13);
        refuse("format 1.2", b, {"1.2"});
    }
    refuse("an SQLite file", cat({Bytes{'S', 'Q', 'L', 'i', 't', 'e', ' ', 'f', 'o', 'r', 'm', 'a', 't', ' ', '3', 0}, Bytes(100, 0)}), {"ROS 2", "SQLite"});
    refuse("an MCAP file", cat({Bytes{0x89, 'M', 'C', 'A', 'P', '0', '\r', '\n'}, Bytes(100, 0)}), {"ROS 2", "MCAP"});
    refuse("something else", Bytes(64, 'x'), {"not a ROS 1 bag"});
    refuse("an empty file", Bytes(), {"not a ROS 1 bag"});
    refuse("only the version line", magic(), {"no connection"});

    // fields and headers
    {
        Bytes h = cat({op(BAG_OP_INDEX), field("ver", u32(1))});
        put_at(h, h.size() - 12, 200);   // the last field's length runs past the header
        refuse("a field past its header", cat({head, record(h, Bytes())}), {"record 1 at byte 4109", "runs past its header"});
        Bytes g2 = op(BAG_OP_INDEX);
        put32(g2, 3); append(g2, str("abc"));
        refuse("a field without =", cat({head, record(g2, Bytes())}), {"record 1", "'='"});
        refuse("no op", cat({head, record(field("conn", u32(0)), Bytes())}), {"record 1 at byte 4109", "op field"});
        refuse("an op of two bytes", cat({head, record(field("op", Bytes(2, 2)), Bytes())}), {"op field"});
        refuse("three bytes where a field length should be", cat({head, record(cat({op(BAG_OP_INDEX), Bytes(3, 0)}), Bytes())}), {"runs past its header"});
        accept("unknown fields are ignored", cat({head, record(cat({field("zzz", Bytes(9, 0xFF)), op(BAG_OP_INDEX), field("=x", str("=="))}), Bytes(5, 0)), chunk(cat({c0, m3}))}), 1, 3, 0, 1, 0);
    }
    refuse("an unknown op", cat({head, record(op(0x09), Bytes())}), {"record 1", "0x09"});
    refuse("op 0x01", cat({head, chunk(cat({c0, m3})), record(op(0x01), Bytes())}), {"record 4", "0x01"});

    // chunks
    refuse("bz2", cat({head, chunk(cat({c0, m3}), "bz2")}), {"bz2", "rosbag decompress", "record 1 at byte 4109"});
    refuse("lz4", cat({head, chunk(cat({c0, m3})), chunk(cat({m3}), "lz4")}), {"lz4", "rosbag decompress", "record 4"});
    refuse("size is not data_len", cat({head, chunk(cat({c0, m3}), "none", 5)}), {"size field"});
    refuse("a chunk without compression", cat({head, record(cat({op(BAG_OP_CHUNK), field("size", u32(0))}), Bytes())}), {"compression"});
    refuse("a chunk in a chunk", cat({head, chunk(cat({c0, chunk(m3)}))}), {"0x05 inside a chunk", "record 3"});
    refuse("a bag header in a chunk", cat({head, chunk(cat({c0, bag_header()}))}), {"0x03 inside a chunk"});
    refuse("index data in a chunk", cat({head, chunk(cat({c0, record(op(BAG_OP_INDEX), Bytes())}))}), {"0x04 inside a chunk"});
    {
        Bytes inner = cat({c0, m3});
        inner.resize(inner.size() - 4);   // the last inner record runs past the chunk's end; the chunk itself is whole
        refuse("an inner record past its chunk", cat({head, chunk(inner), c0}), {"runs past the end of its chunk", "record 3"});
    }

    // connections and the choice
    refuse("a connection redefined", cat({head, chunk(cat({c0, m3})), connection(0, "/other", "dvs_msgs/EventArray")}), {"connection 0", "defined again"});
    refuse("a connection redefined with another type", cat({head, chunk(cat({c0, m3, connection(0, "/dvs/events", "sensor_msgs/Image")}))}), {"defined again"});
    accept("a connection repeated", cat({head, chunk(cat({c0, m3, c0})), c0}), 1, 3, 0, 1, 0);
    refuse("a connection without a type", cat({head, record(cat({op(BAG_OP_CONNECTION), field("conn", u32(0)), field("topic", str("/t"))}), field("topic", str("/t")))}), {"without a type"});
    refuse("a connection without conn", cat({head, record(cat({op(BAG_OP_CONNECTION), field("topic", str("/t"))}), field("type", str("dvs_msgs/EventArray")))}), {"without conn"});
    const Bytes cl = connection(4, "/davis/left/events", "dvs_msgs/EventArray"), cr = connection(5, "/davis/right/events", "dvs_msgs/EventArray");
    const Bytes ml = message(4, event_array(some_events(4), 1)), mr = message(5, event_array(some_events(6), 3));
    const Bytes stereo = cat({head, chunk(cat({cl, ml, cr, mr, ml})), cl, cr});
    refuse("two topics of events", stereo, {"/davis/left/events", "/davis/right/events", "no topic chosen"});
    accept("the left topic", stereo, 2, 8, 1, 1, 0, "/davis/left/events");
    accept("the right topic", stereo, 1, 6, 2, 1, 0, "/davis/right/events");
    refuse("a topic that is not there", stereo, {"/davis/middle", "/davis/left/events (dvs_msgs/EventArray)"}, "/davis/middle");
    refuse("no event type", cat({head, chunk(cat({c1, img})), c1}), {"no connection", "/dvs/image_raw (sensor_msgs/Image)"});
    accept("another type by name", cat({head, chunk(cat({connection(0, "/cam", "my_msgs/Events"), m3, c1, img}))}), 1, 3, 1, 1, 0, "", "my_msgs/Events");
    refuse("the type option replaces the defaults", good, {"my_msgs/Events"}, "", "my_msgs/Events");
    accept("the prophesee type", cat({head, chunk(cat({connection(0, "/cam", "prophesee_event_msgs/EventArray"), m3}))}), 1, 3, 0, 1, 0);

    // messages
    refuse("a message of an undefined connection", cat({head, chunk(cat({c0, message(9, Bytes(40, 0))}))}), {"connection 9", "not defined"});
    refuse("a message without conn", cat({head, chunk(cat({c0, record(op(BAG_OP_MESSAGE), Bytes(40, 0))}))}), {"without conn"});
    {
        Bytes d = event_array(some_events(3), 2);
        d.push_back(0);
        refuse("a message one byte longer", cat({head, chunk(cat({c0, message(0, d)}))}), {"record 3", "28 + L + 13 n"});
        refuse("a message shorter than its fixed part", cat({head, chunk(cat({c0, message(0, Bytes(27, 0))}))}), {"28 + L + 13 n"});
        Bytes e = event_array(some_events(3), 2);
        put_at(e, 12, 0x7FFFFFFF);
        refuse("a frame_id longer than the message", cat({head, chunk(cat({c0, message(0, e)}))}), {"28 + L + 13 n"});
        Bytes f = event_array(some_events(3), 2);
        put_at(f, 16 + 2 + 8, 0xFFFFFFFF);   // n: 13 n wraps 32 bits, not 64
        refuse("an event count that does not fit", cat({head, chunk(cat({c0, message(0, f)}))}), {"28 + L + 13 n"});
    }
    accept("a message at top level", cat({head, c0, m3, c1, img, m5}), 2, 8, 1, 0, 0);
    accept("a message of no events", cat({head, chunk(cat({c0, message(0, event_array(some_events(0), 5)), m3}))}), 2, 3, 0, 1, 0);

    // cut short: outer header, outer data, chunk data between and inside inner records, message data
    const Bytes ch1 = chunk(cat({c0, c1, m3, img})), ch2 = chunk(cat({m5, img, img}));
    const uint64_t at2 = head.size() + ch1.size(), hdr2 = ch2.size() - (m5.size() + 2 * img.size());
    auto cut_to = [&](uint64_t n) { Bytes b = cat({head, ch1, ch2, c0, c1}); b.resize((size_t) n); return b; };
    accept("cut in the second chunk's length", cut_to(at2 + 2), 1, 3, 1, 1, 2);
    accept("cut in the second chunk's header", cut_to(at2 + 10), 1, 3, 1, 1, 10);
    accept("cut at the start of the second chunk's data", cut_to(at2 + hdr2), 1, 3, 1, 2, 0);
    accept("cut in an inner header", cut_to(at2 + hdr2 + 6), 1, 3, 1, 2, 6);
    accept("cut in the message's events", cut_to(at2 + hdr2 + m5.size() - 1), 1, 3, 1, 2, m5.size() - 1);
    accept("cut behind the message", cut_to(at2 + hdr2 + m5.size()), 2, 8, 1, 2, 0);
    accept("cut in a foreign message", cut_to(at2 + hdr2 + m5.size() + img.size() + 20), 2, 8, 2, 2, 20);
    accept("cut in the connection behind the chunks", cut_to(at2 + ch2.size() + 30), 2, 8, 3, 2, 30);
    refuse("cut in the bag header's padding", cut_to(2000), {"no connection"});

    // the table's capacity
    {
        n_cases++;
        uint64_t n = 0;
        BagCounts c;
        std::string err;
        BagMessage one[1];
        const int rc = bag_index_messages(good.data(), good.size(), BagChoice(), one, 1, &n, c, &err);
        if (rc != BAG_RANGE || n != 2 || one[0].n_events != 3 || one[0].reserved != 0) { n_wrong++; printf("case capacity: rc %d, n %llu\n", rc, (unsigned long long) n); }
        n_cases++;
        const int rc0 = bag_index_messages(good.data(), good.size(), BagChoice(), nullptr, 0, &n, c, &err);
        if (rc0 != BAG_RANGE || n != 2 || c.n_raw_events != 8 || c.first_stamp_ns != 1600000000ll * 1000000000ll || c.msg_width != 346 || c.msg_height != 260 || c.n_connections != 2) {
            n_wrong++;
            printf("case count: rc %d, n %llu\n", rc0, (unsigned long long) n);
        }
    }
    // the four words of a record at every residue
    {
        n_cases++;
        uint8_t buf[32];
        bool ok = true;
        for (uint32_t r = 0; r < 4; r++) {
            for (int i = 0; i < 32; i++) buf[i] = (uint8_t) (0xC0 + i);
            const Ev e{0x1234, 0x0105, 0x89ABCDEFu, 0xFEDCBA98u, (uint8_t) (r == 2 ? 0 : 0x80)};
            const Bytes one = event_array(std::vector<Ev>(1, e), 0);
            memcpy(buf + r, one.data() + 28, 13);
            const uint64_t n_bytes = r + 13;   // the record's last byte is the last byte: the fourth word is clipped
            const BagEvent a = bag_event_at(buf + r);
            const BagEvent b = bag_event_from_words(bag_word_clipped(buf, 0, n_bytes), bag_word_clipped(buf, 4, n_bytes), bag_word_clipped(buf, 8, n_bytes),
                                                    bag_word_clipped(buf, 12, n_bytes), r);
            const int64_t t = (int64_t) 0x89ABCDEFu * 1000000000ll + (int64_t) 0xFEDCBA98u;
            ok = ok && a.t_ns == t && b.t_ns == t && a.x == 0x1234 && b.x == 0x1234 && a.y == 0x0105 && b.y == 0x0105 && a.pol == (r == 2 ? 0 : 1) && b.pol == a.pol;
        }
        if (!ok) { n_wrong++; printf("case words: a record differs\n"); }
    }
    printf("indexer: %d cases, %d wrong\n", n_cases, n_wrong);
    return n_wrong;
}

int main() {
    const int w1 = part1(), w2 = part2();
    return w1 || w2 ? 1 : 0;
}
