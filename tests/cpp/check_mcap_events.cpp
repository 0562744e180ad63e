// CPU check of eventcalib_amd/csrc/mcap_events.hpp (tests/test_mcap_decode_host.py compiles it plainly and under AddressSanitizer +
// UndefinedBehaviorSanitizer): the schema parser, the derived STRUCT layouts, the CDR walk, the chain of records, the host decoder
// against answers assembled by hand, the word-wise fetch of the kernels against the byte-wise one, and every refusal with the words
// its text must contain.  The files are built here, byte by byte, by a writer of this file's own.
#include <math.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "mcap_events.hpp"

using namespace ecal_mcap;
typedef std::vector<uint8_t> Bytes;

static int wrong = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            wrong++;                                                             \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                     \
        }                                                                        \
    } while (0)

// ---- a writer ---------------------------------------------------------------------------------------------------------------------------
static void put(Bytes &b, uint64_t v, int n) {
    for (int i = 0; i < n; i++) b.push_back((uint8_t) (v >> (8 * i)));
}
static void append(Bytes &b, const Bytes &o) { b.insert(b.end(), o.begin(), o.end()); }
static void str32(Bytes &b, const std::string &s) {
    put(b, s.size(), 4);
    b.insert(b.end(), s.begin(), s.end());
}
static Bytes record(int op, const Bytes &content) {
    Bytes r;
    put(r, (uint64_t) op, 1);
    put(r, content.size(), 8);
    append(r, content);
    return r;
}
static Bytes schema(int id, const std::string &name, const std::string &enc, const std::string &text) {
    Bytes c;
    put(c, id, 2);
    str32(c, name);
    str32(c, enc);
    str32(c, text);
    return record(MCAP_OP_SCHEMA, c);
}
static Bytes channel(int id, int schema_id, const std::string &topic, const std::string &enc = "cdr") {
    Bytes c;
    put(c, id, 2);
    put(c, schema_id, 2);
    str32(c, topic);
    str32(c, enc);
    put(c, 0, 4);
    return record(MCAP_OP_CHANNEL, c);
}
static Bytes message(int ch, const Bytes &data) {
    Bytes c;
    put(c, ch, 2);
    put(c, 1, 4);
    put(c, 2, 8);
    put(c, 3, 8);
    append(c, data);
    return record(MCAP_OP_MESSAGE, c);
}
static Bytes chunk(const Bytes &records, const std::string &compression = "", int64_t len_delta = 0) {
    Bytes c;
    put(c, 0, 8);
    put(c, 0, 8);
    put(c, records.size(), 8);
    put(c, 0, 4);
    str32(c, compression);
    put(c, records.size() + len_delta, 8);
    append(c, records);
    return record(MCAP_OP_CHUNK, c);
}
static Bytes magic() {
    static const uint8_t m[8] = {0x89, 'M', 'C', 'A', 'P', '0', '\r', '\n'};
    return Bytes(m, m + 8);
}
static Bytes file_of(std::initializer_list<Bytes> records, bool closed = true) {
    Bytes f = magic();
    Bytes h;
    str32(h, "ros2");
    str32(h, "check");
    append(f, record(MCAP_OP_HEADER, h));
    for (const Bytes &r : records) append(f, r);
    if (closed) {
        append(f, record(MCAP_OP_DATA_END, Bytes(4, 0)));
        append(f, record(MCAP_OP_FOOTER, Bytes(20, 0)));
        append(f, magic());
    }
    return f;
}

struct Cdr {
    Bytes b{0, 1, 0, 0};
    void align(size_t a) {
        while ((b.size() - 4) % a) b.push_back(0);
    }
    void prim(uint64_t v, int size) {
        align((size_t) size);
        put(b, v, size);
    }
    void string(const std::string &s) {
        prim(s.size() + 1, 4);
        b.insert(b.end(), s.begin(), s.end());
        b.push_back(0);
    }
    void header(int32_t sec, uint32_t nsec, const std::string &frame) {
        prim((uint32_t) sec, 4);
        prim(nsec, 4);
        string(frame);
    }
};

struct Ev {
    uint32_t x, y;
    int32_t sec;
    uint32_t nsec;
    uint8_t pol;
};

static const char TIME_DEP[] = "================\nMSG: builtin_interfaces/Time\nint32 sec\nuint32 nanosec\n";
static const std::string DVS = std::string("# events\nstd_msgs/Header header\nuint32 height  # rows\nuint32 width\nEvent[] events\n"
                                           "================\nMSG: dvs_msgs/Event\nuint16 x\nuint16 y\nbuiltin_interfaces/Time ts\nbool polarity\n") + TIME_DEP;
static const std::string PACKET = std::string("std_msgs/Header header\nstring encoding\nuint64 seq\nuint64 time_base\nuint32 width\nuint32 height\n"
                                              "bool is_bigendian\nuint8 KIND=3\nuint8[] events\n") + TIME_DEP;

// dvs_msgs/EventArray, CDR, field by field
static Bytes dvs_message(const std::vector<Ev> &ev, const std::string &frame = "cam") {
    Cdr c;
    c.header(5, 6, frame);
    c.prim(260, 4);
    c.prim(346, 4);
    c.prim(ev.size(), 4);
    for (const Ev &e : ev) {
        c.prim(e.x, 2);
        c.prim(e.y, 2);
        c.prim((uint32_t) e.sec, 4);
        c.prim(e.nsec, 4);
        c.prim(e.pol, 1);
    }
    return c.b;
}
static Bytes packet_message(const Bytes &payload, const std::string &encoding, uint64_t time_base, int big = 0, const std::string &frame = "") {
    Cdr c;
    c.header(5, 6, frame);
    c.string(encoding);
    c.prim(9, 8);
    c.prim(time_base, 8);
    c.prim(346, 4);
    c.prim(260, 4);
    c.prim((uint64_t) big, 1);
    c.prim(payload.size(), 4);
    append(c.b, payload);
    return c.b;
}
static Bytes mono_words(const std::vector<Ev> &ev) {   // nsec stands for dt
    Bytes p;
    for (const Ev &e : ev) put(p, (uint64_t) e.nsec | ((uint64_t) e.x << 32) | ((uint64_t) e.y << 48) | ((uint64_t) e.pol << 63), 8);
    return p;
}

struct Decoded {
    int rc;
    std::string err;
    McapCounts c;
    std::vector<uint8_t> rec;
    int64_t base;
};
static Decoded decode(const Bytes &f, const std::string &topic = "", int auto_base = 1, BagFilter flt = BagFilter{0, 0, 0, -INFINITY, 0, 0.0, 0, 0}, bool blockwise = false) {
    Decoded d;
    d.base = 0;
    auto put_rec = [&](const uint8_t *r) { d.rec.insert(d.rec.end(), r, r + 25); };
    d.rc = mcap_decode_sequential(f.data(), f.size(), topic, auto_base, flt, d.c, put_rec, &d.base, &d.err, blockwise);
    return d;
}
static double rec_t(const Decoded &d, size_t k) { double v; memcpy(&v, d.rec.data() + 25 * k, 8); return v; }
static double rec_x(const Decoded &d, size_t k) { double v; memcpy(&v, d.rec.data() + 25 * k + 8, 8); return v; }
static double rec_y(const Decoded &d, size_t k) { double v; memcpy(&v, d.rec.data() + 25 * k + 16, 8); return v; }
static int rec_p(const Decoded &d, size_t k) { return d.rec[25 * k + 24]; }

static int refusals = 0;
static void refused(const Bytes &f, std::initializer_list<const char *> words, const std::string &topic = "") {
    const Decoded d = decode(f, topic);
    refusals++;
    if (d.rc != MCAP_INVALID) {
        wrong++;
        printf("FAILED refusal %d: not refused (rc %d)\n", refusals, d.rc);
        return;
    }
    for (const char *w : words)
        if (d.err.find(w) == std::string::npos) {
            wrong++;
            printf("FAILED refusal %d: '%s' is not in '%s'\n", refusals, w, d.err.c_str());
        }
}

int main() {
    // ---- layouts ------------------------------------------------------------------------------------------------------------------------
    int layouts = 0;
    {
        McapSchemaLayout S;
        std::string err;
        CHECK(mcap_schema_layout(DVS, S, &err) == 1 && !S.packet);
        const McapLayout &L = S.layout;   // the numbers of the contract's paragraph
        CHECK(L.kind == MCAP_STRUCT && L.lead == 14 && L.stride == 16 && L.span[0] == 13 && L.span[1] == 15);
        CHECK(L.x[0] == 0 && L.y[0] == 2 && L.sec[0] == 4 && L.nsec[0] == 8 && L.pol[0] == 12);
        CHECK(L.x[1] == 0 && L.y[1] == 2 && L.sec[1] == 6 && L.nsec[1] == 10 && L.pol[1] == 14 && L.x_bytes == 2 && L.y_bytes == 2);
        const char *why;
        CHECK(mcap_layout_valid(L, &why));
        CHECK(mcap_message_bytes(L, 0) == 0 && mcap_message_bytes(L, 1) == 13 && mcap_message_bytes(L, 2) == 29 && mcap_message_bytes(L, 3) == 45);
        layouts++;
        // uint8 x, y; the package prefix left off; permuted; p and t for the names
        const std::string small = std::string("Header header\nEvent[] events\n===\nMSG: my_msgs/Event\nuint8 x\nuint8 y\nbuiltin_interfaces/Time t\nuint8 p\n") + TIME_DEP;
        CHECK(mcap_schema_layout(small, S, &err) == 1);
        CHECK(L.lead == 13 && L.stride == 12 && L.span[0] == 13 && L.span[1] == 12 && L.x_bytes == 1 && L.y_bytes == 1);
        CHECK(L.x[0] == 0 && L.y[0] == 1 && L.sec[0] == 4 && L.nsec[0] == 8 && L.pol[0] == 12);
        CHECK(L.x[1] == 0 && L.y[1] == 1 && L.sec[1] == 3 && L.nsec[1] == 7 && L.pol[1] == 11);
        layouts++;
        const std::string stamp_first = std::string("prophesee_event_msgs/Event[<=100000] events\nuint32 width\n===\nMSG: prophesee_event_msgs/msg/Event\n"
                                                    "builtin_interfaces/msg/Time stamp # first\nbool polarity\nuint32 x\nuint16 y\n");
        CHECK(mcap_schema_layout(stamp_first, S, &err) == 1);
        CHECK(L.lead == 20 && L.stride == 20 && L.span[0] == 18 && L.span[1] == 18 && L.x_bytes == 4 && L.y_bytes == 2);   // x aligns to 12, y to 16
        for (int w = 0; w < 2; w++) CHECK(L.sec[w] == 0 && L.nsec[w] == 4 && L.pol[w] == 8 && L.x[w] == 12 && L.y[w] == 16);
        layouts++;
        CHECK(mcap_schema_layout(PACKET, S, &err) == 1 && S.packet && S.layout.kind == MCAP_NONE);
        CHECK(mcap_schema_layout("uint32 height\nuint8[] data\n", S, &err) == 0);
        layouts++;
    }
    printf("layouts: %d cases\n", layouts);

    // ---- the parser -------------------------------------------------------------------------------------------------------------------
    int parser = 0;
    {
        const std::vector<McapSection> sec = mcap_parse_definition(
            "# a comment\n\nint32 A=5\nint32 B = 6\nstring NAME=\"x # y\"\nfloat64[9] k  # nine\nuint8[<=4] few\nstring<=10 name\nint16 v 7\n"
            "geometry_msgs/Pose pose\nbuiltin_interfaces/Time stamp\nstd_msgs/msg/Header h\n================\nMSG: geometry_msgs/Pose\nfloat64 x\n");
        CHECK(sec.size() == 2 && sec[0].fields.size() == 7 && sec[1].name == "geometry_msgs/Pose" && sec[1].fields.size() == 1);
        const std::vector<McapField> &f = sec[0].fields;
        CHECK(f[0].kind == MF_ARRAY && f[0].count == 9 && f[0].size == 8 && f[0].name == "k");
        CHECK(f[1].kind == MF_SEQ && f[1].size == 1 && f[2].kind == MF_STRING && f[2].name == "name");
        CHECK(f[3].kind == MF_PRIM && f[3].size == 2 && f[3].name == "v" && f[4].kind == MF_OTHER && f[5].kind == MF_TIME && f[6].kind == MF_HEADER);
        parser += 3;
    }
    printf("parser: %d cases\n", parser);

    // ---- the host decoder against answers by hand ----------------------------------------------------------------------------------------------
    int decodes = 0;
    const int32_t S0 = 1600000000;
    {
        const std::vector<Ev> a = {{10, 20, S0, 1000, 1}, {345, 259, S0, 2000, 0}, {0, 0, S0, 1000000000u, 1}, {346, 5, S0, 3000, 1}};
        const std::vector<Ev> b = {{1, 2, S0 - 1, 999999999u, 1}, {3, 4, S0 + 1, 5, 255}, {7, 8, -1, 0, 1}};
        for (int chunked = 0; chunked < 2; chunked++) {
            Bytes inner;
            append(inner, schema(1, "dvs_msgs/msg/EventArray", "ros2msg", DVS));
            append(inner, channel(3, 1, "/dvs/events"));
            append(inner, channel(4, 0, "/rosout", "json"));
            append(inner, message(3, dvs_message(a, chunked ? "c" : "camera")));
            append(inner, message(4, Bytes(7, 0x55)));
            append(inner, message(3, dvs_message({})));
            append(inner, message(3, dvs_message(b, "")));
            const Bytes f = chunked ? file_of({chunk(inner), record(0x07, Bytes(10, 0))}) : file_of({inner}, false);
            for (int blockwise = 0; blockwise < 2; blockwise++) {
                const Decoded d = decode(f, "", 1, BagFilter{0, 346, 260, -INFINITY, 0, 0.0, 0, 0}, blockwise != 0);
                CHECK(d.rc == MCAP_OK && d.base == (int64_t) S0 * 1000000000ll && d.c.first_stamp_ns == d.base);
                CHECK(d.c.n_messages == 3 && d.c.n_other_messages == 1 && d.c.n_raw_events == 7 && d.c.n_chunks == (uint64_t) chunked);
                CHECK(d.c.n_schemas == 1 && d.c.n_channels == 2 && d.c.msg_width == 346 && d.c.msg_height == 260 && d.c.n_trailing_bytes == 0);
                CHECK(d.c.n_events == 4 && d.c.n_outside == 1 && d.c.n_negative == 2 && d.c.n_before_start == 0 && d.c.n_after_end == 0);
                CHECK(d.rec.size() == 100);
                if (d.rec.size() == 100) {
                    CHECK(rec_t(d, 0) == (double) 1000 * 1e-9 && rec_x(d, 0) == 10 && rec_y(d, 0) == 20 && rec_p(d, 0) == 1);
                    CHECK(rec_t(d, 1) == (double) 2000 * 1e-9 && rec_x(d, 1) == 345 && rec_y(d, 1) == 259 && rec_p(d, 1) == 0);
                    CHECK(rec_t(d, 2) == 1.0 && rec_p(d, 2) == 1);
                    CHECK(rec_t(d, 3) == (double) 1000000005 * 1e-9 && rec_x(d, 3) == 3 && rec_y(d, 3) == 4 && rec_p(d, 3) == 1);
                }
                decodes++;
            }
            // flips, start and end
            const Decoded d = decode(f, "/dvs/events", 0, BagFilter{(int64_t) S0 * 1000000000ll - 1000000000ll, 346, 260, 0.5, 1, 2.0, 1, 1});
            CHECK(d.rc == MCAP_OK && d.c.n_events == 2 && d.c.n_before_start == 0 && d.c.n_after_end == 5 && d.c.n_outside == 0 && d.c.n_negative == 0);
            CHECK(d.rec.size() == 50);
            if (d.rec.size() == 50) CHECK(rec_x(d, 0) == 335 && rec_y(d, 0) == 239 && rec_t(d, 0) == (double) 1000001000 * 1e-9);
            decodes++;
        }
    }
    {   // mono packets: the word's bits, the base of the first event's whole second, a negative time_base
        const std::vector<Ev> a = {{10, 20, 0, 700, 1}, {65535, 32767, 0, 4294967295u, 0}}, b = {{1, 2, 0, 1000, 1}};
        const uint64_t tb = (uint64_t) S0 * 1000000000ull + 999999900ull;
        const Bytes f = file_of({schema(2, "event_camera_msgs/msg/EventPacket", "ros2msg", PACKET), channel(1, 2, "/ev"), message(1, packet_message(mono_words(a), "mono", tb, 0, "ab")),
                                 message(1, packet_message(mono_words(b), "mono", tb + 5))});
        for (int blockwise = 0; blockwise < 2; blockwise++) {
            const Decoded d = decode(f, "", 1, BagFilter{0, 0, 0, -INFINITY, 0, 0.0, 0, 0}, blockwise != 0);
            CHECK(d.rc == MCAP_OK && d.c.layout.kind == MCAP_MONO && d.c.n_raw_events == 3 && d.c.n_events == 3);
            CHECK(d.base == (int64_t) (S0 + 1) * 1000000000ll);   // 999999900 + 700 ns carries into the next second
            if (d.rec.size() == 75) {
                CHECK(rec_t(d, 0) == (double) 600 * 1e-9 && rec_x(d, 0) == 10 && rec_y(d, 0) == 20 && rec_p(d, 0) == 1);
                CHECK(rec_t(d, 1) == (double) (4294967295ll - 100) * 1e-9 && rec_x(d, 1) == 65535 && rec_y(d, 1) == 32767 && rec_p(d, 1) == 0);
                CHECK(rec_t(d, 2) == (double) 905 * 1e-9 && rec_x(d, 2) == 1 && rec_y(d, 2) == 2 && d.c.n_negative == 0);
            }
            decodes++;
        }
        const Bytes g = file_of({schema(2, "P", "ros2msg", PACKET), channel(1, 2, "/ev"), message(1, packet_message(mono_words(b), "mono", (uint64_t) -1500000000ll))});
        const Decoded d = decode(g);
        CHECK(d.rc == MCAP_OK && d.base == -2000000000ll && d.rec.size() == 25 && rec_t(d, 0) == (double) 500001000 * 1e-9);
        decodes++;
    }
    {   // evt3 packets: one payload across messages, the raw ingest's decoder.  TIME_HIGH 1, TIME_LOW 2, ADDR_Y 5 | ADDR_X 7 on
        auto words = [](std::initializer_list<uint16_t> w) {
            Bytes p;
            for (uint16_t v : w) put(p, v, 2);
            return p;
        };
        const Bytes f = file_of({schema(2, "P", "ros2msg", PACKET), channel(1, 2, "/ev"), message(1, packet_message(words({0x8001, 0x6002, 0x0005}), "evt3", 0)),
                                 message(1, packet_message(Bytes(), "evt3", 0)), message(1, packet_message(words({0x2807, 0xE000}), "evt3", 0))});
        const Decoded d = decode(f);
        CHECK(d.rc == MCAP_OK && d.c.layout.kind == MCAP_EVT3 && d.c.n_payload_bytes == 10 && d.c.n_messages == 3 && d.base == 0);
        CHECK(d.c.n_events == 1 && d.c.n_other_words == 1 && d.c.n_raw_events == 1);
        if (d.rec.size() == 25) CHECK(rec_t(d, 0) == (double) ((1 << 12) | 2) * 1e-6 && rec_x(d, 0) == 7 && rec_y(d, 0) == 5 && rec_p(d, 0) == 1);
        decodes++;
    }
    {   // a file cut short: records wholly present count
        Bytes inner;
        append(inner, schema(1, "E", "ros2msg", DVS));
        append(inner, channel(3, 1, "/e"));
        append(inner, message(3, dvs_message({{1, 1, S0, 1, 1}})));
        const size_t one = inner.size();
        append(inner, message(3, dvs_message({{2, 2, S0, 2, 1}, {3, 3, S0, 3, 1}})));
        Bytes f = file_of({chunk(inner)}, false);
        const size_t whole = f.size();
        f.resize(whole - 5);
        const Decoded d = decode(f);
        CHECK(d.rc == MCAP_OK && d.c.n_messages == 1 && d.c.n_events == 1 && d.c.n_trailing_bytes == (whole - 5) - (whole - (inner.size() - one)));
        decodes++;
    }
    printf("decode: %d cases\n", decodes);

    // ---- refusals ------------------------------------------------------------------------------------------------------------------------
    {
        const Bytes sc = schema(1, "dvs_msgs/msg/EventArray", "ros2msg", DVS), ch = channel(3, 1, "/dvs/events");
        const Bytes msg = message(3, dvs_message({{1, 2, S0, 3, 1}}));
        const Bytes psc = schema(2, "event_camera_msgs/msg/EventPacket", "ros2msg", PACKET), pch = channel(5, 2, "/pk");
        refused(Bytes(), {"not an MCAP file"});
        {
            const std::string bag = "#ROSBAG V2.0\n", sq = std::string("SQLite format 3\0", 16);
            refused(Bytes(bag.begin(), bag.end()), {"ROS 1 bag", "bag ingest"});
            refused(Bytes(sq.begin(), sq.end()), {"SQLite", ".db3"});
        }
        Bytes both = sc;
        append(both, ch);
        append(both, msg);
        refused(file_of({chunk(both, "lz4")}), {"lz4", "uncompressed", "record 1 at byte"});
        refused(file_of({chunk(both, "zstd")}), {"zstd", "uncompressed"});
        refused(file_of({chunk(both, "", 1)}), {"records length"});
        refused(file_of({chunk(record(0x01, Bytes(8, 0)))}), {"0x01 inside a chunk"});
        refused(file_of({sc, ch, record(0x10, Bytes())}), {"unknown opcode 0x10", "record 3"});
        refused(file_of({sc, ch, record(0x00, Bytes())}), {"unknown opcode 0x00"});
        refused(file_of({sc, ch, msg, schema(1, "dvs_msgs/msg/EventArray", "ros2msg", DVS + "#")}), {"schema 1", "defined again"});
        refused(file_of({sc, ch, msg, channel(3, 1, "/other")}), {"channel 3", "defined again"});
        refused(file_of({sc, msg}), {"channel 3", "not defined in front"});
        refused(file_of({ch}), {"schema 1", "not defined in front"});
        refused(file_of({sc, channel(3, 1, "/a"), channel(4, 1, "/b")}), {"more than one topic", "/a", "/b"});
        refused(file_of({sc, channel(3, 1, "/a")}), {"no channel", "/nothing", "/a (dvs_msgs/msg/EventArray)"}, "/nothing");
        refused(file_of({schema(9, "sensor_msgs/msg/Image", "ros2msg", "uint8[] data\n"), channel(3, 9, "/img"), channel(4, 1 - 1, "/log", "json")}),
                {"no channel", "/img (sensor_msgs/msg/Image)", "/log"});
        refused(file_of({schema(1, "dvs_msgs/msg/EventArray", "ros2idl", "module dvs_msgs { struct EventArray { sequence<Event> events; }; };"), ch}), {"ros2idl"});
        refused(file_of({schema(1, "E", "ros2msg", "Event[] events\n===\nMSG: x/Event\nuint16 x\nuint16 y\nfloat32 ts\nbool polarity\n"), ch}),
                {"float32 ts", "uint16 x", "not x, y"});
        refused(file_of({schema(1, "E", "ros2msg", "Event[] events\n"), ch}), {"MSG: Event", "not in the schema"});
        refused(file_of({schema(1, "E", "ros2msg", "geometry_msgs/Pose pose\nuint8[] events\n"), ch}), {"pose", "geometry_msgs/Pose"});
        refused(file_of({schema(1, "E", "ros2msg", "uint16[] events\n"), ch}), {"uint16[]"});
        refused(file_of({schema(1, "E", "ros2msg", "uint8[] events\nuint32 width\n"), ch}), {"not an EventPacket"});
        for (int enc = 0; enc < 4; enc++) {
            Bytes data = dvs_message({{1, 2, S0, 3, 1}});
            static const uint8_t id[4] = {0, 3, 7, 0x40};
            static const char *name[4] = {"big-endian CDR", "PL_CDR", "XCDR2", "unknown"};
            data[1] = id[enc];
            refused(file_of({sc, ch, message(3, data)}), {name[enc], "record 3"});
        }
        {
            Bytes data = dvs_message({{1, 2, S0, 3, 1}});
            data.insert(data.end(), 4, 0);   // four bytes too many: a foreign layout
            refused(file_of({sc, ch, message(3, data)}), {"4 bytes in front of the end", "not the layout"});
            data.resize(data.size() - 6);
            refused(file_of({sc, ch, message(3, data)}), {"runs past its data"});
            refused(file_of({sc, ch, message(3, Bytes(3, 0))}), {"fewer than 4 bytes"});
        }
        for (const char *enc : {"libcaer", "libcaer_cmp", "evt2", ""})
            refused(file_of({psc, pch, message(5, packet_message(Bytes(8, 0), enc, 0))}), {"encoding", enc, "mono and evt3"});
        refused(file_of({psc, pch, message(5, packet_message(Bytes(8, 0), "mono", 0, 1))}), {"is_bigendian"});
        refused(file_of({psc, pch, message(5, packet_message(Bytes(12, 0), "mono", 0))}), {"12 bytes", "multiple of 8"});
        refused(file_of({psc, pch, message(5, packet_message(Bytes(7, 0), "evt3", 0))}), {"7 bytes", "odd"});
        refused(file_of({psc, pch, message(5, packet_message(Bytes(8, 0), "mono", 0)), message(5, packet_message(Bytes(8, 0), "evt3", 0))}), {"mixed kinds"});
        refused(file_of({sc, psc, channel(3, 1, "/t"), channel(5, 2, "/t"), msg, message(5, packet_message(Bytes(8, 0), "mono", 0))}), {"mixed kinds"});
        {
            Bytes inner = sc;
            append(inner, ch);
            Bytes m = msg;
            m[1] = (uint8_t) (m[1] + 9);   // the record claims nine bytes more than the chunk holds
            append(inner, m);
            refused(file_of({chunk(inner)}), {"runs past the end of its chunk"});
        }
        refused(file_of({sc, ch, record(MCAP_OP_MESSAGE, Bytes(10, 0))}), {"fewer than 22 bytes"});
    }
    printf("refusals: %d cases\n", refusals);
    printf("wrong: %d\n", wrong);
    return wrong ? 1 : 0;
}
