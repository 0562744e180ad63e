// ROS 2 MCAP recordings of event messages into events — one restatement of include/ecal_mcap.h for the kernels (ecal_mcap.hip), the
// host decoder (EventStream::mcap2bin, host/event.hpp) and the CPU test (tests/cpp/check_mcap_events.cpp).  Compiles with plain g++.
//
// Three things stand between the file and an event: the container (a chain of records, some inside chunks), the message layout (CDR,
// laid out by the message definition the file carries in its Schema records) and the kind of `events` (a sequence of structs, or a
// byte array of "mono" words or of EVT3 words).  mcap_walk goes through the chain ONCE, on the host, parses each schema it needs,
// walks the CDR fields of every chosen message and leaves a table of where the events lie; behind it
//   STRUCT, MONO:  every event is "slot s of the table" and decodes on its own (the bag ingest's scheme, with its filter);
//   EVT3:          the messages' byte arrays are gathered into one payload, which the raw ingest decodes.
// Nothing here is floating point but the filters' one conversion and one multiplication (bag_classify, raw_classify).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "bag_events.hpp"
#include "raw_events.hpp"
#include "ingest_blocks.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_MCAP_HD __host__ __device__ __forceinline__
#else
#define ECAL_MCAP_HD inline
#endif

namespace ecal_mcap {

using ecal_bag::BagEvent;
using ecal_bag::BagFilter;
using ecal_bag::bag_printable;

enum : int { MCAP_OK = 0, MCAP_INVALID = -1, MCAP_RANGE = -6 };                      // ECAL_OK / ECAL_ERR_INVALID / ECAL_ERR_RANGE
enum : uint32_t { MCAP_NONE = 0, MCAP_STRUCT = 1, MCAP_MONO = 2, MCAP_EVT3 = 3 };   // ECAL_MCAP_*

// a decode block of the kernels: 256 threads x 4 consecutive event slots (ecal_mcap_block_events)
constexpr uint32_t MCAP_BLOCK_THREADS = 256;
constexpr uint32_t MCAP_THREAD_EVENTS = 4;
constexpr uint32_t MCAP_BLOCK_EVENTS = MCAP_BLOCK_THREADS * MCAP_THREAD_EVENTS;
// a gather block: 256 threads x one 16-byte store
constexpr uint32_t MCAP_GATHER_BYTES = 256 * 16;
constexpr int64_t MCAP_NS_PER_S = 1000000000ll;

enum : int { MCAP_OP_HEADER = 0x01, MCAP_OP_FOOTER = 0x02, MCAP_OP_SCHEMA = 0x03, MCAP_OP_CHANNEL = 0x04, MCAP_OP_MESSAGE = 0x05, MCAP_OP_CHUNK = 0x06,
             MCAP_OP_SUMMARY_OFFSET = 0x0E, MCAP_OP_DATA_END = 0x0F };

struct McapLayout {   // ecal_mcap_layout
    uint32_t kind, lead, stride, span[2];
    uint8_t x[2], y[2], sec[2], nsec[2], pol[2];
    uint8_t x_bytes, y_bytes;
};
static_assert(sizeof(McapLayout) == 32, "ecal_mcap_layout");

struct McapMessage {   // ecal_mcap_message
    uint64_t offset;
    uint32_t n, reserved;
    int64_t time_base_ns;
};
static_assert(sizeof(McapMessage) == 24, "ecal_mcap_message");

// ---- where an event lies, and its fields ------------------------------------------------------------------------------------------------
ECAL_MCAP_HD uint64_t mcap_event_offset(const McapLayout &L, uint64_t k) { return k ? (uint64_t) L.lead + (k - 1u) * (uint64_t) L.stride : 0u; }

// the bytes a message's n events (EVT3: n payload bytes) take from its offset on
ECAL_MCAP_HD uint64_t mcap_message_bytes(const McapLayout &L, uint64_t n) {
    if (L.kind == MCAP_EVT3) return n;
    if (n == 0) return 0;
    return n == 1 ? (uint64_t) L.span[0] : mcap_event_offset(L, n - 1u) + L.span[1];
}

ECAL_MCAP_HD BagEvent mcap_struct_event(uint32_t x, uint32_t y, uint32_t sec, uint32_t nsec, uint32_t pol_byte) {
    BagEvent e;
    e.t_ns = (int64_t) (int32_t) sec * MCAP_NS_PER_S + (int64_t) nsec;   // sec is SIGNED (builtin_interfaces/Time)
    e.x = x;
    e.y = y;
    e.pol = (uint8_t) ((pol_byte & 0xFFu) != 0u ? 1u : 0u);
    return e;
}

// lo: bits 31..0 of the word (dt in nanoseconds), hi: bits 63..32 (x 15..0, y 30..16, polarity 31)
ECAL_MCAP_HD BagEvent mcap_mono_event(uint32_t lo, uint32_t hi, int64_t time_base_ns) {
    BagEvent e;
    e.t_ns = (int64_t) ((uint64_t) time_base_ns + (uint64_t) lo);
    e.x = hi & 0xFFFFu;
    e.y = (hi >> 16) & 0x7FFFu;
    e.pol = (uint8_t) (hi >> 31);
    return e;
}

// the little-endian value of nb (1, 2 or 4) bytes at byte `pos` of the file, from the one or two aligned words that hold it; bytes at
// or behind n_bytes read as zeros and nothing behind n_bytes is loaded (pos + 8 must not wrap: the callers test the event's extent)
ECAL_MCAP_HD uint32_t mcap_load_field(const uint8_t *__restrict__ file, uint64_t pos, uint32_t nb, uint64_t n_bytes) {
    const uint64_t a = pos & ~3ull;
    const uint32_t sh = 8u * (uint32_t) (pos & 3u);
    uint64_t win = ecal::load32_clipped(file, a, n_bytes);
    if (sh + 8u * nb > 32u) win |= (uint64_t) ecal::load32_clipped(file, a + 4u, n_bytes) << 32;
    const uint32_t v = (uint32_t) (win >> sh);
    return nb >= 4u ? v : v & ((1u << (8u * nb)) - 1u);
}

// event k of the message at m_off, whatever its byte offset.  An event that does not lie within the file (a bad table: an error on the
// host) reads as zeros.  KIND: MCAP_STRUCT or MCAP_MONO
template <uint32_t KIND>
ECAL_MCAP_HD BagEvent mcap_fetch_event(const uint8_t *__restrict__ file, uint64_t n_bytes, const McapLayout &L, uint64_t m_off, uint64_t k, int64_t time_base_ns) {
    const uint64_t off = m_off + mcap_event_offset(L, k);
    const uint32_t span = k ? L.span[1] : L.span[0];
    const bool there = off >= m_off && off + span > off && off + span <= n_bytes;
    const uint64_t al = off & ~3ull;
    const uint32_t r = (uint32_t) (off & 3u);
    if (KIND == MCAP_MONO) {
        if (!there) return mcap_mono_event(0u, 0u, 0);
        // the word's 8 bytes from two or three aligned words
        const uint32_t w0 = ecal::load32_clipped(file, al, n_bytes), w1 = ecal::load32_clipped(file, al + 4u, n_bytes);
        const uint32_t w2 = r ? ecal::load32_clipped(file, al + 8u, n_bytes) : 0u;
        return mcap_mono_event((uint32_t) ((((uint64_t) w1 << 32) | w0) >> (8u * r)), (uint32_t) ((((uint64_t) w2 << 32) | w1) >> (8u * r)), time_base_ns);
    }
    if (!there) return mcap_struct_event(0u, 0u, 0u, 0u, 0u);
    const uint32_t ox = k ? L.x[1] : L.x[0], oy = k ? L.y[1] : L.y[0], os = k ? L.sec[1] : L.sec[0], on = k ? L.nsec[1] : L.nsec[0],
                   op = k ? L.pol[1] : L.pol[0];
    if (r + span <= 24u) {
        // the common structs (dvs_msgs/Event: 15 bytes): the aligned words that cover the event loaded once — those in front of its
        // end, so only the last can reach n_bytes — and every field shifted out of the pair of words that holds it
        uint32_t w[6];
        ECAL_INGEST_UNROLL
        for (uint32_t i = 0; i < 6; i++) w[i] = 4u * i < r + span ? ecal::load32_clipped(file, al + 4u * i, n_bytes) : 0u;
        auto word = [&](uint32_t i) { return i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : i == 3 ? w[3] : i == 4 ? w[4] : i == 5 ? w[5] : 0u; };
        auto field = [&](uint32_t o, uint32_t nb) {
            const uint32_t b = r + o, i = b >> 2;
            const uint32_t v = (uint32_t) ((((uint64_t) word(i + 1u) << 32) | word(i)) >> (8u * (b & 3u)));
            return nb >= 4u ? v : v & ((1u << (8u * nb)) - 1u);
        };
        return mcap_struct_event(field(ox, L.x_bytes), field(oy, L.y_bytes), field(os, 4u), field(on, 4u), field(op, 1u));
    }
    return mcap_struct_event(mcap_load_field(file, off + ox, L.x_bytes, n_bytes), mcap_load_field(file, off + oy, L.y_bytes, n_bytes),
                             mcap_load_field(file, off + os, 4u, n_bytes), mcap_load_field(file, off + on, 4u, n_bytes),
                             mcap_load_field(file, off + op, 1u, n_bytes));
}

inline McapLayout mcap_mono_layout() {
    McapLayout L;
    memset(&L, 0, sizeof(L));
    L.kind = MCAP_MONO;
    L.lead = L.stride = L.span[0] = L.span[1] = 8;
    L.x_bytes = L.y_bytes = 2;
    return L;
}

// what a layout handed to the device form must satisfy; *why says what it does not
inline bool mcap_layout_valid(const McapLayout &L, const char **why) {
    *why = "a kind that is not ECAL_MCAP_STRUCT, _MONO or _EVT3";
    if (L.kind == MCAP_EVT3) return true;
    if (L.kind == MCAP_MONO) {
        *why = "a MONO layout other than lead = stride = span = 8";
        return L.lead == 8 && L.stride == 8 && L.span[0] == 8 && L.span[1] == 8;
    }
    if (L.kind != MCAP_STRUCT) return false;
    *why = "x_bytes / y_bytes that are not 1, 2 or 4";
    if ((L.x_bytes != 1 && L.x_bytes != 2 && L.x_bytes != 4) || (L.y_bytes != 1 && L.y_bytes != 2 && L.y_bytes != 4)) return false;
    *why = "spans, lead or stride out of range (span 10 .. 64, lead >= span[0], stride >= span[1], both <= 64)";
    if (L.span[0] < 10 || L.span[0] > 64 || L.span[1] < 10 || L.span[1] > 64 || L.lead < L.span[0] || L.lead > 64 || L.stride < L.span[1] || L.stride > 64) return false;
    *why = "a field that does not lie within its event's span";
    for (int w = 0; w < 2; w++)
        if (L.x[w] + (uint32_t) L.x_bytes > L.span[w] || L.y[w] + (uint32_t) L.y_bytes > L.span[w] || L.sec[w] + 4u > L.span[w] || L.nsec[w] + 4u > L.span[w] ||
            L.pol[w] + 1u > L.span[w])
            return false;
    return true;
}

// ---- the message definition (ros2msg text) ------------------------------------------------------------------------------------------------
enum : int { MF_PRIM = 0, MF_STRING, MF_TIME, MF_HEADER, MF_ARRAY, MF_SEQ, MF_EVENTS_STRUCT, MF_EVENTS_BYTES, MF_OTHER };
enum : int { MP_OTHER = 0, MP_UNSIGNED = 1, MP_SIGNED = 2, MP_FLOAT = 3 };   // bool, byte and char: integers of one byte for this purpose

struct McapField {
    std::string name, type;   // type: as written (with its brackets)
    std::string base;         // without brackets and bounds
    int kind = MF_OTHER;
    uint32_t size = 0;        // of the primitive (MF_PRIM, MF_ARRAY, MF_SEQ)
    int prim = MP_OTHER;
    uint64_t count = 0;       // MF_ARRAY
};

struct McapSection {
    std::string name;   // "": the top level; else the name behind "MSG:"
    std::vector<McapField> fields;
};

inline bool mcap_primitive(const std::string &t, uint32_t *size, int *prim) {
    static const struct { const char *name; uint32_t size; int prim; } table[] = {
        {"bool", 1, MP_UNSIGNED}, {"byte", 1, MP_UNSIGNED}, {"char", 1, MP_UNSIGNED}, {"int8", 1, MP_SIGNED}, {"uint8", 1, MP_UNSIGNED},
        {"int16", 2, MP_SIGNED}, {"uint16", 2, MP_UNSIGNED}, {"int32", 4, MP_SIGNED}, {"uint32", 4, MP_UNSIGNED}, {"float32", 4, MP_FLOAT},
        {"int64", 8, MP_SIGNED}, {"uint64", 8, MP_UNSIGNED}, {"float64", 8, MP_FLOAT}};
    for (const auto &e : table)
        if (t == e.name) {
            *size = e.size;
            *prim = e.prim;
            return true;
        }
    return false;
}

inline std::string mcap_last_component(const std::string &t) {
    const size_t s = t.rfind('/');
    return s == std::string::npos ? t : t.substr(s + 1);
}

// the text cut into the top-level definition and the dependencies', every field classed but `events` of a message type (MF_OTHER until
// mcap_schema_layout looks its section up)
inline std::vector<McapSection> mcap_parse_definition(const std::string &text) {
    std::vector<McapSection> out(1);
    size_t at = 0;
    while (at <= text.size()) {
        size_t nl = text.find('\n', at);
        if (nl == std::string::npos) nl = text.size();
        std::string line = text.substr(at, nl - at);
        at = nl + 1;
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.erase(hash);
        std::vector<std::string> tok;
        for (size_t i = 0; i < line.size();) {
            while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) i++;
            size_t j = i;
            while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') j++;
            if (j > i) tok.push_back(line.substr(i, j - i));
            i = j;
        }
        if (tok.empty()) continue;
        if (tok[0].size() >= 3 && tok[0].find_first_not_of('=') == std::string::npos) {   // a separator: the next definition
            out.emplace_back();
            out.back().name = "?";
            continue;
        }
        if (tok[0] == "MSG:") {
            if (tok.size() > 1) out.back().name = tok[1];
            continue;
        }
        if (tok.size() < 2) continue;
        if (tok[1].find('=') != std::string::npos || (tok.size() > 2 && tok[2][0] == '=')) continue;   // a constant
        McapField f;
        f.type = tok[0];
        f.name = tok[1];
        std::string base = f.type, suffix;
        bool bracket = false;
        const size_t br = base.find('[');
        if (br != std::string::npos) {
            bracket = true;
            suffix = base.substr(br + 1, base.size() > br + 1 && base.back() == ']' ? base.size() - br - 2 : std::string::npos);
            base.erase(br);
        }
        const size_t le = base.find("<=");
        if (le != std::string::npos) base.erase(le);   // string<=N
        f.base = base;
        const std::string last = mcap_last_component(base);
        const bool is_prim = mcap_primitive(base, &f.size, &f.prim);
        if (!bracket) {
            if (is_prim) f.kind = MF_PRIM;
            else if (base == "string") f.kind = MF_STRING;
            else if (last == "Time" && base != "string") f.kind = MF_TIME;
            else if (last == "Header") f.kind = MF_HEADER;
        } else if (is_prim) {
            if (suffix.empty() || suffix.compare(0, 2, "<=") == 0) {
                f.kind = MF_SEQ;
            } else {
                f.kind = MF_ARRAY;
                f.count = strtoull(suffix.c_str(), nullptr, 10);
            }
        }
        out.back().fields.push_back(f);
    }
    return out;
}

struct McapSchemaLayout {
    std::vector<McapField> fields;   // the top level, in order
    bool packet = false;             // `events` is uint8[]: MONO or EVT3, by the message's encoding string
    McapLayout layout;               // STRUCT: complete; packet: zeros
};

inline uint64_t mcap_align(uint64_t pos, uint64_t a) { return (pos + a - 1u) / a * a; }

// 0: the text declares no top-level field `events` (not a schema of events); 1: S is set; -1: it does, in a shape that is not read
// (*err says which)
inline int mcap_schema_layout(const std::string &text, McapSchemaLayout &S, std::string *err) {
    const std::vector<McapSection> sec = mcap_parse_definition(text);
    S = McapSchemaLayout();
    memset(&S.layout, 0, sizeof(S.layout));
    S.fields = sec[0].fields;
    McapField *ev = nullptr;
    for (McapField &f : S.fields)
        if (f.name == "events" && !ev) ev = &f;
    if (!ev) return 0;
    const bool ev_sequence = ev->type.size() > ev->base.size() && ev->type[ev->base.size()] == '[' &&
                             (ev->type.compare(ev->base.size(), 2, "[]") == 0 || ev->type.compare(ev->base.size(), 3, "[<=") == 0);
    if (!ev_sequence) {
        *err = "field events of type " + bag_printable(ev->type) + ": not a sequence";
        return -1;
    }
    if (ev->kind == MF_SEQ) {
        if (ev->base != "uint8" && ev->base != "byte" && ev->base != "char") {
            *err = "field events of type " + bag_printable(ev->type) + ": a sequence of another primitive than uint8";
            return -1;
        }
        ev->kind = MF_EVENTS_BYTES;
        S.packet = true;
    } else {
        const McapSection *es = nullptr;
        for (size_t i = 1; i < sec.size() && !es; i++)
            if (mcap_last_component(sec[i].name) == mcap_last_component(ev->base)) es = &sec[i];
        if (!es) {
            *err = "field events of type " + bag_printable(ev->type) + ", whose definition (MSG: " + bag_printable(ev->base) + ") is not in the schema";
            return -1;
        }
        // the element's primitives in order: role 0 x, 1 y, 2 sec, 3 nsec, 4 polarity
        struct Prim { int role; uint32_t size; };
        std::vector<Prim> prims;
        int seen[5] = {0, 0, 0, 0, 0};
        std::string types;
        bool ok = true;
        for (const McapField &f : es->fields) {
            if (!types.empty()) types += ", ";
            types += bag_printable(f.type) + " " + bag_printable(f.name);
            const bool coord = f.kind == MF_PRIM && f.prim == MP_UNSIGNED && (f.size == 1 || f.size == 2 || f.size == 4);
            if ((f.name == "x" || f.name == "y") && coord) {
                const int r = f.name == "x" ? 0 : 1;
                (r ? S.layout.y_bytes : S.layout.x_bytes) = (uint8_t) f.size;
                seen[r]++;
                prims.push_back({r, f.size});
            } else if ((f.name == "polarity" || f.name == "p") && f.kind == MF_PRIM && f.size == 1) {
                seen[4]++;
                prims.push_back({4, 1});
            } else if ((f.name == "ts" || f.name == "t" || f.name == "stamp") && f.kind == MF_TIME) {
                seen[2]++;
                seen[3]++;
                prims.push_back({2, 4});
                prims.push_back({3, 4});
            } else {
                ok = false;
            }
        }
        for (int r = 0; r < 5; r++) ok = ok && seen[r] == 1;
        if (!ok) {
            *err = "events of " + bag_printable(ev->base) + " { " + types + " }: not x, y (unsigned, 1, 2 or 4 bytes), polarity or p (1 byte) and ts, t or stamp (Time)";
            return -1;
        }
        // eight events laid out from a 4-byte aligned start (behind the sequence's count): CDR pads no struct tail
        constexpr int NE = 8;
        uint64_t pos = 0, start[NE], span[NE];
        uint32_t off[NE][5];
        for (int k = 0; k < NE; k++) {
            bool first = true;
            for (const Prim &p : prims) {
                pos = mcap_align(pos, p.size);
                if (first) start[k] = pos;
                first = false;
                off[k][p.role] = (uint32_t) (pos - start[k]);
                pos += p.size;
            }
            span[k] = pos - start[k];
        }
        bool constant = start[0] == 0;
        for (int k = 2; k < NE; k++) {
            constant = constant && start[k] - start[k - 1] == start[2] - start[1] && span[k] == span[1];
            for (int r = 0; r < 5; r++) constant = constant && off[k][r] == off[1][r];
        }
        if (!constant) {
            *err = "events of " + bag_printable(ev->base) + " { " + types + " }: the stride is not constant from event 1 on";
            return -1;
        }
        ev->kind = MF_EVENTS_STRUCT;
        McapLayout &L = S.layout;
        L.kind = MCAP_STRUCT;
        L.lead = (uint32_t) (start[1] - start[0]);
        L.stride = (uint32_t) (start[2] - start[1]);
        for (int w = 0; w < 2; w++) {
            L.span[w] = (uint32_t) span[w];
            L.x[w] = (uint8_t) off[w][0];
            L.y[w] = (uint8_t) off[w][1];
            L.sec[w] = (uint8_t) off[w][2];
            L.nsec[w] = (uint8_t) off[w][3];
            L.pol[w] = (uint8_t) off[w][4];
        }
    }
    // every other top-level field must be one the walk can cross
    bool has[5] = {false, false, false, false, false};   // time_base, width, height, encoding, is_bigendian
    for (const McapField &f : S.fields) {
        if (&f == ev) continue;
        if (f.kind == MF_OTHER) {
            *err = "field " + bag_printable(f.name) + " of type " + bag_printable(f.type) + " beside events: only primitives, strings, Header, Time and arrays and sequences of primitives are crossed";
            return -1;
        }
        if (f.kind == MF_ARRAY && (f.count == 0 || f.count > 0xFFFFFFFFull)) {
            *err = "field " + bag_printable(f.name) + " of type " + bag_printable(f.type) + ": an array bound that is not read";
            return -1;
        }
        const bool integer = f.kind == MF_PRIM && f.prim != MP_FLOAT;
        if (f.name == "time_base" && integer) has[0] = true;
        if (f.name == "width" && integer) has[1] = true;
        if (f.name == "height" && integer) has[2] = true;
        if (f.name == "encoding" && f.kind == MF_STRING) has[3] = true;
        if (f.name == "is_bigendian" && f.kind == MF_PRIM && f.size == 1) has[4] = true;
    }
    if (S.packet && !(has[0] && has[1] && has[2] && has[3] && has[4])) {
        *err = "events is uint8[] but the message lacks one of time_base, width, height (integers), encoding (string), is_bigendian (1 byte): not an EventPacket";
        return -1;
    }
    return 1;
}

// ---- one message's CDR fields -------------------------------------------------------------------------------------------------------------
struct McapMessageWalk {
    uint64_t events_offset = 0;   // from byte 0 of the file
    uint64_t events_count = 0;    // the sequence's count
    bool has_width = false, has_height = false;
    uint64_t time_base = 0, width = 0, height = 0, is_bigendian = 0;
    std::string encoding;
};

// data: the file offset of the message's data, dl its length.  false: *why
template <class Read>
inline bool mcap_walk_message(Read &&read, uint64_t data, uint64_t dl, const McapSchemaLayout &S, McapMessageWalk &W, std::string *why) {
    static const char past[] = "the walk over the message's fields runs past its data: not the layout of its schema", unreadable[] = "cannot be read";
    uint8_t w[8];
    if (dl < 4) {
        *why = "a message of fewer than 4 bytes: no CDR encapsulation header";
        return false;
    }
    if (!read(data, w, 4)) {
        *why = unreadable;
        return false;
    }
    if (w[0] != 0 || w[1] != 1) {
        char id[16];
        snprintf(id, sizeof(id), "%02x %02x", w[0], w[1]);
        const unsigned v = w[0] ? 0xFFu : w[1];
        *why = std::string("encapsulation ") + id + ": " +
               (v == 0 ? "big-endian CDR is not read" : v == 2 || v == 3 ? "PL_CDR is not read" : v >= 6 && v <= 11 ? "XCDR2 is not read" : "unknown, not read") +
               " (little-endian CDR, 00 01, is)";
        return false;
    }
    const uint64_t org = data + 4, L = dl - 4;
    uint64_t pos = 0;
    bool ok = true;
    auto need = [&](uint64_t n) {
        if (pos > L || n > L - pos) ok = false;
        return ok;
    };
    auto get = [&](uint64_t n_) {   // little-endian integer of n_ <= 8 bytes at pos
        uint64_t v = 0;
        memset(w, 0, 8);
        if (!read(org + pos, w, (size_t) n_)) {
            ok = false;
            *why = unreadable;
            return v;
        }
        for (int b = 7; b >= 0; b--) v = (v << 8) | w[b];
        return v;
    };
    *why = past;
    auto cross_time = [&]() {
        pos = mcap_align(pos, 4);
        if (need(8)) pos += 8;
    };
    auto cross_string = [&](std::string *keep) {
        pos = mcap_align(pos, 4);
        if (!need(4)) return;
        const uint64_t len = get(4);
        pos += 4;
        if (!ok || !need(len)) return;
        if (keep) {
            uint8_t buf[32];
            const size_t take = (size_t) (len < 32 ? len : 32);
            if (take && !read(org + pos, buf, take)) {
                ok = false;
                *why = unreadable;
                return;
            }
            keep->assign((const char *) buf, take);
            const size_t nul = keep->find('\0');
            if (nul != std::string::npos) keep->erase(nul);
        }
        pos += len;
    };
    for (const McapField &f : S.fields) {
        if (!ok) break;
        switch (f.kind) {
            case MF_PRIM: {
                pos = mcap_align(pos, f.size);
                if (!need(f.size)) break;
                if (f.prim != MP_FLOAT) {
                    if (f.name == "time_base") W.time_base = get(f.size);
                    else if (f.name == "width") { W.width = get(f.size); W.has_width = true; }
                    else if (f.name == "height") { W.height = get(f.size); W.has_height = true; }
                    else if (f.name == "is_bigendian" && f.size == 1) W.is_bigendian = get(1);
                }
                pos += f.size;
                break;
            }
            case MF_STRING: cross_string(f.name == "encoding" ? &W.encoding : nullptr); break;
            case MF_TIME: cross_time(); break;
            case MF_HEADER:
                cross_time();
                if (ok) cross_string(nullptr);
                break;
            case MF_ARRAY:
                pos = mcap_align(pos, f.size);
                if (need(f.count * f.size)) pos += f.count * f.size;
                break;
            case MF_SEQ:
            case MF_EVENTS_BYTES:
            case MF_EVENTS_STRUCT: {
                pos = mcap_align(pos, 4);
                if (!need(4)) break;
                const uint64_t n = get(4);
                pos += 4;
                if (!ok) break;
                uint64_t bytes;
                if (f.kind == MF_EVENTS_STRUCT) {
                    bytes = mcap_message_bytes(S.layout, n);
                } else {
                    if (n) pos = mcap_align(pos, f.size);
                    bytes = n * f.size;
                }
                if (f.kind != MF_SEQ) {
                    W.events_offset = org + pos;
                    W.events_count = n;
                }
                if (need(bytes)) pos += bytes;
                break;
            }
            default: ok = false;
        }
    }
    if (!ok) return false;
    if (L - pos > 3) {
        *why = "the walk over the message's fields ends " + std::to_string(L - pos) + " bytes in front of the end of its data: not the layout of its schema";
        return false;
    }
    return true;
}

// ---- the chain of records -------------------------------------------------------------------------------------------------------------------
// the counters of one decode (ecal_mcap_info's)
struct McapCounts {
    uint64_t n_raw_events, n_events, n_outside, n_negative, n_before_start, n_after_end, n_messages, n_other_messages, n_chunks, n_schemas,
        n_channels, n_trailing_bytes;
    int64_t first_stamp_ns;
    uint32_t msg_width, msg_height;
    uint64_t n_payload_bytes, n_no_state, n_other_words, n_time_wraps;
    McapLayout layout;
};

struct McapSchema {
    uint32_t id;
    std::vector<uint8_t> content;
    std::string name, encoding, text;
};

struct McapChannel {
    uint32_t id, schema_id;
    std::vector<uint8_t> content;
    std::string topic, message_encoding, schema_name;
    bool accepted, chosen;
    McapSchemaLayout S;
};

inline uint64_t mcap_le(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int b = n - 1; b >= 0; b--) v = (v << 8) | p[b];
    return v;
}

inline int64_t mcap_floor_second(int64_t t_ns) {
    int64_t q = t_ns / MCAP_NS_PER_S;
    if (t_ns % MCAP_NS_PER_S < 0) q--;
    return q * MCAP_NS_PER_S;
}

// the 8 magic bytes.  MCAP_INVALID with *err: a ROS 1 bag (named), an SQLite file (named), anything else
inline int mcap_check_magic(const uint8_t *head, size_t n, std::string *err) {
    static const char mcap[] = "\x89MCAP0\r\n", bag[] = "#ROSBAG V", sqlite[] = "SQLite format 3";
    if (n >= 8 && memcmp(head, mcap, 8) == 0) return MCAP_OK;
    std::string why;
    if (n >= 9 && memcmp(head, bag, 9) == 0) why = "a ROS 1 bag: it goes through the bag ingest, not the mcap ingest";
    else if (n >= 16 && memcmp(head, sqlite, 16) == 0) why = "an SQLite file: a .db3 ROS 2 bag is not read (`ros2 bag convert` rewrites it as MCAP)";
    else why = "no MCAP magic at the start: not an MCAP file";
    if (err) *err = why;
    return MCAP_INVALID;
}

// Walks the file: read(pos, dst, n) copies bytes [pos, pos + n) of it (always within n_bytes; false: they cannot be read — the walk ends
// with MCAP_INVALID).  Record headers, schema and channel records and the fields around a chosen message's events are read, so a file
// is indexed without its events.  Every chosen message goes to on_message(const McapMessage &), also one of no events.  c: everything
// but the filter's counters is set.  MCAP_INVALID: a rule of the contract is broken; *err names the record's number (0-based, over all
// records, inner and outer, in file order) and its byte offset.
template <class Read, class OnMessage>
inline int mcap_walk(Read &&read, uint64_t n_bytes, const std::string &topic_choice, McapCounts &c, OnMessage &&on_message, std::string *err) {
    memset(&c, 0, sizeof(c));
    std::string scratch_err;
    if (!err) err = &scratch_err;
    {
        uint8_t head[16];
        const size_t hn = (size_t) (n_bytes < 16 ? n_bytes : 16);
        if (hn && !read(0, head, hn)) {
            *err = "the file cannot be read";
            return MCAP_INVALID;
        }
        if (mcap_check_magic(head, hn, err)) return MCAP_INVALID;
    }
    std::vector<McapSchema> schemas;
    std::vector<McapChannel> channels;
    std::vector<uint8_t> buf;
    std::string event_topic;
    bool have_event_topic = false, have_first_stamp = false, have_first_message = false, truncated = false, ended = false;
    uint64_t number = 0;

    auto list_channels = [&](bool accepted_only) {
        std::string s;
        for (const McapChannel &k : channels) {
            if (accepted_only && !k.accepted) continue;
            bool dup = false;
            for (const McapChannel &j : channels) {
                if (&j == &k) break;
                if (j.topic == k.topic && j.schema_name == k.schema_name && (!accepted_only || j.accepted)) dup = true;
            }
            if (dup) continue;
            if (!s.empty()) s += ", ";
            s += bag_printable(k.topic);
            if (!accepted_only) s += " (" + bag_printable(k.schema_name) + ")";
        }
        return s.empty() ? std::string("none") : s;
    };

    auto chain = [&](auto &self, uint64_t pos, const uint64_t end, const bool inner) -> int {
        const uint64_t lim = end < n_bytes ? end : n_bytes;   // the bytes that are there
        while (pos < end && !truncated && !ended) {
            const uint64_t rec = pos;
            auto fail = [&](const std::string &why) {
                *err = "record " + std::to_string(number) + " at byte " + std::to_string(rec) + ": " + why;
                return MCAP_INVALID;
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
            uint8_t w[48];
            if ((k = need(pos, 9)) <= 0) return k ? fail(past) : MCAP_OK;
            if (!get(pos, w, 9)) return fail(unreadable);
            const int op = w[0];
            const uint64_t len = mcap_le(w + 1, 8), content = pos + 9;
            char opname[16];
            snprintf(opname, sizeof(opname), "0x%02x", (unsigned) op);
            if (inner && op != MCAP_OP_SCHEMA && op != MCAP_OP_CHANNEL && op != MCAP_OP_MESSAGE) return fail(std::string("opcode ") + opname + " inside a chunk");
            if (op < MCAP_OP_HEADER || op > MCAP_OP_DATA_END) return fail(std::string("unknown opcode ") + opname);
            if (len > 0x7FFFFFFFFFFFFFFFull - content) return fail("a record length that is not a file's");
            if (op == MCAP_OP_CHUNK) {
                // start 0, end 8, uncompressed_size 16, crc 24, compression's length 28, its bytes 32, the records' length, the records
                if ((k = need(content, 32)) <= 0) return k ? fail(past) : MCAP_OK;   // (k < 0 cannot be: a chunk is never inner)
                if (!get(content, w, 32)) return fail(unreadable);
                const uint64_t cl = mcap_le(w + 28, 4);
                if (len < 40 || cl > len - 40) return fail("a chunk whose compression string runs past its record");
                if ((k = need(content + 32, cl + 8)) <= 0) return k ? fail(past) : MCAP_OK;
                buf.resize((size_t) cl + 8);
                if (!get(content + 32, buf.data(), (size_t) cl + 8)) return fail(unreadable);
                const std::string compression((const char *) buf.data(), (size_t) cl);
                const uint64_t rl = mcap_le(buf.data() + cl, 8);
                if (rl != len - 40 - cl) return fail("a chunk whose records length is not the rest of its record");
                if (!compression.empty())
                    return fail("a chunk with compression " + bag_printable(compression) +
                                ": compressed chunks are not read (rewrite the file uncompressed first: `ros2 bag convert` or the mcap command line tool can)");
                c.n_chunks++;
                number++;
                const int rc = self(self, content + 40 + cl, content + len, true);   // (of a chunk cut short: the records wholly present)
                if (rc) return rc;
                pos = content + len;
                continue;
            }
            if ((k = need(content, len)) <= 0) return k ? fail(past) : MCAP_OK;   // (a record cut short is not looked at)
            if (op == MCAP_OP_DATA_END || op == MCAP_OP_FOOTER) {
                ended = true;
            } else if (op == MCAP_OP_SCHEMA || op == MCAP_OP_CHANNEL) {
                buf.resize((size_t) len);
                if (!get(content, buf.data(), (size_t) len)) return fail(unreadable);
                const uint8_t *p = buf.data();
                uint64_t at = op == MCAP_OP_SCHEMA ? 2 : 4;
                const char *what = op == MCAP_OP_SCHEMA ? "a schema" : "a channel";
                bool fits = len >= at;
                auto str = [&](std::string *s, int len_bytes) {   // u32 (u64) length + bytes
                    if (!fits || len - at < (uint64_t) len_bytes) {
                        fits = false;
                        return;
                    }
                    const uint64_t sl = mcap_le(p + at, len_bytes);
                    at += len_bytes;
                    if (sl > len - at) {
                        fits = false;
                        return;
                    }
                    if (s) s->assign((const char *) p + at, (size_t) sl);
                    at += sl;
                };
                if (op == MCAP_OP_SCHEMA) {
                    McapSchema s;
                    str(&s.name, 4);
                    str(&s.encoding, 4);
                    str(&s.text, 4);
                    if (!fits) return fail(std::string(what) + " whose fields run past its record");
                    s.id = (uint32_t) mcap_le(p, 2);
                    s.content = buf;
                    McapSchema *old = nullptr;
                    for (McapSchema &q : schemas)
                        if (q.id == s.id) old = &q;
                    if (old) {
                        if (old->content != s.content) return fail("schema " + std::to_string(s.id) + " defined again with another content");
                    } else {
                        schemas.push_back(s);
                        c.n_schemas++;
                    }
                } else {
                    McapChannel q;
                    str(&q.topic, 4);
                    str(&q.message_encoding, 4);
                    str(nullptr, 4);
                    if (!fits) return fail(std::string(what) + " whose fields run past its record");
                    q.id = (uint32_t) mcap_le(p, 2);
                    q.schema_id = (uint32_t) mcap_le(p + 2, 2);
                    q.content = buf;
                    q.accepted = q.chosen = false;
                    McapChannel *old = nullptr;
                    for (McapChannel &j : channels)
                        if (j.id == q.id) old = &j;
                    if (old) {
                        if (old->content != q.content) return fail("channel " + std::to_string(q.id) + " defined again with another content");
                    } else {
                        const McapSchema *s = nullptr;
                        for (const McapSchema &j : schemas)
                            if (j.id == q.schema_id) s = &j;
                        if (q.schema_id && !s)
                            return fail("channel " + std::to_string(q.id) + " names schema " + std::to_string(q.schema_id) + ", which is not defined in front of it");
                        const bool in_choice = topic_choice.empty() || q.topic == topic_choice;
                        if (s) q.schema_name = s->name;
                        if (s && q.message_encoding == "cdr") {
                            if (s->encoding == "ros2msg") {
                                std::string why;
                                const int r = mcap_schema_layout(s->text, q.S, &why);
                                if (r < 0 && in_choice) return fail("schema " + bag_printable(s->name) + " of topic " + bag_printable(q.topic) + ": " + why);
                                q.accepted = r > 0;
                            } else if (s->encoding == "ros2idl" && in_choice && s->text.find("events") != std::string::npos) {
                                return fail("schema " + bag_printable(s->name) + " of topic " + bag_printable(q.topic) +
                                            " has encoding ros2idl: only ros2msg message definitions are read");
                            }
                        }
                        q.chosen = q.accepted && in_choice;
                        channels.push_back(q);
                        c.n_channels++;
                        if (q.accepted && topic_choice.empty()) {
                            if (have_event_topic && q.topic != event_topic)
                                return fail("more than one topic of events and no topic chosen: " + list_channels(true));
                            have_event_topic = true;
                            event_topic = q.topic;
                        }
                        if (q.chosen && !q.S.packet) {   // a STRUCT channel tells the file's kind where it is defined
                            if (c.layout.kind != MCAP_NONE && memcmp(&c.layout, &q.S.layout, sizeof(McapLayout)) != 0)
                                return fail("mixed kinds of events in one file: topic " + bag_printable(q.topic) + " has another kind or layout than the messages before it");
                            c.layout = q.S.layout;
                        }
                    }
                }
            } else if (op == MCAP_OP_MESSAGE) {
                if (len < 22) return fail("a message record of fewer than 22 bytes");
                if (!get(content, w, 2)) return fail(unreadable);
                const uint32_t id = (uint32_t) mcap_le(w, 2);
                const McapChannel *q = nullptr;
                for (const McapChannel &j : channels)
                    if (j.id == id) q = &j;
                if (!q) return fail("a message of channel " + std::to_string(id) + ", which is not defined in front of it");
                if (!q->chosen) {
                    c.n_other_messages++;
                } else {
                    McapMessageWalk W;
                    std::string why;
                    if (!mcap_walk_message(read, content + 22, len - 22, q->S, W, &why)) return fail("a message of topic " + bag_printable(q->topic) + ": " + why);
                    McapLayout L = q->S.layout;
                    if (q->S.packet) {
                        if (W.encoding == "mono") L = mcap_mono_layout();
                        else if (W.encoding == "evt3") L.kind = MCAP_EVT3;
                        else return fail("a packet of encoding " + bag_printable(W.encoding) + ": only mono and evt3 are read");
                        if (W.is_bigendian) return fail("a packet with is_bigendian set: big-endian packets are not read");
                        if (L.kind == MCAP_MONO && W.events_count % 8) return fail("a mono packet of " + std::to_string(W.events_count) + " bytes: not a multiple of 8");
                        if (L.kind == MCAP_EVT3 && W.events_count % 2) return fail("an evt3 packet of " + std::to_string(W.events_count) + " bytes: an odd count");
                        if (c.layout.kind != MCAP_NONE && memcmp(&c.layout, &L, sizeof(McapLayout)) != 0)
                            return fail("mixed kinds of events in one file: this " + bag_printable(W.encoding) + " packet stands behind messages of another kind");
                        c.layout = L;
                    }
                    McapMessage m;
                    m.offset = W.events_offset;
                    m.n = (uint32_t) (L.kind == MCAP_MONO ? W.events_count / 8 : W.events_count);
                    m.reserved = 0;
                    m.time_base_ns = L.kind == MCAP_MONO ? (int64_t) W.time_base : 0;
                    if (!have_first_message) {
                        have_first_message = true;
                        c.msg_width = W.has_width ? (uint32_t) W.width : 0u;
                        c.msg_height = W.has_height ? (uint32_t) W.height : 0u;
                    }
                    if (m.n && !have_first_stamp && L.kind != MCAP_EVT3) {
                        uint8_t e[8];
                        have_first_stamp = true;
                        if (L.kind == MCAP_STRUCT) {
                            if (!get(m.offset + L.sec[0], e, 4)) return fail(unreadable);
                            c.first_stamp_ns = (int64_t) (int32_t) (uint32_t) mcap_le(e, 4) * MCAP_NS_PER_S;
                        } else {
                            if (!get(m.offset, e, 4)) return fail(unreadable);
                            c.first_stamp_ns = mcap_floor_second((int64_t) ((uint64_t) m.time_base_ns + mcap_le(e, 4)));
                        }
                    }
                    c.n_messages++;
                    if (L.kind == MCAP_EVT3) c.n_payload_bytes += m.n; else c.n_raw_events += m.n;
                    on_message(m);
                }
            }   // (a header, an index, an attachment, statistics, metadata, a summary offset: stepped over)
            number++;
            pos = content + len;
        }
        return MCAP_OK;
    };
    const int rc = chain(chain, 8, n_bytes, false);
    if (rc) return rc;
    bool any = false;
    for (const McapChannel &q : channels) any = any || q.chosen;
    if (!any) {
        *err = std::string("no channel of events (message_encoding cdr, a ros2msg schema with a field events)") +
               (topic_choice.empty() ? "" : " on topic " + bag_printable(topic_choice)) + "; the file has: " + list_channels(false);
        return MCAP_INVALID;
    }
    return MCAP_OK;
}

// the same over a file in memory
template <class OnMessage>
inline int mcap_walk_memory(const uint8_t *file, uint64_t n_bytes, const std::string &topic, McapCounts &c, OnMessage &&on_message, std::string *err) {
    return mcap_walk([&](uint64_t pos, uint8_t *dst, size_t n) { memcpy(dst, file + pos, n); return true; }, n_bytes, topic, c, on_message, err);
}

// The table of the chosen messages.  out may be null with capacity 0 (a count).  MCAP_RANGE: more than `capacity` messages —
// *n_messages is the count needed, `out` holds the first `capacity`.
inline int mcap_index_messages(const uint8_t *file, uint64_t n_bytes, const std::string &topic, McapMessage *out, uint64_t capacity, uint64_t *n_messages,
                               McapCounts &c, std::string *err) {
    uint64_t n = 0;
    const int rc = mcap_walk_memory(file, n_bytes, topic, c, [&](const McapMessage &m) {
        if (n < capacity) out[n] = m;
        n++;
    }, err);
    *n_messages = n;
    if (rc) return rc;
    if (n > capacity) {
        if (err) *err = std::to_string(n) + " messages of events, more than the capacity of the table";
        return MCAP_RANGE;
    }
    return MCAP_OK;
}

// the base in force: STRUCT and MONO nanoseconds (automatic: the first event's whole second), EVT3 microseconds (automatic: 0)
inline int64_t mcap_time_base(int auto_time_base, int64_t time_base, const McapCounts &walk) {
    if (!auto_time_base) return time_base;
    return walk.layout.kind == MCAP_EVT3 ? 0 : walk.first_stamp_ns;
}

// ---- sequential host decoder ----------------------------------------------------------------------------------------------------------------
// f.time_base is ignored when auto_time_base is set.  *base_out: the base in force.  blockwise: every STRUCT / MONO event from aligned
// clipped words, as the kernels fetch it (the same events); else from its bytes
template <class PutRecord>
inline int mcap_decode_sequential(const uint8_t *file, uint64_t n_bytes, const std::string &topic, int auto_time_base, BagFilter f, McapCounts &c,
                                  PutRecord &&put, int64_t *base_out, std::string *err, bool blockwise = false) {
    std::vector<McapMessage> tab;
    const int rc = mcap_walk_memory(file, n_bytes, topic, c, [&](const McapMessage &m) { tab.push_back(m); }, err);
    if (rc) return rc;
    const McapLayout L = c.layout;
    f.time_base = mcap_time_base(auto_time_base, f.time_base, c);
    if (base_out) *base_out = f.time_base;
    if (L.kind == MCAP_EVT3) {
        if (f.flip_x || f.flip_y) {
            if (err) *err = "flip_x / flip_y are not available for evt3 packets";
            return MCAP_INVALID;
        }
        std::vector<uint8_t> payload;
        for (const McapMessage &m : tab) payload.insert(payload.end(), file + m.offset, file + m.offset + m.n);
        const ecal_raw::RawFilter rf{f.time_base, f.width, f.height, f.start_time, f.has_end_time, f.end_time};
        ecal_raw::RawCounts rc3;
        ecal_raw::raw_decode_sequential<ecal_raw::Evt3>(payload.data(), payload.size(), rf, rc3, put);
        c.n_raw_events = rc3.n_raw_events;
        c.n_events = rc3.n_events;
        c.n_outside = rc3.n_outside;
        c.n_negative = rc3.n_negative;
        c.n_before_start = rc3.n_before_start;
        c.n_after_end = rc3.n_after_end;
        c.n_no_state = rc3.n_no_state;
        c.n_other_words = rc3.n_other_words;
        c.n_time_wraps = rc3.n_time_wraps;
        return MCAP_OK;
    }
    ecal_bag::BagCounts bc;
    memset(&bc, 0, sizeof(bc));
    ecal_bag::BagSink<PutRecord> sink(f, bc, put);
    for (const McapMessage &m : tab)
        for (uint64_t k = 0; k < m.n; k++) {
            if (blockwise) {
                sink(L.kind == MCAP_MONO ? mcap_fetch_event<MCAP_MONO>(file, n_bytes, L, m.offset, k, m.time_base_ns)
                                         : mcap_fetch_event<MCAP_STRUCT>(file, n_bytes, L, m.offset, k, 0));
                continue;
            }
            const uint8_t *p = file + m.offset + mcap_event_offset(L, k);
            const int w = k ? 1 : 0;
            if (L.kind == MCAP_MONO) sink(mcap_mono_event((uint32_t) mcap_le(p, 4), (uint32_t) mcap_le(p + 4, 4), m.time_base_ns));
            else sink(mcap_struct_event((uint32_t) mcap_le(p + L.x[w], L.x_bytes), (uint32_t) mcap_le(p + L.y[w], L.y_bytes), (uint32_t) mcap_le(p + L.sec[w], 4),
                                        (uint32_t) mcap_le(p + L.nsec[w], 4), p[L.pol[w]]));
        }
    c.n_events = bc.n_events;
    c.n_outside = bc.n_outside;
    c.n_negative = bc.n_negative;
    c.n_before_start = bc.n_before_start;
    c.n_after_end = bc.n_after_end;
    return MCAP_OK;
}

}  // namespace ecal_mcap
