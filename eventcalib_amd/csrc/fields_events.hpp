// Events from columns and back — one restatement of include/ecal.h, "array ingest", for the kernels (ecal_fields.hip), the host entry
// points (ecal_events_from_fields_host, ecal_events_to_fields_host, ecal_npy_parse_header) and the CPU test
// (tests/cpp/check_fields.cpp).
//
// A field is a column: element i at ptr + i * stride, of one of nine little-endian types, at ANY byte offset.  An event carries all
// of its own state, so   sequential: the walk over i = 0 .. n-1   and   block-wise: every block on its own, the stop rule as "the
// least i that reaches end_time"   give the same events.
// Floating point here: one conversion and one multiplication per stamp, one subtraction per flipped coordinate (the translation units
// that include this are built with -ffp-contract=off).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include "event_record.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_FIELDS_HD __host__ __device__ __forceinline__
#else
#define ECAL_FIELDS_HD inline
#endif

namespace ecal_fields {

enum : int { FD_OK = 0, FD_INVALID = -1, FD_RANGE = -6 };   // ECAL_OK / ECAL_ERR_INVALID / ECAL_ERR_RANGE

// ECAL_FIELD_* of ecal.h
enum : uint32_t { FD_U8 = 0, FD_I8 = 1, FD_U16 = 2, FD_I16 = 3, FD_U32 = 4, FD_I32 = 5, FD_I64 = 6, FD_F32 = 7, FD_F64 = 8, FD_N_TYPES = 9 };
enum : int { FD_T = 0, FD_X = 1, FD_Y = 2, FD_P = 3 };

// a block of the kernels: 256 threads x 4 consecutive events (ecal_fields_block_events)
constexpr uint32_t FD_BLOCK_THREADS = 256;
constexpr uint32_t FD_THREAD_EVENTS = 4;
constexpr uint32_t FD_BLOCK_EVENTS = FD_BLOCK_THREADS * FD_THREAD_EVENTS;

struct Field {   // ecal_field of ecal.h
    const void *ptr;
    int64_t stride;
    uint32_t type;
    uint32_t reserved;
};

ECAL_FIELDS_HD uint32_t fd_type_size(uint32_t type) {
    return type <= FD_I8 ? 1u : type <= FD_I16 ? 2u : type <= FD_I32 ? 4u : type == FD_I64 ? 8u : type == FD_F32 ? 4u : 8u;
}
ECAL_FIELDS_HD bool fd_type_is_float(uint32_t type) { return type >= FD_F32; }
inline bool fd_type_takes_stamp(uint32_t type) { return type == FD_U32 || type == FD_I32 || type == FD_I64 || type == FD_F32 || type == FD_F64; }
inline const char *fd_field_name(int k) { return k == FD_T ? "t" : k == FD_X ? "x" : k == FD_Y ? "y" : "p"; }
inline const char *fd_type_name(uint32_t type) {
    static const char *const names[FD_N_TYPES] = {"U8", "I8", "U16", "I16", "U32", "I32", "I64", "F32", "F64"};
    return type < FD_N_TYPES ? names[type] : "unknown";
}

// ---- an element's bytes ------------------------------------------------------------------------------------------------------------------
// The element at byte offset r = address & 3 behind an aligned word, from the aligned little-endian words that hold it: w0 always, w1
// when r + size > 4, w2 when r + size > 8 (a word that holds no byte of the element is not loaded: pass 0).  The bytes behind the
// element's size are whatever lies there: fd_value_* look at the type's bytes only.
ECAL_FIELDS_HD uint64_t fd_bits_from_words(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t r) {
    const uint32_t sh = 8u * r;
    const uint32_t lo = (uint32_t) ((((uint64_t) w1 << 32) | w0) >> sh);
    const uint32_t hi = (uint32_t) ((((uint64_t) w2 << 32) | w1) >> sh);
    return ((uint64_t) hi << 32) | lo;
}

// the same on the host, from the element's own bytes
inline uint64_t fd_bits_at(const void *p, uint32_t size) {
    uint64_t v = 0;
    memcpy(&v, p, size);
    return v;
}

// an integer type's value (not for F32 / F64)
ECAL_FIELDS_HD int64_t fd_value_i64(uint64_t bits, uint32_t type) {
    switch (type) {
        case FD_U8: return (int64_t) (uint8_t) bits;
        case FD_I8: return (int64_t) (int8_t) (uint8_t) bits;
        case FD_U16: return (int64_t) (uint16_t) bits;
        case FD_I16: return (int64_t) (int16_t) (uint16_t) bits;
        case FD_U32: return (int64_t) (uint32_t) bits;
        case FD_I32: return (int64_t) (int32_t) (uint32_t) bits;
        default: return (int64_t) bits;
    }
}

// any type's value as a double (I64: the conversion rounds to nearest beyond 2^53)
ECAL_FIELDS_HD double fd_value_f64(uint64_t bits, uint32_t type) {
    if (type == FD_F64) return __builtin_bit_cast(double, bits);
    if (type == FD_F32) return (double) __builtin_bit_cast(float, (uint32_t) bits);
    return (double) fd_value_i64(bits, type);
}

// value > 0: 0 / 1, bool and -1 / +1 alike; NaN is not
ECAL_FIELDS_HD bool fd_value_positive(uint64_t bits, uint32_t type) {
    return fd_type_is_float(type) ? fd_value_f64(bits, type) > 0.0 : fd_value_i64(bits, type) > 0;
}

// ---- conversion and filter (the bag ingest's, bag_events.hpp, with doubles for x and y and a magnitude for t) -----------------------------
struct FieldsFilter {
    double time_magnitude;    // seconds per tick
    int64_t time_base;        // ticks; 0 for a float stamp
    uint32_t width, height;   // 0: no bound
    double start_time;
    int has_end_time;
    double end_time;
    int flip_x, flip_y;       // need width / height
};

enum : uint8_t { FD_CLASS_KEEP = 0, FD_CLASS_OUTSIDE = 1, FD_CLASS_NEGATIVE = 2, FD_CLASS_BEFORE_START = 3, FD_CLASS_STOP = 4 };

// t_bits / t_type: the stamp's element; x, y: the doubles of the coordinates.  *x_out / *y_out: behind the flips, *t_out: seconds
// (written for every class but OUTSIDE)
ECAL_FIELDS_HD uint8_t fd_classify(uint64_t t_bits, uint32_t t_type, double x, double y, const FieldsFilter &f, double *t_out, double *x_out,
                                   double *y_out) {
    if (f.width && !(x >= 0.0 && x < (double) f.width)) return FD_CLASS_OUTSIDE;     // (a NaN is outside)
    if (f.height && !(y >= 0.0 && y < (double) f.height)) return FD_CLASS_OUTSIDE;
    *x_out = (f.flip_x && f.width) ? (double) (f.width - 1u) - x : x;                // (behind the bounds test)
    *y_out = (f.flip_y && f.height) ? (double) (f.height - 1u) - y : y;
    double t;
    if (fd_type_is_float(t_type)) {
        t = fd_value_f64(t_bits, t_type) * f.time_magnitude;
    } else {
        const int64_t d = (int64_t) ((uint64_t) fd_value_i64(t_bits, t_type) - (uint64_t) f.time_base);
        t = (double) d * f.time_magnitude;   // one subtraction, one conversion, one multiplication
    }
    *t_out = t;
    if (!(t >= 0.0)) return FD_CLASS_NEGATIVE;   // (a NaN stamp lands here)
    if (f.has_end_time && t >= f.end_time) return FD_CLASS_STOP;
    return t >= f.start_time ? FD_CLASS_KEEP : FD_CLASS_BEFORE_START;
}

struct FieldsCounts {
    uint64_t n_raw_events, n_events, n_outside, n_negative, n_before_start, n_after_end;
};

// What the entry points refuse before they look at an element: *which = the field (-1: none in particular), *why = the text.
inline int fd_check_fields(const Field f[4], uint64_t n, int *which, std::string *why) {
    for (int k = 0; k < 4; k++) {
        *which = k;
        if (f[k].type >= FD_N_TYPES) {
            *why = std::string("field ") + fd_field_name(k) + ": unknown type " + std::to_string(f[k].type);
            return FD_INVALID;
        }
        if (k == FD_T && !fd_type_takes_stamp(f[k].type)) {
            *why = std::string("field t: type ") + fd_type_name(f[k].type) + " is not a stamp type (U32, I32, I64, F32, F64 are)";
            return FD_INVALID;
        }
        if (n && !f[k].ptr) {
            *why = std::string("field ") + fd_field_name(k) + ": null pointer";
            return FD_INVALID;
        }
        if (f[k].stride < (int64_t) fd_type_size(f[k].type)) {
            *why = std::string("field ") + fd_field_name(k) + ": stride " + std::to_string(f[k].stride) + " is below the size of " + fd_type_name(f[k].type);
            return FD_INVALID;
        }
        if (n > 1 && (uint64_t) f[k].stride > (~0ull >> 2) / n) {
            *why = std::string("field ") + fd_field_name(k) + ": stride times count does not fit 62 bits";
            return FD_RANGE;
        }
    }
    *which = -1;
    return FD_OK;
}

inline int fd_check_filter(const FieldsFilter &f, uint32_t t_type, std::string *why) {
    if ((f.flip_x && !f.width) || (f.flip_y && !f.height)) {
        *why = "flip_x / flip_y need width / height";
        return FD_INVALID;
    }
    if (fd_type_is_float(t_type) && f.time_base != 0) {
        *why = "field t: a float stamp takes no time_base (it must be 0)";
        return FD_INVALID;
    }
    return FD_OK;
}

// the bytes a field covers: [ptr, ptr + (n - 1) * stride + size), empty for n == 0
inline uint64_t fd_field_span(const Field &f, uint64_t n) { return n ? (n - 1) * (uint64_t) f.stride + fd_type_size(f.type) : 0; }

// the automatic base: element 0's stamp for an integer stamp, 0 for a float stamp and for no events
inline int64_t fd_auto_time_base(const Field &t, uint64_t n) {
    if (!n || fd_type_is_float(t.type)) return 0;
    return fd_value_i64(fd_bits_at(t.ptr, fd_type_size(t.type)), t.type);
}

// ---- the walk: HOST fields in input order, the kept ones to put(const uint8_t rec[25]) ---------------------------------------------------
template <class PutRecord> inline void fd_walk(const Field f[4], uint64_t n, const FieldsFilter &flt, FieldsCounts &c, PutRecord &&put) {
    memset(&c, 0, sizeof(c));
    uint32_t size[4];
    for (int k = 0; k < 4; k++) size[k] = fd_type_size(f[k].type);
    bool stopped = false;
    for (uint64_t i = 0; i < n; i++) {
        c.n_raw_events++;
        if (stopped) {
            c.n_after_end++;
            continue;
        }
        uint64_t b[4];
        for (int k = 0; k < 4; k++) b[k] = fd_bits_at((const uint8_t *) f[k].ptr + i * (uint64_t) f[k].stride, size[k]);
        double t = 0, x = 0, y = 0;
        switch (fd_classify(b[FD_T], f[FD_T].type, fd_value_f64(b[FD_X], f[FD_X].type), fd_value_f64(b[FD_Y], f[FD_Y].type), flt, &t, &x, &y)) {
            case FD_CLASS_OUTSIDE: c.n_outside++; break;
            case FD_CLASS_NEGATIVE: c.n_negative++; break;
            case FD_CLASS_BEFORE_START: c.n_before_start++; break;
            case FD_CLASS_STOP: stopped = true; c.n_after_end++; break;
            default: {
                uint8_t rec[25];
                ecal::pack_record(rec, t, x, y, (uint8_t) (fd_value_positive(b[FD_P], f[FD_P].type) ? 1u : 0u));
                put(rec);
                c.n_events++;
            }
        }
    }
}

// ---- the reverse: a record's t, x, y, polarity byte into an element of a column ---------------------------------------------------------
struct ToFields {
    double ticks_per_second;
    int64_t time_base;       // ticks, added to an integer stamp
    int polarity_signed;     // -1 / +1 instead of 0 / 1
};

ECAL_FIELDS_HD bool fd_int_fits(int64_t v, uint32_t type) {
    switch (type) {
        case FD_U8: return v >= 0 && v <= 0xFF;
        case FD_I8: return v >= -128 && v <= 127;
        case FD_U16: return v >= 0 && v <= 0xFFFF;
        case FD_I16: return v >= -32768 && v <= 32767;
        case FD_U32: return v >= 0 && v <= 0xFFFFFFFFll;
        case FD_I32: return v >= -2147483648ll && v <= 2147483647ll;
        default: return true;
    }
}

// v rounded to the nearest integer, ties to even; false: not finite or beyond int64
ECAL_FIELDS_HD bool fd_round_i64(double v, int64_t *out) {
    if (!(v >= -9223372036854775808.0 && v < 9223372036854775808.0)) return false;
    *out = (int64_t) rint(v);
    return true;
}

ECAL_FIELDS_HD uint64_t fd_float_bits(double v, uint32_t type) {
    return type == FD_F64 ? __builtin_bit_cast(uint64_t, v) : (uint64_t) __builtin_bit_cast(uint32_t, (float) v);
}

// *bits: the element's little-endian bytes in the low fd_type_size(type) bytes.  false: not representable.
ECAL_FIELDS_HD bool fd_stamp_element(double t, uint32_t type, const ToFields &o, uint64_t *bits) {
    if (fd_type_is_float(type)) {
        *bits = fd_float_bits(t, type);
        return true;
    }
    int64_t r = 0, s = 0;
    if (!fd_round_i64(t * o.ticks_per_second, &r)) return false;   // one multiplication, ties to even
    if (__builtin_add_overflow(o.time_base, r, &s)) return false;  // one addition
    *bits = (uint64_t) s;
    return fd_int_fits(s, type);
}

ECAL_FIELDS_HD bool fd_coord_element(double v, uint32_t type, uint64_t *bits) {
    if (fd_type_is_float(type)) {
        *bits = fd_float_bits(v, type);
        return true;
    }
    int64_t r = 0;
    if (!fd_round_i64(v, &r) || (double) r != v) return false;   // an integral value (a sub-pixel one is not representable)
    *bits = (uint64_t) r;
    return fd_int_fits(r, type);
}

ECAL_FIELDS_HD uint64_t fd_polarity_element(uint8_t pol_byte, uint32_t type, const ToFields &o) {
    const int64_t v = pol_byte != 0 ? 1 : (o.polarity_signed ? -1 : 0);
    return fd_type_is_float(type) ? fd_float_bits((double) v, type) : (uint64_t) v;
}

inline bool fd_type_is_unsigned(uint32_t type) { return type == FD_U8 || type == FD_U16 || type == FD_U32; }

inline int fd_check_to_fields(const Field out[4], uint64_t n, const ToFields &o, int *which, std::string *why) {
    const int rc = fd_check_fields(out, n, which, why);
    if (rc) return rc;
    if (o.polarity_signed && fd_type_is_unsigned(out[FD_P].type)) {
        *which = FD_P;
        *why = std::string("field p: a signed polarity does not fit the unsigned type ") + fd_type_name(out[FD_P].type);
        return FD_INVALID;
    }
    if (!(o.ticks_per_second > 0.0) || !(o.ticks_per_second <= 1.79769313486231570e308)) {
        *which = -1;
        *why = "ticks_per_second must be positive and finite";
        return FD_INVALID;
    }
    return FD_OK;
}

inline double fd_load_f64(const uint8_t *p) {
    double v;
    memcpy(&v, p, 8);
    return v;
}

// HOST records into HOST columns; returns the events that are not representable (their elements are left as they were)
inline uint64_t fd_unwalk(const uint8_t *rec, uint64_t n, const Field out[4], const ToFields &o) {
    uint64_t bad = 0;
    uint32_t size[4];
    for (int k = 0; k < 4; k++) size[k] = fd_type_size(out[k].type);
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *r = rec + i * 25u;
        uint64_t b[4];
        bool ok = fd_stamp_element(fd_load_f64(r), out[FD_T].type, o, &b[FD_T]);
        ok = fd_coord_element(fd_load_f64(r + 8), out[FD_X].type, &b[FD_X]) && ok;
        ok = fd_coord_element(fd_load_f64(r + 16), out[FD_Y].type, &b[FD_Y]) && ok;
        b[FD_P] = fd_polarity_element(r[24], out[FD_P].type, o);
        if (!ok) {
            bad++;
            continue;
        }
        for (int k = 0; k < 4; k++) memcpy((uint8_t *) out[k].ptr + i * (uint64_t) out[k].stride, &b[k], size[k]);
    }
    return bad;
}

// ---- .npy headers (host) -----------------------------------------------------------------------------------------------------------------
struct NpyLayout {   // ecal_npy_layout of ecal.h
    uint64_t data_offset;   // of element 0, from byte 0 of the file
    uint64_t n_events;
    uint64_t item_stride;   // bytes from one event to the next
    struct {
        uint64_t offset;    // of the field inside an item
        uint32_t type;
        uint32_t reserved;
    } field[4];             // t, x, y, p
    uint32_t version_major, version_minor;
};

struct NpyChoice {
    std::string name[4];   // empty: the aliases (t|ts|time|timestamp, x, y, p|pol|polarity), without case
    std::string columns;   // of a 2-D array; empty: "txyp"
};

inline std::string npy_printable(const std::string &s) {
    std::string o;
    for (size_t i = 0; i < s.size() && i < 64; i++) o += (s[i] >= 0x20 && s[i] <= 0x7E) ? s[i] : '?';
    return o;
}

// a cursor over the header's text: just the literals numpy writes
struct NpyCursor {
    const char *p, *end;
    void ws() {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
    }
    bool take(char c) {
        ws();
        if (p < end && *p == c) {
            p++;
            return true;
        }
        return false;
    }
    bool peek(char c) {
        ws();
        return p < end && *p == c;
    }
    bool string(std::string *out) {
        ws();
        if (p >= end || (*p != '\'' && *p != '"')) return false;
        const char q = *p++;
        out->clear();
        while (p < end && *p != q) {
            if (*p == '\\') return false;   // (numpy's field names and type codes carry no escapes)
            out->push_back(*p++);
        }
        if (p >= end) return false;
        p++;
        return true;
    }
    bool number(uint64_t *out) {
        ws();
        if (p >= end || *p < '0' || *p > '9') return false;
        uint64_t v = 0;
        while (p < end && *p >= '0' && *p <= '9') {
            if (v > (~0ull - 9) / 10) return false;
            v = v * 10 + (uint64_t) (*p++ - '0');
        }
        if (p < end && (*p == 'L' || *p == 'l')) p++;   // (a Python 2 long)
        *out = v;
        return true;
    }
    bool word(const char *w) {
        ws();
        const size_t n = strlen(w);
        if ((size_t) (end - p) >= n && memcmp(p, w, n) == 0) {
            p += n;
            return true;
        }
        return false;
    }
};

struct NpyCode {
    bool big_endian, object;
    uint32_t type;    // FD_N_TYPES: not one of the nine
    uint64_t size;    // bytes; 0: not understood
};

// a type code as numpy writes it: an optional byte-order mark, a kind letter, the size in bytes (U: in characters of 4 bytes)
inline NpyCode npy_parse_code(const std::string &code) {
    NpyCode c{false, false, FD_N_TYPES, 0};
    size_t i = 0;
    char order = '|';
    if (i < code.size() && (code[i] == '<' || code[i] == '>' || code[i] == '|' || code[i] == '=')) order = code[i++];
    if (i >= code.size()) return c;
    const char kind = code[i++];
    if (kind == 'O') {
        c.object = true;
        return c;
    }
    if (kind == '?') {   // (the one-letter bool)
        c.type = FD_U8;
        c.size = 1;
        return c;
    }
    uint64_t n = 0;
    size_t digits = 0;
    while (i < code.size() && code[i] >= '0' && code[i] <= '9' && n < (1ull << 40)) {
        n = n * 10 + (uint64_t) (code[i++] - '0');
        digits++;
    }
    if (!digits) return c;
    if (i < code.size() && !((kind == 'M' || kind == 'm') && code[i] == '[')) return c;
    if (!strchr("biufcSVaUMm", kind)) return c;
    c.size = kind == 'U' ? 4 * n : n;
    c.big_endian = order == '>' && c.size > 1 && kind != 'S' && kind != 'V' && kind != 'a';
    if (kind == 'b' && n == 1) c.type = FD_U8;
    else if (kind == 'u') c.type = n == 1 ? FD_U8 : n == 2 ? FD_U16 : n == 4 ? FD_U32 : FD_N_TYPES;
    else if (kind == 'i') c.type = n == 1 ? FD_I8 : n == 2 ? FD_I16 : n == 4 ? FD_I32 : n == 8 ? FD_I64 : FD_N_TYPES;
    else if (kind == 'f') c.type = n == 4 ? FD_F32 : n == 8 ? FD_F64 : FD_N_TYPES;
    return c;
}

inline bool npy_name_equal_nocase(const std::string &a, const char *b) {
    const size_t n = strlen(b);
    if (a.size() != n) return false;
    for (size_t i = 0; i < n; i++) {
        const char x = a[i] >= 'A' && a[i] <= 'Z' ? (char) (a[i] + 32) : a[i], y = b[i] >= 'A' && b[i] <= 'Z' ? (char) (b[i] + 32) : b[i];
        if (x != y) return false;
    }
    return true;
}

// which of t, x, y, p the field `name` is (-1: none)
inline int npy_role_of(const std::string &name, const NpyChoice &ch) {
    static const char *const alias[4][5] = {{"t", "ts", "time", "timestamp", nullptr}, {"x", nullptr}, {"y", nullptr}, {"p", "pol", "polarity", nullptr}};
    for (int k = 0; k < 4; k++) {
        if (!ch.name[k].empty()) {
            if (name == ch.name[k]) return k;
            continue;
        }
        for (int a = 0; alias[k][a]; a++)
            if (npy_name_equal_nocase(name, alias[k][a])) return k;
    }
    return -1;
}

// bytes [0, n_bytes): the front of the file, the whole header at least.  file_bytes: the file's size (0: n_bytes is the whole file).
// FD_INVALID with *err: whatever the contract refuses, by name.
inline int npy_parse_header(const uint8_t *bytes, uint64_t n_bytes, uint64_t file_bytes, const NpyChoice &choice, NpyLayout &L, std::string *err) {
    std::string scratch;
    if (!err) err = &scratch;
    memset(&L, 0, sizeof(L));
    if (!file_bytes) file_bytes = n_bytes;
    auto fail = [&](const std::string &why) {
        *err = why;
        return FD_INVALID;
    };
    if (n_bytes < 10 || memcmp(bytes, "\x93NUMPY", 6) != 0) return fail("no \\x93NUMPY magic: not a .npy file");
    const uint32_t major = bytes[6], minor = bytes[7];
    if (major < 1 || major > 3 || minor != 0) return fail("format version " + std::to_string(major) + "." + std::to_string(minor) + " is not read (1.0, 2.0 and 3.0 are)");
    uint64_t start, hlen;
    if (major == 1) {
        start = 10;
        hlen = (uint64_t) bytes[8] | ((uint64_t) bytes[9] << 8);
    } else {
        if (n_bytes < 12) return fail("the header is cut short (" + std::to_string(n_bytes) + " bytes)");
        start = 12;
        hlen = (uint64_t) bytes[8] | ((uint64_t) bytes[9] << 8) | ((uint64_t) bytes[10] << 16) | ((uint64_t) bytes[11] << 24);
    }
    if (hlen > n_bytes - start) return fail("the header is cut short: " + std::to_string(hlen) + " bytes announced, " + std::to_string(n_bytes - start) + " there");
    L.version_major = major;
    L.version_minor = minor;
    L.data_offset = start + hlen;
    NpyCursor c{(const char *) bytes + start, (const char *) bytes + start + hlen};
    static const char malformed[] = "the header is not a dict as numpy writes it";
    if (!c.take('{')) return fail(malformed);

    struct Entry {
        std::string name, code;
    };
    std::vector<Entry> entries;
    std::string plain;
    std::vector<uint64_t> shape;
    bool have_descr = false, structured = false, have_order = false, fortran = false, have_shape = false;
    while (!c.peek('}')) {
        std::string key;
        if (!c.string(&key) || !c.take(':')) return fail(malformed);
        if (key == "descr") {
            have_descr = true;
            if (c.peek('[')) {
                structured = true;
                c.take('[');
                while (!c.peek(']')) {
                    Entry e;
                    if (!c.take('(')) return fail(malformed);
                    if (c.peek('(')) return fail("descr: a field with a title is not read");
                    if (!c.string(&e.name) || !c.take(',')) return fail(malformed);
                    if (c.peek('[')) return fail("descr: field '" + npy_printable(e.name) + "' is a nested structure, which is not read");
                    if (!c.string(&e.code)) return fail(malformed);
                    if (c.take(',') && !c.peek(')')) return fail("descr: field '" + npy_printable(e.name) + "' is a sub-array, which is not read");
                    if (!c.take(')')) return fail(malformed);
                    entries.push_back(e);
                    if (!c.take(',') && !c.peek(']')) return fail(malformed);
                    if (entries.size() > 4096) return fail("descr: more than 4096 fields");
                }
                c.take(']');
            } else if (c.peek('{')) {
                return fail("descr: a dict of names, formats and offsets is not read (numpy writes a list)");
            } else if (!c.string(&plain)) {
                return fail(malformed);
            }
        } else if (key == "fortran_order") {
            have_order = true;
            if (c.word("True")) fortran = true;
            else if (c.word("False")) fortran = false;
            else return fail(malformed);
        } else if (key == "shape") {
            have_shape = true;
            if (!c.take('(')) return fail(malformed);
            while (!c.peek(')')) {
                uint64_t v;
                if (!c.number(&v)) return fail(malformed);
                shape.push_back(v);
                if (!c.take(',') && !c.peek(')')) return fail(malformed);
                if (shape.size() > 32) return fail(malformed);
            }
            c.take(')');
        } else {
            return fail("the header has the key '" + npy_printable(key) + "' (descr, fortran_order and shape are read)");
        }
        if (!c.take(',') && !c.peek('}')) return fail(malformed);
    }
    if (!have_descr || !have_order || !have_shape) return fail("the header lacks descr, fortran_order or shape");

    if (structured) {
        if (shape.size() != 1) return fail("a structured array of " + std::to_string(shape.size()) + " dimensions (1 is read)");
        bool found[4] = {false, false, false, false};
        uint64_t off = 0;
        for (const Entry &e : entries) {
            const NpyCode code = npy_parse_code(e.code);
            const int role = e.name.empty() ? -1 : npy_role_of(e.name, choice);
            if (role >= 0) {
                if (found[role]) return fail(std::string("duplicate field for ") + fd_field_name(role) + ": '" + npy_printable(e.name) + "'");
                if (code.object) return fail("field '" + npy_printable(e.name) + "' is an object dtype");
                if (code.big_endian) return fail("field '" + npy_printable(e.name) + "' is big-endian (" + npy_printable(e.code) + "): little-endian data is read");
                if (code.type >= FD_N_TYPES || (role == FD_T && !fd_type_takes_stamp(code.type)))
                    return fail("field '" + npy_printable(e.name) + "' has type " + npy_printable(e.code) + ", which field " + fd_field_name(role) + " does not take");
                found[role] = true;
                L.field[role].offset = off;
                L.field[role].type = code.type;
            } else {
                if (code.object) return fail("field '" + npy_printable(e.name) + "' is an object dtype");
                if (!code.size) return fail("field '" + npy_printable(e.name) + "' has type " + npy_printable(e.code) + ", whose size is not known");
            }
            if (code.size > (1ull << 40) || (off += code.size) > (1ull << 40)) return fail("descr: an item of more than 2^40 bytes");
        }
        for (int k = 0; k < 4; k++)
            if (!found[k])
                return fail(std::string("missing field ") + fd_field_name(k) + (choice.name[k].empty() ? "" : " ('" + npy_printable(choice.name[k]) + "')"));
        L.item_stride = off;
        L.n_events = shape[0];
    } else {
        const NpyCode code = npy_parse_code(plain);
        if (code.object) return fail("an object dtype");
        if (code.big_endian) return fail("big-endian data (" + npy_printable(plain) + "): little-endian data is read");
        if (code.type >= FD_N_TYPES || !fd_type_takes_stamp(code.type))
            return fail("a plain array of type " + npy_printable(plain) + " (U32, I32, I64, F32, F64 hold a stamp column)");
        if (shape.size() != 2 || shape[1] != 4) {
            std::string s;
            for (uint64_t v : shape) s += std::to_string(v) + ",";
            return fail("a plain array of shape (" + s + "): (N, 4) is read");
        }
        if (fortran) return fail("fortran_order: True on 2-D data: C order is read");
        const std::string cols = choice.columns.empty() ? std::string("txyp") : choice.columns;
        bool found[4] = {false, false, false, false};
        if (cols.size() != 4) return fail("columns '" + npy_printable(cols) + "': four letters of t, x, y, p");
        for (uint32_t j = 0; j < 4; j++) {
            const int role = cols[j] == 't' ? FD_T : cols[j] == 'x' ? FD_X : cols[j] == 'y' ? FD_Y : cols[j] == 'p' ? FD_P : -1;
            if (role < 0 || found[role]) return fail("columns '" + npy_printable(cols) + "': four letters of t, x, y, p, each once");
            found[role] = true;
            L.field[role].offset = j * code.size;
            L.field[role].type = code.type;
        }
        L.item_stride = 4 * code.size;
        L.n_events = shape[0];
    }
    const uint64_t have = file_bytes > L.data_offset ? file_bytes - L.data_offset : 0;
    if (L.item_stride && L.n_events > (~0ull >> 2) / L.item_stride) return fail("the shape does not fit 62 bits of payload");
    const uint64_t need = L.n_events * L.item_stride;
    if (have < need) return fail("the payload is shorter than the shape says: " + std::to_string(have) + " bytes there, " + std::to_string(need) + " needed");
    return FD_OK;
}

// the header of a file whose payload is n packed 25-byte records: version 1.0, padded to a multiple of 64 bytes as numpy pads it
inline std::string npy_records_header(uint64_t n) {
    std::string dict = "{'descr': [('t', '<f8'), ('x', '<f8'), ('y', '<f8'), ('p', '|u1')], 'fortran_order': False, 'shape': (" + std::to_string(n) + ",), }";
    const size_t unpadded = 10 + dict.size() + 1;
    dict.append((64 - unpadded % 64) % 64, ' ');
    dict.push_back('\n');
    std::string h("\x93NUMPY\x01\x00", 8);
    h.push_back((char) (dict.size() & 0xFF));
    h.push_back((char) (dict.size() >> 8));
    return h + dict;
}

}  // namespace ecal_fields
