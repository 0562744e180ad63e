// One line of a text event file ("stamp x y polarity", the input of the reference's EventStream::txt2bin,
// event/src/EventStream.cpp:25-67) into its fields — one restatement for the kernel (ecal_text.hip), the host fallback behind
// it and the CPU test (tests/cpp/check_text_parse.cpp).  The grammar and the conversion rules: include/ecal.h, "text ingest".
//
// A decimal is converted here only when one IEEE operation gives the correctly rounded double: at most 15 significant digits
// (the mantissa m is then exact as a double) and a decimal exponent e with |e| <= 22 (10^|e| is exact), so m * 10^e or
// m / 10^-e is rounded once.  Every other well-formed number makes the line TEXT_NEEDS_HOST: the host parses that line with
// strtoll / strtod (text_parse_line_host).  Nothing here may be contracted into an FMA (there is no a * b + c to contract; the
// translation units that include this are built with -ffp-contract=off all the same).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <errno.h>
#include <stdlib.h>
#include <string>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_TEXT_HD __host__ __device__
#else
#define ECAL_TEXT_HD
#endif

namespace ecal_text {

enum : uint8_t { TEXT_OK = 0, TEXT_BLANK = 1, TEXT_NEEDS_HOST = 2, TEXT_MALFORMED = 3 };

// a longer line is not looked at on the device (TEXT_NEEDS_HOST); a record line of the format is 17 - 22 bytes
constexpr uint32_t TEXT_MAX_DEVICE_LINE = 128;

struct TextRecord {
    int64_t stamp;
    double x, y;
    uint8_t p;
    uint8_t status;
};

ECAL_TEXT_HD inline bool text_is_blank(uint8_t c) { return c == ' ' || c == '\t'; }
ECAL_TEXT_HD inline bool text_is_digit(uint8_t c) { return (uint8_t) (c - '0') < 10u; }

// 10^k, k = 0 .. 22: the powers of ten a double holds exactly
ECAL_TEXT_HD inline double text_pow10(int k) {
    constexpr double tab[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return tab[k];
}

// [+-]?[0-9]+ that fits an int64: TEXT_OK or TEXT_MALFORMED
ECAL_TEXT_HD inline uint8_t text_parse_stamp(const uint8_t *s, uint32_t n, int64_t *out) {
    uint32_t i = 0;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
    if (i == n) return TEXT_MALFORMED;
    while (i < n && s[i] == '0' && i + 1 < n) i++;   // leading zeros (the last digit stays)
    if (n - i > 19) return TEXT_MALFORMED;           // (or a non-digit among them: found below)
    uint64_t u = 0;
    for (; i < n; i++) {
        if (!text_is_digit(s[i])) return TEXT_MALFORMED;
        u = u * 10u + (uint64_t) (s[i] - '0');       // at most 19 digits: below 10^19 < 2^64
    }
    const uint64_t lim = neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull;
    if (u > lim) return TEXT_MALFORMED;
    *out = neg ? (int64_t) (0ull - u) : (int64_t) u;
    return TEXT_OK;
}

// [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?: TEXT_OK with the correctly rounded value, TEXT_NEEDS_HOST for a well-formed number
// outside the fast class, TEXT_MALFORMED
ECAL_TEXT_HD inline uint8_t text_parse_decimal(const uint8_t *s, uint32_t n, double *out) {
    uint32_t i = 0;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
    uint64_t m = 0;
    uint32_t sig = 0, n_int = 0, n_frac = 0;   // significant digits gathered; digits before / after the point
    for (; i < n && text_is_digit(s[i]); i++, n_int++) {
        if (sig || s[i] != '0') {
            if (sig < 19) m = m * 10u + (uint64_t) (s[i] - '0');
            sig++;
        }
    }
    if (i < n && s[i] == '.') {
        i++;
        for (; i < n && text_is_digit(s[i]); i++, n_frac++) {
            if (sig || s[i] != '0') {
                if (sig < 19) m = m * 10u + (uint64_t) (s[i] - '0');
                sig++;
            }
        }
    }
    if (n_int + n_frac == 0) return TEXT_MALFORMED;
    int32_t ex = 0;
    if (i < n && (s[i] == 'e' || s[i] == 'E')) {
        i++;
        bool eneg = false;
        if (i < n && (s[i] == '+' || s[i] == '-')) eneg = s[i++] == '-';
        if (i == n) return TEXT_MALFORMED;
        for (; i < n && text_is_digit(s[i]); i++)
            if (ex < 100000) ex = ex * 10 + (int32_t) (s[i] - '0');   // (saturates: far outside the fast class either way)
        if (eneg) ex = -ex;
    }
    if (i != n) return TEXT_MALFORMED;
    if (sig > 15 || n_frac > 100000u) return TEXT_NEEDS_HOST;
    const int32_t e = ex - (int32_t) n_frac;
    if (e > 22 || e < -22) return TEXT_NEEDS_HOST;
    const double v = e >= 0 ? (double) m * text_pow10(e) : (double) m / text_pow10(-e);
    *out = neg ? -v : v;
    return TEXT_OK;
}

// the four fields of the line s[0, len) (the line break not included): TEXT_OK, TEXT_BLANK (only blanks, with or without a
// closing '\r') or TEXT_MALFORMED (not four fields).  Blanks are ' ' and '\t'; one '\r' may close the line.
ECAL_TEXT_HD inline uint8_t text_split_line(const uint8_t *s, uint64_t len, uint64_t beg[4], uint32_t cnt[4]) {
    while (len && text_is_blank(s[len - 1])) len--;
    if (len && s[len - 1] == '\r') len--;
    while (len && text_is_blank(s[len - 1])) len--;
    uint64_t i = 0;
    int f = 0;
    for (;;) {
        while (i < len && text_is_blank(s[i])) i++;
        if (i == len) break;
        if (f == 4) return TEXT_MALFORMED;
        const uint64_t b = i;
        while (i < len && !text_is_blank(s[i])) i++;
        if (i - b > 0x7FFFFFFFull) return TEXT_MALFORMED;
        beg[f] = b;
        cnt[f] = (uint32_t) (i - b);
        f++;
    }
    if (f == 0) return TEXT_BLANK;
    return f == 4 ? TEXT_OK : TEXT_MALFORMED;
}

// The line parser of the kernel.  TEXT_OK: all fields set.  TEXT_NEEDS_HOST: nothing set (a number outside the fast class, or a
// line of more than TEXT_MAX_DEVICE_LINE bytes, which is not looked at).  A malformed field wins over a number for the host.
ECAL_TEXT_HD inline TextRecord text_parse_line(const uint8_t *s, uint64_t len) {
    TextRecord r{0, 0.0, 0.0, 0, TEXT_MALFORMED};
    if (len > TEXT_MAX_DEVICE_LINE) {
        r.status = TEXT_NEEDS_HOST;
        return r;
    }
    uint64_t beg[4];
    uint32_t cnt[4];
    const uint8_t sp = text_split_line(s, len, beg, cnt);
    if (sp != TEXT_OK) {
        r.status = sp;
        return r;
    }
    const uint8_t a = text_parse_stamp(s + beg[0], cnt[0], &r.stamp);
    const uint8_t b = text_parse_decimal(s + beg[1], cnt[1], &r.x);
    const uint8_t c = text_parse_decimal(s + beg[2], cnt[2], &r.y);
    const bool pol = cnt[3] == 1 && (s[beg[3]] == '0' || s[beg[3]] == '1');
    if (a == TEXT_MALFORMED || b == TEXT_MALFORMED || c == TEXT_MALFORMED || !pol) return r;
    r.p = (uint8_t) (s[beg[3]] - '0');
    r.status = (b == TEXT_NEEDS_HOST || c == TEXT_NEEDS_HOST) ? TEXT_NEEDS_HOST : TEXT_OK;
    return r;
}

// The host's parser for the lines the kernel hands back: the same grammar without the length limit, the values from strtoll /
// strtod (correctly rounded on glibc, what `is >> double` gives there).  TEXT_OK, TEXT_BLANK or TEXT_MALFORMED.
inline TextRecord text_parse_line_host(const uint8_t *s, uint64_t len) {
    TextRecord r{0, 0.0, 0.0, 0, TEXT_MALFORMED};
    uint64_t beg[4];
    uint32_t cnt[4];
    const uint8_t sp = text_split_line(s, len, beg, cnt);
    if (sp != TEXT_OK) {
        r.status = sp;
        return r;
    }
    int64_t stamp_check;
    if (text_parse_stamp(s + beg[0], cnt[0], &stamp_check) != TEXT_OK) return r;
    if (!(cnt[3] == 1 && (s[beg[3]] == '0' || s[beg[3]] == '1'))) return r;
    double v[2] = {0.0, 0.0};
    for (int f = 0; f < 2; f++) {
        const uint8_t st = text_parse_decimal(s + beg[1 + f], cnt[1 + f], &v[f]);   // (the grammar: strtod alone takes more)
        if (st == TEXT_MALFORMED) return r;
        const std::string tok((const char *) s + beg[1 + f], cnt[1 + f]);
        char *end = nullptr;
        v[f] = strtod(tok.c_str(), &end);
        if (end != tok.c_str() + tok.size()) return r;
    }
    {
        const std::string tok((const char *) s + beg[0], cnt[0]);
        char *end = nullptr;
        errno = 0;
        const long long q = strtoll(tok.c_str(), &end, 10);
        if (errno != 0 || end != tok.c_str() + tok.size()) return r;
        r.stamp = (int64_t) q;
    }
    r.x = v[0];
    r.y = v[1];
    r.p = (uint8_t) (s[beg[3]] - '0');
    r.status = TEXT_OK;
    return r;
}

// The filter of the contract after the end-stamp break (include/ecal.h): the class of one record line
enum : uint8_t { TEXT_CLASS_NONE = 0, TEXT_CLASS_KEEP = 1, TEXT_CLASS_NEGATIVE = 2, TEXT_CLASS_BEFORE_START = 3, TEXT_CLASS_STOP = 4 };
ECAL_TEXT_HD inline uint8_t text_classify(int64_t stamp, int64_t base, double magnitude, double start_time, int has_end_time,
                                          double end_time, double *t_out) {
    const int64_t d = (int64_t) ((uint64_t) stamp - (uint64_t) base);   // (a difference outside int64 wraps: not defended)
    const double t = (double) d * magnitude;                           // one subtraction, one conversion, one multiplication
    *t_out = t;
    if (t < 0) return TEXT_CLASS_NEGATIVE;
    if (has_end_time && t >= end_time) return TEXT_CLASS_STOP;
    return t >= start_time ? TEXT_CLASS_KEEP : TEXT_CLASS_BEFORE_START;
}

}  // namespace ecal_text
