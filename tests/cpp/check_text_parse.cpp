// CPU check of the text line parser (eventcalib_amd/csrc/text_events.hpp), the functions the parse kernel and the host fallback
// call, against strtoll / strtod on tokens cut by a plain loop of this file's own.
//   - 200 000 seeded random lines of the fast class (integers, decimals of 1 - 15 significant digits with 0 - 22 fraction
//     digits, exponents, signs, -0, leading zeros, tabs, '\r', blanks in front and behind): TEXT_OK and bit-equal fields
//   - 20 000 lines built to leave the fast class (16 - 19 digit mantissas, decimal exponent beyond +-22, lines longer than the
//     device limit): TEXT_NEEDS_HOST from the kernel's parser, never a value; the host parser equals strtoll / strtod
//   - malformed lines: TEXT_MALFORMED from both; blank lines: TEXT_BLANK
// Built twice by tests/test_text_parse_host.py: plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "text_events.hpp"

using namespace ecal_text;

namespace {

std::mt19937_64 rng(20240607);
uint64_t rnd(uint64_t n) { return rng() % n; }   // [0, n)

std::string digits(int n, bool first_nonzero) {
    std::string s;
    for (int i = 0; i < n; i++) s.push_back((char) ('0' + (i == 0 && first_nonzero ? 1 + rnd(9) : rnd(10))));
    return s;
}

std::string sign(bool allow_plus = true) {
    const uint64_t r = rnd(6);
    return r == 0 ? "-" : (r == 1 && allow_plus) ? "+" : "";
}

// nd significant digits, nf of them (and zeros in front where nf > nd) behind the point
std::string decimal_body(int nd, int nf) {
    const std::string d = digits(nd, true);
    std::string s;
    if (nf >= nd) {
        s = (rnd(3) ? "0." : ".") + std::string((size_t) (nf - nd), '0') + d;
    } else {
        s = d.substr(0, (size_t) (nd - nf));
        if (nf > 0) s += "." + d.substr((size_t) (nd - nf));
        else if (rnd(8) == 0) s += ".";
        if (rnd(6) == 0) s = std::string(1 + rnd(3), '0') + s;   // leading zeros
    }
    return s;
}

std::string fast_decimal() {
    switch (rnd(10)) {
    case 0: return rnd(2) ? "-0" : "-0.0";
    case 1: return rnd(2) ? "0" : "0.000";
    case 2:
    case 3:
    case 4: return std::to_string(rnd(1280));   // a sensor pixel
    case 5: {                                   // with a written exponent: |written - fraction digits| <= 22
        const int nd = 1 + (int) rnd(15), nf = (int) rnd(23);
        const int e = -22 + (int) rnd(45), written = e + nf;
        const char *E = rnd(2) ? "e" : "E";
        return sign() + decimal_body(nd, nf) + E + (written < 0 ? "-" : rnd(2) ? "+" : "") + (rnd(4) ? "" : "0") +
               std::to_string(written < 0 ? -written : written);
    }
    default: return sign() + decimal_body(1 + (int) rnd(15), (int) rnd(23));
    }
}

std::string slow_decimal() {
    switch (rnd(3)) {
    case 0: return sign() + decimal_body(16 + (int) rnd(4), (int) rnd(16));   // 16 - 19 significant digits
    case 1: {                                                                // decimal exponent beyond +-22
        const int nd = 1 + (int) rnd(15), nf = (int) rnd(10);
        const int e = (rnd(2) ? 1 : -1) * (23 + (int) rnd(260)), written = e + nf;
        return sign() + decimal_body(nd, nf) + "e" + std::to_string(written);
    }
    default: return sign() + decimal_body(1 + (int) rnd(15), 23 + (int) rnd(10));   // more than 22 fraction digits
    }
}

std::string stamp_token() {
    std::string s = sign() + (rnd(10) == 0 ? std::string(1 + rnd(3), '0') : "") + digits(1 + (int) rnd(18), rnd(4) != 0);
    return s;
}

std::string blanks(int lo, int hi) {
    std::string s;
    for (int n = lo + (int) rnd((uint64_t) (hi - lo + 1)); n > 0; n--) s.push_back(rnd(4) ? ' ' : '\t');
    return s;
}

std::string join(const std::string &a, const std::string &b, const std::string &c, const std::string &d) {
    std::string s = blanks(0, 2) + a + blanks(1, 3) + b + blanks(1, 3) + c + blanks(1, 3) + d + blanks(0, 2);
    if (rnd(4) == 0) s += "\r";
    return s;
}

// the oracle: tokens cut at ' ' '\t' '\r', strtoll / strtod on them
struct Ref {
    long long stamp;
    double x, y;
    int p;
};
Ref oracle(const std::string &line) {
    std::vector<std::string> tok;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) i++;
        size_t b = i;
        while (i < line.size() && !(line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) i++;
        if (i > b) tok.push_back(line.substr(b, i - b));
    }
    if (tok.size() != 4) {
        fprintf(stderr, "generator: %zu tokens in '%s'\n", tok.size(), line.c_str());
        exit(2);
    }
    Ref r;
    errno = 0;
    r.stamp = strtoll(tok[0].c_str(), nullptr, 10);
    r.x = strtod(tok[1].c_str(), nullptr);
    r.y = strtod(tok[2].c_str(), nullptr);
    r.p = atoi(tok[3].c_str());
    if (errno) {
        fprintf(stderr, "generator: out of range in '%s'\n", line.c_str());
        exit(2);
    }
    return r;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int failures = 0;
void fail(const char *what, const std::string &line) {
    if (failures++ < 20) fprintf(stderr, "FAIL %s: '%s'\n", what, line.c_str());
}

bool equal(const TextRecord &r, const Ref &o) {
    return r.stamp == (int64_t) o.stamp && same_bits(r.x, o.x) && same_bits(r.y, o.y) && r.p == (uint8_t) o.p;
}

// the parser must look at nothing outside [s, s + len): the line in a buffer of exactly its size (AddressSanitizer watches)
TextRecord parse_tight(const std::string &line, bool host) {
    std::vector<uint8_t> buf(line.begin(), line.end());
    const uint8_t *p = buf.empty() ? (const uint8_t *) "" : buf.data();
    return host ? text_parse_line_host(p, buf.size()) : text_parse_line(p, buf.size());
}

}  // namespace

int main() {
    // ---- the fast class
    const int N_FAST = 200000;
    long n_neg_zero = 0;
    for (int i = 0; i < N_FAST; i++) {
        const std::string line = join(stamp_token(), fast_decimal(), fast_decimal(), rnd(2) ? "1" : "0");
        if (line.size() > TEXT_MAX_DEVICE_LINE) {   // (cannot happen: 2 + 20 + 3 + 2 * (3 + 32) + 1 + 2 + 1 bytes at most)
            fprintf(stderr, "generator: fast line of %zu bytes\n", line.size());
            return 2;
        }
        const Ref o = oracle(line);
        const TextRecord r = parse_tight(line, false);
        if (r.status != TEXT_OK) fail("fast line not TEXT_OK", line);
        else if (!equal(r, o)) fail("fast line differs from strtoll / strtod", line);
        if (r.status == TEXT_OK && r.x == 0.0 && std::signbit(r.x)) n_neg_zero++;
        const TextRecord h = parse_tight(line, true);
        if (h.status != TEXT_OK || !equal(h, o)) fail("host parser differs on a fast line", line);
    }
    if (n_neg_zero == 0) fail("no -0 among the fast lines", "");
    // ---- lines that leave the fast class
    const int N_SLOW = 20000;
    for (int i = 0; i < N_SLOW; i++) {
        std::string line;
        const uint64_t kind = rnd(3);
        if (kind == 0) line = join(stamp_token(), slow_decimal(), fast_decimal(), "1");
        else if (kind == 1) line = join(stamp_token(), fast_decimal(), slow_decimal(), "0");
        else {
            line = join(stamp_token(), fast_decimal(), fast_decimal(), "1");
            const std::string pad(TEXT_MAX_DEVICE_LINE + 1 + (size_t) rnd(40), rnd(2) ? ' ' : '\t');
            line = rnd(2) ? pad + line : line.substr(0, line.find_last_not_of("\r") + 1) + pad;
        }
        const Ref o = oracle(line);
        const TextRecord r = parse_tight(line, false);
        if (r.status != TEXT_NEEDS_HOST) fail("line outside the fast class not TEXT_NEEDS_HOST", line);
        const TextRecord h = parse_tight(line, true);
        if (h.status != TEXT_OK || !equal(h, o)) fail("host parser differs from strtoll / strtod", line);
    }
    // ---- malformed lines
    const char *bad[] = {"1 2 3",                          // 3 fields
                         "1 2 3 1 5",                      // 5 fields
                         "1 2 3 2",                        // polarity 2
                         "12.5 1 2 1",                     // stamp 12.5
                         "9223372036854775808 1 2 1",      // stamp beyond int64
                         "1 1e 2 1",                       // an empty exponent
                         "1 - 2 1",                        // a lone '-'
                         "-9223372036854775809 1 2 0", "1 2 3 01", "1 2 3 +1", "1 0x10 2 1", "1 inf 2 1", "1 2 nan 1", "1 . 2 1", "1 1e+ 2 1",
                         "+ 1 2 1", "1 2\r 3 1", "1 2 3 1\r\r", "1 1.2.3 2 1", "1 2 3e1.5 1", "1,2,3,1", "1 2 3 1 \v",
                         "99999999999999999999 1 2 1", "1 1e5x 2 1", "1 --1 2 1"};
    for (const char *b : bad) {
        if (parse_tight(b, false).status != TEXT_MALFORMED) fail("not TEXT_MALFORMED (kernel's parser)", b);
        if (parse_tight(b, true).status != TEXT_MALFORMED) fail("not TEXT_MALFORMED (host parser)", b);
        const std::string lng = std::string(b) + std::string(TEXT_MAX_DEVICE_LINE, ' ');   // over-long: the host decides
        if (parse_tight(lng, false).status != TEXT_NEEDS_HOST) fail("over-long line not TEXT_NEEDS_HOST", b);
        if (parse_tight(lng, true).status != TEXT_MALFORMED) fail("over-long malformed line not TEXT_MALFORMED on the host", b);
    }
    // ---- blank lines, and the ends of the stamp's range
    const char *blank[] = {"", " ", "\t", "\r", "  \t \r", " \r "};
    for (const char *b : blank) {
        if (parse_tight(b, false).status != TEXT_BLANK) fail("not TEXT_BLANK (kernel's parser)", b);
        if (parse_tight(b, true).status != TEXT_BLANK) fail("not TEXT_BLANK (host parser)", b);
    }
    {
        const TextRecord lo = parse_tight("-9223372036854775808 .5 5. 0", false), hi = parse_tight("+9223372036854775807 -.5e1 1E0 1", false);
        if (lo.status != TEXT_OK || lo.stamp != INT64_MIN || lo.x != 0.5 || lo.y != 5.0 || lo.p != 0) fail("INT64_MIN line", "");
        if (hi.status != TEXT_OK || hi.stamp != INT64_MAX || hi.x != -5.0 || hi.y != 1.0 || hi.p != 1) fail("INT64_MAX line", "");
    }
    // ---- the filter's classes
    {
        double t;
        const double inf = 1.0 / 0.0;
        if (text_classify(7, 5, 1e-6, -inf, 0, 0.0, &t) != TEXT_CLASS_KEEP || t != 2 * 1e-6) fail("classify keep", "");
        if (text_classify(4, 5, 1e-6, -inf, 0, 0.0, &t) != TEXT_CLASS_NEGATIVE) fail("classify negative", "");
        if (text_classify(5, 5, 1e-6, 1e-6, 0, 0.0, &t) != TEXT_CLASS_BEFORE_START) fail("classify before start", "");
        if (text_classify(9, 5, 1e-6, 1.0, 1, 4e-6, &t) != TEXT_CLASS_STOP) fail("classify stop (before the start test)", "");
        if (text_classify(8, 5, 1e-6, -inf, 1, 4e-6, &t) != TEXT_CLASS_KEEP) fail("classify below the end", "");
    }
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("%d lines equal, %d lines for the host, %zu malformed, %ld negative zeros\n", N_FAST, N_SLOW, sizeof(bad) / sizeof(bad[0]), n_neg_zero);
    return 0;
}
