// CPU check of the raw decoders (eventcalib_amd/csrc/raw_events.hpp: the word step, the summary monoid and the filter the
// kernels of ecal_raw.hip and EventStream::raw2bin call).  Per format, 2 000 seeded random word streams of 0 - 4 000 words — all word
// types occur, TIME_HIGH is weighted up in a third of the streams so that wraps occur, a random filter (sensor bounds, time base,
// start and end time) on each — are decoded
//   - by a plain decoder of this file's own that keeps the contract's state in plain variables (include/ecal.h, "raw ingest"),
//   - by raw_decode_sequential (the step from the identity state),
//   - by raw_decode_blockwise (summaries, their scan with combine, every block from its incoming state) with blocks of 1, 2, 7, 64
//     words and of the kernels' block (raw_block_words),
// and the records, the drop counts and the wrap counts must be identical across all of them.  Then the header parser's cases.
// Built twice by tests/test_raw_decode_host.py: plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "raw_events.hpp"

using namespace ecal_raw;

namespace {

std::mt19937_64 rng(20240917);
uint64_t rnd(uint64_t n) { return rng() % n; }   // [0, n)

struct Decoded {
    std::vector<uint8_t> records;
    RawCounts c;
};

bool same(const Decoded &a, const Decoded &b) { return a.records == b.records && memcmp(&a.c, &b.c, sizeof(RawCounts)) == 0; }

// the filter of the contract on one event of the plain decoders below
struct Plain {
    const RawFilter &f;
    Decoded &d;
    bool stopped = false;
    Plain(const RawFilter &f_, Decoded &d_) : f(f_), d(d_) { memset(&d.c, 0, sizeof(d.c)); }
    void event(bool has_state, int64_t t_us, uint32_t x, uint32_t y, uint8_t pol) {
        d.c.n_raw_events++;
        if (stopped) { d.c.n_after_end++; return; }
        if (!has_state) { d.c.n_no_state++; return; }
        if ((f.width && x >= f.width) || (f.height && y >= f.height)) { d.c.n_outside++; return; }
        const double t = (double) (t_us - f.time_base) * 1e-6;
        if (t < 0) { d.c.n_negative++; return; }
        if (f.has_end_time && t >= f.end_time) { stopped = true; d.c.n_after_end++; return; }
        if (!(t >= f.start_time)) { d.c.n_before_start++; return; }
        const double xd = (double) x, yd = (double) y;
        uint8_t rec[25];
        memcpy(rec, &t, 8);
        memcpy(rec + 8, &xd, 8);
        memcpy(rec + 16, &yd, 8);
        rec[24] = pol;
        d.records.insert(d.records.end(), rec, rec + 25);
        d.c.n_events++;
    }
};

Decoded plain_evt3(const std::vector<uint8_t> &bytes, const RawFilter &f) {
    Decoded d;
    Plain out(f, d);
    d.c.n_words = bytes.size() / 2;
    d.c.n_trailing_bytes = bytes.size() % 2;
    bool has_y = false, has_high = false, has_base = false;
    uint32_t y = 0, high = 0, low = 0, base_x = 0, vpol = 0;
    uint64_t wraps = 0;
    for (uint64_t k = 0; k < d.c.n_words; k++) {
        const uint32_t w = (uint32_t) bytes[2 * k] | ((uint32_t) bytes[2 * k + 1] << 8), type = w >> 12;
        const int64_t t_us = (int64_t) ((wraps << 24) | ((uint64_t) high << 12) | low);
        if (type == 0x0) {
            y = w & 0x7FF;
            has_y = true;
        } else if (type == 0x2) {
            out.event(has_y && has_high, t_us, w & 0x7FF, y, (uint8_t) ((w >> 11) & 1));
        } else if (type == 0x3) {
            base_x = w & 0x7FF;
            vpol = (w >> 11) & 1;
            has_base = true;
        } else if (type == 0x4 || type == 0x5) {
            const uint32_t nbits = type == 0x4 ? 12 : 8;
            for (uint32_t i = 0; i < nbits; i++)
                if (w >> i & 1) out.event(has_y && has_high && has_base, t_us, base_x + i, y, (uint8_t) vpol);
            if (has_base) base_x += nbits;
        } else if (type == 0x6) {
            low = w & 0xFFF;
        } else if (type == 0x8) {
            const uint32_t q = w & 0xFFF;
            if (has_high && q < high && high - q > 2048) wraps++;
            high = q;
            has_high = true;
        } else {
            d.c.n_other_words++;
        }
    }
    d.c.n_time_wraps = wraps;
    return d;
}

Decoded plain_evt2(const std::vector<uint8_t> &bytes, const RawFilter &f) {
    Decoded d;
    Plain out(f, d);
    d.c.n_words = bytes.size() / 4;
    d.c.n_trailing_bytes = bytes.size() % 4;
    bool has_high = false;
    uint64_t high = 0;
    for (uint64_t k = 0; k < d.c.n_words; k++) {
        uint32_t w;
        memcpy(&w, bytes.data() + 4 * k, 4);   // (the test runs on little-endian hosts, as the library's record layout assumes)
        const uint32_t type = w >> 28;
        if (type <= 1) out.event(has_high, (int64_t) ((high << 6) | ((w >> 22) & 0x3F)), (w >> 11) & 0x7FF, w & 0x7FF, (uint8_t) type);
        else if (type == 0x8) { high = w & 0x0FFFFFFF; has_high = true; }
        else d.c.n_other_words++;
    }
    return d;
}

template <class F> Decoded sequential(const std::vector<uint8_t> &bytes, const RawFilter &f) {
    Decoded d;
    raw_decode_sequential<F>(bytes.data(), bytes.size(), f, d.c, [&](const uint8_t *rec) { d.records.insert(d.records.end(), rec, rec + 25); });
    return d;
}

template <class F> Decoded blockwise(const std::vector<uint8_t> &bytes, uint64_t block_words, const RawFilter &f) {
    Decoded d;
    raw_decode_blockwise<F>(bytes.data(), bytes.size(), block_words, f, d.c,
                            [&](const uint8_t *rec) { d.records.insert(d.records.end(), rec, rec + 25); });
    return d;
}

void put_word(std::vector<uint8_t> &b, uint32_t w, int n) {
    for (int i = 0; i < n; i++) b.push_back((uint8_t) (w >> (8 * i)));
}

std::vector<uint8_t> random_evt3(bool many_highs) {
    std::vector<uint8_t> b;
    const uint64_t n = rnd(4001);
    // the first state words late in some streams, so that no-state drops occur
    const uint64_t quiet = rnd(4) == 0 ? rnd(60) : 0;
    uint32_t high = (uint32_t) rnd(4096);
    for (uint64_t k = 0; k < n; k++) {
        uint32_t type;
        const uint64_t r = rnd(100);
        if (k < quiet) type = r < 50 ? 0x2 : r < 75 ? 0x4 : 0x5;
        else if (many_highs && r < 35) type = 0x8;
        else if (r < 4) type = 0x8;
        else if (r < 14) type = 0x6;
        else if (r < 24) type = 0x0;
        else if (r < 32) type = 0x3;
        else if (r < 60) type = 0x2;
        else if (r < 75) type = 0x4;
        else if (r < 88) type = 0x5;
        else type = (uint32_t) rnd(16);   // every type, the skipped ones among them
        uint32_t payload = (uint32_t) rnd(4096);
        if (type == 0x8) {   // mostly forward steps, some wraps, some small backward steps, the two edges of the rule
            const uint64_t s = rnd(20);
            if (s < 12) high = (high + (uint32_t) rnd(40)) & 0xFFF;
            else if (s < 15) high = (uint32_t) rnd(4096);
            else if (s < 17) high = high >= 2048 ? high - 2048 : high;
            else if (s < 19) high = high >= 2049 ? high - 2049 : high;
            payload = high;
        }
        put_word(b, (type << 12) | payload, 2);
    }
    if (rnd(3) == 0) b.push_back((uint8_t) rnd(256));
    return b;
}

std::vector<uint8_t> random_evt2(bool many_highs) {
    std::vector<uint8_t> b;
    const uint64_t n = rnd(4001);
    const uint64_t quiet = rnd(4) == 0 ? rnd(60) : 0;
    uint32_t high = (uint32_t) rnd(1u << 20);
    for (uint64_t k = 0; k < n; k++) {
        uint32_t type;
        const uint64_t r = rnd(100);
        if (k < quiet) type = (uint32_t) rnd(2);
        else if (r < (many_highs ? 35u : 5u)) type = 0x8;
        else if (r < 90) type = (uint32_t) rnd(2);
        else type = (uint32_t) rnd(16);
        uint32_t payload = (uint32_t) rnd(1u << 28);
        if (type == 0x8) {
            high = rnd(10) ? (high + (uint32_t) rnd(3)) & 0x0FFFFFFF : (uint32_t) rnd(1u << 28);
            payload = high;
        }
        put_word(b, (type << 28) | payload, 4);
    }
    const uint64_t tail = rnd(3) == 0 ? 1 + rnd(3) : 0;
    for (uint64_t i = 0; i < tail; i++) b.push_back((uint8_t) rnd(256));
    return b;
}

RawFilter random_filter(int64_t t_span_us) {
    RawFilter f{0, 0, 0, -INFINITY, 0, 0.0};
    if (rnd(2)) { f.width = 1 + (uint32_t) rnd(2100); f.height = 1 + (uint32_t) rnd(2048); }
    if (rnd(3) == 0) f.time_base = (int64_t) rnd((uint64_t) t_span_us);
    if (rnd(3) == 0) f.start_time = 1e-6 * (double) rnd((uint64_t) t_span_us);
    if (rnd(3) == 0) { f.has_end_time = 1; f.end_time = 1e-6 * (double) rnd((uint64_t) t_span_us); }
    return f;
}

template <class F> int check_format(const char *name, std::vector<uint8_t> (*make)(bool), Decoded (*plain)(const std::vector<uint8_t> &, const RawFilter &),
                                    int64_t t_span_us) {
    const uint64_t sizes[5] = {1, 2, 7, 64, raw_block_words<F>()};
    uint64_t events = 0, wraps = 0, no_state = 0, stopped = 0;
    for (int s = 0; s < 2000; s++) {
        const std::vector<uint8_t> bytes = make(s % 3 == 0);
        const RawFilter f = random_filter(t_span_us);
        const Decoded want = plain(bytes, f);
        const Decoded seq = sequential<F>(bytes, f);
        if (!same(want, seq)) {
            std::printf("%s stream %d: the sequential decoder differs from the plain one (%llu vs %llu records)\n", name, s,
                        (unsigned long long) seq.c.n_events, (unsigned long long) want.c.n_events);
            return 1;
        }
        for (uint64_t bw : sizes) {
            if (!same(want, blockwise<F>(bytes, bw, f))) {
                std::printf("%s stream %d: blocks of %llu words differ\n", name, s, (unsigned long long) bw);
                return 1;
            }
        }
        events += want.c.n_events;
        wraps += want.c.n_time_wraps;
        no_state += want.c.n_no_state;
        stopped += want.c.n_after_end ? 1 : 0;
    }
    std::printf("%s: 2000 streams equal (%llu records, %llu wraps, %llu events without state, %llu streams ended early)\n", name,
                (unsigned long long) events, (unsigned long long) wraps, (unsigned long long) no_state, (unsigned long long) stopped);
    // the test means nothing if the generator never reaches these
    return (events > 100000 && no_state > 100 && stopped > 100 && (F::FORMAT != RAW_FORMAT_EVT3 || wraps > 1000)) ? 0 : 1;
}

int check_headers() {
    struct Case { std::string text; bool whole; bool ok; int format; uint64_t bytes; };
    const std::string p = "\x12\x34";
    const Case cases[] = {
        {"% evt 3.0\n" + p, true, true, RAW_FORMAT_EVT3, 10},
        {"% evt 2.0\n% end\n" + p, true, true, RAW_FORMAT_EVT2, 16},
        {"% camera x\n% format EVT3\n" + p, true, true, RAW_FORMAT_EVT3, 25},
        {"% format EVT2;height=720;width=1280\n% end\n" + p, true, true, RAW_FORMAT_EVT2, 42},
        {"% format EVT3\n% end\n% evt 2.0\n", true, true, RAW_FORMAT_EVT3, 20},     // "% end" closes it: the third line is payload
        {"% format EVT33\n" + p, true, true, RAW_FORMAT_NONE, 15},
        {"% date 2024\n" + p, true, true, RAW_FORMAT_NONE, 12},
        {p, true, true, RAW_FORMAT_NONE, 0},
        {"", true, true, RAW_FORMAT_NONE, 0},
        {"% evt 3.0", true, true, RAW_FORMAT_EVT3, 9},                               // a last line without its line break
        {"% evt 3.0", false, false, RAW_FORMAT_NONE, 0},                             // ... in a buffer that is not the whole file
    };
    int n = 0;
    for (const Case &c : cases) {
        int format = -1;
        uint64_t bytes = ~0ull;
        const bool ok = raw_parse_header((const uint8_t *) c.text.data(), c.text.size(), c.whole, &format, &bytes);
        if (ok != c.ok || (ok && (format != c.format || bytes != c.bytes))) {
            std::printf("header case %d: ok %d format %d bytes %llu\n", n, (int) ok, format, (unsigned long long) bytes);
            return 1;
        }
        n++;
    }
    std::printf("headers: %d cases\n", n);
    return 0;
}

}  // namespace

int main() {
    if (check_format<Evt3>("EVT3", random_evt3, plain_evt3, 1ll << 26)) return 1;
    if (check_format<Evt2>("EVT2", random_evt2, plain_evt2, 1ll << 28)) return 1;
    return check_headers();
}
