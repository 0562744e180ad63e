// Prophesee EVT3 (16-bit words) and EVT2 (32-bit words) payloads into events — one restatement of include/ecal.h, "raw ingest",
// for the kernels (ecal_raw.hip), the host decoder (EventStream::raw2bin, host/event.hpp) and the CPU test
// (tests/cpp/check_raw_decode.cpp).
//
// Both encodings are stateful streams.  The decoder's state in front of a word is the SUMMARY of all the words before it, and
// summaries form a monoid: summary(u ++ v) = combine(summary(u), summary(v)), identity() for no words.  So
//   sequential:  state = identity(); for every word { emit(state, word); state = combine(state, of_word(word)); }
//   block-wise:  summaries of blocks, an exclusive scan of them with combine, then every block decoded from its incoming state
// give the same events.  What a summary holds:
//   EVT3   y:         the last ADDR_Y, or none
//          low:       the last TIME_LOW, or none (an event's low is 0 until the first one)
//          time high: none, or {first, last, wraps inside}; combine counts the wrap between a.last and b.first
//          base:      "set: x behind the words, vector polarity", or "advance by k" (no VECT_BASE_X among the words: the advances
//                     of VECT_12 / VECT_8 add up until a set is met; without any set in front they mean nothing)
//   EVT2   the last TIME_HIGH, or none
// Nothing here is floating point but raw_classify's one conversion and one multiplication (no a * b + c to contract; the
// translation units that include this are built with -ffp-contract=off all the same).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "event_record.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_RAW_HD __host__ __device__ __forceinline__   // (not inlined, a summary passed by reference lives in scratch memory)
#else
#define ECAL_RAW_HD inline
#endif

namespace ecal_raw {

enum : int { RAW_FORMAT_NONE = 0, RAW_FORMAT_EVT2 = 2, RAW_FORMAT_EVT3 = 3 };   // ECAL_RAW_AUTO / _EVT2 / _EVT3 of ecal.h

ECAL_RAW_HD uint32_t raw_popcount(uint32_t v) {
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
}

// one decoded event in front of the filter; valid = 0: a piece of state was missing (dropped as n_no_state)
struct RawEvent {
    int64_t t_us;
    uint32_t x, y;
    uint8_t pol, valid;
};

// ---- EVT3 ---------------------------------------------------------------------------------------------------------------------------
struct Evt3Summary {   // 20 bytes: five 32-bit words for the shuffles of the scans
    uint16_t y, low;              // 0xFFFF: none
    uint16_t th_first, th_last;   // 0xFFFF: no TIME_HIGH
    uint32_t wraps;
    uint32_t base;                // base_flags & 1: x behind the words; else the advance
    uint32_t base_flags;          // bit 0: set, bit 1: vector polarity
};

struct Evt3 {
    typedef uint16_t Word;
    typedef Evt3Summary Summary;
    static constexpr int FORMAT = RAW_FORMAT_EVT3;
    static constexpr uint32_t WORD_BYTES = 2;
    static constexpr uint16_t NONE = 0xFFFFu;

    ECAL_RAW_HD static Summary identity() { return Summary{NONE, NONE, NONE, NONE, 0u, 0u, 0u}; }
    // one wrap between consecutive TIME_HIGH values p then q: a backward step of more than 2048
    ECAL_RAW_HD static uint32_t wrap(uint32_t p, uint32_t q) { return (q < p && p - q > 2048u) ? 1u : 0u; }

    ECAL_RAW_HD static Summary of_word(Word w) {
        Summary s = identity();
        const uint16_t v11 = (uint16_t) (w & 0x7FFu), v12 = (uint16_t) (w & 0xFFFu);
        switch (w >> 12) {
            case 0x0: s.y = v11; break;
            case 0x3: s.base = v11; s.base_flags = 1u | ((uint32_t) ((w >> 11) & 1u) << 1); break;
            case 0x4: s.base = 12u; break;
            case 0x5: s.base = 8u; break;
            case 0x6: s.low = v12; break;
            case 0x8: s.th_first = s.th_last = v12; break;
            default: break;
        }
        return s;
    }
    ECAL_RAW_HD static Summary combine(const Summary &a, const Summary &b) {
        Summary r;
        r.y = b.y != NONE ? b.y : a.y;
        r.low = b.low != NONE ? b.low : a.low;
        if (a.th_first == NONE) {
            r.th_first = b.th_first; r.th_last = b.th_last; r.wraps = a.wraps + b.wraps;
        } else if (b.th_first == NONE) {
            r.th_first = a.th_first; r.th_last = a.th_last; r.wraps = a.wraps + b.wraps;
        } else {
            r.th_first = a.th_first; r.th_last = b.th_last; r.wraps = a.wraps + b.wraps + wrap(a.th_last, b.th_first);
        }
        if (b.base_flags & 1u) {
            r.base = b.base; r.base_flags = b.base_flags;
        } else {
            r.base = a.base + b.base; r.base_flags = a.base_flags;
        }
        return r;
    }
    ECAL_RAW_HD static uint32_t wraps(const Summary &s) { return s.wraps; }
    // events the word emits, whatever the state
    ECAL_RAW_HD static uint32_t count(Word w) {
        const uint32_t t = w >> 12;
        return t == 0x2 ? 1u : t == 0x4 ? raw_popcount(w & 0xFFFu) : t == 0x5 ? raw_popcount(w & 0xFFu) : 0u;
    }
    ECAL_RAW_HD static bool is_other(Word w) {
        const uint32_t t = w >> 12;
        return !(t == 0x0 || t == 0x2 || t == 0x3 || t == 0x4 || t == 0x5 || t == 0x6 || t == 0x8);
    }
    // the word's events with the state `s` in front of it, in order, through put(const RawEvent &)
    template <class Put> ECAL_RAW_HD static void emit(const Summary &s, Word w, Put &&put) {
        const uint32_t t = w >> 12;
        if (t != 0x2 && t != 0x4 && t != 0x5) return;
        RawEvent e;
        e.t_us = (int64_t) (((uint64_t) s.wraps << 24) | ((uint64_t) (s.th_last & 0xFFFu) << 12) | (uint64_t) (s.low == NONE ? 0u : s.low));
        e.y = s.y;
        const bool timed = s.th_first != NONE && s.y != NONE;
        // ADDR_X as a vector of one bit at its own x: one loop, one place where put is called
        const bool single = t == 0x2;
        const uint32_t mask = single ? 1u : t == 0x4 ? (w & 0xFFFu) : (w & 0xFFu), x0 = single ? (w & 0x7FFu) : s.base;
        e.pol = (uint8_t) (single ? (w >> 11) & 1u : (s.base_flags >> 1) & 1u);
        e.valid = (timed && (single || (s.base_flags & 1u))) ? 1 : 0;
        for (uint32_t i = 0; mask >> i; i++) {
            if (mask >> i & 1u) {
                e.x = x0 + i;
                put(e);
            }
        }
    }
};

// ---- EVT2 ---------------------------------------------------------------------------------------------------------------------------
struct Evt2Summary {
    uint32_t high;   // 0xFFFFFFFF: no TIME_HIGH (a value has 28 bits)
};

struct Evt2 {
    typedef uint32_t Word;
    typedef Evt2Summary Summary;
    static constexpr int FORMAT = RAW_FORMAT_EVT2;
    static constexpr uint32_t WORD_BYTES = 4;
    static constexpr uint32_t NONE = 0xFFFFFFFFu;

    ECAL_RAW_HD static Summary identity() { return Summary{NONE}; }
    ECAL_RAW_HD static Summary of_word(Word w) { return Summary{(w >> 28) == 0x8u ? (w & 0x0FFFFFFFu) : NONE}; }
    ECAL_RAW_HD static Summary combine(const Summary &a, const Summary &b) { return b.high != NONE ? b : a; }
    ECAL_RAW_HD static uint32_t wraps(const Summary &) { return 0u; }   // no wrap handling: 2^34 us are 4.7 h
    ECAL_RAW_HD static uint32_t count(Word w) { return (w >> 28) <= 0x1u ? 1u : 0u; }
    ECAL_RAW_HD static bool is_other(Word w) { return (w >> 28) > 0x1u && (w >> 28) != 0x8u; }
    template <class Put> ECAL_RAW_HD static void emit(const Summary &s, Word w, Put &&put) {
        if ((w >> 28) > 0x1u) return;
        RawEvent e;
        e.t_us = (int64_t) (((uint64_t) (s.high & 0x0FFFFFFFu) << 6) | (uint64_t) ((w >> 22) & 0x3Fu));
        e.x = (w >> 11) & 0x7FFu;
        e.y = w & 0x7FFu;
        e.pol = (uint8_t) (w >> 28);
        e.valid = s.high != NONE ? 1 : 0;
        put(e);
    }
};

// a decode block of the kernels: 256 threads x one 128-bit load (ecal_raw_block_words)
constexpr uint32_t RAW_BLOCK_THREADS = 256;
template <class F> constexpr uint32_t raw_block_words() { return RAW_BLOCK_THREADS * 16u / F::WORD_BYTES; }

// ---- conversion and filter ----------------------------------------------------------------------------------------------------------
struct RawFilter {
    int64_t time_base;
    uint32_t width, height;   // 0: no bound
    double start_time;
    int has_end_time;
    double end_time;
};

enum : uint8_t { RAW_CLASS_KEEP = 0, RAW_CLASS_NO_STATE = 1, RAW_CLASS_OUTSIDE = 2, RAW_CLASS_NEGATIVE = 3, RAW_CLASS_BEFORE_START = 4, RAW_CLASS_STOP = 5 };

ECAL_RAW_HD uint8_t raw_classify(const RawEvent &e, const RawFilter &f, double *t_out) {
    if (!e.valid) return RAW_CLASS_NO_STATE;
    if ((f.width && e.x >= f.width) || (f.height && e.y >= f.height)) return RAW_CLASS_OUTSIDE;
    const int64_t d = (int64_t) ((uint64_t) e.t_us - (uint64_t) f.time_base);
    const double t = (double) d * 1e-6;   // one subtraction, one conversion, one multiplication
    *t_out = t;
    if (t < 0) return RAW_CLASS_NEGATIVE;
    if (f.has_end_time && t >= f.end_time) return RAW_CLASS_STOP;
    return t >= f.start_time ? RAW_CLASS_KEEP : RAW_CLASS_BEFORE_START;
}

ECAL_RAW_HD uint32_t raw_load_word(const uint8_t *p, uint16_t) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8); }
ECAL_RAW_HD uint32_t raw_load_word(const uint8_t *p, uint32_t) {
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}

// the counters of one decode (ecal_raw_info's, without the header's)
struct RawCounts {
    uint64_t n_words, n_raw_events, n_events, n_no_state, n_outside, n_negative, n_before_start, n_after_end, n_other_words,
        n_trailing_bytes, n_time_wraps;
};

// Words [w0, w1) of the payload decoded from the state `s` in front of word w0 (advanced to the state behind word w1 - 1):
// every event to on_event(const RawEvent &)
template <class F, class OnEvent>
inline void raw_decode_words(const uint8_t *payload, uint64_t w0, uint64_t w1, typename F::Summary &s, OnEvent &&on_event) {
    for (uint64_t k = w0; k < w1; k++) {
        const typename F::Word w = (typename F::Word) raw_load_word(payload + k * F::WORD_BYTES, typename F::Word());
        F::emit(s, w, on_event);
        s = F::combine(s, F::of_word(w));
    }
}

template <class F> inline typename F::Summary raw_summarize_words(const uint8_t *payload, uint64_t w0, uint64_t w1, uint64_t *n_other) {
    typename F::Summary s = F::identity();
    for (uint64_t k = w0; k < w1; k++) {
        const typename F::Word w = (typename F::Word) raw_load_word(payload + k * F::WORD_BYTES, typename F::Word());
        s = F::combine(s, F::of_word(w));
        if (n_other && F::is_other(w)) (*n_other)++;
    }
    return s;
}

// The filter in file order over a stream of events: counts into c, the kept ones to put(const uint8_t rec[25]).  The first event
// that reaches end_time ends the stream: it and every event behind it count as n_after_end and nothing else.
template <class PutRecord> struct RawSink {
    const RawFilter &f;
    RawCounts &c;
    PutRecord &put;
    bool stopped = false;
    RawSink(const RawFilter &f_, RawCounts &c_, PutRecord &put_) : f(f_), c(c_), put(put_) {}
    void operator()(const RawEvent &e) {
        c.n_raw_events++;
        if (stopped) {
            c.n_after_end++;
            return;
        }
        double t = 0;
        switch (raw_classify(e, f, &t)) {
            case RAW_CLASS_NO_STATE: c.n_no_state++; break;
            case RAW_CLASS_OUTSIDE: c.n_outside++; break;
            case RAW_CLASS_NEGATIVE: c.n_negative++; break;
            case RAW_CLASS_BEFORE_START: c.n_before_start++; break;
            case RAW_CLASS_STOP: stopped = true; c.n_after_end++; break;
            default: {
                uint8_t rec[25];
                ecal::pack_record(rec, t, (double) e.x, (double) e.y, e.pol);
                put(rec);
                c.n_events++;
            }
        }
    }
};

// The plain sequential decoder: word by word from the identity state
template <class F, class PutRecord>
inline void raw_decode_sequential(const uint8_t *payload, uint64_t n_bytes, const RawFilter &f, RawCounts &c, PutRecord &&put) {
    memset(&c, 0, sizeof(c));
    c.n_words = n_bytes / F::WORD_BYTES;
    c.n_trailing_bytes = n_bytes % F::WORD_BYTES;
    RawSink<PutRecord> sink(f, c, put);
    typename F::Summary s = F::identity();
    raw_decode_words<F>(payload, 0, c.n_words, s, sink);
    (void) raw_summarize_words<F>(payload, 0, c.n_words, &c.n_other_words);
    c.n_time_wraps = F::wraps(s);
}

// The same block by block, as the kernels do it: the blocks' summaries, their exclusive scan, every block from its incoming state
template <class F, class PutRecord>
inline void raw_decode_blockwise(const uint8_t *payload, uint64_t n_bytes, uint64_t block_words, const RawFilter &f, RawCounts &c,
                                 PutRecord &&put) {
    memset(&c, 0, sizeof(c));
    c.n_words = n_bytes / F::WORD_BYTES;
    c.n_trailing_bytes = n_bytes % F::WORD_BYTES;
    const uint64_t nb = (c.n_words + block_words - 1) / block_words;
    typename F::Summary *in = new typename F::Summary[nb + 1];
    typename F::Summary run = F::identity();
    for (uint64_t b = 0; b < nb; b++) {
        const uint64_t w0 = b * block_words, w1 = w0 + block_words < c.n_words ? w0 + block_words : c.n_words;
        in[b] = run;
        run = F::combine(run, raw_summarize_words<F>(payload, w0, w1, &c.n_other_words));
    }
    c.n_time_wraps = F::wraps(run);
    RawSink<PutRecord> sink(f, c, put);
    for (uint64_t b = 0; b < nb; b++) {
        const uint64_t w0 = b * block_words, w1 = w0 + block_words < c.n_words ? w0 + block_words : c.n_words;
        typename F::Summary s = in[b];
        raw_decode_words<F>(payload, w0, w1, s, sink);
    }
    delete[] in;
}

// ---- file header --------------------------------------------------------------------------------------------------------------------
// The maximal run of lines that begin with '%' at the start of `data` (the first n bytes of the file; whole_file: these are all of
// it).  "% end" closes it.  *format = the first of "% evt 3.0" / "% evt 2.0" / "% format EVT3|EVT2[;...]", or RAW_FORMAT_NONE.
// false: the header does not end within the n bytes.
inline bool raw_parse_header(const uint8_t *data, size_t n, bool whole_file, int *format, uint64_t *header_bytes) {
    *format = RAW_FORMAT_NONE;
    size_t pos = 0;
    while (pos < n && data[pos] == '%') {
        const void *nl = memchr(data + pos, '\n', n - pos);
        if (!nl && !whole_file) return false;
        const size_t end = nl ? (size_t) ((const uint8_t *) nl - data) : n, len = end - pos;
        const char *ln = (const char *) data + pos;
        pos = nl ? end + 1 : n;
        auto is = [&](const char *s) { return len == strlen(s) && memcmp(ln, s, len) == 0; };
        auto starts = [&](const char *s) { return len >= strlen(s) && memcmp(ln, s, strlen(s)) == 0 && (len == strlen(s) || ln[strlen(s)] == ';'); };
        if (*format == RAW_FORMAT_NONE) {
            if (is("% evt 3.0") || starts("% format EVT3")) *format = RAW_FORMAT_EVT3;
            else if (is("% evt 2.0") || starts("% format EVT2")) *format = RAW_FORMAT_EVT2;
        }
        if (is("% end")) break;
    }
    *header_bytes = pos;
    return true;
}

}  // namespace ecal_raw
