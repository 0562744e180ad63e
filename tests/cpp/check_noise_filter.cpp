// CPU check of eventcalib_amd/csrc/noise_filter.hpp (tests/test_noise_filter_host.py builds and runs it, plainly and under
// AddressSanitizer + UndefinedBehaviorSanitizer): what the kernels of ecal_noise.hip and ecal_noise_verdict_host decide with.
//   streams  nf_verdict_indexed (the kernels' scheme: keys, a stable sort, the start table, a binary search per neighbour pixel)
//            against nf_verdict_sequential (the rule as it is stated) on 1200 seeded random streams: grids from 1 x 1 to 40 x 30,
//            stamps quantised to a handful of values, sorted and shuffled, dt in {0, small, +inf}, every radius, both include_self
//            values, min_support in {1, 2, 8, 9, 49}, off-grid, NaN-coordinate and NaN-stamp events mixed in
//   known    two events on adjacent pixels exactly dt apart and one ulp further; the same pixel twice with include_self 0 and 1; a
//            1 x 1 sensor; corner pixels; the square's clipping; the key bits; the search on empty and one-entry lists
//   options  what nf_options_error refuses
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <limits>
#include <random>
#include <vector>
#include "noise_filter.hpp"

using namespace ecal_noise;

static int g_wrong = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            if (g_wrong++ < 20) printf("line %d: %s\n", __LINE__, #cond); \
        }                                                               \
    } while (0)

static const double INF = std::numeric_limits<double>::infinity(), QNAN = std::numeric_limits<double>::quiet_NaN();

static void put_record(uint8_t *r, double t, double x, double y, uint8_t pol) {
    memcpy(r, &t, 8);
    memcpy(r + 8, &x, 8);
    memcpy(r + 16, &y, 8);
    r[24] = pol;
}

struct Ev {
    double t, x, y;
};

static std::vector<uint8_t> pack(const std::vector<Ev> &ev) {
    std::vector<uint8_t> rec(ev.size() * PA_RECORD_BYTES + 1);   // (one spare byte: an empty stream still has an address)
    for (size_t i = 0; i < ev.size(); i++) put_record(rec.data() + i * PA_RECORD_BYTES, ev[i].t, ev[i].x, ev[i].y, (uint8_t) (i & 1));
    return rec;
}

// both forms on one stream; returns the sequential verdicts
static std::vector<uint8_t> both(const std::vector<Ev> &ev, const NoiseOptions &o, FilterTotals *tot = nullptr) {
    CHECK(nf_options_error(o) == nullptr);
    const std::vector<uint8_t> rec = pack(ev);
    std::vector<uint8_t> a(ev.size() + 1, 0xAA), b(ev.size() + 1, 0xBB);
    const FilterTotals ta = nf_verdict_sequential(rec.data(), ev.size(), o, a.data());
    const FilterTotals tb = nf_verdict_indexed(rec.data(), ev.size(), o, b.data());
    CHECK(a[ev.size()] == 0xAA && b[ev.size()] == 0xBB);   // nothing behind the verdicts is written
    a.resize(ev.size());
    b.resize(ev.size());
    CHECK(a == b);
    CHECK(ta.n_events == ev.size() && ta.n_events == tb.n_events && ta.n_off_grid == tb.n_off_grid && ta.n_removed == tb.n_removed &&
          ta.n_kept == tb.n_kept && ta.n_kept + ta.n_removed == ta.n_events);
    uint64_t kept = 0;
    for (uint8_t v : a) {
        CHECK(v <= 1);
        kept += v;
    }
    CHECK(kept == ta.n_kept);
    // the compaction by these verdicts: the kept records' own bytes in input order, nothing behind them written
    std::vector<uint8_t> out(ev.size() * PA_RECORD_BYTES + 1, 0xCC);
    CHECK(nf_compact(rec.data(), ev.size(), a.data(), out.data()) == kept);
    size_t at = 0;
    for (size_t i = 0; i < ev.size(); i++)
        if (a[i]) {
            CHECK(memcmp(out.data() + at * PA_RECORD_BYTES, rec.data() + i * PA_RECORD_BYTES, PA_RECORD_BYTES) == 0);
            at++;
        }
    for (size_t k = kept * PA_RECORD_BYTES; k < out.size(); k++) CHECK(out[k] == 0xCC);
    if (tot) *tot = ta;
    return a;
}

// ---- streams -----------------------------------------------------------------------------------------------------------------------------------
static int check_streams() {
    const uint32_t supports[] = {1, 2, 8, 9, 49};
    const double off_kinds[] = {QNAN, INF, -INF, -1.0, 0.5, -0.5, 9007199254740992.0, -4.9e-324, 1e-300};
    int n_streams = 0;
    uint64_t n_kept = 0, n_removed = 0, n_off = 0;
    for (uint32_t seed = 0; seed < 1200; seed++) {
        std::mt19937_64 rng(seed * 7919u + 13u);
        auto below = [&](uint32_t n) { return (uint32_t) (rng() % n); };
        NoiseOptions o = nf_default_options();
        o.width = seed % 60 == 0 ? 1 : 1 + below(40);
        o.height = seed % 60 == 0 ? 1 : 1 + below(30);
        if (seed % 7 == 3) o.width = 1 + below(4), o.height = 1 + below(4);   // (long lists: many events per pixel)
        o.radius = 1 + seed % 3;
        o.include_self = (seed / 3) % 2;
        o.min_support = supports[(seed / 6) % 5];
        const double step = 0.001;
        o.dt = (seed / 30) % 3 == 0 ? 0.0 : (seed / 30) % 3 == 1 ? step * (double) (1 + below(3)) : INF;
        const uint32_t n = seed % 50 == 0 ? below(3) : 1 + below(400);
        const uint32_t n_values = 1 + below(8);   // the stamps take a handful of values: many are tied
        std::vector<Ev> ev(n);
        for (uint32_t i = 0; i < n; i++) {
            ev[i].t = 5.0 + step * (double) ((uint64_t) i * n_values / (n ? n : 1));   // ascending
            ev[i].x = (double) below(o.width);
            ev[i].y = (double) below(o.height);
        }
        if (seed % 2)   // shuffled: the stamps are not monotone
            for (uint32_t i = n; i > 1; i--) std::swap(ev[i - 1].t, ev[below(i)].t);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t roll = below(100);
            if (roll < 6) ev[i].x = off_kinds[below(9)];
            else if (roll < 12) ev[i].y = off_kinds[below(9)];
            else if (roll < 14) ev[i].x = (double) o.width;
            else if (roll < 16) ev[i].y = (double) o.height;
            else if (roll < 20) ev[i].t = QNAN;
            else if (roll < 21) ev[i].t = below(2) ? INF : -INF;
            else if (roll < 23) ev[i].x = -0.0;
        }
        FilterTotals t;
        both(ev, o, &t);
        n_kept += t.n_kept;
        n_removed += t.n_removed;
        n_off += t.n_off_grid;
        n_streams++;
    }
    CHECK(n_kept > 10000 && n_removed > 10000 && n_off > 10000);   // the streams exercise both verdicts
    printf("streams: %d streams equal (%llu kept, %llu removed, %llu off the grid)\n", n_streams, (unsigned long long) n_kept,
           (unsigned long long) n_removed, (unsigned long long) n_off);
    return n_streams;
}

// ---- known answers ---------------------------------------------------------------------------------------------------------------------------
static int check_known() {
    int n = 0;
    NoiseOptions o = nf_default_options();
    typedef std::vector<uint8_t> V;
    // two events on adjacent pixels exactly dt apart: the second is kept; one ulp further apart: removed
    {
        const double t0 = 5.0, t1 = 5.0 + o.dt;   // (5.005 - 5.0 in f64 is what is compared, so state dt as that difference)
        NoiseOptions e = o;
        e.dt = t1 - t0;
        CHECK(both({{t0, 10, 10}, {t1, 11, 10}}, e) == (V{0, 1}));
        CHECK(both({{t0, 10, 10}, {nextafter(t1, INF), 11, 10}}, e) == (V{0, 0}));
        CHECK(both({{t0, 10, 10}, {t1, 11, 11}}, e) == (V{0, 1}));            // the diagonal neighbour
        CHECK(both({{t0, 10, 10}, {t1, 12, 10}}, e) == (V{0, 0}));            // two pixels away, radius 1
        e.radius = 2;
        CHECK(both({{t0, 10, 10}, {t1, 12, 10}}, e) == (V{0, 1}));
        CHECK(both({{t0, 10, 10}, {t1, 13, 10}}, e) == (V{0, 0}));
        e.radius = 3;
        CHECK(both({{t0, 10, 10}, {t1, 13, 13}}, e) == (V{0, 1}));
        n += 7;
    }
    // the same pixel twice
    {
        NoiseOptions e = o;
        CHECK(both({{5.0, 7, 3}, {5.001, 7, 3}}, e) == (V{0, 0}));
        e.include_self = 1;
        CHECK(both({{5.0, 7, 3}, {5.001, 7, 3}}, e) == (V{0, 1}));
        CHECK(both({{5.0, 7, 3}, {5.001, 7, 3}, {5.1, 7, 3}}, e) == (V{0, 1, 0}));   // the last stamp counts, and it is too old
        n += 3;
    }
    // a 1 x 1 sensor: only the own pixel exists
    {
        NoiseOptions e = o;
        e.width = e.height = 1;
        e.radius = 3;
        CHECK(both({{5.0, 0, 0}, {5.0, 0, 0}, {5.0, 0, 0}}, e) == (V{0, 0, 0}));
        e.include_self = 1;
        CHECK(both({{5.0, 0, 0}, {5.0, 0, 0}, {5.0, 1, 0}, {5.0, -0.0, 0}}, e) == (V{0, 1, 1, 1}));   // (the third is off the grid: kept)
        e.min_support = 2;
        CHECK(both({{5.0, 0, 0}, {5.0, 0, 0}, {5.0, 0, 0}}, e) == (V{0, 0, 0}));   // one pixel supports once
        n += 3;
    }
    // corner pixels: the square is clipped, the corner's three neighbours support it
    {
        NoiseOptions e = o;
        const double W = e.width - 1, H = e.height - 1;
        CHECK(both({{5.0, 1, 0}, {5.0, 0, 1}, {5.0, 1, 1}, {5.0, 0, 0}}, e) == (V{0, 1, 1, 1}));
        e.min_support = 3;
        CHECK(both({{5.0, 1, 0}, {5.0, 0, 1}, {5.0, 1, 1}, {5.0, 0, 0}}, e) == (V{0, 0, 0, 1}));
        CHECK(both({{5.0, W - 1, H}, {5.0, W, H - 1}, {5.0, W - 1, H - 1}, {5.0, W, H}}, e) == (V{0, 0, 0, 1}));
        CHECK(both({{5.0, W - 1, 0}, {5.0, W, 1}, {5.0, W - 1, 1}, {5.0, W, 0}}, e) == (V{0, 0, 0, 1}));
        CHECK(both({{5.0, 1, H}, {5.0, 0, H - 1}, {5.0, 1, H - 1}, {5.0, 0, H}}, e) == (V{0, 0, 0, 1}));
        e.min_support = 4;
        CHECK(both({{5.0, 1, 0}, {5.0, 0, 1}, {5.0, 1, 1}, {5.0, 0, 0}}, e) == (V{0, 0, 0, 0}));
        // across the row end is not a neighbour: (W, 0) and (0, 1) are adjacent in memory only
        e.min_support = 1;
        CHECK(both({{5.0, W, 0}, {5.0, 0, 1}}, e) == (V{0, 0}));
        n += 7;
    }
    // ties, NaN, +inf, an unsorted stream, off-grid events that support nothing
    {
        NoiseOptions e = o;
        e.dt = 0.0;
        CHECK(both({{5.0, 4, 4}, {5.0, 5, 4}, {5.0, 4, 4}}, e) == (V{0, 1, 1}));   // equal stamps support one another in file order
        CHECK(both({{5.0, 4, 4}, {4.0, 5, 4}}, e) == (V{0, 1}));                   // unsorted: the neighbour's stamp lies in the future, 4 - 5 <= 0
        n += 2;
        CHECK(both({{4.0, 4, 4}, {5.0, 5, 4}}, e) == (V{0, 0}));
        e.dt = INF;
        CHECK(both({{4.0, 4, 4}, {5e9, 5, 4}, {QNAN, 4, 5}, {6.0, 5, 5}}, e) == (V{0, 1, 0, 1}));
        CHECK(both({{QNAN, 4, 4}, {5.0, 5, 4}}, e) == (V{0, 0}));                  // a NaN stamp supports nothing
        CHECK(both({{INF, 4, 4}, {INF, 5, 4}}, e) == (V{0, 0}));                   // inf - inf is NaN
        CHECK(both({{5.0, QNAN, 4}, {5.0, 4, 4}, {5.0, 4.5, 4}, {5.0, 5, 4}}, e) == (V{1, 0, 1, 1}));
        n += 5;
    }
    // min_support counts pixels, not events
    {
        NoiseOptions e = o;
        e.min_support = 2;
        CHECK(both({{5.0, 4, 4}, {5.0, 4, 4}, {5.0, 4, 4}, {5.0, 5, 4}}, e) == (V{0, 0, 0, 0}));
        CHECK(both({{5.0, 4, 4}, {5.0, 6, 4}, {5.0, 5, 4}}, e) == (V{0, 0, 1}));
        n += 2;
    }
    // the pieces: the window, the key bits, the search
    uint32_t x0, x1, y0, y1;
    nf_window(0, 259, 3, 346, 260, &x0, &x1, &y0, &y1);
    CHECK(x0 == 0 && x1 == 3 && y0 == 256 && y1 == 259);
    nf_window(0, 0, 3, 1, 1, &x0, &x1, &y0, &y1);
    CHECK(x0 == 0 && x1 == 0 && y0 == 0 && y1 == 0);
    nf_window(4095, 2, 1, 4096, 4096, &x0, &x1, &y0, &y1);
    CHECK(x0 == 4094 && x1 == 4095 && y0 == 1 && y1 == 3);
    CHECK(nf_key_bits(1) == 1 && nf_key_bits(2) == 2 && nf_key_bits(3) == 2 && nf_key_bits(4) == 3 && nf_key_bits(346 * 260) == 17 &&
          nf_key_bits(131071) == 17 && nf_key_bits(131072) == 18 && nf_key_bits(4096u * 4096u) == 25);
    const uint32_t list[] = {3, 5, 5, 9};
    CHECK(nf_last_before(list, 0, 0, 7) == NF_NONE && nf_last_before(list, 2, 2, 7) == NF_NONE);
    CHECK(nf_last_before(list, 0, 1, 3) == NF_NONE && nf_last_before(list, 0, 1, 4) == 0);
    CHECK(nf_last_before(list, 0, 4, 0) == NF_NONE && nf_last_before(list, 0, 4, 5) == 0 && nf_last_before(list, 0, 4, 6) == 2 &&
          nf_last_before(list, 0, 4, 9) == 2 && nf_last_before(list, 0, 4, 0xFFFFFFFFu) == 3 && nf_last_before(list, 1, 4, 4) == NF_NONE);
    n += 7;
    printf("known: %d cases\n", n);
    return n;
}

// ---- options -------------------------------------------------------------------------------------------------------------------------------------
static int check_options() {
    int n = 0;
    const NoiseOptions d = nf_default_options();
    CHECK(d.width == 346 && d.height == 260 && d.radius == 1 && d.min_support == 1 && d.include_self == 0 && d.reserved == 0 && d.dt == 0.005);
    CHECK(sizeof(NoiseOptions) == 32 && nf_options_error(d) == nullptr);
    auto bad = [&](void (*change)(NoiseOptions &), const char *word) {
        NoiseOptions o = nf_default_options();
        change(o);
        const char *e = nf_options_error(o);
        CHECK(e != nullptr && strstr(e, word) != nullptr);
        n++;
    };
    bad([](NoiseOptions &o) { o.radius = 0; }, "radius");
    bad([](NoiseOptions &o) { o.radius = 4; }, "radius");
    bad([](NoiseOptions &o) { o.min_support = 0; }, "min_support");
    bad([](NoiseOptions &o) { o.include_self = 2; }, "include_self");
    bad([](NoiseOptions &o) { o.reserved = 1; }, "reserved");
    bad([](NoiseOptions &o) { o.dt = -1e-300; }, "dt");
    bad([](NoiseOptions &o) { o.dt = QNAN; }, "dt");
    bad([](NoiseOptions &o) { o.dt = -INF; }, "dt");
    bad([](NoiseOptions &o) { o.width = 4097; }, "width");
    bad([](NoiseOptions &o) { o.height = 4097; }, "height");
    bad([](NoiseOptions &o) { o.width = 0; }, "width");
    bad([](NoiseOptions &o) { o.height = 0; }, "height");
    auto good = [&](void (*change)(NoiseOptions &)) {
        NoiseOptions o = nf_default_options();
        change(o);
        CHECK(nf_options_error(o) == nullptr);
        n++;
    };
    good([](NoiseOptions &o) { o.dt = 0.0; });
    good([](NoiseOptions &o) { o.dt = -0.0; });
    good([](NoiseOptions &o) { o.dt = INF; });
    good([](NoiseOptions &o) { o.radius = 3, o.min_support = 49, o.include_self = 1, o.width = o.height = 4096; });
    good([](NoiseOptions &o) { o.min_support = 0xFFFFFFFFu; });
    printf("options: %d cases\n", n);
    return n;
}

int main() {
    check_streams();
    check_known();
    check_options();
    printf("wrong: %d\n", g_wrong);
    return g_wrong ? 1 : 0;
}
