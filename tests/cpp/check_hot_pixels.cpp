// CPU check of eventcalib_amd/csrc/pixel_activity.hpp (tests/test_hot_pixels_host.py builds and runs it, plainly and under
// AddressSanitizer + UndefinedBehaviorSanitizer): what the kernels of ecal_activity.hip and ecal_hot_pixel_mask decide with.
//   pixels   the classification of a coordinate on its edge values
//   rule     pa_hot_pixel_mask against a brute-force restatement (full sort, one pixel at a time) on seeded random count maps and
//            on the special ones: all zero, a single active pixel, quantile_permille 0 and 1000, exact ties at factor * Q and at
//            min_count, an extra mask
//   streams  the block-wise compaction with blocks of 1, 2, 7, 64 and 4096 events against the sequential one on 1000 seeded random
//            streams with every off-grid kind mixed in; the count map against the filter's totals
#include <stdio.h>
#include <stdlib.h>
#include <limits>
#include <random>
#include <vector>
#include "pixel_activity.hpp"

using namespace ecal_activity;

static int g_wrong = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            if (g_wrong++ < 20) printf("line %d: %s\n", __LINE__, #cond); \
        }                                                               \
    } while (0)

static void put_record(uint8_t *r, double t, double x, double y, uint8_t pol) {
    memcpy(r, &t, 8);
    memcpy(r + 8, &x, 8);
    memcpy(r + 16, &y, 8);
    r[24] = pol;
}

// ---- pixels ----------------------------------------------------------------------------------------------------------------------------------
static int check_pixels() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const uint32_t W = 346, H = 260;
    struct Case {
        double v;
        uint32_t n;
        bool on;
        uint32_t cell;
    };
    const Case cases[] = {
        {-0.0, W, true, 0},        {0.0, W, true, 0},          {0.5, W, false, 0},        {-1.0, W, false, 0},      {(double) (W - 1), W, true, W - 1},
        {(double) W, W, false, 0}, {nan, W, false, 0},         {inf, W, false, 0},        {-inf, W, false, 0},      {9007199254740992.0, W, false, 0},
        {345.5, W, false, 0},      {344.99999999999994, W, false, 0}, {-4.9e-324, W, false, 0},  {4.9e-324, W, false, 0},  {1.0, 1, false, 0},
        {0.0, 1, true, 0},         {4095.0, 4096, true, 4095}, {4096.0, 4096, false, 0},  {-0.5, W, false, 0},      {259.0, H, true, 259},
        {260.0, H, false, 0},      {9007199254740992.0, 4096, false, 0},
    };
    int n = 0;
    for (const Case &c : cases) {
        uint32_t cell = 0xDEADu;
        const bool on = pa_on_axis(c.v, c.n, &cell);
        CHECK(on == c.on);
        if (on && c.on) CHECK(cell == c.cell);
        n++;
    }
    // the pixel index, the plane, keep / remove through a record
    uint8_t r[25];
    std::vector<uint8_t> mask((size_t) W * H, 0);
    mask[(size_t) 3 * W + 7] = 1;
    bool og;
    put_record(r, 1.0, 7.0, 3.0, 0);
    CHECK(pa_record_pixel(r, W, H) == 3 * W + 7 && pa_record_plane(r) == 0 && pa_record_keep(r, mask.data(), W, H, &og) == 0 && !og);
    put_record(r, 1.0, 3.0, 7.0, 255);
    CHECK(pa_record_pixel(r, W, H) == 7 * W + 3 && pa_record_plane(r) == 1 && pa_record_keep(r, mask.data(), W, H, &og) == 1 && !og);
    put_record(r, 1.0, 7.0, nan, 1);
    CHECK(pa_record_pixel(r, W, H) == PA_OFF_GRID && pa_record_keep(r, mask.data(), W, H, &og) == 1 && og);
    put_record(r, 1.0, -0.0, -0.0, 2);
    CHECK(pa_record_pixel(r, W, H) == 0 && pa_record_plane(r) == 1);
    put_record(r, 1.0, 345.0, 259.0, 0);
    CHECK(pa_record_pixel(r, W, H) == W * H - 1);
    put_record(r, 1.0, 346.0, 0.0, 0);   // (not the first pixel of the next row)
    CHECK(pa_record_pixel(r, W, H) == PA_OFF_GRID);
    CHECK(pa_size_ok(1, 1) && pa_size_ok(4096, 4096) && !pa_size_ok(0, 5) && !pa_size_ok(5, 0) && !pa_size_ok(4097, 1) && !pa_size_ok(1, 4097));
    return n + 7;
}

// ---- rule ------------------------------------------------------------------------------------------------------------------------------------
// one pixel at a time, the quantile from a full sort
static void brute_rule(const std::vector<uint32_t> &counts, const HotOptions &o, const uint8_t *extra, std::vector<uint8_t> &mask, HotInfo &I) {
    const size_t plane = (size_t) o.width * o.height;
    std::vector<uint64_t> A;
    for (size_t p = 0; p < plane; p++)
        if ((uint64_t) counts[p] + counts[plane + p]) A.push_back((uint64_t) counts[p] + counts[plane + p]);
    std::sort(A.begin(), A.end());
    const uint64_t Q = A.empty() ? 0 : A[(size_t) (((uint64_t) A.size() - 1) * o.quantile_permille / 1000)];
    memset(&I, 0, sizeof(I));
    I.n_active_pixels = (uint32_t) A.size();
    I.quantile_count = pa_sat32(Q);
    mask.assign(plane, 0);
    for (size_t p = 0; p < plane; p++) {
        const uint64_t c = (uint64_t) counts[p] + counts[plane + p];
        bool hot = false;
        if (!A.empty() && c >= o.min_count) {
            const double lhs = (double) c, rhs = o.factor * (double) Q;
            hot = lhs > rhs;
        }
        const bool m = hot || (extra && extra[p]);
        mask[p] = m;
        I.n_events += c;
        I.n_hot_pixels += hot;
        I.n_masked_pixels += m;
        if (m) I.n_removed += c;
        if (!m && c > I.max_kept_count) I.max_kept_count = pa_sat32(c);
        if (c > I.max_count) I.max_count = pa_sat32(c);
    }
    I.n_kept = I.n_events - I.n_removed;
}

static bool same_info(const HotInfo &a, const HotInfo &b) {
    return a.n_events == b.n_events && a.n_off_grid == b.n_off_grid && a.n_removed == b.n_removed && a.n_kept == b.n_kept &&
           a.n_active_pixels == b.n_active_pixels && a.n_hot_pixels == b.n_hot_pixels && a.n_masked_pixels == b.n_masked_pixels &&
           a.quantile_count == b.quantile_count && a.max_count == b.max_count && a.max_kept_count == b.max_kept_count;
}

static bool rule_case(const std::vector<uint32_t> &counts, const HotOptions &o, const uint8_t *extra, uint32_t want_hot = 0xFFFFFFFFu) {
    const size_t plane = (size_t) o.width * o.height;
    std::vector<uint8_t> got(plane, 0xAA), want;
    HotInfo gi, wi;
    memset(&gi, 0xAA, sizeof(gi));
    const int rc = pa_hot_pixel_mask(counts.data(), o, extra, got.data(), &gi);
    brute_rule(counts, o, extra, want, wi);
    const bool ok = rc == PA_OK && got == want && same_info(gi, wi) && (want_hot == 0xFFFFFFFFu || gi.n_hot_pixels == want_hot);
    CHECK(ok);
    return ok;
}

static int check_rule() {
    int n = 0;
    std::mt19937_64 rng(20240917);
    // seeded random maps: sizes, sparsity, a few hot pixels, every quantile kind
    for (int it = 0; it < 400; it++) {
        HotOptions o;
        o.width = 1 + (uint32_t) (rng() % (it % 7 == 0 ? 97 : 23));
        o.height = 1 + (uint32_t) (rng() % 19);
        const uint32_t qs[] = {0, 1, 500, 990, 999, 1000};
        o.quantile_permille = it % 3 ? qs[rng() % 6] : (uint32_t) (rng() % 1001);
        o.min_count = (uint32_t) (rng() % 5 == 0 ? 0 : rng() % 100);
        const double fs[] = {0.0, 0.5, 1.0, 2.0, 8.0, 7.999999999999999, 1e300};
        o.factor = fs[rng() % 7];
        const size_t plane = (size_t) o.width * o.height;
        std::vector<uint32_t> counts(2 * plane, 0);
        const uint32_t fill = (uint32_t) (rng() % 101), top = 1 + (uint32_t) (rng() % 40);
        for (size_t p = 0; p < 2 * plane; p++)
            if (rng() % 100 < fill) counts[p] = (uint32_t) (rng() % top);
        for (int h = (int) (rng() % 4); h > 0; h--) counts[rng() % (2 * plane)] = (uint32_t) (rng() % 100000);
        if (it % 50 == 0) counts[rng() % (2 * plane)] = 0xFFFFFFFFu, counts[rng() % (2 * plane)] = 0xFFFFFFFFu;   // (c beyond 32 bits)
        std::vector<uint8_t> extra(plane, 0);
        for (size_t p = 0; p < plane; p++) extra[p] = rng() % 10 == 0 ? (uint8_t) (1 + rng() % 255) : 0;
        rule_case(counts, o, it % 2 ? extra.data() : nullptr);
        n++;
    }
    const HotOptions def{8, 4, PA_DEFAULT_QUANTILE_PERMILLE, PA_DEFAULT_MIN_COUNT, PA_DEFAULT_FACTOR};
    const size_t plane = 32;
    {   // all zero: nothing hot, whatever the options
        std::vector<uint32_t> c(2 * plane, 0);
        HotOptions o = def;
        rule_case(c, o, nullptr, 0);
        o.min_count = 0;
        o.factor = 0.0;
        rule_case(c, o, nullptr, 0);
        std::vector<uint8_t> extra(plane, 0);
        extra[5] = 1;
        rule_case(c, o, extra.data(), 0);
        n += 3;
    }
    {   // a single active pixel: it is its own quantile, c > factor * c only for factor < 1
        std::vector<uint32_t> c(2 * plane, 0);
        c[3] = 500;
        c[plane + 3] = 500;
        HotOptions o = def;
        rule_case(c, o, nullptr, 0);
        o.factor = 1.0;
        rule_case(c, o, nullptr, 0);
        o.factor = 0.999;
        rule_case(c, o, nullptr, 1);
        o.min_count = 1001;
        rule_case(c, o, nullptr, 0);
        o.min_count = 1000;   // (c == min_count counts)
        rule_case(c, o, nullptr, 1);
        n += 5;
    }
    {   // quantile_permille 0 (the smallest non-zero count) and 1000 (the largest): 30 pixels of 10, one of 5, one of 100
        std::vector<uint32_t> c(2 * plane, 0);
        for (size_t p = 0; p < 30; p++) c[p] = 4, c[plane + p] = 6;
        c[30] = 5;
        c[plane + 31] = 100;
        HotOptions o = def;
        o.quantile_permille = 0;   // Q = 5, bound 40: the pixel of 100
        rule_case(c, o, nullptr, 1);
        o.quantile_permille = 1000;   // Q = 100: nothing beats 800
        rule_case(c, o, nullptr, 0);
        o.quantile_permille = 990;   // index 30 of 32: Q = 10, bound 80
        rule_case(c, o, nullptr, 1);
        o.quantile_permille = 1001;
        std::vector<uint8_t> m(plane);
        CHECK(pa_hot_pixel_mask(c.data(), o, nullptr, m.data(), nullptr) == PA_INVALID);
        o = def;
        o.factor = -1.0;
        CHECK(pa_hot_pixel_mask(c.data(), o, nullptr, m.data(), nullptr) == PA_INVALID);
        o.factor = std::numeric_limits<double>::quiet_NaN();
        CHECK(pa_hot_pixel_mask(c.data(), o, nullptr, m.data(), nullptr) == PA_INVALID);
        o.factor = std::numeric_limits<double>::infinity();
        CHECK(pa_hot_pixel_mask(c.data(), o, nullptr, m.data(), nullptr) == PA_INVALID);
        o = def;
        o.width = 0;
        CHECK(pa_hot_pixel_mask(c.data(), o, nullptr, m.data(), nullptr) == PA_INVALID);
        n += 8;
    }
    {   // exact ties at factor * Q: 80 is not above 8 * 10, 81 is; split over the planes
        std::vector<uint32_t> c(2 * plane, 0);
        for (size_t p = 0; p < 28; p++) c[p] = 10;
        c[28] = 80;
        c[29] = 79, c[plane + 29] = 2;
        c[plane + 30] = 80;
        c[31] = 40, c[plane + 31] = 41;
        HotOptions o = def;   // index (31 * 990) / 1000 = 30 -> the sorted list's 31st value ... 28 tens, then 80 80 81 81: Q = 81
        rule_case(c, o, nullptr, 0);
        o.quantile_permille = 500;   // Q = 10
        rule_case(c, o, nullptr, 2);
        o.min_count = 81;
        rule_case(c, o, nullptr, 2);
        o.min_count = 82;
        rule_case(c, o, nullptr, 0);
        o.min_count = 64;
        o.factor = 7.9;   // (7.9 * 10 rounds to 79 exactly) the four large ones
        rule_case(c, o, nullptr, 4);
        n += 5;
    }
    return n;
}

// ---- streams ----------------------------------------------------------------------------------------------------------------------------------
static int check_streams() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::mt19937_64 rng(77001);
    const uint32_t blocks[] = {1, 2, 7, 64, PA_BLOCK_EVENTS};
    int equal = 0;
    for (int it = 0; it < 1000; it++) {
        const uint32_t W = it % 10 == 0 ? 1 : 1 + (uint32_t) (rng() % 40), H = it % 10 == 0 ? 1 : 1 + (uint32_t) (rng() % 30);
        const uint64_t n = it % 25 == 0 ? 0 : (it % 9 == 0 ? 4090 + rng() % 5000 : rng() % 700);
        std::vector<uint8_t> rec((size_t) n * 25), mask((size_t) W * H);
        const uint32_t dens = (uint32_t) (rng() % 101);
        for (auto &m : mask) m = rng() % 100 < dens ? (uint8_t) (1 + rng() % 255) : 0;
        if (it % 17 == 0) std::fill(mask.begin(), mask.end(), 0);
        if (it % 19 == 0) std::fill(mask.begin(), mask.end(), 1);
        auto coord = [&](uint32_t lim) -> double {
            switch (rng() % 16) {
            case 0: return nan;
            case 1: return inf;
            case 2: return -inf;
            case 3: return -0.0;
            case 4: return (double) (rng() % lim) + 0.5;
            case 5: return -1.0;
            case 6: return (double) lim;
            case 7: return 9007199254740992.0;
            default: return (double) (rng() % lim);
            }
        };
        double t = 5.0;
        for (uint64_t i = 0; i < n; i++) {
            t += (double) (rng() % 3) * 1e-6;   // (equal stamps too)
            put_record(rec.data() + i * 25, t, coord(W), coord(H), (uint8_t) (rng() % 4 == 0 ? rng() % 256 : rng() % 2));
        }
        std::vector<uint8_t> seq((size_t) n * 25 + 1, 0xCD), blk((size_t) n * 25 + 1);
        const FilterTotals ts = pa_filter_sequential(rec.data(), n, mask.data(), W, H, seq.data());
        bool ok = ts.n_events == n && ts.n_removed + ts.n_kept == n && seq[(size_t) n * 25] == 0xCD;
        for (uint32_t b : blocks) {
            std::fill(blk.begin(), blk.end(), 0xCD);
            const FilterTotals tb = pa_filter_blockwise(rec.data(), n, mask.data(), W, H, b, blk.data());
            ok = ok && tb.n_events == ts.n_events && tb.n_off_grid == ts.n_off_grid && tb.n_removed == ts.n_removed && tb.n_kept == ts.n_kept &&
                 memcmp(blk.data(), seq.data(), (size_t) ts.n_kept * 25) == 0 && blk[(size_t) n * 25] == 0xCD;
        }
        // the count map and the filter speak of the same events
        std::vector<uint32_t> counts(2 * (size_t) W * H);
        const ActivityTotals ta = pa_count_events(rec.data(), n, W, H, counts.data());
        uint64_t sum = 0, masked = 0;
        for (size_t p = 0; p < (size_t) W * H; p++) {
            sum += (uint64_t) counts[p] + counts[(size_t) W * H + p];
            if (mask[p]) masked += (uint64_t) counts[p] + counts[(size_t) W * H + p];
        }
        ok = ok && ta.n_events == n && ta.n_on_grid + ta.n_off_grid == n && sum == ta.n_on_grid && ta.n_off_grid == ts.n_off_grid && masked == ts.n_removed;
        CHECK(ok);
        equal += ok;
    }
    return equal;
}

int main() {
    const int np = check_pixels();
    printf("pixels: %d cases\n", np);
    const int nr = check_rule();
    printf("rule: %d maps\n", nr);
    const int ns = check_streams();
    printf("streams: %d streams equal\n", ns);
    printf("wrong: %d\n", g_wrong);
    return g_wrong ? 1 : 0;
}
