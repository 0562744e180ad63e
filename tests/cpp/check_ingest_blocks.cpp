// CPU check of the host/device pieces the ingest kernels share (eventcalib_amd/csrc/ingest_blocks.hpp, event_record.hpp), compiled
// for the host; tests/test_ingest_blocks_host.py builds it plainly and under AddressSanitizer + UndefinedBehaviorSanitizer and runs it
// with nothing preloaded.  Every buffer is a heap block of exactly n_bytes, so a read at or behind n_bytes is the sanitizer's find.
//   load32_clipped  every buffer size up to 48 bytes x every aligned offset from 0 to behind the buffer (words that end at n_bytes,
//                   1 - 3 bytes behind it, wholly behind it), against a bytewise reference
//   table_find      fixed tables (empty entries in front, in the middle, at the end; one entry; an entry over several blocks) and
//                   seeded random ones, random ranges [lo, hi] around the entry of a random slot, against a linear search
//   table_count_outside  entries that end at, one byte behind and far behind n_bytes, offsets behind it, lengths and sums that wrap 64
//                   bits, every start and step of a strided walk, against 128-bit arithmetic
//   pack_record     against the bytes of '<dddB', printed for the Python side too
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "event_record.hpp"
#include "ingest_blocks.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// every aligned offset from 0 to behind a heap buffer of exactly n bytes, n = 1 .. 48
static void check_loads(uint64_t *cases, uint64_t *wrong) {
    for (uint64_t n = 1; n <= 48; n++) {
        uint8_t *buf = (uint8_t *) malloc(n);   // exactly n_bytes, 16-byte aligned
        for (uint64_t i = 0; i < n; i++) buf[i] = (uint8_t) (rnd() | 1u);   // (no zero byte: a clipped byte shows)
        for (uint64_t a = 0; a <= n + 8; a += 4) {
            uint32_t want = 0;
            for (uint32_t b = 0; b < 4; b++)
                if (a + b < n) want |= (uint32_t) buf[a + b] << (8u * b);
            (*cases)++;
            if (ecal::load32_clipped(buf, a, n) != want && !(*wrong)++)
                printf("load32_clipped: n_bytes %llu, offset %llu differs\n", (unsigned long long) n, (unsigned long long) a);
        }
        free(buf);
    }
}

// the entry that holds slot s, the long way
static uint32_t linear_entry(const std::vector<unsigned long long> &first, uint64_t s) {
    for (uint32_t e = 0; e + 1 < first.size(); e++)
        if (first[e] <= s && s < first[e + 1]) return e;
    return 0xFFFFFFFFu;
}

static void check_table(const std::vector<uint32_t> &counts, uint64_t *cases, uint64_t *wrong) {
    const uint32_t n = (uint32_t) counts.size();
    std::vector<unsigned long long> first(n + 1, 0ull);   // exactly n + 1 words: first[n] is the last one read
    for (uint32_t e = 0; e < n; e++) first[e + 1] = first[e] + counts[e];
    const uint64_t n_slots = first[n];
    // table_find on its own: the last entry in [lo, hi] that does not start behind s
    for (int k = 0; k < 200 && n_slots; k++) {
        const uint64_t s = rnd() % n_slots;
        const uint32_t holds = linear_entry(first, s);
        const uint32_t lo = (uint32_t) (rnd() % (holds + 1u)), hi = holds + (uint32_t) (rnd() % (n - holds));
        uint32_t want = lo;
        for (uint32_t e = lo; e <= hi; e++)
            if (first[e] <= s) want = e;
        (*cases)++;
        if (ecal::table_find(first.data(), lo, hi, s) != want && !(*wrong)++) printf("table_find: %u entries, slot %llu differs\n", n, (unsigned long long) s);
    }
}

// entries around the end of the file and around 2^64, counted by strided walks that together visit every entry once
static void check_outside(uint64_t *cases, uint64_t *wrong) {
    struct Entry { uint64_t off, len; };
    const uint64_t top = ~0ull;
    for (uint64_t n_bytes : std::vector<uint64_t>{0u, 1u, 13u, 4096u, top - 1u, top}) {
        std::vector<Entry> tab;
        for (uint64_t off : std::vector<uint64_t>{0u, 1u, n_bytes / 2u, n_bytes - 1u, n_bytes, n_bytes + 1u, top - 7u, top})
            for (uint64_t len : std::vector<uint64_t>{0u, 1u, 8u, n_bytes - off, n_bytes - off + 1u, n_bytes, top - off, top - off + 1u, top}) tab.push_back(Entry{off, len});
        for (int k = 0; k < 64; k++) tab.push_back(Entry{rnd() >> (rnd() % 64), rnd() >> (rnd() % 64)});
        unsigned long long want = 0;
        for (const Entry &e : tab) want += (unsigned __int128) e.off + e.len > (unsigned __int128) n_bytes ? 1u : 0u;
        for (uint64_t step : std::vector<uint64_t>{1u, 3u, 64u, 1024u}) {
            unsigned long long got = 0;
            for (uint64_t start = 0; start < step; start++)
                got += ecal::table_count_outside(tab.size(), n_bytes, start, step, [&](uint64_t p) { return tab[p].off; }, [&](uint64_t p) { return tab[p].len; });
            (*cases)++;
            if (got != want && !(*wrong)++) printf("table_count_outside: n_bytes %llu, step %llu differs\n", (unsigned long long) n_bytes, (unsigned long long) step);
        }
    }
}

int main() {
    uint64_t cases = 0, wrong = 0;
    check_loads(&cases, &wrong);
    printf("loads: %llu cases, %llu wrong\n", (unsigned long long) cases, (unsigned long long) wrong);
    uint64_t failures = wrong;

    cases = wrong = 0;
    check_table({5}, &cases, &wrong);                                        // one entry
    check_table({1}, &cases, &wrong);
    check_table({0, 0, 0, 3, 2}, &cases, &wrong);                            // empty entries in front
    check_table({4, 0, 0, 0, 0, 9, 1}, &cases, &wrong);                      // ... in the middle
    check_table({2, 6, 0, 0, 0}, &cases, &wrong);                            // ... at the end
    check_table({0, 0, 1, 0, 0, 1, 0, 0}, &cases, &wrong);
    check_table({3, 5000, 2}, &cases, &wrong);                               // an entry over several blocks
    check_table({0, 1023, 0, 1, 0, 1025, 0, 2047, 1}, &cases, &wrong);       // entries that end at, before and behind a block's edge
    for (int k = 0; k < 120; k++) {
        std::vector<uint32_t> counts(1 + rnd() % 40);
        uint64_t total = 0;
        for (auto &c : counts) {
            const uint64_t kind = rnd() % 8;
            c = kind < 3 ? 0u : kind < 6 ? (uint32_t) (rnd() % 9) : kind < 7 ? (uint32_t) (rnd() % 300) : (uint32_t) (rnd() % 3000);
            total += c;
        }
        if (!total) counts[rnd() % counts.size()] = 1;   // (a table of no slots launches no block)
        check_table(counts, &cases, &wrong);
    }
    printf("tables: %llu cases, %llu wrong\n", (unsigned long long) cases, (unsigned long long) wrong);
    failures += wrong;

    cases = wrong = 0;
    check_outside(&cases, &wrong);
    printf("outside: %llu cases, %llu wrong\n", (unsigned long long) cases, (unsigned long long) wrong);
    failures += wrong;

    // '<dddB' of (1.0, 2.0, -0.5, 1), by hand; then what the Python side packs itself
    static const uint8_t want[25] = {0, 0, 0, 0, 0, 0, 0xF0, 0x3F, 0, 0, 0, 0, 0, 0, 0x00, 0x40, 0, 0, 0, 0, 0, 0, 0xE0, 0xBF, 1};
    uint8_t rec[25 + 2];
    memset(rec, 0xAA, sizeof(rec));
    ecal::pack_record(rec + 1, 1.0, 2.0, -0.5, 1);
    wrong = (memcmp(rec + 1, want, 25) != 0 || rec[0] != 0xAA || rec[26] != 0xAA) ? 1u : 0u;
    ecal::pack_record(rec + 1, 0.123456789012345678, 345.0, 259.0, 0);
    printf("record:");
    for (int b = 0; b < 25; b++) printf(" %02x", rec[1 + b]);
    printf("\npack_record: %llu wrong\n", (unsigned long long) wrong);
    failures += wrong;
    return failures ? 1 : 0;
}
