// CPU check of the AEDAT 4 ingest's host/device header (eventcalib_amd/csrc/aedat4_events.hpp): 2 000 seeded random files written by
// this program's own FlatBuffer and LZ4 encoders — both compressions, linked and independent blocks, packets of 0 to 6 000 events (so
// frames of several 64 KiB blocks occur), foreign streams between the event packets, a quarter of the files cut short at a random
// byte — each decoded by this program's own book-keeping (it knows what it wrote), by the header's sequential decoder and block-wise
// with blocks of 1, 2, 7, 64 events and of the kernels' block: records and every counter identical.  Then the header, indexer and
// malformed-frame case tables, and — where liblz4.so.1 can be loaded — frames made by LZ4F_compressFrame inflated by the header's
// inflater, byte for byte.  A stand-alone program: build plainly or with -fsanitize=address,undefined; link with -ldl.
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <string>
#include <vector>
#include "aedat4_events.hpp"

using namespace ecal_aedat4;
typedef std::vector<uint8_t> Bytes;
typedef std::mt19937_64 Rng;

struct Ev {
    int64_t t;
    int16_t x, y;
    uint8_t on;
};

static void put16(Bytes &v, uint32_t x) { v.push_back((uint8_t) x); v.push_back((uint8_t) (x >> 8)); }
static void put32(Bytes &v, uint32_t x) { put16(v, x & 0xFFFFu); put16(v, x >> 16); }
static void put64(Bytes &v, uint64_t x) { put32(v, (uint32_t) x); put32(v, (uint32_t) (x >> 32)); }
static void set32(Bytes &v, size_t at, uint32_t x) { for (int b = 0; b < 4; b++) v[at + b] = (uint8_t) (x >> (8 * b)); }
static void append(Bytes &v, const Bytes &w) { v.insert(v.end(), w.begin(), w.end()); }
static uint32_t pick(Rng &r, uint32_t n) { return (uint32_t) (r() % n); }

// ---- this program's writer ---------------------------------------------------------------------------------------------------------------
static Bytes io_header(int compression, int64_t position, bool omit_compression = false, bool omit_position = false, const char *ident = "IOHE") {
    Bytes b;
    put32(b, 20);   // root: the table at byte 20
    b.insert(b.end(), ident, ident + 4);
    put16(b, 10); put16(b, 20); put16(b, omit_compression ? 0 : 4); put16(b, omit_position ? 0 : 8); put16(b, 16); put16(b, 0);
    put32(b, 12);   // the table: its vtable 12 bytes in front
    put32(b, (uint32_t) compression);
    put64(b, (uint64_t) position);
    put32(b, 4);
    const std::string xml = "<dv version=\"2.0\"></dv>";
    put32(b, (uint32_t) xml.size());
    b.insert(b.end(), xml.begin(), xml.end());
    b.push_back(0);
    while (b.size() % 8) b.push_back(0);
    Bytes out;
    put32(out, (uint32_t) b.size());
    append(out, b);
    return out;
}

static Bytes fb_packet(const std::vector<Ev> &ev, bool vt_after, uint32_t extra, bool absent, int vec_mod, const char *ident = "EVTS") {
    const uint32_t nf = 1 + extra, table_bytes = 4 + 4 * nf;
    uint32_t vt_bytes = 4 + 2 * nf;
    const uint32_t vt_padded = (vt_bytes + 3) / 4 * 4;
    const uint32_t table_at = vt_after ? 12 : 12 + vt_padded, vt_at = vt_after ? 12 + table_bytes : 12;
    uint32_t vec_at = 12 + vt_padded + table_bytes;
    if (vec_mod >= 0) vec_at += ((uint32_t) vec_mod + 32u - ((vec_at + 4) % 16)) % 16;
    Bytes b(vec_at, 0);
    set32(b, 4, table_at - 4);
    memcpy(&b[8], ident, 4);
    set32(b, table_at, (uint32_t) ((int32_t) table_at - (int32_t) vt_at));
    set32(b, table_at + 4, vec_at - (table_at + 4));
    for (uint32_t k = 1; k < nf; k++) set32(b, table_at + 4 + 4 * k, 0xA5A50000u + k);
    b[vt_at] = (uint8_t) vt_bytes; b[vt_at + 2] = (uint8_t) table_bytes;
    for (uint32_t k = 0; k < nf; k++) b[vt_at + 4 + 2 * k] = (uint8_t) ((absent && k == 0) ? 0 : 4 + 4 * k);
    if (!absent) {
        put32(b, (uint32_t) ev.size());
        for (const Ev &e : ev) {
            put64(b, (uint64_t) e.t);
            put16(b, (uint16_t) e.x); put16(b, (uint16_t) e.y);
            b.push_back(e.on); b.push_back(0); b.push_back(0); b.push_back(0);
        }
    }
    set32(b, 0, (uint32_t) b.size() - 4);
    return b;
}

static void put_length(Bytes &out, size_t v) {   // the extension of a nibble of 15: v = length - 15
    while (v >= 255) { out.push_back(255); v -= 255; }
    out.push_back((uint8_t) v);
}
static void put_sequence(Bytes &out, const uint8_t *lit, size_t ll, uint32_t off, size_t ml) {   // off 0: the last sequence
    out.push_back((uint8_t) (((ll < 15 ? ll : 15) << 4) | (off ? (ml - 4 < 15 ? ml - 4 : 15) : 0)));
    if (ll >= 15) put_length(out, ll - 15);
    out.insert(out.end(), lit, lit + ll);
    if (off) {
        put16(out, off);
        if (ml - 4 >= 15) put_length(out, ml - 4 - 15);
    }
}
// a plain greedy matcher over data[start, start + len); matches reach back to data[floor] (the frame's first byte, or the block's own)
static Bytes lz4_block(const uint8_t *data, size_t floor, size_t start, size_t len) {
    Bytes out;
    std::vector<int64_t> table(1 << 13, -1);
    auto hash = [&](size_t i) { return (uint32_t) ((a4_le32(data + i) * 2654435761u) >> 19); };
    const size_t end = start + len;
    for (size_t i = (start > floor + 65535 ? start - 65535 : floor); i + 4 <= start; i++) table[hash(i)] = (int64_t) i;
    size_t anchor = start, i = start;
    while (i + 12 < end) {
        const uint32_t h = hash(i);
        const int64_t c = table[h];
        table[h] = (int64_t) i;
        if (c >= (int64_t) floor && i - (size_t) c <= 65535 && a4_le32(data + c) == a4_le32(data + i)) {
            size_t ml = 4;
            while (i + ml < end - 5 && data[c + ml] == data[i + ml]) ml++;
            put_sequence(out, data + anchor, i - anchor, (uint32_t) (i - (size_t) c), ml);
            i += ml;
            anchor = i;
        } else {
            i++;
        }
    }
    put_sequence(out, data + anchor, end - anchor, 0, 0);
    return out;
}
static Bytes lz4_frame(const Bytes &data, Rng &r, bool linked, bool stored_only = false) {
    const bool bsum = pick(r, 4) == 0, csize = pick(r, 3) == 0, csum = pick(r, 4) == 0;
    const uint32_t bm = pick(r, 8) == 0 ? 5 : 4;
    const size_t block_max = (size_t) 1 << (8 + 2 * bm);
    Bytes f;
    put32(f, 0x184D2204u);
    f.push_back((uint8_t) (0x40 | (linked ? 0 : 0x20) | (bsum ? 0x10 : 0) | (csize ? 8 : 0) | (csum ? 4 : 0)));
    f.push_back((uint8_t) (bm << 4));
    if (csize) put64(f, data.size());
    f.push_back((uint8_t) r());   // the header checksum: stepped over
    for (size_t a = 0; a < data.size(); a += block_max) {
        const size_t len = data.size() - a < block_max ? data.size() - a : block_max;
        Bytes blk;
        const bool stored = stored_only || pick(r, 10) < 3;
        if (!stored) blk = lz4_block(data.data(), linked ? 0 : a, a, len);
        if (stored || blk.size() >= len) {
            put32(f, 0x80000000u | (uint32_t) len);
            f.insert(f.end(), data.begin() + a, data.begin() + a + len);
        } else {
            put32(f, (uint32_t) blk.size());
            append(f, blk);
        }
        if (bsum) put32(f, (uint32_t) r());
    }
    if (data.empty() && pick(r, 2)) put32(f, 0x80000000u);   // a stored block of nothing
    put32(f, 0);
    if (csum) put32(f, (uint32_t) r());
    return f;
}

// ---- this program's filter ------------------------------------------------------------------------------------------------------------
struct Expect {
    Bytes records;
    A4Counts c;
};
static void own_filter(const std::vector<Ev> &ev, const A4Filter &f, Expect &x) {
    bool stopped = false;
    for (const Ev &e : ev) {
        x.c.n_raw_events++;
        if (stopped) { x.c.n_after_end++; continue; }
        if (e.x < 0 || e.y < 0 || (f.width && (uint32_t) e.x >= f.width) || (f.height && (uint32_t) e.y >= f.height)) { x.c.n_outside++; continue; }
        const uint32_t px = f.flip_x ? f.width - 1 - (uint32_t) e.x : (uint32_t) e.x, py = f.flip_y ? f.height - 1 - (uint32_t) e.y : (uint32_t) e.y;
        const double t = (double) (e.t - f.time_base) * 1e-6;
        if (t < 0) { x.c.n_negative++; continue; }
        if (f.has_end_time && t >= f.end_time) { stopped = true; x.c.n_after_end++; continue; }
        if (t < f.start_time) { x.c.n_before_start++; continue; }
        const double dx = px, dy = py;
        uint8_t rec[25];
        memcpy(rec, &t, 8); memcpy(rec + 8, &dx, 8); memcpy(rec + 16, &dy, 8);
        rec[24] = e.on ? 1 : 0;
        x.records.insert(x.records.end(), rec, rec + 25);
        x.c.n_events++;
    }
}

static bool same_counts(const A4Counts &a, const A4Counts &b, std::string &what) {
#define CMP(f) if (a.f != b.f) { what = std::string(#f) + " " + std::to_string((long long) a.f) + " vs " + std::to_string((long long) b.f); return false; }
    CMP(n_raw_events) CMP(n_events) CMP(n_outside) CMP(n_negative) CMP(n_before_start) CMP(n_after_end) CMP(n_packets) CMP(n_other_packets)
    CMP(n_trailing_bytes) CMP(n_compressed_bytes) CMP(n_inflated_bytes) CMP(first_stamp_us) CMP(time_base) CMP(compression) CMP(stream_id)
#undef CMP
    return true;
}

static int random_files() {
    int bad = 0;
    const uint64_t blocks[5] = {1, 2, 7, 64, A4_BLOCK_EVENTS};
    uint64_t total_events = 0, multi_block_frames = 0, cut_files = 0, refused = 0;
    for (int file = 0; file < 2000; file++) {
        Rng r(1000 + file);
        const int compression = file % 2 ? A4_COMP_LZ4 : A4_COMP_NONE;
        const bool linked = pick(r, 2), cut = file % 4 == 3;
        const int ev_stream = (int) pick(r, 4);
        const uint32_t n_packets = pick(r, 6) == 0 ? pick(r, 2) : 1 + pick(r, 7);
        struct Written { int sid; size_t begin, end, data_bytes, fb_bytes; std::vector<Ev> ev; };
        std::vector<Written> written;
        Bytes chain;
        int64_t t = 1600000000000000ll + (int64_t) pick(r, 2000000) - (pick(r, 8) == 0 ? 3200000000000000ll : 0);
        const bool big = pick(r, 12) == 0;
        for (uint32_t p = 0; p < n_packets; p++) {
            Written w;
            const bool foreign = pick(r, 4) == 0;
            w.sid = foreign ? ev_stream + 1 + (int) pick(r, 2) : ev_stream;
            Bytes fb;
            if (foreign) {
                fb.resize(12 + pick(r, 3000));
                for (auto &b : fb) b = (uint8_t) r();
                memcpy(&fb[8], pick(r, 2) ? "FRME" : "IMUS", 4);
            } else {
                const uint32_t kind = pick(r, 10);
                const uint32_t n = kind == 0 ? 0 : kind < 4 ? pick(r, 40) : big && kind == 9 ? 4097 + pick(r, 1904) : pick(r, 700);
                for (uint32_t k = 0; k < n; k++) {
                    t += pick(r, 50) - (pick(r, 40) == 0 ? 30 : 0);
                    w.ev.push_back(Ev{t, (int16_t) ((int) pick(r, 360) - 4), (int16_t) ((int) pick(r, 270) - 3), (uint8_t) (pick(r, 3) == 0 ? pick(r, 256) : pick(r, 2))});
                }
                const bool absent = n == 0 && pick(r, 2);
                fb = fb_packet(w.ev, pick(r, 2), pick(r, 3), absent, pick(r, 2) ? (int) pick(r, 16) : -1);
            }
            w.fb_bytes = fb.size();
            Bytes data = compression == A4_COMP_NONE ? fb : lz4_frame(fb, r, linked, foreign && pick(r, 2));
            if (compression != A4_COMP_NONE && fb.size() > 65536) multi_block_frames++;
            w.data_bytes = data.size();
            w.begin = chain.size();
            put32(chain, (uint32_t) w.sid);
            put32(chain, (uint32_t) data.size());
            append(chain, data);
            w.end = chain.size();
            written.push_back(std::move(w));
        }
        const bool with_table = !cut && pick(r, 2);
        Bytes header = io_header(compression, -1);
        const size_t begin = 14 + header.size();
        if (with_table) header = io_header(compression, (int64_t) (begin + chain.size()));
        Bytes f;
        f.insert(f.end(), "#!AER-DAT4.0\r\n", "#!AER-DAT4.0\r\n" + 14);
        append(f, header);
        append(f, chain);
        if (with_table) for (int k = 0; k < 24; k++) f.push_back((uint8_t) r());
        size_t n_bytes = f.size();
        if (cut) {
            n_bytes = pick(r, 10) == 0 ? pick(r, (uint32_t) begin + 1) : begin + pick(r, (uint32_t) chain.size() + 1);
            cut_files++;
        }
        Bytes file_bytes(f.begin(), f.begin() + n_bytes);   // (a copy of the exact size: the sanitizer sees every read behind it)
        // options
        A4DecodeOptions o;
        memset(&o, 0, sizeof(o));
        o.stream_id = pick(r, 2) ? ev_stream : -1;
        o.auto_time_base = pick(r, 2);
        o.filter.time_base = 1600000000000000ll + (int64_t) pick(r, 1000000);
        o.filter.width = pick(r, 3) ? 346 : 0;
        o.filter.height = pick(r, 3) ? 260 : 0;
        o.filter.flip_x = o.filter.width && pick(r, 3) == 0;
        o.filter.flip_y = o.filter.height && pick(r, 3) == 0;
        o.filter.start_time = pick(r, 3) == 0 ? 0.002 * pick(r, 10) : -INFINITY;
        o.filter.has_end_time = pick(r, 3) == 0;
        o.filter.end_time = 0.001 * pick(r, 60);
        o.max_inflated_bytes = A4_DEFAULT_MAX_INFLATED;
        // what this program expects
        Expect x;
        memset(&x.c, 0, sizeof(x.c));
        bool expect_invalid = n_bytes < begin;
        std::vector<Ev> all;
        if (!expect_invalid) {
            size_t whole = 0;
            while (whole < written.size() && begin + written[whole].end <= n_bytes) whole++;
            const size_t chain_end = begin + (whole ? written[whole - 1].end : 0);
            x.c.n_trailing_bytes = with_table ? 0 : n_bytes - chain_end;
            bool any_event_packet = false, stamped = false;
            for (size_t p = 0; p < whole; p++) {
                const Written &w = written[p];
                if (w.sid != ev_stream) { x.c.n_other_packets++; continue; }
                any_event_packet = true;
                x.c.n_packets++;
                x.c.n_compressed_bytes += w.data_bytes;
                x.c.n_inflated_bytes += w.fb_bytes;
                if (!stamped && !w.ev.empty()) {
                    int64_t q = w.ev[0].t / 1000000;
                    if (w.ev[0].t % 1000000 < 0) q--;
                    x.c.first_stamp_us = q * 1000000;
                    stamped = true;
                }
                all.insert(all.end(), w.ev.begin(), w.ev.end());
            }
            x.c.compression = compression;
            x.c.stream_id = ev_stream;
            if (o.stream_id < 0 && !any_event_packet) {
                if (whole) expect_invalid = true;   // only foreign streams: no stream of events
                else x.c.stream_id = -1;
            }
        }
        A4Filter flt = o.filter;
        if (o.auto_time_base) flt.time_base = x.c.first_stamp_us;
        x.c.time_base = flt.time_base;
        if (!expect_invalid) own_filter(all, flt, x);
        total_events += all.size();
        // the header's decoders
        for (int form = 0; form < 6; form++) {
            Bytes got;
            A4Counts c;
            std::string err, what;
            auto put = [&](const uint8_t *rec) { got.insert(got.end(), rec, rec + 25); };
            const int rc = form == 0 ? a4_decode_sequential(file_bytes.data(), n_bytes, o, c, put, &err)
                                     : a4_decode_blockwise(file_bytes.data(), n_bytes, o, blocks[form - 1], c, put, &err);
            if (expect_invalid) {
                if (rc != A4_INVALID || err.find("AEDAT 4") == std::string::npos) {
                    printf("file %d form %d: expected a refusal that says AEDAT 4, got %d \"%s\"\n", file, form, rc, err.c_str());
                    bad++;
                }
                if (form == 0) refused++;
                continue;
            }
            if (rc != A4_OK) {
                printf("file %d form %d: status %d \"%s\"\n", file, form, rc, err.c_str());
                bad++;
            } else if (got != x.records) {
                printf("file %d form %d: records differ (%zu vs %zu bytes)\n", file, form, got.size(), x.records.size());
                bad++;
            } else if (!same_counts(c, x.c, what)) {
                printf("file %d form %d: %s\n", file, form, what.c_str());
                bad++;
            }
            if (bad > 20) return bad;
        }
    }
    printf("AEDAT 4: 2000 files %s (%llu events, %llu frames of several blocks, %llu files cut short, %llu refused)\n", bad ? "DIFFER" : "equal",
           (unsigned long long) total_events, (unsigned long long) multi_block_frames, (unsigned long long) cut_files, (unsigned long long) refused);
    return bad;
}

// ---- case tables -----------------------------------------------------------------------------------------------------------------------
static Bytes file_of(const Bytes &header, const Bytes &chain) {
    Bytes f;
    f.insert(f.end(), "#!AER-DAT4.0\r\n", "#!AER-DAT4.0\r\n" + 14);
    append(f, header);
    append(f, chain);
    return f;
}
static Bytes chain_packet(int sid, const Bytes &data) {
    Bytes c;
    put32(c, (uint32_t) sid);
    put32(c, (uint32_t) data.size());
    append(c, data);
    return c;
}

static int header_cases() {
    int n = 0, wrong = 0;
    auto check = [&](const char *name, const Bytes &f, bool whole, int want_rc, const char *want_text, int want_compression = 0, int64_t want_pos = -1) {
        A4Header h;
        std::string err;
        static const uint8_t none = 0;
        int rc = a4_parse_header(f.empty() ? &none : f.data(), f.size(), whole, &h, &err);
        uint64_t end = 0;
        if (!rc) rc = a4_packets_end(h, f.size(), &end, &err);
        n++;
        bool ok = rc == want_rc;
        if (ok && rc) ok = err.find("AEDAT 4") != std::string::npos && err.find(want_text) != std::string::npos;
        if (ok && !rc) ok = h.compression == want_compression && h.data_table_position == want_pos && h.packets_begin == 14 + io_header(0, -1).size() &&
                            end == (want_pos >= 0 ? (uint64_t) want_pos : f.size());
        if (!ok) {
            printf("header case %s: status %d \"%s\"\n", name, rc, err.c_str());
            wrong++;
        }
    };
    const size_t begin = 14 + io_header(0, -1).size();
    check("plain lz4", file_of(io_header(1, -1), Bytes(40, 0)), true, A4_OK, "", 1, -1);
    check("none, table position", file_of(io_header(0, (int64_t) begin + 10), Bytes(40, 0)), true, A4_OK, "", 0, (int64_t) begin + 10);
    check("lz4 high", file_of(io_header(2, -1), Bytes()), true, A4_OK, "", 2, -1);
    check("defaults", file_of(io_header(1, 5, true, true), Bytes()), true, A4_OK, "", 0, -1);
    check("position at the end", file_of(io_header(1, (int64_t) begin), Bytes()), true, A4_OK, "", 1, (int64_t) begin);
    check("zstd", file_of(io_header(3, -1), Bytes()), true, A4_INVALID, "ZSTD compression is not read: record with LZ4");
    check("zstd high", file_of(io_header(4, -1), Bytes()), true, A4_INVALID, "ZSTD_HIGH");
    check("compression 7", file_of(io_header(7, -1), Bytes()), true, A4_INVALID, "compression value 7");
    check("compression -2", file_of(io_header(-2, -1), Bytes()), true, A4_INVALID, "compression value -2");
    check("wrong identifier", file_of(io_header(1, -1, false, false, "IOHX"), Bytes()), true, A4_INVALID, "IOHE");
    check("position in front of the packets", file_of(io_header(1, (int64_t) begin - 1), Bytes(8, 0)), true, A4_INVALID, "dataTablePosition");
    check("position behind the end", file_of(io_header(1, (int64_t) begin + 9), Bytes(8, 0)), true, A4_INVALID, "dataTablePosition");
    check("the version line alone", Bytes((const uint8_t *) "#!AER-DAT4.0\r\n", (const uint8_t *) "#!AER-DAT4.0\r\n" + 14), true, A4_INVALID, "cut short");
    check("empty", Bytes(), true, A4_INVALID, "cut short");
    check("another version", Bytes((const uint8_t *) "#!AER-DAT3.1\r\n#!END", (const uint8_t *) "#!AER-DAT3.1\r\n#!END" + 19), true, A4_INVALID, "first line");
    {
        Bytes f = file_of(io_header(1, -1), Bytes());
        f.resize(f.size() - 5);
        check("cut inside the header", f, true, A4_INVALID, "cut short");
        Bytes g = file_of(io_header(1, -1), Bytes());
        set32(g, 14, 2u << 20);
        check("a header beyond the first MiB", g, false, A4_INVALID, "first MiB");
        Bytes k = file_of(io_header(1, -1), Bytes());
        set32(k, 18, 4000);   // the root points outside
        check("a table outside the header", k, true, A4_INVALID, "table");
    }
    printf("headers: %d cases, %d wrong\n", n, wrong);
    return wrong;
}

static int indexer_cases() {
    int n = 0, wrong = 0;
    std::vector<Ev> ev3 = {{1600000001999999ll, 1, 2, 1}, {1600000002000001ll, 3, 4, 0}, {1600000002000002ll, 5, 6, 1}};
    const Bytes evts = fb_packet(ev3, false, 0, false, -1), none_ev = fb_packet({}, false, 0, false, -1);
    Bytes frame(200, 7);
    memcpy(&frame[8], "FRME", 4);
    auto check = [&](const char *name, const Bytes &f, int sid, int want_rc, const char *want_text, uint64_t want_packets = 0, uint64_t want_other = 0,
                     uint64_t want_trailing = 0, int want_sid = 0, int64_t want_stamp = 0) {
        std::vector<A4Packet> table;
        A4Counts c;
        std::string err;
        const int rc = a4_index_file_memory(f.data(), f.size(), sid, table, c, &err);
        n++;
        bool ok = rc == want_rc;
        if (ok && rc) ok = err.find("AEDAT 4") != std::string::npos && err.find(want_text) != std::string::npos;
        if (ok && !rc) ok = table.size() == want_packets && c.n_packets == want_packets && c.n_other_packets == want_other && c.n_trailing_bytes == want_trailing &&
                            c.stream_id == want_sid && c.first_stamp_us == want_stamp;
        for (size_t k = 0; ok && k < table.size(); k++) ok = table[k].offset + table[k].n_bytes <= f.size() && table[k].zero == 0;
        if (!ok) {
            printf("indexer case %s: status %d \"%s\" packets %zu other %llu trailing %llu stream %d stamp %lld\n", name, rc, err.c_str(), table.size(),
                   (unsigned long long) c.n_other_packets, (unsigned long long) c.n_trailing_bytes, c.stream_id, (long long) c.first_stamp_us);
            wrong++;
        }
    };
    Bytes c1 = chain_packet(0, frame);
    append(c1, chain_packet(1, none_ev));
    append(c1, chain_packet(1, evts));
    append(c1, chain_packet(2, frame));
    append(c1, chain_packet(1, evts));
    check("found by its identifier", file_of(io_header(0, -1), c1), -1, A4_OK, "", 3, 2, 0, 1, 1600000001000000ll);
    check("named", file_of(io_header(0, -1), c1), 1, A4_OK, "", 3, 2, 0, 1, 1600000001000000ll);
    check("named, a stream that is not of events", file_of(io_header(0, -1), c1), 2, A4_INVALID, "event packet 0");
    check("a stream that does not occur", file_of(io_header(0, -1), c1), 9, A4_OK, "", 0, 5, 0, 9, 0);
    check("no packets", file_of(io_header(0, -1), Bytes()), -1, A4_OK, "", 0, 0, 0, -1, 0);
    {
        Bytes f = file_of(io_header(0, -1), c1);
        f.resize(f.size() - 1);
        check("cut inside data", f, -1, A4_OK, "", 2, 2, 8 + evts.size() - 1, 1, 1600000001000000ll);
        f.resize(f.size() - evts.size() - 3);
        check("cut inside a header", f, -1, A4_OK, "", 2, 2, 4, 1, 1600000001000000ll);
    }
    {
        Bytes c2 = chain_packet(0, evts);
        append(c2, chain_packet(3, evts));
        check("two streams of events", file_of(io_header(0, -1), c2), -1, A4_INVALID, "stream ids 0, 3");
        check("two streams of events, one named", file_of(io_header(0, -1), c2), 3, A4_OK, "", 1, 1, 0, 3, 1600000001000000ll);
        Bytes c3 = chain_packet(4, frame);
        append(c3, chain_packet(6, frame));
        check("no stream of events", file_of(io_header(0, -1), c3), -1, A4_INVALID, "stream ids 4, 6");
        Bytes c4 = chain_packet(0, evts);
        put32(c4, 0);
        put32(c4, 0xFFFFFFF0u);
        append(c4, Bytes(32, 0));
        check("a negative size", file_of(io_header(0, -1), c4), -1, A4_INVALID, "packet 1 at byte");
    }
    {
        Rng r(5);
        Bytes c5 = chain_packet(0, lz4_frame(frame, r, true));
        append(c5, chain_packet(1, lz4_frame(evts, r, true)));
        const size_t begin = 14 + io_header(1, -1).size();
        Bytes f = file_of(io_header(1, (int64_t) (begin + c5.size())), c5);
        append(f, Bytes(30, 0x5A));
        check("lz4, a table behind the packets", f, -1, A4_OK, "", 1, 1, 0, 1, 1600000001000000ll);
        Bytes c6 = chain_packet(1, Bytes(20, 1));
        check("lz4, a first packet that is no frame", file_of(io_header(1, -1), c6), -1, A4_INVALID, "the first of stream 1");
    }
    printf("indexer: %d cases, %d wrong\n", n, wrong);
    return wrong;
}

static int frame_cases() {
    int n = 0, wrong = 0;
    auto frame = [](uint8_t flg, uint8_t bd, const Bytes &body, uint32_t magic = 0x184D2204u, int64_t content = -1) {
        Bytes f;
        put32(f, magic);
        f.push_back(flg); f.push_back(bd);
        if (content >= 0) put64(f, (uint64_t) content);
        f.push_back(0);
        append(f, body);
        return f;
    };
    auto blk = [](const Bytes &data, bool stored = false) {
        Bytes b;
        put32(b, (uint32_t) data.size() | (stored ? 0x80000000u : 0u));
        append(b, data);
        return b;
    };
    auto cat = [](std::initializer_list<Bytes> parts) {
        Bytes b;
        for (const Bytes &p : parts) append(b, p);
        return b;
    };
    const Bytes END = {0, 0, 0, 0};
    auto check = [&](const char *name, const Bytes &f, int want, const Bytes *want_out = nullptr) {
        Bytes exact(f), out;   // (exact size: the sanitizer sees a read behind the frame)
        const int why = a4_lz4_inflate(exact.data(), exact.size(), out);
        uint64_t size = 0;
        const int why2 = a4_lz4_size(exact.data(), exact.size(), &size);
        n++;
        bool ok = why == want && why2 == want && (want || size == out.size()) && (!want_out || out == *want_out);
        if (!ok) {
            printf("frame case %s: %d / %d (%s), wanted %d\n", name, why, why2, a4_why(why), want);
            wrong++;
        }
    };
    const Bytes abcd = {'a', 'b', 'c', 'd'};
    // "abcd" then a match of 8 at offset 4 then "xy":  token 0x44, literals, offset, then the last sequence 0x20 'x' 'y'
    const Bytes good = {0x44, 'a', 'b', 'c', 'd', 4, 0, 0x20, 'x', 'y'};
    const Bytes good_out = {'a', 'b', 'c', 'd', 'a', 'b', 'c', 'd', 'a', 'b', 'c', 'd', 'x', 'y'};
    check("a good frame", frame(0x40, 0x40, cat({blk(good), END})), A4E_NONE, &good_out);
    check("every flag", frame(0x7C, 0x70, cat({blk(good), Bytes(4, 9), END, Bytes(4, 9)}), 0x184D2204u, 14), A4E_NONE, &good_out);
    {
        const Bytes run = {0x1F, 'z', 1, 0, 250, 0x00}, stored_then = cat({blk(abcd, true), blk(Bytes{0x04, 4, 0, 0x00}), END});
        Bytes run_out(1 + 269, 'z'), linked_out = {'a', 'b', 'c', 'd', 'a', 'b', 'c', 'd', 'a', 'b', 'c', 'd'}, empty;   // (stored abcd, then a match of 8)
        check("offset 1 is a run", frame(0x40, 0x40, cat({blk(run), END})), A4E_NONE, &run_out);
        check("a match into the block before", frame(0x40, 0x40, stored_then), A4E_NONE, &linked_out);
        check("an empty block and a stored block of nothing", frame(0x40, 0x40, cat({blk(Bytes{0x00}), blk(Bytes(), true), END})), A4E_NONE, &empty);
        check("no block at all", frame(0x40, 0x40, END), A4E_NONE, &empty);
    }
    check("cut short", Bytes{4, 0x22, 0x4D, 0x18, 0x40}, A4E_FRAME_SHORT);
    check("no magic", frame(0x40, 0x40, END, 0x12345678u), A4E_MAGIC);
    check("legacy magic", frame(0x40, 0x40, END, 0x184C2102u), A4E_LEGACY);
    check("skippable magic", frame(0x40, 0x40, END, 0x184D2A53u), A4E_SKIPPABLE);
    check("version 00", frame(0x00, 0x40, END), A4E_VERSION);
    check("version 10", frame(0x80, 0x40, END), A4E_VERSION);
    check("reserved FLG bit", frame(0x42, 0x40, END), A4E_RESERVED);
    check("dictionary id", frame(0x41, 0x40, cat({Bytes(4, 0), END})), A4E_DICT);
    check("reserved BD bits", frame(0x40, 0x41, END), A4E_RESERVED);
    check("reserved BD bit 7", frame(0x40, 0xC0, END), A4E_RESERVED);
    check("block maximum 3", frame(0x40, 0x30, END), A4E_BLOCK_MAX);
    check("content size cut short", Bytes{4, 0x22, 0x4D, 0x18, 0x48, 0x40, 1, 2, 3}, A4E_FRAME_SHORT);
    check("no end mark", frame(0x40, 0x40, blk(good)), A4E_NO_END_MARK);
    check("an end mark cut short", frame(0x40, 0x40, cat({blk(good), Bytes{0, 0}})), A4E_NO_END_MARK);
    check("a block checksum cut short", frame(0x50, 0x40, cat({blk(good), Bytes{1, 2}})), A4E_NO_END_MARK);
    check("a content checksum cut short", frame(0x44, 0x40, cat({blk(good), END, Bytes{1, 2}})), A4E_FRAME_SHORT);
    check("bytes behind the frame", frame(0x40, 0x40, cat({blk(good), END, Bytes{1}})), A4E_BYTES_BEHIND);
    check("a block past the packet", frame(0x40, 0x40, cat({Bytes{200, 0, 0, 0}, good, END})), A4E_BLOCK_PAST_PACKET);
    check("a stored block past the packet", frame(0x40, 0x40, cat({Bytes{200, 0, 0, 0x80}, good, END})), A4E_BLOCK_PAST_PACKET);
    check("a wrong content size", frame(0x48, 0x40, cat({blk(good), END}), 0x184D2204u, 15), A4E_CONTENT_SIZE);
    check("offset 0", frame(0x40, 0x40, cat({blk(Bytes{0x44, 'a', 'b', 'c', 'd', 0, 0, 0x00}), END})), A4E_OFFSET_ZERO);
    check("an offset in front of the frame", frame(0x40, 0x40, cat({blk(Bytes{0x44, 'a', 'b', 'c', 'd', 5, 0, 0x00}), END})), A4E_OFFSET_FRONT);
    check("an offset in front of the frame, second block", frame(0x40, 0x40, cat({blk(abcd, true), blk(Bytes{0x04, 5, 0, 0x00}), END})), A4E_OFFSET_FRONT);
    check("literals past the block", frame(0x40, 0x40, cat({blk(Bytes{0x50, 'a', 'b'}), END})), A4E_LIT_PAST);
    check("a literal extension past the block", frame(0x40, 0x40, cat({blk(Bytes{0xF0, 255, 255}), END})), A4E_EXT_PAST);
    check("a match extension past the block", frame(0x40, 0x40, cat({blk(Bytes{0x1F, 'a', 1, 0, 255}), END})), A4E_EXT_PAST);
    check("one offset byte", frame(0x40, 0x40, cat({blk(Bytes{0x10, 'a', 1}), END})), A4E_OFFSET_PAST);
    check("a block that ends on a match", frame(0x40, 0x40, cat({blk(Bytes{0x10, 'a', 1, 0}), END})), A4E_TOKEN_PAST);
    {
        Bytes big(65537, 'q');
        check("a stored block beyond the maximum", frame(0x40, 0x40, cat({blk(big, true), END})), A4E_BLOCK_TOO_BIG);
        big.resize(65536);
        check("a stored block of the maximum", frame(0x40, 0x40, cat({blk(big, true), END})), A4E_NONE, &big);
        // 1 literal, then a run of 65 535 more = the maximum exactly: match length 65 535 = 4 + 15 + 256 * 255 + 236
        Bytes run = {0x1F, 'q', 1, 0};
        for (int k = 0; k < 256; k++) run.push_back(255);
        run.push_back(236);
        run.push_back(0x00);
        check("a match that ends at the block maximum", frame(0x40, 0x40, cat({blk(run), END})), A4E_NONE, &big);
        run[run.size() - 2] = 237;
        check("a match beyond the block maximum", frame(0x40, 0x40, cat({blk(run), END})), A4E_BLOCK_TOO_BIG);
    }
    printf("frames: %d cases, %d wrong\n", n, wrong);
    return wrong;
}

static int locator_cases() {
    int n = 0, wrong = 0;
    std::vector<Ev> ev = {{5, 1, 2, 1}, {6, -3, 4, 0}, {7, 5, -6, 2}};
    auto check = [&](const char *name, const Bytes &b, int want, uint32_t want_count = 0) {
        Bytes exact(b);
        uint64_t first = 0;
        uint32_t count = 0;
        const int why = a4_locate_events(exact.data(), exact.size(), &first, &count);
        n++;
        bool ok = why == want && (want || count == want_count);
        if (ok && !want && count) {
            const A4Event e = a4_event_at(exact.data() + first + 16 * (count - 1));
            ok = e.t_us == ev[count - 1].t && e.x == ev[count - 1].x && e.y == ev[count - 1].y && e.on == (ev[count - 1].on != 0);
        }
        if (!ok) {
            printf("locator case %s: %d (%s) count %u\n", name, why, a4_why(why), count);
            wrong++;
        }
    };
    for (int mod = 0; mod < 16; mod++)
        for (int after = 0; after < 2; after++) check("vector placement", fb_packet(ev, after, mod % 3, false, mod), A4E_NONE, 3);
    check("field 0 absent", fb_packet({}, false, 1, true, -1), A4E_NONE, 0);
    check("no events", fb_packet({}, true, 0, false, -1), A4E_NONE, 0);
    check("nothing at all", Bytes(), A4E_NONE, 0);
    check("another identifier", fb_packet(ev, false, 0, false, -1, "FRME"), A4E_FB_IDENT);
    check("cut short", Bytes(11, 0), A4E_FB_SHORT);
    {
        Bytes b = fb_packet(ev, false, 0, false, -1);
        Bytes c = b;
        c.resize(c.size() - 1);
        check("a vector cut short", c, A4E_FB_VECTOR);
        c = b;
        set32(c, 4, 100000);
        check("a root outside", c, A4E_FB_TABLE);
        c = b;
        set32(c, 4 + a4_le32(&b[4]), 0x7FFFFFF0u);
        check("a vtable in front of the packet", c, A4E_FB_VTABLE);
        c = b;
        set32(c, 4 + a4_le32(&b[4]), 0x80000010u);
        check("a vtable behind the packet", c, A4E_FB_VTABLE);
        c = b;
        c[12 + 4] = 0xF0; c[12 + 5] = 0xFF;
        check("field 0 outside", c, A4E_FB_FIELD);
        c = b;
        set32(c, 4 + a4_le32(&b[4]) + 4, 0xFFFFFF00u);
        check("a vector outside", c, A4E_FB_VECTOR);
        c = b;
        set32(c, c.size() - 48 - 4, 0x10000000u);
        check("a count beyond the packet", c, A4E_FB_VECTOR);
    }
    printf("locator: %d cases, %d wrong\n", n, wrong);
    return wrong;
}

// ---- the independent anchor: frames made by liblz4 ------------------------------------------------------------------------------------------
static int liblz4_frames() {
    void *lib = dlopen("liblz4.so.1", RTLD_NOW | RTLD_LOCAL);
    typedef size_t (*BoundFn)(size_t, const void *);
    typedef size_t (*CompressFn)(void *, size_t, const void *, size_t, const void *);
    typedef unsigned (*IsErrorFn)(size_t);
    BoundFn bound = lib ? (BoundFn) dlsym(lib, "LZ4F_compressFrameBound") : nullptr;
    CompressFn compress = lib ? (CompressFn) dlsym(lib, "LZ4F_compressFrame") : nullptr;
    IsErrorFn is_error = lib ? (IsErrorFn) dlsym(lib, "LZ4F_isError") : nullptr;
    if (!bound || !compress || !is_error) {
        printf("liblz4: skipped (liblz4.so.1 cannot be loaded)\n");
        return 0;
    }
    int wrong = 0, n = 0;
    for (int k = 0; k < 200; k++) {
        Rng r(77 + k);
        std::vector<Ev> ev;
        int64_t t = 1700000000000000ll;
        const uint32_t count = k % 20 == 0 ? 5000 + pick(r, 4000) : pick(r, 900);
        for (uint32_t e = 0; e < count; e++) {
            t += pick(r, 30);
            ev.push_back(Ev{t, (int16_t) pick(r, 346), (int16_t) pick(r, 260), (uint8_t) pick(r, 2)});
        }
        const Bytes fb = fb_packet(ev, pick(r, 2), 0, false, -1);
        Bytes frame(bound(fb.size(), nullptr));
        const size_t got = compress(frame.data(), frame.size(), fb.data(), fb.size(), nullptr);
        if (is_error(got)) {
            printf("liblz4: LZ4F_compressFrame failed\n");
            return 1;
        }
        frame.resize(got);
        Bytes exact(frame), out;
        const int why = a4_lz4_inflate(exact.data(), exact.size(), out);
        n++;
        if (why || out != fb) {
            printf("liblz4 frame %d: %d (%s), %zu bytes for %zu\n", k, why, a4_why(why), out.size(), fb.size());
            wrong++;
        }
    }
    printf("liblz4: %d frames, %d wrong\n", n, wrong);
    dlclose(lib);
    return wrong;
}

int main() {
    int bad = random_files();
    bad += header_cases();
    bad += indexer_cases();
    bad += frame_cases();
    bad += locator_cases();
    bad += liblz4_frames();
    return bad ? 1 : 0;
}
