// CPU check of the array ingest's shared header (eventcalib_amd/csrc/fields_events.hpp), stand-alone: built plainly and under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_fields_host.py.
//   walk     seeded random columns — every type, strides from the type's size to 24, every byte offset — through fd_walk (the
//            element's own bytes) and block by block the way the kernels do it: every element from the aligned words that hold at
//            least one of its bytes, out of a buffer that ENDS with the last such word (a load of a word too many is an overflow the
//            sanitizer reports), the stop rule as "the least event that reaches end_time".  Records and counters identical.  Then the
//            records back into columns of random types against a per-element restatement.
//   headers  .npy headers as numpy writes them, cut at every length, with every byte replaced in turn, and the hostile ones by name.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "fields_events.hpp"

using namespace ecal_fields;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            failures++;                                                \
        }                                                              \
    } while (0)

struct Column {
    std::vector<uint32_t> words;   // the aligned words; the element bytes start `shift` bytes in and the last word holds the last byte
    Field f;
};

static Column make_column(std::mt19937_64 &rng, uint32_t type, uint64_t n, int role) {
    Column c;
    const uint32_t size = fd_type_size(type);
    const uint32_t shift = (uint32_t) (rng() % 4);
    const int64_t stride = size + (int64_t) (rng() % 4 == 0 ? rng() % (25 - size) : 0);
    const uint64_t span = n ? (n - 1) * (uint64_t) stride + size : 0;
    c.words.assign((size_t) ((shift + span + 3) / 4) + (n ? 0 : 1), 0xA5A5A5A5u);
    uint8_t *base = (uint8_t *) c.words.data() + shift;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t bits;
        const uint64_t r = rng();
        if (type == FD_F64 || type == FD_F32) {
            double v = role == FD_T ? (double) (r % 5000000) * 1e-6 : role == FD_P ? (double) ((int) (r % 3) - 1) : (double) (r % 400) - 20.0 + (double) (r >> 60) / 16.0;
            if (r % 97 == 0) v = NAN;
            if (r % 101 == 0) v = -v;
            bits = type == FD_F64 ? __builtin_bit_cast(uint64_t, v) : (uint64_t) __builtin_bit_cast(uint32_t, (float) v);
        } else {
            bits = role == FD_T ? 1000000 + r % 5000000 : role == FD_P ? (r % 3 == 0 ? (uint64_t) -1 : r % 2) : r % 400 - (r % 13 == 0 ? 20 : 0);
            if (r % 89 == 0) bits = r;   // (any bit pattern)
        }
        memcpy(base + i * (uint64_t) stride, &bits, size);
    }
    c.f = Field{base, stride, type, 0};
    return c;
}

// the kernels' load: the aligned words that hold at least one byte of the element
static uint64_t load_by_words(const Field &f, uint64_t i) {
    const uint32_t size = fd_type_size(f.type);
    const uintptr_t a = (uintptr_t) f.ptr + i * (uint64_t) f.stride;
    const uint32_t r = (uint32_t) (a & 3u);
    const uint32_t *w = (const uint32_t *) (a - r);
    return fd_bits_from_words(w[0], r + size > 4u ? w[1] : 0u, r + size > 8u ? w[2] : 0u, r);
}

static void blockwise(const Field f[4], uint64_t n, const FieldsFilter &flt, uint64_t block, FieldsCounts &c, std::vector<uint8_t> &out) {
    memset(&c, 0, sizeof(c));
    c.n_raw_events = n;
    uint64_t first_stop = ~0ull;
    std::vector<uint8_t> cls((size_t) n);
    std::vector<double> t((size_t) n), x((size_t) n), y((size_t) n);
    for (uint64_t b0 = 0; b0 < n; b0 += block)      // pass 1: every block on its own
        for (uint64_t i = b0; i < n && i < b0 + block; i++) {
            cls[i] = fd_classify(load_by_words(f[FD_T], i), f[FD_T].type, fd_value_f64(load_by_words(f[FD_X], i), f[FD_X].type),
                                 fd_value_f64(load_by_words(f[FD_Y], i), f[FD_Y].type), flt, &t[i], &x[i], &y[i]);
            if (cls[i] == FD_CLASS_STOP && i < first_stop) first_stop = i;
        }
    for (uint64_t i = 0; i < n && i < first_stop; i++) {   // pass 2: below the first offender
        if (cls[i] == FD_CLASS_OUTSIDE) c.n_outside++;
        else if (cls[i] == FD_CLASS_NEGATIVE) c.n_negative++;
        else if (cls[i] == FD_CLASS_BEFORE_START) c.n_before_start++;
        else {
            uint8_t rec[25];
            ecal::pack_record(rec, t[i], x[i], y[i], (uint8_t) (fd_value_positive(load_by_words(f[FD_P], i), f[FD_P].type) ? 1u : 0u));
            out.insert(out.end(), rec, rec + 25);
            c.n_events++;
        }
    }
    c.n_after_end = first_stop == ~0ull ? 0 : n - first_stop;
}

static void check_walks() {
    std::mt19937_64 rng(20260101);
    static const uint32_t stamp_types[5] = {FD_U32, FD_I32, FD_I64, FD_F32, FD_F64};
    int equal = 0;
    for (int it = 0; it < 400; it++) {
        const uint64_t n = it < 8 ? (uint64_t) it : 1 + rng() % 3000;
        Column col[4] = {make_column(rng, stamp_types[rng() % 5], n, FD_T), make_column(rng, (uint32_t) (rng() % FD_N_TYPES), n, FD_X),
                         make_column(rng, (uint32_t) (rng() % FD_N_TYPES), n, FD_Y), make_column(rng, (uint32_t) (rng() % FD_N_TYPES), n, FD_P)};
        Field f[4] = {col[0].f, col[1].f, col[2].f, col[3].f};
        FieldsFilter flt{};
        const bool float_stamp = fd_type_is_float(f[FD_T].type);
        flt.time_magnitude = float_stamp ? 1.0 : 1e-6;
        flt.time_base = float_stamp ? 0 : (int64_t) (rng() % 3 == 0 ? 1500000 : 0);
        if (rng() % 2) flt.width = 346, flt.height = 260;
        flt.flip_x = flt.width && rng() % 2;
        flt.flip_y = flt.height && rng() % 2;
        flt.start_time = rng() % 2 ? 1.2 : 0.0;
        flt.has_end_time = (int) (rng() % 2);
        flt.end_time = 1.0 + (double) (rng() % 5000) * 1e-3;
        int which = 0;
        std::string why;
        EXPECT(fd_check_fields(f, n, &which, &why) == FD_OK && fd_check_filter(flt, f[FD_T].type, &why) == FD_OK);
        FieldsCounts cs, cb;
        std::vector<uint8_t> seq, blk;
        fd_walk(f, n, flt, cs, [&](const uint8_t *rec) { seq.insert(seq.end(), rec, rec + 25); });
        const uint64_t blocks[4] = {1, 7, 64, FD_BLOCK_EVENTS};
        bool same = cs.n_events + cs.n_outside + cs.n_negative + cs.n_before_start + cs.n_after_end == cs.n_raw_events && cs.n_raw_events == n;
        for (uint64_t b : blocks) {
            blk.clear();
            blockwise(f, n, flt, b, cb, blk);
            same = same && blk == seq && memcmp(&cs, &cb, sizeof(cs)) == 0;
        }
        // the reverse, into columns of random types, against the element rules one by one
        ToFields o{1e6, (int64_t) (rng() % 1000), 0};
        Column dst[4] = {make_column(rng, stamp_types[rng() % 5], cs.n_events, FD_T), make_column(rng, (uint32_t) (rng() % FD_N_TYPES), cs.n_events, FD_X),
                         make_column(rng, (uint32_t) (rng() % FD_N_TYPES), cs.n_events, FD_Y), make_column(rng, (uint32_t) (rng() % FD_N_TYPES), cs.n_events, FD_P)};
        Field g[4] = {dst[0].f, dst[1].f, dst[2].f, dst[3].f};
        o.polarity_signed = !fd_type_is_unsigned(g[FD_P].type) && rng() % 2;
        EXPECT(fd_check_to_fields(g, cs.n_events, o, &which, &why) == FD_OK);
        const std::vector<uint32_t> before[4] = {dst[0].words, dst[1].words, dst[2].words, dst[3].words};
        const uint64_t bad = fd_unwalk(seq.data(), cs.n_events, g, o);
        uint64_t bad_want = 0;
        for (uint64_t i = 0; i < cs.n_events; i++) {
            const uint8_t *r = seq.data() + i * 25;
            uint64_t b[4];
            bool ok = fd_stamp_element(fd_load_f64(r), g[FD_T].type, o, &b[FD_T]);
            ok = fd_coord_element(fd_load_f64(r + 8), g[FD_X].type, &b[FD_X]) && ok;
            ok = fd_coord_element(fd_load_f64(r + 16), g[FD_Y].type, &b[FD_Y]) && ok;
            b[FD_P] = fd_polarity_element(r[24], g[FD_P].type, o);
            bad_want += ok ? 0 : 1;
            for (int k = 0; k < 4 && ok; k++) {
                const uint32_t size = fd_type_size(g[k].type);
                const uint64_t mask = size == 8 ? ~0ull : (1ull << (8 * size)) - 1;
                same = same && (load_by_words(g[k], i) & mask) == (b[k] & mask);
                if (k != FD_P && fd_type_is_float(g[k].type) == false && k == FD_X)   // an integer x came from an integral value
                    same = same && (double) fd_value_i64(b[k], g[k].type) == fd_load_f64(r + 8);
            }
        }
        same = same && bad == bad_want;
        // only the elements' own bytes were stored: the bytes between them are as before
        for (int k = 0; k < 4; k++) {
            const uint32_t size = fd_type_size(g[k].type);
            const uint8_t *now = (const uint8_t *) dst[k].words.data(), *was = (const uint8_t *) before[k].data(), *base = (const uint8_t *) g[k].ptr;
            for (size_t q = 0; q < dst[k].words.size() * 4; q++) {
                const ptrdiff_t rel = (now + q) - base;
                const bool inside = cs.n_events && rel >= 0 && (uint64_t) rel < fd_field_span(g[k], cs.n_events) && (uint64_t) rel % (uint64_t) g[k].stride < size;
                if (!inside) same = same && now[q] == was[q];
            }
        }
        EXPECT(same);
        equal += same ? 1 : 0;
    }
    printf("walk: %d inputs equal\n", equal);
}

static std::string npy_file(int major, const std::string &dict_in, uint64_t payload) {
    std::string dict = dict_in;
    const size_t pre = major == 1 ? 10 : 12;
    dict.append((64 - (pre + dict.size() + 1) % 64) % 64, ' ');
    dict.push_back('\n');
    std::string h("\x93NUMPY", 6);
    h.push_back((char) major);
    h.push_back(0);
    for (int b = 0; b < (major == 1 ? 2 : 4); b++) h.push_back((char) ((dict.size() >> (8 * b)) & 0xFF));
    return h + dict + std::string((size_t) payload, '\0');
}

static int parse(const std::string &file, NpyLayout &L, std::string *err, const NpyChoice &ch = NpyChoice()) {
    std::vector<uint8_t> copy(file.begin(), file.end());   // (a heap buffer of the exact size: an over-read is reported)
    return npy_parse_header(copy.data(), copy.size(), 0, ch, L, err);
}

static void check_headers() {
    int wrong = 0, cases = 0;
    NpyLayout L;
    std::string err;
    auto expect = [&](const std::string &file, int rc, const char *text, const NpyChoice &ch = NpyChoice()) {
        cases++;
        err.clear();
        const int got = parse(file, L, &err, ch);
        if (got != rc || (text && err.find(text) == std::string::npos)) {
            wrong++;
            printf("header case %d: rc %d (wanted %d), text '%s' (wanted '%s')\n", cases, got, rc, err.c_str(), text ? text : "");
        }
    };
    const std::string packed = "{'descr': [('t', '<i8'), ('x', '<u2'), ('y', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (5,), }";
    const std::string aligned = "{'descr': [('Timestamp', '<i8'), ('X', '<u2'), ('y', '<u2'), ('POL', '|b1'), ('', '|V3')], 'fortran_order': False, 'shape': (5,), }";
    const std::string plain = "{'descr': '<f8', 'fortran_order': False, 'shape': (5, 4), }";
    for (int major = 1; major <= 3; major++) {
        expect(npy_file(major, packed, 65), FD_OK, nullptr);
        EXPECT(L.n_events == 5 && L.item_stride == 13 && L.field[FD_T].offset == 0 && L.field[FD_X].offset == 8 && L.field[FD_Y].offset == 10 &&
               L.field[FD_P].offset == 12 && L.field[FD_T].type == FD_I64 && L.field[FD_X].type == FD_U16 && L.field[FD_P].type == FD_U8 &&
               L.data_offset % 64 == 0 && L.version_major == (uint32_t) major);
        expect(npy_file(major, aligned, 80), FD_OK, nullptr);
        EXPECT(L.item_stride == 16 && L.field[FD_P].offset == 12 && L.field[FD_P].type == FD_U8);
        expect(npy_file(major, plain, 160), FD_OK, nullptr);
        EXPECT(L.item_stride == 32 && L.field[FD_Y].offset == 16 && L.field[FD_T].type == FD_F64);
        expect(npy_file(major, packed, 64), FD_INVALID, "64 bytes there, 65 needed");
    }
    NpyChoice ch;
    ch.columns = "xytp";
    expect(npy_file(1, plain, 160), FD_OK, nullptr, ch);
    EXPECT(L.field[FD_X].offset == 0 && L.field[FD_Y].offset == 8 && L.field[FD_T].offset == 16 && L.field[FD_P].offset == 24);
    ch.columns = "xxtp";
    expect(npy_file(1, plain, 160), FD_INVALID, "each once", ch);
    NpyChoice names;
    names.name[FD_T] = "stamp";
    expect(npy_file(1, "{'descr': [('stamp', '<u4'), ('t', '<f8'), ('x', '<i2'), ('y', '<i2'), ('p', '|i1')], 'fortran_order': False, 'shape': (2,), }", 34), FD_OK, nullptr, names);
    EXPECT(L.field[FD_T].type == FD_U32 && L.field[FD_X].offset == 12 && L.item_stride == 17);
    expect(npy_file(1, packed, 65), FD_INVALID, "missing field t ('stamp')", names);
    expect(npy_file(1, "{'descr': [('t', '>i8'), ('x', '<u2'), ('y', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (5,), }", 65), FD_INVALID, "big-endian");
    expect(npy_file(1, "{'descr': '>f8', 'fortran_order': False, 'shape': (5, 4), }", 160), FD_INVALID, "big-endian");
    expect(npy_file(1, "{'descr': [('t', '<i8'), ('x', '<u2', (2,)), ('p', '|u1')], 'fortran_order': False, 'shape': (5,), }", 65), FD_INVALID, "sub-array");
    expect(npy_file(1, "{'descr': [('t', '<i8'), ('x', '<u2'), ('y', '<u2'), ('p', '|O')], 'fortran_order': False, 'shape': (5,), }", 100), FD_INVALID, "object dtype");
    expect(npy_file(1, "{'descr': '|O', 'fortran_order': False, 'shape': (5, 4), }", 160), FD_INVALID, "object dtype");
    expect(npy_file(1, "{'descr': '<f8', 'fortran_order': True, 'shape': (5, 4), }", 160), FD_INVALID, "fortran_order: True on 2-D data");
    expect(npy_file(1, "{'descr': '<f8', 'fortran_order': False, 'shape': (5, 3), }", 160), FD_INVALID, "(N, 4) is read");
    expect(npy_file(1, "{'descr': '<u2', 'fortran_order': False, 'shape': (5, 4), }", 160), FD_INVALID, "hold a stamp column");
    expect(npy_file(1, "{'descr': [('t', '<i8'), ('x', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (5,), }", 65), FD_INVALID, "missing field y");
    expect(npy_file(1, "{'descr': [('t', '<i8'), ('ts', '<i8'), ('x', '<u2'), ('y', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (5,), }", 200), FD_INVALID,
           "duplicate field for t");
    expect(npy_file(1, "{'descr': [('t', '<u2'), ('x', '<u2'), ('y', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (5,), }", 65), FD_INVALID, "which field t does not take");
    expect(npy_file(1, "{'descr': [('t', '<i8'), ('x', '<u8'), ('y', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (5,), }", 165), FD_INVALID, "which field x does not take");
    expect(npy_file(1, "{'descr': [('t', '<i8'), ('x', '<u2'), ('y', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (5, 2), }", 165), FD_INVALID, "2 dimensions");
    expect(npy_file(1, packed, 65).replace(6, 1, "\x04"), FD_INVALID, "version 4.0");
    expect(std::string("PK\x03\x04 not a numpy file at all, but long enough"), FD_INVALID, "not a .npy file");
    expect(std::string(), FD_INVALID, "not a .npy file");
    expect(npy_file(1, "{'descr': [('t', '<i8'), ('x', '<u2'), ('y', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (99999999999999999999999,), }", 65), FD_INVALID, nullptr);
    expect(npy_file(1, "{'descr': [('t', '<i8'), ('x', '<u2'), ('y', '<u2'), ('p', '|u1')], 'fortran_order': False, 'shape': (4611686018427387904,), }", 65), FD_INVALID, nullptr);
    // cut at every length: never OK (the header or the payload is short), never a read outside the bytes
    for (const std::string &dict : {packed, aligned, plain}) {
        const std::string file = npy_file(2, dict, 160);
        for (size_t cut = 0; cut < file.size(); cut++) {
            cases++;
            const int rc = parse(file.substr(0, cut), L, &err);
            const bool payload_cut = cut >= L.data_offset && rc == FD_OK;   // (a cut inside the spare payload bytes leaves a whole file)
            if (rc != FD_INVALID && !(payload_cut && cut - L.data_offset >= L.n_events * L.item_stride)) wrong++;
        }
        // every byte of the header replaced by every one of a few hostile bytes: any verdict, no crash, and an OK layout lies within the file
        static const char hostile[] = {'\0', '\'', '(', ')', '[', ']', '{', '}', ',', '9', '\\', (char) 0xFF, ' '};
        for (size_t at = 0; at < file.size() - 160; at++)
            for (char h : hostile) {
                std::string m = file;
                m[at] = h;
                cases++;
                if (parse(m, L, &err) == FD_OK) {
                    bool ok = L.data_offset <= m.size() && L.n_events * L.item_stride <= m.size() - L.data_offset;
                    for (int k = 0; k < 4; k++) ok = ok && L.field[k].type < FD_N_TYPES && L.field[k].offset + fd_type_size(L.field[k].type) <= L.item_stride;
                    if (!ok) wrong++;
                }
            }
    }
    EXPECT(wrong == 0);
    printf("headers: %d wrong of %d cases\n", wrong, cases);
    // the header this library writes is one numpy reads (and this parser)
    const std::string own = npy_records_header(7) + std::string(175, '\0');
    EXPECT(parse(own, L, &err) == FD_OK && L.n_events == 7 && L.item_stride == 25 && L.data_offset % 64 == 0 && L.field[FD_P].offset == 24 &&
           L.field[FD_Y].type == FD_F64);
}

int main() {
    check_walks();
    check_headers();
    if (failures) {
        printf("%d checks FAILED\n", failures);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
