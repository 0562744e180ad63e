// Plain-g++ build of eventcalib_amd/csrc/undistort_point.hpp (no HIP, no library): tests/test_undistort_host.py compares what it
// writes with the numpy restatement of the rule.
//   check_undistort points <in> <out>   in: the camera (112 bytes), u64 n, uv f64 [n][2]  ->  out: f64 [n][2], flag u8 [n]
//   check_undistort events <in> <out>   in: the camera, the options (32 bytes), u64 n, records [n][25]  ->  out: totals (4 u64), the kept records
//   check_undistort self                the rounding and the reference canvas, checked here; prints "self ok"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <cmath>

#include "../../eventcalib_amd/csrc/undistort_point.hpp"

using namespace ecal_undistort;

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> b;
    FILE *f = fopen(path, "rb");
    if (!f) return b;
    uint8_t chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) b.insert(b.end(), chunk, chunk + got);
    fclose(f);
    return b;
}

static int fail(const char *what) {
    fprintf(stderr, "check_undistort: %s\n", what);
    return 1;
}

static int self_check() {
    const double below_half = 0.49999999999999994;
    const struct {
        double a, want;
    } cases[] = {{0.5, 1.0},  {-0.5, -1.0}, {1.5, 2.0},  {-1.5, -2.0}, {below_half, 0.0}, {-below_half, -0.0}, {4503599627370497.0, 4503599627370497.0},
                 {2.5, 3.0},  {-2.5, -3.0}, {0.0, 0.0},  {1.4999999999999998, 1.0}};
    for (const auto &c : cases) {
        if (ud_round_half_away(c.a) != c.want) return fail("ud_round_half_away");
        if (ud_round_half_away(c.a) != std::round(c.a)) return fail("ud_round_half_away is not std::round");
    }
    const uint32_t sizes[4][4] = {{346, 260, 415, 312}, {640, 480, 768, 576}, {1280, 720, 1536, 864}, {5, 3, 6, 4}};
    for (const auto &s : sizes) {
        const Options o = ud_reference_canvas(s[0], s[1]);
        if (o.mode != UD_PIXEL || o.out_width != s[2] || o.out_height != s[3] || o.off_x != s[0] * 0.1 || o.off_y != s[1] * 0.1 || o.reserved != 0)
            return fail("ud_reference_canvas");
        if (ud_options_error(o)) return fail("the reference canvas is refused");
    }
    printf("self ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "self") return self_check();
    if (argc != 4) return fail("usage: check_undistort points|events <in> <out> | self");
    const std::string mode = argv[1];
    const std::vector<uint8_t> in = slurp(argv[2]);
    Camera cam;
    size_t at = 0;
    if (in.size() < sizeof(cam)) return fail("short input");
    memcpy(&cam, in.data(), sizeof(cam));
    at += sizeof(cam);
    if (ud_camera_error(cam)) return fail(ud_camera_error(cam));
    Options opt;
    memset(&opt, 0, sizeof(opt));
    if (mode == "events") {
        if (in.size() < at + sizeof(opt)) return fail("short input");
        memcpy(&opt, in.data() + at, sizeof(opt));
        at += sizeof(opt);
        if (ud_options_error(opt)) return fail(ud_options_error(opt));
    }
    uint64_t n = 0;
    if (in.size() < at + 8) return fail("short input");
    memcpy(&n, in.data() + at, 8);
    at += 8;
    FILE *f = fopen(argv[3], "wb");
    if (!f) return fail("cannot write the output");
    if (mode == "points") {
        if (in.size() != at + n * 16) return fail("the input's size");
        std::vector<double> uv(2 * n + 1), out(2 * n + 1, 0.0);
        std::vector<uint8_t> flag(n + 1, 0);
        memcpy(uv.data(), in.data() + at, n * 16);
        for (uint64_t i = 0; i < n; i++) {
            double up = 0.0, vp = 0.0;
            const bool ok = ud_point(cam, uv[2 * i], uv[2 * i + 1], &up, &vp);
            out[2 * i] = ok ? up : 0.0;
            out[2 * i + 1] = ok ? vp : 0.0;
            flag[i] = ok ? 0 : 1;
        }
        fwrite(out.data(), 16, n, f);
        fwrite(flag.data(), 1, n, f);
    } else if (mode == "events") {
        if (in.size() != at + n * UD_RECORD_BYTES) return fail("the input's size");
        std::vector<uint8_t> out(n * UD_RECORD_BYTES + 1);
        const Totals t = ud_events_sequential(cam, opt, in.data() + at, n, out.data());
        if (t.n_events != t.n_invalid + t.n_outside + t.n_kept) return fail("the totals do not add up");
        fwrite(&t, sizeof(t), 1, f);
        fwrite(out.data(), UD_RECORD_BYTES, t.n_kept, f);
    } else {
        fclose(f);
        return fail("unknown mode");
    }
    fclose(f);
    printf("%llu %s\n", (unsigned long long) n, mode.c_str());
    return 0;
}
