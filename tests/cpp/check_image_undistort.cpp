// A plain-g++ build of eventcalib_amd/csrc/image_undistort.hpp (no HIP, no library): the rules of include/ecal.h, "image undistortion",
// as the host compiler states them, for tests/test_image_undistort_host.py.
//   check_image_undistort self              a few known answers
//   check_image_undistort table  in out     in: camera (112 bytes), u32 W, H, options (40 bytes) -> out: u64 n_entries, u64 n_invalid_sources,
//                                           u64 n_empty, u64 max_neighbours, off [canvas + 1] u32, idx [n] u32, w [n] f64
//   check_image_undistort maps   in out     the same input -> out: map_x, map_y [canvas] f32, valid [canvas] u8, f64 r_lim, u64 truncated
//   check_image_undistort image  in out     the same input, then the frame [H][W][C] u8 -> out: the picture [canvas][C] u8, min, max f32
//   check_image_undistort points in out     in: camera, u32 W, H, u64 n, uv [n][2] f64 -> out: [n][2] f64, flag [n] u8
#include <stdio.h>
#include <string>
#include <vector>

#include "../../eventcalib_amd/csrc/image_undistort.hpp"

using namespace ecal_image;

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t) n);
    if (n && fread(v.data(), 1, (size_t) n, f) != (size_t) n) v.clear();
    fclose(f);
    return v;
}

struct Out {
    FILE *f;
    template <class T> void put(const T *p, size_t n) { fwrite(p, sizeof(T), n, f); }
    template <class T> void one(T v) { fwrite(&v, sizeof(T), 1, f); }
};

static int self_test() {
    static_assert(sizeof(Options) == 40 && sizeof(Info) == 112 && sizeof(Camera) == 112, "the C ABI's layouts");
    int bad = 0;
    const Options r = img_reference_options(346, 260);
    bad += !(r.out_width == 415 && r.out_height == 312 && r.off_x == 35.0 && r.off_y == 26.0 && r.channels == 3 && r.normalize == 1);
    bad += !(img_weight(0.0) == 1.0 / (100.0 * 2.220446049250313e-16) && img_weight(2.0) == 0.5);
    bad += !(img_to_u8(254.5f) == 255 && img_to_u8(0.49f) == 0 && img_to_u8(300.0f) == 255);
    bad += !(img_norm_scale(3.0f, 3.0f) == 0.0 && img_norm_scale(0.0f, 255.0f) == 1.0);
    bad += !(img_to_u8_normalized(0.5f, 0.0f, 1.0) == 0 && img_to_u8_normalized(1.5f, 0.0f, 1.0) == 2);   // ties to even
    // the barrel camera at 37 x 29 on the reference canvas, both methods, both channel counts: the walk itself
    Camera c;
    memset(&c, 0, sizeof(c));
    const double intr[9] = {30.0, 29.0, 17.7, 14.1, -0.21, 0.07, -0.012, 0.0011, -0.00004};
    for (int i = 0; i < 9; i++) c.intr[i] = intr[i];
    for (int i = 0; i < 4; i++) c.out_k[i] = intr[i];
    const uint32_t W = 37, H = 29;
    for (uint32_t method = 0; method < 2; method++)
        for (uint32_t C = 1; C <= 3; C += 2) {
            Options o = img_reference_options(W, H);
            o.method = method;
            o.channels = C;
            std::vector<uint8_t> src((size_t) W * H * C), dst((size_t) o.out_width * o.out_height * C);
            for (size_t k = 0; k < src.size(); k++) src[k] = (uint8_t) (k * 37u + 11u);
            float mm[2];
            Info I;
            img_undistort_sequential(c, W, H, o, src.data(), dst.data(), mm, &I);
            bad += !(mm[0] == 0.0f && mm[1] > 200.0f && I.n_empty > 0 && I.n_empty < dst.size() / C);
            bad += method == IMG_REFERENCE ? !(I.max_neighbours == 19 && I.n_entries > 10000) : !(I.truncated == 0 && I.n_not_converged == 0);
        }
    // a camera whose g' turns negative inside the sensor
    c.intr[4] = -50.0, c.intr[5] = c.intr[6] = c.intr[7] = c.intr[8] = 0.0;
    const Forward f = img_forward(c, W, H);
    bad += !(f.truncated == 1 && f.r_lim > 0.0 && f.r_lim < 0.09);   // (g' = 1 - 150 r^2 = 0 at r = 0.0816)
    double u, v;
    bad += !(img_distort_point(c, f, NAN, 1.0, &u, &v) == IMG_DISTORT_INVALID && img_distort_point(c, f, INFINITY, 1.0, &u, &v) == IMG_DISTORT_INVALID);
    printf(bad ? "self FAILED (%d)\n" : "self ok\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "self") return self_test();
    if (argc != 4) {
        fprintf(stderr, "usage: check_image_undistort self | table|maps|image|points in out\n");
        return 2;
    }
    const std::string what = argv[1];
    const std::vector<uint8_t> in = slurp(argv[2]);
    if (in.size() < sizeof(Camera) + 8) return 2;
    Camera c;
    uint32_t W, H;
    memcpy(&c, in.data(), sizeof(c));
    memcpy(&W, in.data() + sizeof(c), 4);
    memcpy(&H, in.data() + sizeof(c) + 4, 4);
    const uint8_t *rest = in.data() + sizeof(c) + 8;
    const size_t rest_bytes = in.size() - sizeof(c) - 8;
    Out out{fopen(argv[3], "wb")};
    if (!out.f) return 2;
    if (what == "points") {
        uint64_t n;
        if (rest_bytes < 8) return 2;
        memcpy(&n, rest, 8);
        if (rest_bytes < 8 + n * 16) return 2;
        std::vector<double> uv(2 * n), res(2 * n, 0.0);
        std::vector<uint8_t> flag(n);
        memcpy(uv.data(), rest + 8, n * 16);
        const Forward f = img_forward(c, W, H);
        for (uint64_t i = 0; i < n; i++) {
            double u = 0.0, v = 0.0;
            flag[i] = img_distort_point(c, f, uv[2 * i], uv[2 * i + 1], &u, &v);
            if (flag[i] != IMG_DISTORT_INVALID) res[2 * i] = u, res[2 * i + 1] = v;
        }
        out.put(res.data(), res.size());
        out.put(flag.data(), flag.size());
        fclose(out.f);
        return 0;
    }
    Options o;
    if (rest_bytes < sizeof(o)) return 2;
    memcpy(&o, rest, sizeof(o));
    if (img_options_error(o) || img_sensor_error(W, H)) return 3;
    const size_t np = (size_t) o.out_width * o.out_height;
    if (what == "table") {
        const Table t = img_table_sequential(c, W, H, o);
        out.one<uint64_t>(t.idx.size());
        out.one<uint64_t>(t.n_invalid_sources);
        out.one<uint64_t>(t.n_empty);
        out.one<uint64_t>(t.max_neighbours);
        out.put(t.off.data(), t.off.size());
        out.put(t.idx.data(), t.idx.size());
        out.put(t.w.data(), t.w.size());
    } else if (what == "maps") {
        const Forward f = img_forward(c, W, H);
        const Maps m = img_maps_sequential(c, f, o);
        out.put(m.mx.data(), np);
        out.put(m.my.data(), np);
        out.put(m.valid.data(), np);
        out.one<double>(f.r_lim);
        out.one<uint64_t>(f.truncated);
    } else if (what == "image") {
        const size_t src_bytes = (size_t) W * H * o.channels;
        if (rest_bytes < sizeof(o) + src_bytes) return 2;
        std::vector<uint8_t> dst(np * o.channels);
        float mm[2];
        img_undistort_sequential(c, W, H, o, rest + sizeof(o), dst.data(), mm, nullptr);
        out.put(dst.data(), dst.size());
        out.put(mm, 2);
    } else {
        return 2;
    }
    fclose(out.f);
    return 0;
}
