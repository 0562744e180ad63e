// The PinholeCamera shim (host/pinhole_camera.hpp) from a small program:
//   test_image_shims <camera: 112 bytes> <width> <height> <frame: width * height * 3 bytes> <out dir>
// writes <out>/picture.rgb (width, height as two u32, then the bytes of undistortImage), <out>/maps.bin (width, height, map_x, map_y of
// undistortMaps on the sensor's canvas) and prints a few points; tests/test_gpu_image_undistort.py compares them with the Python layer's.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../eventcalib_amd/csrc/host/pinhole_camera.hpp"

using namespace opengv2;

static bool put(const std::string &path, uint32_t w, uint32_t h, const void *a, size_t an, const void *b, size_t bn) {
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const uint32_t wh[2] = {w, h};
    std::fwrite(wh, 4, 2, f);
    std::fwrite(a, 1, an, f);
    if (b) std::fwrite(b, 1, bn, f);
    return std::fclose(f) == 0;
}

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    ecal_undistort_camera cam;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(&cam, sizeof(cam), 1, f) != 1) return 2;
    std::fclose(f);
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    std::vector<uint8_t> frame((size_t) W * H * 3);
    f = std::fopen(argv[4], "rb");
    if (!f || std::fread(frame.data(), 1, frame.size(), f) != frame.size()) return 2;
    std::fclose(f);
    const std::string out = argv[5];
    PinholeCamera pc({(double) W, (double) H}, {cam.intr[0], 0.0, cam.intr[2], 0.0, cam.intr[1], cam.intr[3], 0.0, 0.0, 1.0},
                     std::vector<double>(cam.intr + 4, cam.intr + 9), cam.model == ECAL_CAMERA_FISHEYE);
    const ecal_undistort_camera back = pc.camera();
    if (std::memcmp(&back, &cam, sizeof(cam)) != 0) return 3;
    // points: there and back
    const std::array<double, 2> p{W * 0.75, H * 0.25};
    const std::array<double, 2> ideal = pc.undistortPoint(p);
    bool valid = false;
    const std::array<double, 2> again = pc.distortPoint(ideal, &valid);
    std::printf("point %.17g %.17g %.17g %.17g %d\n", ideal[0], ideal[1], again[0], again[1], valid ? 1 : 0);
    (void) pc.distortPoint({1e9, 1e9}, &valid);
    if (valid) return 4;
    try {
        (void) pc.distortPoint({1e9, 1e9});
        return 4;
    } catch (const std::domain_error &) {
    }
    const std::vector<double> b = PinholeCamera::inverseRadialDistortion({-0.1, 0.01, 0.0, 0.0});
    std::printf("inverse %.17g %.17g %.17g %.17g %.17g\n", b[0], b[1], b[2], b[3], b[4]);
    // the picture, twice: one plan
    int w = 0, h = 0;
    const std::vector<uint8_t> pic = pc.undistortImage(frame, 3, &w, &h);
    const std::vector<uint8_t> pic2 = pc.undistortImage(frame);
    if (pic != pic2 || pc.plansBuilt() != 1) return 5;
    if (!put(out + "/picture.rgb", (uint32_t) w, (uint32_t) h, pic.data(), pic.size(), nullptr, 0)) return 6;
    // ... and a new one when the camera has changed
    pc.inverseRadialPoly()[0] *= 0.5;
    const std::vector<uint8_t> pic3 = pc.undistortImage(frame);
    if (pc.plansBuilt() != 2 || pic3 == pic) return 5;
    pc.inverseRadialPoly()[0] *= 2.0;
    try {
        (void) pc.undistortImage(std::vector<uint8_t>((size_t) W * H), 1);
        return 7;
    } catch (const std::logic_error &e) {
        if (std::string(e.what()) != "only support CV_8UC3 for now.") return 7;
    }
    std::vector<float> mx, my;
    const ecal_image_info info = pc.undistortMaps(mx, my);
    if ((int) info.opt.out_width != W || (int) info.opt.out_height != H || info.n_not_converged != 0) return 8;
    if (!put(out + "/maps.bin", info.opt.out_width, info.opt.out_height, mx.data(), mx.size() * 4, my.data(), my.size() * 4)) return 6;
    // no coefficients: the reference hands the point and the picture back
    PinholeCamera plain({(double) W, (double) H}, pc.K());
    if (plain.undistortPoint(p) != p || plain.undistortImage(frame) != frame) return 9;
    std::printf("shims ok\n");
    return 0;
}
