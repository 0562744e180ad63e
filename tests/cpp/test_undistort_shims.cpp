// The undistortion shims of host/event.hpp on a .bin file: EventContainer::undistorted and EventFrame::undistortedImage.
//   test_undistort_shims <events.bin> <camera: 112 bytes> <t0> <t1> <t0 of a window with one polarity> <t1> <out dir>
// writes <out>/sub.bin, <out>/pixel.bin (the undistorted streams), <out>/frame.rgb (width, height as two u32, then the bytes) and prints
// the totals; tests/test_gpu_undistort_driver.py compares them with the Python layer's.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../eventcalib_amd/csrc/host/event.hpp"

using namespace opengv2;

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    ecal_undistort_camera cam;
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f || std::fread(&cam, sizeof(cam), 1, f) != 1) return 2;
    std::fclose(f);
    const std::string out = argv[7];
    EventContainer::Ptr c = std::make_shared<EventContainer>();
    c->loadFile(argv[1], -1e300);
    ecal_ctx *ctx = ecal_host::thread_ctx();
    ecal_undistort_totals t;
    EventContainer::Ptr sub = c->undistorted(cam, nullptr, &t);
    if (sub->size() != t.n_kept || ecal_stream_to_bin_file(ctx, sub->device(), (out + "/sub.bin").c_str()) != ECAL_OK) return 3;
    std::printf("sub %llu %llu %llu %llu\n", (unsigned long long) t.n_events, (unsigned long long) t.n_invalid, (unsigned long long) t.n_outside,
                (unsigned long long) t.n_kept);
    ecal_undistort_options canvas;
    ecal_undistort_reference_canvas((uint32_t) c->cameraSize[0], (uint32_t) c->cameraSize[1], &canvas);
    EventContainer::Ptr pix = c->undistorted(cam, &canvas, &t);
    if (pix->size() != t.n_kept || ecal_stream_to_bin_file(ctx, pix->device(), (out + "/pixel.bin").c_str()) != ECAL_OK) return 3;
    std::printf("pixel %llu %llu %llu %llu\n", (unsigned long long) t.n_events, (unsigned long long) t.n_invalid, (unsigned long long) t.n_outside,
                (unsigned long long) t.n_kept);
    if (c->size() != t.n_events) return 4;   // the container itself is untouched
    EventFrame frame(c, {std::atof(argv[3]), std::atof(argv[4])});
    int w = 0, h = 0;
    ecal_undistort_frame_totals ft;
    const std::vector<uint8_t> rgb = frame.undistortedImage(cam, &w, &h, &ft);
    f = std::fopen((out + "/frame.rgb").c_str(), "wb");
    if (!f) return 3;
    const uint32_t wh[2] = {(uint32_t) w, (uint32_t) h};
    std::fwrite(wh, 4, 2, f);
    std::fwrite(rgb.data(), 1, rgb.size(), f);
    std::fclose(f);
    std::printf("frame %u %u %u %u\n", ft.n_pos, ft.n_neg, ft.n_invalid, ft.n_outside);
    EventFrame lone(c, {std::atof(argv[5]), std::atof(argv[6])});
    try {
        (void) lone.undistortedImage(cam);
        return 5;
    } catch (const std::logic_error &e) {
        if (std::string(e.what()) != "Events in Frame was cleared.") return 5;
    }
    ecal_undistort_camera bad = cam;
    bad.intr[0] = 0.0;
    try {
        (void) c->undistorted(bad);
        return 6;
    } catch (const std::invalid_argument &e) {
        if (std::string(e.what()).find("fx ") == std::string::npos) return 6;
    }
    std::printf("shims ok\n");
    return 0;
}
