// The driver's .npy writer (eventcalib_amd/csrc/host/npy_writer.hpp) on its own: check_npy_writer <rows> <cols> <out.npy> writes the
// float32 array a[r][c] = r * 1000 + c + 0.25, and -1 in its last element; tests/test_image_undistort_host.py reads it with numpy.load.
#include <cstdlib>
#include <vector>

#include "../../eventcalib_amd/csrc/host/npy_writer.hpp"

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const size_t rows = (size_t) std::atol(argv[1]), cols = (size_t) std::atol(argv[2]);
    std::vector<float> a(rows * cols);
    for (size_t r = 0; r < rows; r++)
        for (size_t c = 0; c < cols; c++) a[r * cols + c] = (float) (r * 1000 + c) + 0.25f;
    if (!a.empty()) a.back() = -1.0f;
    if (ecal_host::npy_header_f32(rows, cols).size() % 64 != 0) return 3;
    return ecal_host::write_npy_f32(argv[3], rows, cols, a.data()) ? 0 : 1;
}
