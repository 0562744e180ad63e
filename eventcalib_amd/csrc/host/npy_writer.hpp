// Minimal .npy writer (format 1.0, little-endian f32, C order, two dimensions; no dependency) for the driver's
// saveDir/undistort_map_x.npy and undistort_map_y.npy: what numpy.load reads back as a float32 array of shape (rows, cols).
#ifndef ECAL_HOST_NPY_WRITER_H_
#define ECAL_HOST_NPY_WRITER_H_

#include <cstdint>
#include <cstdio>
#include <string>

namespace ecal_host {

// The header of a (rows, cols) float32 array: magic, version 1.0, a u16 length, the dict padded with spaces so that the data start at
// a multiple of 64 bytes, a newline last
inline std::string npy_header_f32(size_t rows, size_t cols) {
    std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(rows) + ", " + std::to_string(cols) + "), }";
    const size_t unpadded = 10 + dict.size() + 1;
    dict.append((64 - unpadded % 64) % 64, ' ');
    dict.push_back('\n');
    std::string h("\x93NUMPY\x01\x00", 8);
    h.push_back((char) (dict.size() & 0xFF));
    h.push_back((char) (dict.size() >> 8));
    return h + dict;
}

// data: rows * cols floats of this (little-endian) machine.  Returns false when the file cannot be written.
inline bool write_npy_f32(const std::string &path, size_t rows, size_t cols, const float *data) {
    const size_t n = rows * cols;
    if (!data && n != 0) return false;
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const std::string h = npy_header_f32(rows, cols);
    bool ok = std::fwrite(h.data(), 1, h.size(), f) == h.size();
    if (n != 0) ok = ok && std::fwrite(data, sizeof(float), n, f) == n;
    return (std::fclose(f) == 0) && ok;
}

}  // namespace ecal_host
#endif
