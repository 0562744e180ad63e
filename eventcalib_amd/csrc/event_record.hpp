// The packed 25-byte event record every ingest writes: f64 t, f64 x, f64 y, u8 polarity (little endian).  One restatement for the
// write kernels (ecal_text.hip, ecal_raw.hip, ecal_aedat.hip, ecal_aedat4.hip, ecal_bag.hip), the host decoders of the *_events.hpp
// headers and the CPU tests.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAL_RECORD_HD __host__ __device__ __forceinline__
#else
#define ECAL_RECORD_HD inline
#endif

namespace ecal {

ECAL_RECORD_HD void put64(uint8_t *d, uint64_t u) {
    for (int b = 0; b < 8; b++) d[b] = (uint8_t) (u >> (8 * b));
}

// byte by byte: rec may stand at any address (a record's place in LDS or in a file's buffer is a multiple of 25)
ECAL_RECORD_HD void pack_record(uint8_t rec[25], double t, double x, double y, uint8_t pol) {
    put64(rec, __builtin_bit_cast(uint64_t, t));
    put64(rec + 8, __builtin_bit_cast(uint64_t, x));
    put64(rec + 16, __builtin_bit_cast(uint64_t, y));
    rec[24] = pol;
}

}  // namespace ecal
