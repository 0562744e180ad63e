// The bins of the calibration quality reports, shared by ecal_report.hip (board units) and ecal_report_px.hip (pixels): one bin's
// statistics in registers, a family's bins in LDS, their flush into ecal_bin_stats records, and the keyframe of a time.  Device
// code only; the including translation unit is compiled without contraction where these are used.
#pragma once
#include <hip/hip_runtime.h>
#include "ecal_solver_state.hpp"

namespace ecal {

constexpr uint32_t RP_KF_LDS = 64;      // keyframes of a chunk that get bins in LDS (a chunk of the benchmark meets ~5)
constexpr uint32_t RP_MAX_LM = 1024;    // landmarks (40 bytes of LDS each)
constexpr uint32_t RP_MAX_CELLS = 8192; // sensor cells (12 bytes of LDS each)
constexpr uint32_t RP_MAX_HIST = 256;

// one bin's running statistics in a thread's registers
struct BinAcc {
    uint32_t n = 0, n_out = 0;
    double sum_r = 0.0, sum_r2 = 0.0, sum_abs = 0.0, max_abs = 0.0;
    __device__ __forceinline__ void add(double r, double ar, double r2, bool out) {
        n++;
        n_out += out ? 1u : 0u;
        sum_r += r;
        sum_r2 += r2;
        sum_abs += ar;
        max_abs = fmax(max_abs, ar);
    }
};

// |r| as an integer: the order of non-negative doubles is the order of their bit patterns
__device__ __forceinline__ unsigned long long abs_bits(double a) { return (unsigned long long) __double_as_longlong(a); }

__device__ __forceinline__ void bin_add_global(ecal_bin_stats *b, const BinAcc &a) {
    atomicAdd((unsigned long long *) &b->n, (unsigned long long) a.n);
    if (a.n_out) atomicAdd((unsigned long long *) &b->n_out, (unsigned long long) a.n_out);
    atomicAdd(&b->sum_r, a.sum_r);
    atomicAdd(&b->sum_r2, a.sum_r2);
    atomicAdd(&b->sum_abs, a.sum_abs);
    atomicMax((unsigned long long *) &b->max_abs, abs_bits(a.max_abs));
}

// LDS bins of a family: counts [2][n] (n, n_out), sums [3][n] (sum_r, sum_r2, sum_abs) and max_abs [n] as bits
struct LdsBins {
    uint32_t *cnt;
    double *sum;
    unsigned long long *mx;
    uint32_t n;
    __device__ __forceinline__ void add(uint32_t i, const BinAcc &a) const {
        atomicAdd(&cnt[i], a.n);
        if (a.n_out) atomicAdd(&cnt[n + i], a.n_out);
        atomicAdd(&sum[i], a.sum_r);
        atomicAdd(&sum[n + i], a.sum_r2);
        atomicAdd(&sum[2 * n + i], a.sum_abs);
        atomicMax(&mx[i], abs_bits(a.max_abs));
    }
    // bins [0, n) into out[base ..]: one global atomic per non-empty bin and field
    __device__ __forceinline__ void flush(ecal_bin_stats *out, uint32_t base, uint32_t count, int tid) const {
        for (uint32_t i = (uint32_t) tid; i < count; i += NE_T) {
            BinAcc a;
            a.n = cnt[i];
            if (!a.n) continue;
            a.n_out = cnt[n + i];
            a.sum_r = sum[i];
            a.sum_r2 = sum[n + i];
            a.sum_abs = sum[2 * n + i];
            a.max_abs = __longlong_as_double((long long) mx[i]);
            bin_add_global(out + base + i, a);
        }
    }
};

// The keyframe of time t in the ascending table of K times by the association's rule (ecal_associate.hip, associate_one): the
// first index a with time >= t — known to lie in [lo, hi] — against its predecessor, the predecessor on a tie.  kt holds the
// table from index `first` on (the whole table, or the chunk's keyframes staged in LDS).
__device__ __forceinline__ uint32_t nearest_keyframe(const double *kt, uint32_t first, uint32_t K, uint32_t lo, uint32_t hi, double t) {
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if (kt[m - first] < t) lo = m + 1; else hi = m;
    }
    const uint32_t a = lo;
    if (a == K) return K - 1;
    if (a > 0) {
        const double d0 = t - kt[a - 1 - first], d1 = kt[a - first] - t;
        if (__dmul_rn(d0, d0) <= __dmul_rn(d1, d1)) return a - 1;
    }
    return a;
}

}  // namespace ecal
