// Image undistortion with the solved camera (include/ecal.h, "image undistortion"): batches of u8 frames onto the ideal pinhole
// camera's canvas, by the reference's scattered-data average (REFERENCE) or through rectification maps and a bilinear sample
// (BILINEAR), and the forward projection the maps are made of.  What decides — positions, neighbours, weights, the order of
// accumulation, the Newton steps, the bilinear sample, the rounding to u8 — is image_undistort.hpp's (shared with the host entry
// points and the CPU test); design/22_image_undistort.md has the reasoning and what was measured.
//
// A plan holds what depends on the camera, the sensor and the canvas alone; applying it reads tables and frames.  NO workgroup waits on
// another, and nothing depends on the order in which atomics land (they are integer sums, minima and maxima).
//
// REFERENCE, the plan:
//   image_position_kernel   a thread per source pixel: its canvas position (cu, cv) and cell key, val = idx
//   rocPRIM radix sort      the pairs, stably, on the bits that hold every key: a cell's sources are one run of ascending idx, and a
//                           row of four cells is one run too
//   image_start_kernel      start[c] for the cells + 1 (a lower-bound search of the sorted keys each)
//   image_count_kernel      a thread per canvas pixel: its neighbours among the 4 x 4 cells that can hold one; per-block sums
//   ecal_scan_blocks        the blocks' first entry
//   image_fill_kernel       the pixel's first entry (a scan inside the block) and its entries (u32 idx, f64 w) in the stated order
// REFERENCE, applying:
//   image_gather_kernel     a thread per canvas pixel and IMG_FRAMES frames: an entry is read once for those frames; the averages go to
//                           context scratch as f32, the frames' min / max (values >= 0: their bit patterns order as u32) are reduced in
//                           the workgroup and stored, a pair per workgroup and frame
//   image_minmax_kernel     a workgroup per frame: the min / max over those pairs (merging them with atomicMin / atomicMax into one
//                           word a frame was nine tenths of the gather's time: design/22_image_undistort.md)
//   image_finish_kernel     f32 -> u8 by the options' normalize, four bytes a thread, aligned 4-byte stores
// BILINEAR:
//   image_maps_kernel       a thread per canvas pixel: eight Newton steps, map_x, map_y, valid
//   image_remap_kernel      a thread per four canvas pixels and IMG_FRAMES frames: a map word is read once for those frames; u8 straight
//                           out with aligned 4-byte stores (normalize 0, no min / max asked), else f32 to scratch and image_finish_kernel
#include "ecal_ctx.hpp"
#include "block_utils.hpp"
#include "image_undistort.hpp"

#include <rocprim/rocprim.hpp>   // (behind ecal_ctx.hpp, as in ecal_sort.hip: its headers use the host's string.h)

struct ecal_image_plan {
    ecal_ctx *ctx = nullptr;
    ecal_image::Camera cam;
    ecal_image::Options opt;
    ecal_image::Forward fwd;
    ecal_image::Info info;
    uint32_t W = 0, H = 0;
    ecal_devbuf off, idx, w;       // REFERENCE: u32 [canvas pixels + 1], u32 [n_entries], f64 [n_entries]
    ecal_devbuf mx, my, valid;     // BILINEAR: f32, f32, u8 [canvas pixels]
};

namespace ecal {

using namespace ecal_image;

constexpr int IMG_T = 256;
constexpr uint32_t IMG_FRAMES = 4;            // frames per thread of the applying kernels
constexpr uint32_t IMG_MIN_INIT = 0x7F800000u;   // +inf: above every value

// counters: [0] invalid sources
__global__ __launch_bounds__(IMG_T) void image_position_kernel(const Camera cam, const Options opt, uint32_t W, uint32_t n_src, uint32_t n_cells,
                                                               double *__restrict__ cu, double *__restrict__ cv, uint32_t *__restrict__ key,
                                                               uint32_t *__restrict__ val, unsigned long long *__restrict__ counters) {
    __shared__ uint32_t s_red[IMG_T / 64];
    const uint32_t idx = blockIdx.x * IMG_T + threadIdx.x;
    uint32_t inv = 0;
    if (idx < n_src) {
        double x, y;
        bool invalid;
        const uint32_t k = img_source_cell(cam, opt, idx % W, idx / W, &x, &y, &invalid);
        cu[idx] = x;
        cv[idx] = y;
        key[idx] = k == IMG_NO_CELL ? n_cells : k;
        val[idx] = idx;
        inv = invalid ? 1u : 0u;
    }
    inv = block_sum<IMG_T>(inv, s_red);
    if (threadIdx.x == 0 && inv) atomicAdd(&counters[0], (unsigned long long) inv);
}

// thread c: start[c] = the first sorted position whose key is >= c, for c <= n_cells
__global__ __launch_bounds__(IMG_T) void image_start_kernel(const uint32_t *__restrict__ skey, uint32_t n_src, uint32_t n_cells,
                                                            uint32_t *__restrict__ start) {
    const uint32_t c = blockIdx.x * IMG_T + threadIdx.x;
    if (c > n_cells) return;
    uint32_t a = 0, b = n_src;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2u;
        if (skey[m] < c) a = m + 1u;
        else b = m;
    }
    start[c] = a;
}

// cnt [np]: the pixel's neighbours; block_cnt: their sum over the block; counters: [1] empty pixels, [2] the most neighbours of a pixel
__global__ __launch_bounds__(IMG_T) void image_count_kernel(const Options opt, uint32_t np, const uint32_t *__restrict__ start,
                                                            const uint32_t *__restrict__ sidx, const double *__restrict__ cu,
                                                            const double *__restrict__ cv, uint32_t *__restrict__ cnt,
                                                            uint32_t *__restrict__ block_cnt, unsigned long long *__restrict__ counters) {
    __shared__ uint32_t s_red[2][IMG_T / 64];
    const uint32_t p = blockIdx.x * IMG_T + threadIdx.x;
    uint32_t n = 0, empty = 0;
    if (p < np) {
        n = img_neighbours(opt, p % opt.out_width, p / opt.out_width, start, sidx, cu, cv, [](uint32_t, double) {});
        cnt[p] = n;
        empty = n ? 0u : 1u;
    }
    uint32_t most = n;
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_down(most, o, 64);
        most = other > most ? other : most;
    }
    if ((threadIdx.x & 63) == 0 && most) atomicMax(&counters[2], (unsigned long long) most);
    const uint32_t total = block_sum<IMG_T>(n, s_red[0]);
    empty = block_sum<IMG_T>(empty, s_red[1]);
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = total;
        if (empty) atomicAdd(&counters[1], (unsigned long long) empty);
    }
}

// cnt_off [np + 1]: in, the pixel's neighbours (each thread reads its own word alone); out, its first entry, and the total behind
__global__ __launch_bounds__(IMG_T) void image_fill_kernel(const Options opt, uint32_t np, const uint32_t *__restrict__ start,
                                                           const uint32_t *__restrict__ sidx, const double *__restrict__ cu,
                                                           const double *__restrict__ cv, const uint32_t *__restrict__ block_off,
                                                           uint32_t *__restrict__ cnt_off, uint32_t *__restrict__ t_idx, double *__restrict__ t_w) {
    __shared__ uint32_t s_wsum[IMG_T / 64];
    const uint32_t p = blockIdx.x * IMG_T + threadIdx.x;
    const uint32_t mine = p < np ? cnt_off[p] : 0u;
    const uint32_t before = block_exscan_u32<IMG_T>(mine, s_wsum);
    if (p >= np) return;
    const uint32_t first = block_off[blockIdx.x] + before;
    cnt_off[p] = first;
    if (p == np - 1u) cnt_off[np] = first + mine;
    uint32_t at = first;
    (void) img_neighbours(opt, p % opt.out_width, p / opt.out_width, start, sidx, cu, cv, [&](uint32_t idx, double w) {
        t_idx[at] = idx;   // (at < first + mine: the counting pass walked the same sources with the same test)
        t_w[at] = w;
        at++;
    });
}

// A frame's min and max over the workgroup, without atomics: the waves' own (shuffles; the values are >= 0, so their f32 bit patterns
// order as u32) into s_mm[slot], and behind one barrier img_store_minmax writes the workgroup's pair to part[frame][blockIdx.x]
__device__ __forceinline__ void img_wave_minmax(float lo, float hi, uint32_t (*s_mm)[2][IMG_T / 64], uint32_t slot) {
    uint32_t a = __float_as_uint(lo), b = __float_as_uint(hi);
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t oa = __shfl_down(a, o, 64), ob = __shfl_down(b, o, 64);
        a = oa < a ? oa : a;
        b = ob > b ? ob : b;
    }
    if ((threadIdx.x & 63) == 0) {
        s_mm[slot][0][threadIdx.x >> 6] = a;
        s_mm[slot][1][threadIdx.x >> 6] = b;
    }
}
// part [N][gridDim.x][2]; called by every thread of the workgroup once all nf slots are written
__device__ __forceinline__ void img_store_minmax(uint32_t (*s_mm)[2][IMG_T / 64], uint32_t f0, uint32_t nf, uint32_t *__restrict__ part) {
    __syncthreads();
    if (threadIdx.x < nf) {
        uint32_t a = s_mm[threadIdx.x][0][0], b = s_mm[threadIdx.x][1][0];
        for (int w = 1; w < IMG_T / 64; w++) {
            a = s_mm[threadIdx.x][0][w] < a ? s_mm[threadIdx.x][0][w] : a;
            b = s_mm[threadIdx.x][1][w] > b ? s_mm[threadIdx.x][1][w] : b;
        }
        uint32_t *d = part + ((size_t) (f0 + threadIdx.x) * gridDim.x + blockIdx.x) * 2u;
        d[0] = a;
        d[1] = b;
    }
}

// frame f = blockIdx.x: mm[f] = the min and max over its n_parts workgroup pairs
__global__ __launch_bounds__(IMG_T) void image_minmax_kernel(const uint32_t *__restrict__ part, uint32_t n_parts, uint32_t *__restrict__ mm) {
    __shared__ uint32_t s_mm[1][2][IMG_T / 64];
    const uint32_t *p = part + (size_t) blockIdx.x * n_parts * 2u;
    uint32_t a = IMG_MIN_INIT, b = 0u;
    for (uint32_t k = threadIdx.x; k < n_parts; k += IMG_T) {
        a = p[2u * k] < a ? p[2u * k] : a;
        b = p[2u * k + 1u] > b ? p[2u * k + 1u] : b;
    }
    img_wave_minmax(__uint_as_float(a), __uint_as_float(b), s_mm, 0);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < IMG_T / 64; w++) {
            a = s_mm[0][0][w] < a ? s_mm[0][0][w] : a;
            b = s_mm[0][1][w] > b ? s_mm[0][1][w] : b;
        }
        mm[2u * blockIdx.x] = a;
        mm[2u * blockIdx.x + 1u] = b;
    }
}

// blockIdx.y: frames f0 = IMG_FRAMES * blockIdx.y .. ; val [N][np][C] f32
template <uint32_t C>
__global__ __launch_bounds__(IMG_T) void image_gather_kernel(const uint32_t *__restrict__ off, const uint32_t *__restrict__ t_idx,
                                                             const double *__restrict__ t_w, const uint8_t *__restrict__ src, uint32_t n_src,
                                                             uint32_t np, uint32_t N, float *__restrict__ val, uint32_t *__restrict__ part) {
    __shared__ uint32_t s_mm[IMG_FRAMES][2][IMG_T / 64];
    const uint32_t p = blockIdx.x * IMG_T + threadIdx.x;
    const uint32_t f0 = blockIdx.y * IMG_FRAMES, nf = N - f0 < IMG_FRAMES ? N - f0 : IMG_FRAMES;   // (the same for the whole block)
    float acc[IMG_FRAMES][C];
#pragma unroll
    for (uint32_t f = 0; f < IMG_FRAMES; f++)
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) acc[f][ch] = 0.0f;
    double wsum = 0.0;
    const bool live = p < np;
    const uint32_t a = live ? off[p] : 0u, b = live ? off[p + 1u] : 0u;
    for (uint32_t e = a; e < b; e++) {
        const uint32_t id = t_idx[e];
        const double w = t_w[e];
        wsum = wsum + w;
#pragma unroll
        for (uint32_t f = 0; f < IMG_FRAMES; f++) {
            if (f < nf) {
                const uint8_t *s = src + ((size_t) (f0 + f) * n_src + id) * C;
#pragma unroll
                for (uint32_t ch = 0; ch < C; ch++) acc[f][ch] = img_accumulate(acc[f][ch], w, s[ch]);
            }
        }
    }
#pragma unroll
    for (uint32_t f = 0; f < IMG_FRAMES; f++) {
        if (f < nf) {
            float lo = __uint_as_float(IMG_MIN_INIT), hi = 0.0f;
            if (live) {
                float *d = val + ((size_t) (f0 + f) * np + p) * C;
#pragma unroll
                for (uint32_t ch = 0; ch < C; ch++) {
                    const float v = img_average(acc[f][ch], wsum, b > a);
                    d[ch] = v;
                    lo = v < lo ? v : lo;
                    hi = v > hi ? v : hi;
                }
            }
            img_wave_minmax(lo, hi, s_mm, f);
        }
    }
    img_store_minmax(s_mm, f0, nf, part);
}

// thread q: canvas pixels 4q .. 4q + 3 of frames f0 .. ; dst (DIRECT) [N][np][C] u8, else val [N][np][C] f32 and mm
template <uint32_t C, bool DIRECT>
__global__ __launch_bounds__(IMG_T) void image_remap_kernel(const float *__restrict__ map_x, const float *__restrict__ map_y,
                                                            const uint8_t *__restrict__ src, uint32_t W, uint32_t H, uint32_t np, uint32_t N,
                                                            uint8_t *__restrict__ dst, float *__restrict__ val, uint32_t *__restrict__ part) {
    __shared__ uint32_t s_mm[DIRECT ? 1 : IMG_FRAMES][2][IMG_T / 64];
    const uint32_t p0 = (blockIdx.x * IMG_T + threadIdx.x) * 4u;
    const uint32_t f0 = blockIdx.y * IMG_FRAMES, nf = N - f0 < IMG_FRAMES ? N - f0 : IMG_FRAMES;   // (the same for the whole block)
    const uint32_t have = p0 < np ? (np - p0 < 4u ? np - p0 : 4u) : 0u;
    float mx[4], my[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        mx[k] = k < have ? map_x[p0 + k] : -1.0f;
        my[k] = k < have ? map_y[p0 + k] : -1.0f;
    }
    const size_t n_src = (size_t) W * H;
#pragma unroll
    for (uint32_t f = 0; f < IMG_FRAMES; f++) {
        if (f < nf) {
            const uint8_t *s = src + (size_t) (f0 + f) * n_src * C;
            float v[4][C];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
                for (uint32_t ch = 0; ch < C; ch++) v[k][ch] = k < have ? img_bilinear(s, W, H, C, ch, mx[k], my[k]) : 0.0f;
            const size_t at = ((size_t) (f0 + f) * np + p0) * C;
            if (DIRECT) {
                uint8_t bytes[4 * C];
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
                    for (uint32_t ch = 0; ch < C; ch++) bytes[k * C + ch] = img_to_u8(v[k][ch]);
                uint8_t *d = dst + at;
                if (have == 4u && ((uintptr_t) d & 3u) == 0u) {   // whole, aligned words
#pragma unroll
                    for (uint32_t wd = 0; wd < C; wd++) {
                        const uint32_t word = (uint32_t) bytes[4 * wd] | ((uint32_t) bytes[4 * wd + 1] << 8) | ((uint32_t) bytes[4 * wd + 2] << 16) |
                                              ((uint32_t) bytes[4 * wd + 3] << 24);
                        reinterpret_cast<uint32_t *>(d)[wd] = word;
                    }
                } else {
                    for (uint32_t j = 0; j < have * C; j++) d[j] = bytes[j];
                }
            } else {
                float lo = __uint_as_float(IMG_MIN_INIT), hi = 0.0f;
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    if (k < have) {
#pragma unroll
                        for (uint32_t ch = 0; ch < C; ch++) {
                            val[at + k * C + ch] = v[k][ch];
                            lo = v[k][ch] < lo ? v[k][ch] : lo;
                            hi = v[k][ch] > hi ? v[k][ch] : hi;
                        }
                    }
                }
                img_wave_minmax(lo, hi, s_mm, f);
            }
        }
    }
    if (!DIRECT) img_store_minmax(s_mm, f0, nf, part);
}

// val [total] f32 -> dst [total] u8, frames of frame_bytes values each; thread t: the four bytes of an aligned word of dst (the
// bytes in front of the first boundary and behind the last whole word go to the threads of the first block one by one)
__global__ __launch_bounds__(IMG_T) void image_finish_kernel(const float *__restrict__ val, const uint32_t *__restrict__ mm, uint64_t frame_bytes,
                                                             uint64_t total, uint32_t normalize, uint8_t *__restrict__ dst) {
    uint64_t head = (uint64_t) ((4u - ((uintptr_t) dst & 3u)) & 3u);
    head = head < total ? head : total;
    const uint64_t nw = (total - head) / 4u, tail0 = head + 4u * nw;
    auto convert = [&](uint64_t g0, uint32_t n, uint8_t *out) {   // bytes g0 .. g0 + n - 1
        uint64_t f = g0 / frame_bytes, rem = g0 - f * frame_bytes;
        float mn = 0.0f;
        double scale = 0.0;
        bool known = false;
        for (uint32_t k = 0; k < n; k++) {
            if (rem >= frame_bytes) rem = 0, f++, known = false;
            if (normalize && !known) {
                mn = __uint_as_float(mm[2u * f]);
                scale = img_norm_scale(mn, __uint_as_float(mm[2u * f + 1u]));
                known = true;
            }
            const float v = val[g0 + k];
            out[k] = normalize ? img_to_u8_normalized(v, mn, scale) : img_to_u8(v);
            rem++;
        }
    };
    const uint64_t t = (uint64_t) blockIdx.x * IMG_T + threadIdx.x;
    if (t < nw) {
        uint8_t b[4];
        convert(head + 4u * t, 4u, b);
        *reinterpret_cast<uint32_t *>(dst + head + 4u * t) = (uint32_t) b[0] | ((uint32_t) b[1] << 8) | ((uint32_t) b[2] << 16) | ((uint32_t) b[3] << 24);
    }
    if (blockIdx.x == 0) {
        uint8_t b;
        if (threadIdx.x < head) convert(threadIdx.x, 1u, &b), dst[threadIdx.x] = b;
        if (threadIdx.x >= 64 && tail0 + (threadIdx.x - 64u) < total) convert(tail0 + (threadIdx.x - 64u), 1u, &b), dst[tail0 + (threadIdx.x - 64u)] = b;
    }
}

// counters: [0] invalid, [1] not converged
__global__ __launch_bounds__(IMG_T) void image_maps_kernel(const Camera cam, const Forward fwd, const Options opt, uint32_t np,
                                                           float *__restrict__ map_x, float *__restrict__ map_y, uint8_t *__restrict__ valid,
                                                           unsigned long long *__restrict__ counters) {
    __shared__ uint32_t s_red[2][IMG_T / 64];
    const uint32_t p = blockIdx.x * IMG_T + threadIdx.x;
    uint32_t inv = 0, slow = 0;
    if (p < np) {
        float mx, my;
        uint8_t ok;
        const uint8_t flag = img_map_pixel(cam, fwd, opt, p % opt.out_width, p / opt.out_width, &mx, &my, &ok);
        map_x[p] = mx;
        map_y[p] = my;
        valid[p] = ok;
        inv = flag == IMG_DISTORT_INVALID ? 1u : 0u;
        slow = flag == IMG_DISTORT_NOT_CONVERGED ? 1u : 0u;
    }
    inv = block_sum<IMG_T>(inv, s_red[0]);
    slow = block_sum<IMG_T>(slow, s_red[1]);
    if (threadIdx.x == 0 && inv) atomicAdd(&counters[0], (unsigned long long) inv);
    if (threadIdx.x == 1 && slow) atomicAdd(&counters[1], (unsigned long long) slow);
}

// uv [n][2] -> out [n][2] (0, 0 where invalid), flag [n]
__global__ __launch_bounds__(IMG_T) void image_distort_points_kernel(const Camera cam, const Forward fwd, const double *__restrict__ uv, uint64_t n,
                                                                     double *__restrict__ out, uint8_t *__restrict__ flag) {
    const uint64_t i = (uint64_t) blockIdx.x * IMG_T + threadIdx.x;
    if (i >= n) return;
    double u = 0.0, v = 0.0;
    const uint8_t fl = img_distort_point(cam, fwd, uv[2 * i], uv[2 * i + 1], &u, &v);
    const bool ok = fl != IMG_DISTORT_INVALID;
    out[2 * i] = ok ? u : 0.0;
    out[2 * i + 1] = ok ? v : 0.0;
    flag[i] = fl;
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_image_options) == sizeof(Options) && sizeof(ecal_image_options) == 40, "the options are the shared header's, no padding");
static_assert(sizeof(ecal_image_info) == sizeof(Info) && sizeof(ecal_image_info) == 112, "the info is the shared header's");
static_assert(ECAL_IMAGE_REFERENCE == IMG_REFERENCE && ECAL_IMAGE_BILINEAR == IMG_BILINEAR, "the shared header's constants");
static_assert(ECAL_DISTORT_INVALID == IMG_DISTORT_INVALID && ECAL_DISTORT_NOT_CONVERGED == IMG_DISTORT_NOT_CONVERGED, "the shared header's flags");

static Camera image_camera(const ecal_undistort_camera *cam) {
    Camera c;
    memcpy(&c, cam, sizeof(c));
    return c;
}

// NULL: the reference's options can only be had for a sensor — a missing pointer is refused
static bool image_options(const ecal_image_options *opt, Options *o) {
    if (!opt) return false;
    memcpy(o, opt, sizeof(*o));
    return true;
}

extern "C" void ecal_image_reference_options(uint32_t width, uint32_t height, ecal_image_options *opt) {
    if (!opt) return;
    const Options o = img_reference_options(width, height);
    memcpy(opt, &o, sizeof(o));
}

extern "C" const char *ecal_image_options_error(const ecal_image_options *opt) {
    Options o;
    if (!image_options(opt, &o)) return "null options";
    return img_options_error(o);
}

// the camera, the sensor and the options of an entry point without a context: NULL, or the refused field
static const char *image_arguments_error(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt) {
    if (const char *bad = ecal_undistort_camera_error(cam)) return bad;
    if (const char *bad = img_sensor_error(width, height)) return bad;
    return ecal_image_options_error(opt);
}

extern "C" int ecal_camera_monotone_radius(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, double *r_lim, uint32_t *truncated) {
    if (ecal_undistort_camera_error(cam) || img_sensor_error(width, height)) return ECAL_ERR_INVALID;
    const Forward f = img_forward(image_camera(cam), width, height);
    if (r_lim) *r_lim = f.r_lim;
    if (truncated) *truncated = f.truncated;
    return ECAL_OK;
}

extern "C" int ecal_distort_points_host(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const double *uv, uint64_t n, double *out,
                                        uint8_t *flag) {
    if (ecal_undistort_camera_error(cam) || img_sensor_error(width, height) || (n && (!uv || !out || !flag))) return ECAL_ERR_INVALID;
    const Camera c = image_camera(cam);
    const Forward f = img_forward(c, width, height);
    for (uint64_t i = 0; i < n; i++) {
        double u = 0.0, v = 0.0;
        const uint8_t fl = img_distort_point(c, f, uv[2 * i], uv[2 * i + 1], &u, &v);
        const bool ok = fl != IMG_DISTORT_INVALID;
        out[2 * i] = ok ? u : 0.0;
        out[2 * i + 1] = ok ? v : 0.0;
        flag[i] = fl;
    }
    return ECAL_OK;
}

extern "C" int ecal_undistort_image_host(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt,
                                         const uint8_t *src, uint8_t *dst, float *minmax, ecal_image_info *info) {
    if (info) memset(info, 0, sizeof(*info));
    if (image_arguments_error(cam, width, height, opt) || !src || !dst) return ECAL_ERR_INVALID;
    Options o;
    image_options(opt, &o);
    Info I;
    img_undistort_sequential(image_camera(cam), width, height, o, src, dst, minmax, &I);
    if (info) memcpy(info, &I, sizeof(I));
    return ECAL_OK;
}

extern "C" int ecal_image_table_host(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt, uint32_t *off,
                                     uint32_t *idx, double *w, uint64_t capacity, ecal_image_info *info) {
    if (info) memset(info, 0, sizeof(*info));
    if (image_arguments_error(cam, width, height, opt) || !off || (capacity && (!idx || !w))) return ECAL_ERR_INVALID;
    Options o;
    image_options(opt, &o);
    if (o.method != IMG_REFERENCE) return ECAL_ERR_INVALID;
    const Table t = img_table_sequential(image_camera(cam), width, height, o);
    memcpy(off, t.off.data(), t.off.size() * sizeof(uint32_t));
    const size_t n = t.idx.size() < capacity ? t.idx.size() : (size_t) capacity;
    if (n) memcpy(idx, t.idx.data(), n * sizeof(uint32_t)), memcpy(w, t.w.data(), n * sizeof(double));
    if (info) {
        Info I;
        memset(&I, 0, sizeof(I));
        I.opt = o, I.width = width, I.height = height;
        I.n_invalid_sources = t.n_invalid_sources, I.n_empty = t.n_empty, I.n_entries = t.idx.size(), I.max_neighbours = t.max_neighbours;
        memcpy(info, &I, sizeof(I));
    }
    return ECAL_OK;
}

extern "C" int ecal_image_maps_host(const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt, float *map_x,
                                    float *map_y, uint8_t *valid, ecal_image_info *info) {
    if (info) memset(info, 0, sizeof(*info));
    if (image_arguments_error(cam, width, height, opt) || !map_x || !map_y) return ECAL_ERR_INVALID;
    Options o;
    image_options(opt, &o);
    const Camera c = image_camera(cam);
    const Forward f = img_forward(c, width, height);
    const Maps m = img_maps_sequential(c, f, o);
    memcpy(map_x, m.mx.data(), m.mx.size() * sizeof(float));
    memcpy(map_y, m.my.data(), m.my.size() * sizeof(float));
    if (valid) memcpy(valid, m.valid.data(), m.valid.size());
    if (info) {
        Info I;
        memset(&I, 0, sizeof(I));
        I.opt = o, I.width = width, I.height = height;
        I.r_lim = f.r_lim, I.truncated = f.truncated, I.n_invalid = m.n_invalid, I.n_not_converged = m.n_not_converged, I.n_empty = m.n_invalid;
        memcpy(info, &I, sizeof(I));
    }
    return ECAL_OK;
}

extern "C" int ecal_distort_points_dev(ecal_ctx *ctx, const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const double *d_uv, uint64_t n,
                                       double *d_out, uint8_t *d_flag, void *stream) {
    const ecal_range range__(ctx, "ecal_distort_points");
    if (!ctx) return ECAL_ERR_INVALID;
    if (n && (!d_uv || !d_out || !d_flag)) {
        ctx->last_error = "ecal_distort_points: null pointer (uv, out or flag)";
        return ECAL_ERR_INVALID;
    }
    const char *bad = ecal_undistort_camera_error(cam);
    if (!bad) bad = img_sensor_error(width, height);
    if (bad) {
        ctx->last_error = std::string("ecal_distort_points: ") + bad;
        return ECAL_ERR_INVALID;
    }
    if (n > 0xFFFFFFFFull) {
        ctx->last_error = "ecal_distort_points: more than 2^32-1 points";
        return ECAL_ERR_RANGE;
    }
    if (!n) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Camera c = image_camera(cam);
    hipLaunchKernelGGL(image_distort_points_kernel, dim3((uint32_t) ((n + IMG_T - 1) / IMG_T)), dim3(IMG_T), 0, (hipStream_t) stream, c,
                       img_forward(c, width, height), d_uv, n, d_out, d_flag);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

namespace {
inline size_t up256(size_t v) { return (v + 255) & ~(size_t) 255; }
// ctx->image_scratch while a REFERENCE plan is built
struct plan_layout {
    size_t o_cu, o_cv, o_kin, o_kout, o_vin, o_vout, o_start, o_bcnt, o_boff, o_counters, o_tmp, total;
    plan_layout(size_t n_src, size_t n_cells, size_t nb, size_t tmp_bytes) {
        size_t at = 0;
        o_cu = at, at += up256(n_src * 8);
        o_cv = at, at += up256(n_src * 8);
        o_kin = at, at += up256(n_src * 4);
        o_kout = at, at += up256(n_src * 4);
        o_vin = at, at += up256(n_src * 4);
        o_vout = at, at += up256(n_src * 4);
        o_start = at, at += up256((n_cells + 1) * 4);
        o_bcnt = at, at += up256(nb * 4);
        o_boff = at, at += up256((nb + 1) * 4);
        o_counters = at, at += 256;
        o_tmp = at, at += tmp_bytes;
        total = at;
    }
};
uint32_t key_bits(uint32_t largest) {
    uint32_t b = 1;
    while (b < 32 && (largest >> b) != 0u) b++;
    return b;
}
}  // namespace

static int image_build_reference(ecal_ctx *ctx, ecal_image_plan *pl, hipStream_t st) {
    const Options &o = pl->opt;
    const uint32_t n_src = pl->W * pl->H, n_cells = img_cell_count(o), np = o.out_width * o.out_height;   // <= 8192^2, 8196^2
    const uint32_t nb = (np + IMG_T - 1) / IMG_T, bits = key_bits(n_cells);
    size_t tmp_bytes = 0;
    uint32_t *k_in = nullptr, *k_out = nullptr, *v_in = nullptr, *v_out = nullptr;
    ECAL_HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, (size_t) n_src, 0, bits, st));
    const plan_layout L(n_src, n_cells, nb, tmp_bytes);
    int rc = ecal_ensure(ctx, ctx->image_scratch, L.total);
    if (rc) return rc;
    if ((rc = ecal_ensure(ctx, pl->off, ((size_t) np + 1) * 4))) return rc;
    uint8_t *base = ctx->image_scratch.as<uint8_t>();
    double *cu = reinterpret_cast<double *>(base + L.o_cu), *cv = reinterpret_cast<double *>(base + L.o_cv);
    k_in = reinterpret_cast<uint32_t *>(base + L.o_kin), k_out = reinterpret_cast<uint32_t *>(base + L.o_kout);
    v_in = reinterpret_cast<uint32_t *>(base + L.o_vin), v_out = reinterpret_cast<uint32_t *>(base + L.o_vout);
    uint32_t *start = reinterpret_cast<uint32_t *>(base + L.o_start), *bcnt = reinterpret_cast<uint32_t *>(base + L.o_bcnt);
    uint32_t *boff = reinterpret_cast<uint32_t *>(base + L.o_boff), *cnt_off = pl->off.as<uint32_t>();
    unsigned long long *counters = reinterpret_cast<unsigned long long *>(base + L.o_counters);
    ECAL_HIP_TRY(ctx, hipMemsetAsync(counters, 0, 256, st));
    hipLaunchKernelGGL(image_position_kernel, dim3((n_src + IMG_T - 1) / IMG_T), dim3(IMG_T), 0, st, pl->cam, o, pl->W, n_src, n_cells, cu, cv, k_in, v_in,
                       counters);
    ECAL_HIP_TRY(ctx, rocprim::radix_sort_pairs(base + L.o_tmp, tmp_bytes, k_in, k_out, v_in, v_out, (size_t) n_src, 0, bits, st));   // (stable)
    hipLaunchKernelGGL(image_start_kernel, dim3((n_cells + 1 + IMG_T - 1) / IMG_T), dim3(IMG_T), 0, st, (const uint32_t *) k_out, n_src, n_cells, start);
    hipLaunchKernelGGL(image_count_kernel, dim3(nb), dim3(IMG_T), 0, st, o, np, (const uint32_t *) start, (const uint32_t *) v_out, (const double *) cu,
                       (const double *) cv, cnt_off, bcnt, counters);
    if ((rc = ecal_scan_blocks(ctx, bcnt, nb, boff, st))) return rc;
    unsigned long long h_counters[3] = {0, 0, 0};
    uint32_t n_entries = 0;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(&n_entries, boff + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    if ((rc = ecal_ensure(ctx, pl->idx, ((size_t) n_entries + 1) * 4)) || (rc = ecal_ensure(ctx, pl->w, ((size_t) n_entries + 1) * 8))) return rc;
    hipLaunchKernelGGL(image_fill_kernel, dim3(nb), dim3(IMG_T), 0, st, o, np, (const uint32_t *) start, (const uint32_t *) v_out, (const double *) cu,
                       (const double *) cv, (const uint32_t *) boff, cnt_off, pl->idx.as<uint32_t>(), pl->w.as<double>());
    ECAL_HIP_TRY(ctx, hipGetLastError());
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));   // (the scratch is the context's: the next plan may take it)
    pl->info.n_invalid_sources = h_counters[0];
    pl->info.n_empty = h_counters[1];
    pl->info.max_neighbours = (uint32_t) h_counters[2];
    pl->info.n_entries = n_entries;
    pl->info.bytes = pl->off.cap + pl->idx.cap + pl->w.cap;
    return ECAL_OK;
}

static int image_build_bilinear(ecal_ctx *ctx, ecal_image_plan *pl, hipStream_t st) {
    const Options &o = pl->opt;
    const uint32_t np = o.out_width * o.out_height;
    int rc;
    if ((rc = ecal_ensure(ctx, pl->mx, (size_t) np * 4)) || (rc = ecal_ensure(ctx, pl->my, (size_t) np * 4)) || (rc = ecal_ensure(ctx, pl->valid, np)) ||
        (rc = ecal_ensure(ctx, ctx->image_scratch, 256)))
        return rc;
    unsigned long long *counters = ctx->image_scratch.as<unsigned long long>();
    ECAL_HIP_TRY(ctx, hipMemsetAsync(counters, 0, 256, st));
    hipLaunchKernelGGL(image_maps_kernel, dim3((np + IMG_T - 1) / IMG_T), dim3(IMG_T), 0, st, pl->cam, pl->fwd, o, np, pl->mx.as<float>(),
                       pl->my.as<float>(), pl->valid.as<uint8_t>(), counters);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    unsigned long long h_counters[2] = {0, 0};
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    pl->info.n_invalid = h_counters[0];
    pl->info.n_not_converged = h_counters[1];
    pl->info.n_empty = h_counters[0];
    pl->info.r_lim = pl->fwd.r_lim;
    pl->info.truncated = pl->fwd.truncated;
    pl->info.bytes = pl->mx.cap + pl->my.cap + pl->valid.cap;
    return ECAL_OK;
}

extern "C" int ecal_image_plan_create(ecal_ctx *ctx, const ecal_undistort_camera *cam, uint32_t width, uint32_t height, const ecal_image_options *opt,
                                      ecal_image_plan **plan) {
    const ecal_range range__(ctx, "ecal_image_plan_create");
    if (!ctx || !plan) return ECAL_ERR_INVALID;
    *plan = nullptr;
    if (const char *bad = image_arguments_error(cam, width, height, opt)) {
        ctx->last_error = std::string("ecal_image_plan_create: ") + bad;
        return ECAL_ERR_INVALID;
    }
    Options o;
    image_options(opt, &o);
    // every source neighbours at most 13 canvas pixels
    if (o.method == IMG_REFERENCE && (uint64_t) width * height * IMG_MAX_PER_SOURCE > 0xFFFFFFFFull) {
        ctx->last_error = "ecal_image_plan_create: more than 2^32-1 table entries";
        return ECAL_ERR_RANGE;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ecal_image_plan *pl = new (std::nothrow) ecal_image_plan();
    if (!pl) return ECAL_ERR_NOMEM;
    pl->ctx = ctx;
    pl->cam = image_camera(cam);
    pl->opt = o;
    pl->W = width, pl->H = height;
    pl->fwd = img_forward(pl->cam, width, height);
    memset(&pl->info, 0, sizeof(pl->info));
    pl->info.opt = o;
    pl->info.width = width, pl->info.height = height;
    const int rc = o.method == IMG_REFERENCE ? image_build_reference(ctx, pl, ctx->stream) : image_build_bilinear(ctx, pl, ctx->stream);
    if (rc) {
        (void) hipStreamSynchronize(ctx->stream);
        delete pl;
        return rc;
    }
    *plan = pl;
    return ECAL_OK;
}

extern "C" void ecal_image_plan_destroy(ecal_image_plan *plan) {
    if (!plan) return;
    (void) hipSetDevice(plan->ctx->device);
    delete plan;
}

extern "C" int ecal_image_plan_info(const ecal_image_plan *plan, ecal_image_info *info) {
    if (!plan || !info) return ECAL_ERR_INVALID;
    memcpy(info, &plan->info, sizeof(*info));
    return ECAL_OK;
}

extern "C" int ecal_image_plan_maps_dev(const ecal_image_plan *plan, float *d_map_x, float *d_map_y, uint8_t *d_valid, void *stream) {
    if (!plan) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = plan->ctx;
    if (plan->opt.method != IMG_BILINEAR) {
        ctx->last_error = "ecal_image_plan_maps: a REFERENCE plan has no maps";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    const size_t np = (size_t) plan->opt.out_width * plan->opt.out_height;
    if (d_map_x) ECAL_HIP_TRY(ctx, hipMemcpyAsync(d_map_x, plan->mx.ptr, np * 4, hipMemcpyDeviceToDevice, st));
    if (d_map_y) ECAL_HIP_TRY(ctx, hipMemcpyAsync(d_map_y, plan->my.ptr, np * 4, hipMemcpyDeviceToDevice, st));
    if (d_valid) ECAL_HIP_TRY(ctx, hipMemcpyAsync(d_valid, plan->valid.ptr, np, hipMemcpyDeviceToDevice, st));
    return ECAL_OK;
}

extern "C" int ecal_image_plan_maps(const ecal_image_plan *plan, float *map_x, float *map_y, uint8_t *valid) {
    if (!plan) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = plan->ctx;
    if (plan->opt.method != IMG_BILINEAR) {
        ctx->last_error = "ecal_image_plan_maps: a REFERENCE plan has no maps";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t) plan->opt.out_width * plan->opt.out_height;
    if (map_x) ECAL_HIP_TRY(ctx, hipMemcpyAsync(map_x, plan->mx.ptr, np * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (map_y) ECAL_HIP_TRY(ctx, hipMemcpyAsync(map_y, plan->my.ptr, np * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (valid) ECAL_HIP_TRY(ctx, hipMemcpyAsync(valid, plan->valid.ptr, np, hipMemcpyDeviceToHost, ctx->stream));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ECAL_OK;
}

extern "C" int ecal_image_plan_table(const ecal_image_plan *plan, uint32_t *off, uint32_t *idx, double *w) {
    if (!plan) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = plan->ctx;
    if (plan->opt.method != IMG_REFERENCE) {
        ctx->last_error = "ecal_image_plan_table: a BILINEAR plan has no table";
        return ECAL_ERR_INVALID;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t) plan->opt.out_width * plan->opt.out_height, ne = (size_t) plan->info.n_entries;
    if (off) ECAL_HIP_TRY(ctx, hipMemcpyAsync(off, plan->off.ptr, (np + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (idx && ne) ECAL_HIP_TRY(ctx, hipMemcpyAsync(idx, plan->idx.ptr, ne * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (w && ne) ECAL_HIP_TRY(ctx, hipMemcpyAsync(w, plan->w.ptr, ne * 8, hipMemcpyDeviceToHost, ctx->stream));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ECAL_OK;
}

extern "C" int ecal_undistort_images_dev(ecal_ctx *ctx, const ecal_image_plan *plan, const uint8_t *d_src, uint32_t n_frames, uint8_t *d_dst,
                                         float *d_minmax, void *stream) {
    const ecal_range range__(ctx, "ecal_undistort_images");
    if (!ctx) return ECAL_ERR_INVALID;
    if (!plan || plan->ctx != ctx) {
        ctx->last_error = "ecal_undistort_images: the plan is null or another context's";
        return ECAL_ERR_INVALID;
    }
    if (n_frames && (!d_src || !d_dst)) {
        ctx->last_error = "ecal_undistort_images: null pointer (source or destination)";
        return ECAL_ERR_INVALID;
    }
    const Options &o = plan->opt;
    const uint32_t np = o.out_width * o.out_height, C = o.channels, N = n_frames;
    if ((uint64_t) N * np > 0xFFFFFFFFull) {
        ctx->last_error = "ecal_undistort_images: more than 2^32-1 frames x canvas pixels";
        return ECAL_ERR_RANGE;
    }
    const uint32_t groups = N / IMG_FRAMES + (N % IMG_FRAMES ? 1u : 0u);
    if (groups > 65535u) {   // (the grid's second dimension)
        ctx->last_error = "ecal_undistort_images: more than 262140 frames in one call";
        return ECAL_ERR_RANGE;
    }
    if (!N) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    const bool direct = o.method == IMG_BILINEAR && !o.normalize && !d_minmax;
    float *val = nullptr;
    uint32_t *mm = nullptr, *part = nullptr;
    const uint64_t total = (uint64_t) N * np * C;
    // the workgroups of the applying launch along x: each leaves one min / max pair a frame
    const uint32_t n_parts = o.method == IMG_REFERENCE ? (np + IMG_T - 1) / IMG_T : ((np + 3) / 4 + IMG_T - 1) / IMG_T;
    if (!direct) {
        // min / max bits [N][2] | the workgroups' min / max [N][n_parts][2] | the values [N][np][C]
        const size_t o_part = up256((size_t) N * 8), o_val = o_part + up256((size_t) N * n_parts * 8);
        const int rc = ecal_ensure(ctx, ctx->image_values, o_val + (size_t) total * 4);
        if (rc) return rc;
        mm = ctx->image_values.as<uint32_t>();
        part = reinterpret_cast<uint32_t *>(ctx->image_values.as<uint8_t>() + o_part);
        val = reinterpret_cast<float *>(ctx->image_values.as<uint8_t>() + o_val);
    }
    if (o.method == IMG_REFERENCE) {
        const dim3 grid(n_parts, groups);
        const uint32_t *off = plan->off.as<uint32_t>(), *idx = plan->idx.as<uint32_t>();
        const double *w = plan->w.as<double>();
        if (C == 1) hipLaunchKernelGGL(image_gather_kernel<1>, grid, dim3(IMG_T), 0, st, off, idx, w, d_src, plan->W * plan->H, np, N, val, part);
        else hipLaunchKernelGGL(image_gather_kernel<3>, grid, dim3(IMG_T), 0, st, off, idx, w, d_src, plan->W * plan->H, np, N, val, part);
    } else {
        const dim3 grid(n_parts, groups);
        const float *mx = plan->mx.as<float>(), *my = plan->my.as<float>();
        if (C == 1 && direct) hipLaunchKernelGGL((image_remap_kernel<1, true>), grid, dim3(IMG_T), 0, st, mx, my, d_src, plan->W, plan->H, np, N, d_dst, val, part);
        else if (C == 1) hipLaunchKernelGGL((image_remap_kernel<1, false>), grid, dim3(IMG_T), 0, st, mx, my, d_src, plan->W, plan->H, np, N, d_dst, val, part);
        else if (direct) hipLaunchKernelGGL((image_remap_kernel<3, true>), grid, dim3(IMG_T), 0, st, mx, my, d_src, plan->W, plan->H, np, N, d_dst, val, part);
        else hipLaunchKernelGGL((image_remap_kernel<3, false>), grid, dim3(IMG_T), 0, st, mx, my, d_src, plan->W, plan->H, np, N, d_dst, val, part);
    }
    if (!direct) {
        hipLaunchKernelGGL(image_minmax_kernel, dim3(N), dim3(IMG_T), 0, st, (const uint32_t *) part, n_parts, mm);
        const uint64_t words = total / 4 + 1;
        hipLaunchKernelGGL(image_finish_kernel, dim3((uint32_t) ((words + IMG_T - 1) / IMG_T)), dim3(IMG_T), 0, st, (const float *) val,
                           (const uint32_t *) mm, (uint64_t) np * C, total, o.normalize, d_dst);
        if (d_minmax) ECAL_HIP_TRY(ctx, hipMemcpyAsync(d_minmax, mm, (size_t) N * 8, hipMemcpyDeviceToDevice, st));
    }
    ECAL_HIP_TRY(ctx, hipGetLastError());
    return ECAL_OK;
}

extern "C" int ecal_undistort_images(ecal_ctx *ctx, const ecal_image_plan *plan, const uint8_t *src, uint32_t n_frames, uint8_t *dst, float *minmax) {
    if (!ctx) return ECAL_ERR_INVALID;
    if (!plan || plan->ctx != ctx) {
        ctx->last_error = "ecal_undistort_images: the plan is null or another context's";
        return ECAL_ERR_INVALID;
    }
    if (n_frames && (!src || !dst)) {
        ctx->last_error = "ecal_undistort_images: null pointer (source or destination)";
        return ECAL_ERR_INVALID;
    }
    const Options &o = plan->opt;
    const uint64_t np = (uint64_t) o.out_width * o.out_height;
    if ((uint64_t) n_frames * np > 0xFFFFFFFFull) {
        ctx->last_error = "ecal_undistort_images: more than 2^32-1 frames x canvas pixels";
        return ECAL_ERR_RANGE;
    }
    if (!n_frames) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the frames | the pictures | min / max
    const size_t in_bytes = (size_t) n_frames * plan->W * plan->H * o.channels, out_bytes = (size_t) n_frames * np * o.channels;
    const size_t o_dst = up256(in_bytes), o_mm = o_dst + up256(out_bytes);
    int rc = ecal_ensure(ctx, ctx->image_io, o_mm + (size_t) n_frames * 8);
    if (rc) return rc;
    uint8_t *base = ctx->image_io.as<uint8_t>();
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(base, src, in_bytes, hipMemcpyHostToDevice, st));
    rc = ecal_undistort_images_dev(ctx, plan, base, n_frames, base + o_dst, minmax ? reinterpret_cast<float *>(base + o_mm) : nullptr, st);
    if (rc) {
        (void) hipStreamSynchronize(st);
        return rc;
    }
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(dst, base + o_dst, out_bytes, hipMemcpyDeviceToHost, st));
    if (minmax) ECAL_HIP_TRY(ctx, hipMemcpyAsync(minmax, base + o_mm, (size_t) n_frames * 8, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}
