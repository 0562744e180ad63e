// Array ingest (include/ecal.h, "array ingest"): events held as four columns — any of nine element types, any stride, any byte
// offset — packed into 25-byte records in HBM, the reverse, and the .npy forms.  The element loads, the conversion, the filter, the
// reverse's rules and the .npy header parser are fields_events.hpp's (shared with the host entry points and the CPU test);
// design/21_array_ingest.md has the reasoning.
//
// A block is FDK_T threads x 4 consecutive events = 1024 events (ecal_fields_block_events).  Launches, with NO waiting between
// workgroups — state crosses blocks only between launches, or inside the one-workgroup scan:
//   1. fields_verdict_kernel   every event's t, x, y loaded and classed; the kept events per block; the first event that reaches
//                              end_time (64-bit atomic minimum)
//   2. ecal_scan_blocks        the blocks' first kept index
//   3. fields_write_kernel     loaded and classed again, with p; the kept events below the first offender get their index
//                              (in-workgroup scan), are packed into LDS and copied out with aligned 32-bit stores; the totals
//   fields_unpack_kernel       the reverse, one launch: a thread a record, every column's element stored by the thread of its event
//                              (neighbouring threads, neighbouring addresses)
// The element types are kernel arguments: every branch on them is the same for the whole grid.  An element is put together from the
// aligned 32-bit words that hold at least one of its bytes (one to three), so nothing outside those words is loaded.
// The tails of passes 1 and 3 are ingest_blocks.hpp's, shared with the other ingests; the record's bytes are event_record.hpp's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <math.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include "ecal_ctx.hpp"
#include "block_utils.hpp"
#include "ingest_blocks.hpp"
#include "fields_events.hpp"

namespace ecal {

using namespace ecal_fields;

static_assert(ECAL_ERR_INVALID == FD_INVALID && ECAL_ERR_RANGE == FD_RANGE && ECAL_OK == FD_OK, "status codes");
static_assert(sizeof(ecal_field) == sizeof(Field) && sizeof(ecal_field) == 24, "field");
static_assert(sizeof(ecal_npy_layout) == sizeof(NpyLayout), "npy layout");
static_assert(ECAL_FIELD_U8 == FD_U8 && ECAL_FIELD_I64 == FD_I64 && ECAL_FIELD_F32 == FD_F32 && ECAL_FIELD_F64 == FD_F64, "type codes");

constexpr int FDK_T = FD_BLOCK_THREADS;
constexpr uint32_t FDK_PER = FD_THREAD_EVENTS;
constexpr uint32_t FDK_BLOCK = FD_BLOCK_EVENTS;   // events per block, and records staged in LDS (25 600 bytes: six workgroups a CU)
constexpr unsigned long long FDK_NONE = ~0ull;

// the counters of one ingest (device)
struct FdWords {
    unsigned long long first_stop;   // the first event that reaches end_time (FDK_NONE: none)
    unsigned long long n_events, n_outside, n_negative, n_before_start;
};

struct FdSource {
    Field f[4];   // t, x, y, p over device memory
    uint64_t n;
};

// element i of a column from the aligned words that hold it
__device__ __forceinline__ uint64_t fd_load(const Field &f, uint32_t size, uint64_t i) {
    const uintptr_t a = (uintptr_t) f.ptr + i * (uint64_t) f.stride;
    const uint32_t r = (uint32_t) (a & 3u);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(a - r);
    const uint32_t w0 = w[0];
    const uint32_t w1 = r + size > 4u ? w[1] : 0u;
    const uint32_t w2 = r + size > 8u ? w[2] : 0u;
    return fd_bits_from_words(w0, w1, w2, r);
}

// the class of every event, the kept events per block, the first event that reaches end_time
__global__ __launch_bounds__(FDK_T) void fields_verdict_kernel(FdSource src, FieldsFilter flt, uint32_t *__restrict__ blk_keep, FdWords *__restrict__ w) {
    const int tid = threadIdx.x;
    const uint64_t s0 = ((uint64_t) blockIdx.x * FDK_T + tid) * FDK_PER;
    const uint32_t st = fd_type_size(src.f[FD_T].type), sx = fd_type_size(src.f[FD_X].type), sy = fd_type_size(src.f[FD_Y].type);
    uint32_t keep = 0, stop = 0xFFFFFFFFu;   // (stop: an event within the block)
#pragma unroll
    for (uint32_t j = 0; j < FDK_PER; j++) {
        if (s0 + j < src.n) {
            const uint64_t bt = fd_load(src.f[FD_T], st, s0 + j);
            const double x = fd_value_f64(fd_load(src.f[FD_X], sx, s0 + j), src.f[FD_X].type);
            const double y = fd_value_f64(fd_load(src.f[FD_Y], sy, s0 + j), src.f[FD_Y].type);
            double t, xo, yo;
            const uint8_t c = fd_classify(bt, src.f[FD_T].type, x, y, flt, &t, &xo, &yo);
            keep += c == FD_CLASS_KEEP ? 1u : 0u;
            const uint32_t at = (uint32_t) tid * FDK_PER + j;
            if (c == FD_CLASS_STOP && at < stop) stop = at;
        }
    }
    block_keep_and_stop<FDK_T>(keep, stop, blk_keep, &w->first_stop, [] { return (unsigned long long) blockIdx.x * FDK_BLOCK; });
}

// the kept events below the first offender, packed in LDS and copied out; the totals
__global__ __launch_bounds__(FDK_T) void fields_write_kernel(FdSource src, const uint32_t *__restrict__ blk_koff, FieldsFilter flt,
                                                            uint8_t *__restrict__ events, uint64_t capacity, FdWords *__restrict__ w) {
    __shared__ unsigned long long s_scan[FDK_T / 64];
    __shared__ uint32_t s_cnt[3];
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[FDK_BLOCK * 25];
    const int tid = threadIdx.x;
    const unsigned long long X = w->first_stop;
    const uint64_t ev0 = (uint64_t) blockIdx.x * FDK_BLOCK;
    if (ev0 >= X) return;   // (the whole block lies behind the offender; the same for every thread)
    const uint64_t s0 = ev0 + (uint64_t) tid * FDK_PER;
    // events of this block below the offender: in-block event < lim
    const uint32_t lim = X - ev0 < (unsigned long long) FDK_BLOCK ? (uint32_t) (X - ev0) : FDK_BLOCK;
    const uint32_t st = fd_type_size(src.f[FD_T].type), sx = fd_type_size(src.f[FD_X].type), sy = fd_type_size(src.f[FD_Y].type),
                   sp = fd_type_size(src.f[FD_P].type);
    if (tid < 3) s_cnt[tid] = 0;
    uint32_t keep = 0, kept_mask = 0, pol_mask = 0, drop[3] = {0u, 0u, 0u};
    double kt[FDK_PER], kx[FDK_PER], ky[FDK_PER];
#pragma unroll
    for (uint32_t j = 0; j < FDK_PER; j++) {
        kt[j] = kx[j] = ky[j] = 0.0;
        if (s0 + j < src.n && (uint32_t) tid * FDK_PER + j < lim) {
            const uint64_t bt = fd_load(src.f[FD_T], st, s0 + j);
            const double x = fd_value_f64(fd_load(src.f[FD_X], sx, s0 + j), src.f[FD_X].type);
            const double y = fd_value_f64(fd_load(src.f[FD_Y], sy, s0 + j), src.f[FD_Y].type);
            const uint8_t c = fd_classify(bt, src.f[FD_T].type, x, y, flt, &kt[j], &kx[j], &ky[j]);
            if (c == FD_CLASS_KEEP) {
                keep++;
                kept_mask |= 1u << j;
                if (fd_value_positive(fd_load(src.f[FD_P], sp, s0 + j), src.f[FD_P].type)) pol_mask |= 1u << j;
            }
            drop[0] += c == FD_CLASS_OUTSIDE ? 1u : 0u;
            drop[1] += c == FD_CLASS_NEGATIVE ? 1u : 0u;
            drop[2] += c == FD_CLASS_BEFORE_START ? 1u : 0u;
        }
    }
    uint32_t kex, eb, ktot, tb;
    block_exscan_pair<FDK_T>(keep, 0u, s_scan, &kex, &eb, &ktot, &tb);   // (its barriers order the zeroing of s_cnt too)
    block_add_drops<3>(drop, s_cnt);
    // at most FDK_BLOCK kept events: one chunk of LDS holds them all
    uint32_t k = kex;
#pragma unroll
    for (uint32_t j = 0; j < FDK_PER; j++) {
        if (kept_mask >> j & 1u) {
            pack_record(s_rec + k * 25u, kt[j], kx[j], ky[j], (uint8_t) (pol_mask >> j & 1u));
            k++;
        }
    }
    __syncthreads();
    if (tid < 3 && s_cnt[tid])
        atomicAdd(tid == 0 ? &w->n_outside : tid == 1 ? &w->n_negative : &w->n_before_start, (unsigned long long) s_cnt[tid]);
    if (tid == 0 && ktot) atomicAdd(&w->n_events, (unsigned long long) ktot);
    block_copy_out<FDK_T>(s_rec, ktot, events, blk_koff[blockIdx.x], capacity);
}

// an element's low `size` bytes to ptr + i * stride: one store of the type's width where the address allows it, else byte by byte
__device__ __forceinline__ void fd_store(const Field &f, uint32_t size, uint64_t i, uint64_t bits) {
    uint8_t *a = (uint8_t *) const_cast<void *>(f.ptr) + i * (uint64_t) f.stride;
    if (((uintptr_t) a & (size - 1u)) == 0u) {
        if (size == 1u) *a = (uint8_t) bits;
        else if (size == 2u) *reinterpret_cast<uint16_t *>(a) = (uint16_t) bits;
        else if (size == 4u) *reinterpret_cast<uint32_t *>(a) = (uint32_t) bits;
        else *reinterpret_cast<uint64_t *>(a) = bits;
    } else {
        for (uint32_t b = 0; b < size; b++) a[b] = (uint8_t) (bits >> (8u * b));
    }
}

__device__ __forceinline__ double fd_record_f64(const uint8_t *p) {
    double v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// records into columns; *bad: the events that are not representable (nothing of theirs is stored)
__global__ __launch_bounds__(FDK_T) void fields_unpack_kernel(const uint8_t *__restrict__ rec, uint64_t n, FdSource out, ToFields o,
                                                             unsigned long long *__restrict__ bad) {
    const uint64_t i = (uint64_t) blockIdx.x * FDK_T + threadIdx.x;
    bool ok = true;
    if (i < n) {
        const uint8_t *r = rec + i * 25u;
        uint64_t b[4];
        ok = fd_stamp_element(fd_record_f64(r), out.f[FD_T].type, o, &b[FD_T]);
        ok = fd_coord_element(fd_record_f64(r + 8), out.f[FD_X].type, &b[FD_X]) && ok;
        ok = fd_coord_element(fd_record_f64(r + 16), out.f[FD_Y].type, &b[FD_Y]) && ok;
        b[FD_P] = fd_polarity_element(r[24], out.f[FD_P].type, o);
        if (ok) {
#pragma unroll
            for (int k = 0; k < 4; k++) fd_store(out.f[k], fd_type_size(out.f[k].type), i, b[k]);
        }
    }
    const uint32_t c = (uint32_t) __popcll(__ballot(!ok));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(bad, (unsigned long long) c);
}

}  // namespace ecal

using namespace ecal;

extern "C" void ecal_fields_default_options(ecal_fields_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->time_magnitude = 1e-6;
}

extern "C" void ecal_to_fields_default_options(ecal_to_fields_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->ticks_per_second = 1e6;
}

extern "C" void ecal_npy_default_options(ecal_npy_options *opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    ecal_fields_default_options(&opt->fields);
}

extern "C" uint32_t ecal_fields_block_events(void) { return FDK_BLOCK; }

namespace {

void fd_put_error(char *err, uint64_t cap, const std::string &text) {
    if (err && cap) snprintf(err, (size_t) cap, "%s", text.c_str());
}

FieldsFilter fd_filter(const ecal_fields_options &o) {
    return FieldsFilter{o.time_magnitude, o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
}

void fd_info_from_counts(ecal_fields_info &I, const FieldsCounts &c) {
    I.n_raw_events = c.n_raw_events;
    I.n_events = c.n_events;
    I.n_outside = c.n_outside;
    I.n_negative = c.n_negative;
    I.n_before_start = c.n_before_start;
    I.n_after_end = c.n_after_end;
}

const Field *as_fields(const ecal_field *f) { return reinterpret_cast<const Field *>(f); }

bool fd_overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// f over DEVICE memory, checked; flt.time_base: the base in force.
// own_events != null: the records go into a buffer allocated here for n events (the caller's to hipFree, null when there is nothing to
// free); else into d_events / capacity
int fields_ingest(ecal_ctx *ctx, const Field f[4], uint64_t n, const FieldsFilter &flt, uint8_t *d_events, uint64_t capacity, uint8_t **own_events,
                  ecal_fields_info &I, hipStream_t st) {
    if (own_events) *own_events = nullptr;
    I.time_base = flt.time_base;
    I.n_raw_events = n;
    if (!n) return ECAL_OK;
    if (n > 0xFFFFFFFFull) {
        I.n_events = n;
        ctx->last_error = "array ingest: more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    const uint32_t nb = (uint32_t) ((n + FDK_BLOCK - 1) / FDK_BLOCK);
    ecal_load_timer tm("array", ctx->sw.load_trace, st);
    const size_t o_keep = 0, o_koff = o_keep + up16(((size_t) nb + 1) * 4), o_words = o_koff + up16(((size_t) nb + 1) * 4), total = o_words + sizeof(FdWords);
    ecal_devbuf scratch;
    int rc;
    if ((rc = ecal_ensure(ctx, scratch, total))) return rc;
    uint8_t *base = scratch.as<uint8_t>();
    uint32_t *keep = (uint32_t *) (base + o_keep), *koff = (uint32_t *) (base + o_koff);
    FdWords *d_w = (FdWords *) (base + o_words);
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(FdWords), &d_w->first_stop, st))) return rc;
    if (own_events) {
        capacity = n;
        if ((rc = ecal_ingest_alloc_records(ctx, "array ingest", capacity, own_events))) return rc;
        d_events = *own_events;
    }
    auto fail = [&](int code) { return ecal_ingest_drop_records(own_events, code); };
    auto launched = [&]() -> int {
        ECAL_HIP_TRY(ctx, hipGetLastError());
        return ECAL_OK;
    };
    FdSource src;
    for (int k = 0; k < 4; k++) src.f[k] = f[k];
    src.n = n;
    tm.mark("start");
    hipLaunchKernelGGL(fields_verdict_kernel, dim3(nb), dim3(FDK_T), 0, st, src, flt, keep, d_w);
    if ((rc = launched())) return fail(rc);
    tm.mark("verdict");
    if ((rc = ecal_scan_blocks(ctx, keep, nb, koff, st))) return fail(rc);
    tm.mark("scan");
    hipLaunchKernelGGL(fields_write_kernel, dim3(nb), dim3(FDK_T), 0, st, src, (const uint32_t *) koff, flt, d_events, capacity, d_w);
    if ((rc = launched())) return fail(rc);
    tm.mark("write");
    FdWords W;
    if ((rc = ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st))) return fail(rc);
    I.n_events = W.n_events;
    I.n_outside = W.n_outside;
    I.n_negative = W.n_negative;
    I.n_before_start = W.n_before_start;
    // every event in front of the offender has one of the four classes
    I.n_after_end = W.first_stop == FDK_NONE ? 0 : n - (W.n_events + W.n_outside + W.n_negative + W.n_before_start);
    if (I.n_events > capacity) {
        ctx->last_error = "array ingest: " + std::to_string(I.n_events) + " records, more than the capacity";
        return fail(ECAL_ERR_RANGE);
    }
    return ECAL_OK;
}

int fd_check_all(const Field f[4], uint64_t n, const ecal_fields_options &o, std::string *why) {
    int which = -1;
    const int rc = fd_check_fields(f, n, &which, why);
    return rc ? rc : fd_check_filter(fd_filter(o), f[FD_T].type, why);
}

// `len` bytes of host memory into device memory through the context's pinned staging, a chunk at a time
int fd_upload_bytes(ecal_ctx *ctx, uint8_t *d_dst, const uint8_t *src, uint64_t len) {
    const size_t CH = 32u << 20;
    unsigned char *stage = len ? ecal_fetch_pinned(ctx, (size_t) std::min<uint64_t>(CH, len)) : nullptr;
    for (uint64_t at = 0; at < len; at += CH) {
        const size_t m = (size_t) std::min<uint64_t>(CH, len - at);
        if (stage) {
            memcpy(stage, src + at, m);
            ECAL_HIP_TRY(ctx, hipMemcpyAsync(d_dst + at, stage, m, hipMemcpyHostToDevice, ctx->stream));
            ECAL_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the one staging buffer is filled again)
        } else {
            ECAL_HIP_TRY(ctx, hipMemcpy(d_dst + at, src + at, m, hipMemcpyHostToDevice));
        }
    }
    return ECAL_OK;
}

// The bytes that HOST columns cover, uploaded: spans that overlap or touch (the columns of a structured array) go up once.  d_f: the
// same columns over the device copies; allocs: what the caller hipFrees.
int fd_upload_fields(ecal_ctx *ctx, const Field f[4], uint64_t n, Field d_f[4], std::vector<void *> &allocs) {
    struct Span {
        uintptr_t lo, hi;
        uint8_t *d_base;
    };
    std::vector<Span> spans;
    for (int k = 0; k < 4; k++) spans.push_back(Span{(uintptr_t) f[k].ptr, (uintptr_t) f[k].ptr + fd_field_span(f[k], n), nullptr});
    std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
    std::vector<Span> merged;
    for (const Span &s : spans) {
        if (!merged.empty() && s.lo <= merged.back().hi) merged.back().hi = std::max(merged.back().hi, s.hi);
        else merged.push_back(s);
    }
    for (Span &s : merged) {
        void *d = nullptr;
        // 16 spare bytes on either side: the aligned words around the first and the last element lie within the allocation
        hipError_t e = hipMalloc(&d, (size_t) (s.hi - s.lo) + 48);
        if (e != hipSuccess) {
            ctx->last_error = std::string("array ingest: ") + hipGetErrorString(e);
            return e == hipErrorOutOfMemory ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;
        }
        allocs.push_back(d);
        s.d_base = (uint8_t *) d + 16 + (s.lo & 15u);   // (the columns keep their alignment)
        const int rc = fd_upload_bytes(ctx, s.d_base, (const uint8_t *) s.lo, s.hi - s.lo);
        if (rc) return rc;
    }
    for (int k = 0; k < 4; k++) {
        d_f[k] = f[k];
        for (const Span &s : merged)
            if ((uintptr_t) f[k].ptr >= s.lo && (uintptr_t) f[k].ptr < s.hi) d_f[k].ptr = s.d_base + ((uintptr_t) f[k].ptr - s.lo);
    }
    return ECAL_OK;
}

NpyChoice npy_choice(const ecal_npy_options *o) {
    NpyChoice ch;
    if (!o) return ch;
    const char *names[4] = {o->t_name, o->x_name, o->y_name, o->p_name};
    for (int k = 0; k < 4; k++)
        if (names[k]) ch.name[k] = names[k];
    if (o->columns) ch.columns = o->columns;
    return ch;
}

// file -> (header on the host) -> payload in HBM -> records in a device buffer of their own (null for none), the payload freed
int npy_file_to_events(ecal_ctx *ctx, const char *path, const ecal_npy_options *opt, uint8_t **d_events, ecal_fields_info &I) {
    *d_events = nullptr;
    ecal_npy_options o;
    if (opt) o = *opt; else ecal_npy_default_options(&o);
    const int fd = open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) {
        if (fd >= 0) close(fd);
        ctx->last_error = std::string("npy ingest: cannot open ") + path;
        return ECAL_ERR_INVALID;
    }
    // (a version 1.0 header is below 64 KiB; a larger one of version 2.0 / 3.0 would be a dtype of thousands of fields)
    std::vector<uint8_t> head((size_t) std::min<uint64_t>((uint64_t) sb.st_size, 1u << 20));
    NpyLayout L;
    std::string err = "the file cannot be read";
    int rc = (head.empty() || ecal_ingest_pread_all(fd, head.data(), head.size(), 0)) ? npy_parse_header(head.data(), head.size(), (uint64_t) sb.st_size, npy_choice(&o), L, &err)
                                                                              : ECAL_ERR_INVALID;
    uint64_t first_stamp = 0;
    if (!rc && L.n_events && !ecal_ingest_pread_all(fd, &first_stamp, fd_type_size(L.field[FD_T].type), L.data_offset + L.field[FD_T].offset)) {
        rc = ECAL_ERR_INVALID;
        err = "the file cannot be read";
    }
    close(fd);
    if (rc) {
        ctx->last_error = "npy ingest: " + err + " (" + path + ")";
        return rc;
    }
    Field f[4];
    for (int k = 0; k < 4; k++) f[k] = Field{nullptr, (int64_t) L.item_stride, L.field[k].type, 0u};
    if (o.fields.auto_time_base) o.fields.time_base = L.n_events && !fd_type_is_float(f[FD_T].type) ? fd_value_i64(first_stamp, f[FD_T].type) : 0;
    I.time_base = o.fields.time_base;
    I.n_raw_events = L.n_events;
    if ((rc = fd_check_filter(fd_filter(o.fields), f[FD_T].type, &err))) {
        ctx->last_error = "npy ingest: " + err;
        return rc;
    }
    if (!L.n_events) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint8_t *d_file = nullptr;
    uint64_t n_bytes = 0;
    if ((rc = ecal_upload_file(ctx, "npy ingest", path, L.data_offset, &d_file, &n_bytes))) return rc;
    if (n_bytes < L.n_events * L.item_stride) {
        (void) hipFree(d_file);
        ctx->last_error = std::string("npy ingest: the file changed while it was read (") + path + ")";
        return ECAL_ERR_INVALID;
    }
    for (int k = 0; k < 4; k++) f[k].ptr = d_file + L.field[k].offset;
    rc = fields_ingest(ctx, f, L.n_events, fd_filter(o.fields), nullptr, 0, d_events, I, ctx->stream);
    (void) hipFree(d_file);
    return rc;
}

}  // namespace

extern "C" int ecal_events_from_fields_host(const ecal_field f[4], uint64_t n, const ecal_fields_options *opt, uint8_t *events, uint64_t capacity,
                                            ecal_fields_info *info, char *err, uint64_t err_cap) {
    ecal_fields_info I;
    memset(&I, 0, sizeof(I));
    if (info) *info = I;
    if (!f || (capacity && !events)) {
        fd_put_error(err, err_cap, "array ingest: null fields or record buffer");
        return ECAL_ERR_INVALID;
    }
    ecal_fields_options o;
    if (opt) o = *opt; else ecal_fields_default_options(&o);
    std::string why;
    const Field *F = as_fields(f);
    int which = -1;
    int rc = fd_check_fields(F, n, &which, &why);
    if (!rc) {
        if (o.auto_time_base) o.time_base = fd_auto_time_base(F[FD_T], n);
        rc = fd_check_filter(fd_filter(o), F[FD_T].type, &why);
    }
    if (rc) {
        fd_put_error(err, err_cap, "array ingest: " + why);
        return rc;
    }
    FieldsCounts c;
    uint64_t put = 0;
    fd_walk(F, n, fd_filter(o), c, [&](const uint8_t rec[25]) {
        if (put < capacity) memcpy(events + put * 25u, rec, 25);
        put++;
    });
    fd_info_from_counts(I, c);
    I.time_base = o.time_base;
    if (info) *info = I;
    if (c.n_events > capacity) {
        fd_put_error(err, err_cap, "array ingest: " + std::to_string(c.n_events) + " records, more than the capacity");
        return ECAL_ERR_RANGE;
    }
    return ECAL_OK;
}

extern "C" int ecal_events_from_fields_dev(ecal_ctx *ctx, const ecal_field f[4], uint64_t n, const ecal_fields_options *opt, uint8_t *d_events,
                                           uint64_t capacity, ecal_fields_info *info, void *stream) {
    const ecal_range range__(ctx, "ecal_events_from_fields");
    if (!ctx) return ECAL_ERR_INVALID;
    ecal_fields_info I;
    memset(&I, 0, sizeof(I));
    if (info) *info = I;
    if (!f) {
        ctx->last_error = "array ingest: null fields";
        return ECAL_ERR_INVALID;
    }
    ecal_fields_options o;
    if (opt) o = *opt; else ecal_fields_default_options(&o);
    std::string why;
    const Field *F = as_fields(f);
    int rc = fd_check_all(F, n, o, &why);
    if (rc) {
        ctx->last_error = "array ingest: " + why;
        return rc;
    }
    if (o.auto_time_base) {
        ctx->last_error = "array ingest: the device form takes an explicit time base (auto_time_base must be 0; element 0's stamp is the automatic one)";
        return ECAL_ERR_INVALID;
    }
    if (capacity && !d_events) {
        ctx->last_error = "array ingest: null record buffer";
        return ECAL_ERR_INVALID;
    }
    if (capacity > (~0ull >> 2) / 25u) {
        ctx->last_error = "array ingest: the capacity does not fit 62 bits of records";
        return ECAL_ERR_RANGE;
    }
    for (int k = 0; k < 4; k++)
        if (fd_overlap(d_events, capacity * 25u, F[k].ptr, fd_field_span(F[k], n))) {
            ctx->last_error = std::string("array ingest: the record buffer overlaps field ") + fd_field_name(k);
            return ECAL_ERR_INVALID;
        }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = fields_ingest(ctx, F, n, fd_filter(o), d_events, capacity, nullptr, I, (hipStream_t) stream);
    if (info) *info = I;
    return rc;
}

extern "C" int ecal_stream_create_from_fields(ecal_ctx *ctx, const ecal_field f[4], uint64_t n, const ecal_fields_options *opt, ecal_stream **out,
                                              ecal_fields_info *info) {
    if (!ctx || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    ecal_fields_info I;
    memset(&I, 0, sizeof(I));
    if (info) *info = I;
    if (!f) {
        ctx->last_error = "array ingest: null fields";
        return ECAL_ERR_INVALID;
    }
    ecal_fields_options o;
    if (opt) o = *opt; else ecal_fields_default_options(&o);
    std::string why;
    const Field *F = as_fields(f);
    int which = -1;
    int rc = fd_check_fields(F, n, &which, &why);
    if (!rc) {
        if (o.auto_time_base) o.time_base = fd_auto_time_base(F[FD_T], n);
        rc = fd_check_filter(fd_filter(o), F[FD_T].type, &why);
    }
    if (!rc && n > 0xFFFFFFFFull) {
        rc = ECAL_ERR_RANGE;
        why = "more than 2^32-1 events";
    }
    if (rc) {
        ctx->last_error = "array ingest: " + why;
        return rc;
    }
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint8_t *d_events = nullptr;
    std::vector<void *> allocs;
    Field d_f[4];
    rc = n ? fd_upload_fields(ctx, F, n, d_f, allocs) : ECAL_OK;
    if (!rc) rc = fields_ingest(ctx, d_f, n, fd_filter(o), nullptr, 0, &d_events, I, ctx->stream);
    for (void *p : allocs) (void) hipFree(p);
    I.time_base = o.time_base;
    if (info) *info = I;
    if (rc) return rc;
    return ecal_stream_from_events(ctx, "ecal_stream_create_from_fields", d_events, I.n_events, out);
}

extern "C" int ecal_events_to_fields_host(const uint8_t *events, uint64_t n, const ecal_field out[4], const ecal_to_fields_options *opt,
                                          ecal_to_fields_info *info, char *err, uint64_t err_cap) {
    if (info) memset(info, 0, sizeof(*info));
    if (!out || (n && !events)) {
        fd_put_error(err, err_cap, "array export: null fields or records");
        return ECAL_ERR_INVALID;
    }
    ecal_to_fields_options o;
    if (opt) o = *opt; else ecal_to_fields_default_options(&o);
    const ToFields T{o.ticks_per_second, o.time_base, o.polarity_signed};
    std::string why;
    int which = -1;
    const int rc = fd_check_to_fields(as_fields(out), n, T, &which, &why);
    if (rc) {
        fd_put_error(err, err_cap, "array export: " + why);
        return rc;
    }
    const uint64_t bad = fd_unwalk(events, n, as_fields(out), T);
    if (info) {
        info->n_events = n;
        info->n_unrepresentable = bad;
    }
    if (bad) {
        fd_put_error(err, err_cap, "array export: " + std::to_string(bad) + " events are not representable in the output types");
        return ECAL_ERR_RANGE;
    }
    return ECAL_OK;
}

extern "C" int ecal_events_to_fields_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n, const ecal_field out[4], const ecal_to_fields_options *opt,
                                         ecal_to_fields_info *info, void *stream) {
    const ecal_range range__(ctx, "ecal_events_to_fields");
    if (!ctx) return ECAL_ERR_INVALID;
    if (info) memset(info, 0, sizeof(*info));
    if (!out || (n && !d_events)) {
        ctx->last_error = "array export: null fields or records";
        return ECAL_ERR_INVALID;
    }
    ecal_to_fields_options o;
    if (opt) o = *opt; else ecal_to_fields_default_options(&o);
    const ToFields T{o.ticks_per_second, o.time_base, o.polarity_signed};
    const Field *F = as_fields(out);
    std::string why;
    int which = -1;
    int rc = fd_check_to_fields(F, n, T, &which, &why);
    if (rc) {
        ctx->last_error = "array export: " + why;
        return rc;
    }
    if (n > 0xFFFFFFFFull) {
        ctx->last_error = "array export: more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    for (int k = 0; k < 4; k++)
        if (fd_overlap(d_events, n * 25u, F[k].ptr, fd_field_span(F[k], n))) {
            ctx->last_error = std::string("array export: field ") + fd_field_name(k) + " overlaps the records";
            return ECAL_ERR_INVALID;
        }
    if (info) info->n_events = n;
    if (!n) return ECAL_OK;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    ecal_load_timer tm("array export", ctx->sw.load_trace, st);
    ecal_devbuf words;
    if ((rc = ecal_ensure(ctx, words, 16))) return rc;
    ECAL_HIP_TRY(ctx, hipMemsetAsync(words.ptr, 0, 16, st));
    FdSource dst;
    for (int k = 0; k < 4; k++) dst.f[k] = F[k];
    dst.n = n;
    tm.mark("start");
    hipLaunchKernelGGL(fields_unpack_kernel, dim3((uint32_t) ((n + FDK_T - 1) / FDK_T)), dim3(FDK_T), 0, st, d_events, n, dst, T, words.as<unsigned long long>());
    ECAL_HIP_TRY(ctx, hipGetLastError());
    tm.mark("unpack");
    unsigned long long bad = 0;
    if ((rc = ecal_ingest_fetch_words(ctx, &bad, words.ptr, sizeof(bad), st))) return rc;
    if (info) info->n_unrepresentable = bad;
    if (bad) {
        ctx->last_error = "array export: " + std::to_string(bad) + " events are not representable in the output types";
        return ECAL_ERR_RANGE;
    }
    return ECAL_OK;
}

extern "C" int ecal_npy_parse_header(ecal_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t file_bytes, const ecal_npy_options *opt,
                                     ecal_npy_layout *layout, char *err, uint64_t err_cap) {
    if (!layout || (n_bytes && !bytes)) return ECAL_ERR_INVALID;
    std::string why;
    NpyLayout L;
    const int rc = npy_parse_header(bytes, n_bytes, file_bytes, npy_choice(opt), L, &why);
    memcpy(layout, &L, sizeof(L));
    if (rc) {
        fd_put_error(err, err_cap, "npy ingest: " + why);
        if (ctx) ctx->last_error = "npy ingest: " + why;
    }
    return rc;
}

extern "C" int ecal_stream_create_from_npy_file(ecal_ctx *ctx, const char *path, const ecal_npy_options *opt, ecal_stream **out, ecal_fields_info *info) {
    if (!ctx || !path || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    uint8_t *d_events = nullptr;
    ecal_fields_info I;
    memset(&I, 0, sizeof(I));
    const int rc = npy_file_to_events(ctx, path, opt, &d_events, I);
    if (info) *info = I;
    if (rc) return rc;
    return ecal_stream_from_events(ctx, "ecal_stream_create_from_npy_file", d_events, I.n_events, out);
}

extern "C" int ecal_npy_to_bin_file(ecal_ctx *ctx, const char *npy_path, const char *bin_path, const ecal_npy_options *opt, ecal_fields_info *info) {
    if (!ctx || !npy_path || !bin_path) return ECAL_ERR_INVALID;
    uint8_t *d_events = nullptr;
    ecal_fields_info I;
    memset(&I, 0, sizeof(I));
    const int rc = npy_file_to_events(ctx, npy_path, opt, &d_events, I);
    if (info) *info = I;
    return rc ? rc : ecal_ingest_records_to_bin(ctx, "ecal_npy_to_bin_file", d_events, I.n_events, bin_path);
}

extern "C" int ecal_stream_to_npy_file(ecal_ctx *ctx, const ecal_stream *s, const char *npy_path) {
    if (!ctx || !s || !npy_path) return ECAL_ERR_INVALID;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t n = ecal_stream_size(s);
    const std::string header = npy_records_header(n);
    return ecal_write_records_file(ctx, "ecal_stream_to_npy_file", ecal_stream_data(s), n, npy_path, &header);
}
