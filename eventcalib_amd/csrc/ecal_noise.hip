// The background-activity filter (include/ecal.h, "noise filter"): an event stays iff enough pixels around its own fired at most dt
// before it.  What decides — the pixel of a record, the neighbourhood, the support test, the search — is noise_filter.hpp's (shared
// with the host entry point and the CPU test); design/19_noise_filter.md has the reasoning.
//
// A verdict depends on the input stream alone, so every event is judged on its own, from an index of the stream by pixel, and NO
// workgroup waits on another:
//   noise_key_kernel       key[i] = the pixel of event i (off-grid: width * height), val[i] = i
//   rocPRIM radix sort     the pairs, stably, on the ceil(log2(plane + 1)) bits that hold every key: every pixel's events are one
//                          contiguous list of ascending stream indices
//   noise_index_kernel     start[p] for the plane + 1 pixels (a lower-bound search of the sorted keys each) and the stamps gathered
//                          into sorted order, so that the support test reads sts[pos] instead of chasing an index into the records
//   noise_support_kernel   one thread per sorted position: a wave works on one pixel or a few adjacent ones and its searches walk the
//                          same lists.  For each neighbour pixel a binary search of its list for the last entry in front of event i,
//                          one support test; the verdict byte goes to verdict[i]; the totals are reduced in the block.
//   noise_count_kernel     the kept events of every block of PA_BLOCK_EVENTS verdict bytes
//   ecal_compact_copy_by_verdict   the hot-pixel filter's scan and writing pass (ecal_activity.hip)
// Nothing behind n_events * 25 bytes of the input is loaded and nothing behind the kept records is stored: any caller tensor will do.
#include "ecal_ctx.hpp"
#include "noise_filter.hpp"
#include "stream_compact.hpp"

#include <rocprim/rocprim.hpp>   // (behind ecal_ctx.hpp, as in ecal_sort.hip: its headers use the host's string.h)

namespace ecal {

using namespace ecal_noise;
using ecal_activity::PA_BLOCK_EVENTS;

constexpr int NF_T = SC_T;

__global__ __launch_bounds__(NF_T) void noise_key_kernel(const uint8_t *__restrict__ rec, uint32_t n_events, uint32_t width, uint32_t height,
                                                         uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
    const uint64_t i = (uint64_t) blockIdx.x * NF_T + threadIdx.x;
    if (i >= (uint64_t) n_events) return;
    key[i] = nf_record_key(rec + (size_t) i * PA_RECORD_BYTES, width, height);
    val[i] = (uint32_t) i;
}

// thread j: start[j] for j <= plane, sts[j] for j < n_events
__global__ __launch_bounds__(NF_T) void noise_index_kernel(const uint8_t *__restrict__ rec, uint32_t n_events, const uint32_t *__restrict__ skey,
                                                           const uint32_t *__restrict__ sval, uint32_t plane, uint32_t *__restrict__ start,
                                                           double *__restrict__ sts) {
    const uint64_t j = (uint64_t) blockIdx.x * NF_T + threadIdx.x;
    if (j <= (uint64_t) plane) {
        uint32_t a = 0, b = n_events;   // the first position whose key is >= j
        while (a < b) {
            const uint32_t m = a + (b - a) / 2u;
            if (skey[m] < (uint32_t) j) a = m + 1u;
            else b = m;
        }
        start[j] = a;
    }
    if (j < (uint64_t) n_events) sts[j] = ecal_activity::pa_load_f64(rec + (size_t) sval[j] * PA_RECORD_BYTES);
}

// verdict [n_events]: one byte per event (1 keep, 0 remove), written at the event's stream index; totals (may be null): n_events,
// n_off_grid, n_removed, n_kept, zero before the launch
__global__ __launch_bounds__(NF_T) void noise_support_kernel(uint32_t n_events, const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                             const double *__restrict__ sts, const uint32_t *__restrict__ start, uint32_t width,
                                                             uint32_t height, uint32_t radius, uint32_t min_support, uint32_t include_self,
                                                             double dt, uint8_t *__restrict__ verdict, unsigned long long *__restrict__ totals) {
    __shared__ uint32_t s_red[2][NF_T / 64];
    const uint64_t pos = (uint64_t) blockIdx.x * NF_T + threadIdx.x;
    uint32_t keep = 0, off = 0;
    if (pos < (uint64_t) n_events) {
        bool og;
        const uint8_t v = nf_position_verdict((uint32_t) pos, skey, sval, sts, start, width, height, radius, min_support, include_self, dt, &og);
        verdict[sval[pos]] = v;
        keep = v;
        off = og ? 1u : 0u;
    }
    if (!totals) return;
    keep = block_sum<NF_T>(keep, s_red[0]);
    off = block_sum<NF_T>(off, s_red[1]);
    const uint32_t count = stream_block_count<NF_T>(n_events, (uint64_t) blockIdx.x * NF_T);
    const int tid = threadIdx.x;
    if (tid == 0) atomicAdd(&totals[0], (unsigned long long) count);
    if (tid == 1 && off) atomicAdd(&totals[1], (unsigned long long) off);
    if (tid == 2 && count - keep) atomicAdd(&totals[2], (unsigned long long) (count - keep));
    if (tid == 3 && keep) atomicAdd(&totals[3], (unsigned long long) keep);
}

// verdict: rounded up to whole blocks, 16-byte aligned (the bytes behind n_events are read and masked); block_cnt [blocks]
__global__ __launch_bounds__(NF_T) void noise_count_kernel(const uint8_t *__restrict__ verdict, uint32_t n_events, uint32_t *__restrict__ block_cnt) {
    __shared__ uint32_t s_red[NF_T / 64];
    const uint64_t base = (uint64_t) blockIdx.x * PA_BLOCK_EVENTS;
    const uint32_t bits = verdict_keep_bits<0u>(verdict, base, (uint32_t) threadIdx.x * SC_PER, stream_block_count(n_events, base));
    const uint32_t keep = block_sum<NF_T>((uint32_t) __popc(bits), s_red);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = keep;
}

}  // namespace ecal

using namespace ecal;

static_assert(sizeof(ecal_noise_options) == sizeof(NoiseOptions) && sizeof(ecal_noise_options) == 32, "the options are the shared header's, no padding");
static_assert(sizeof(ecal_filter_totals) == sizeof(FilterTotals), "the totals are the shared header's");

extern "C" void ecal_noise_default_options(ecal_noise_options *opt) {
    if (!opt) return;
    const NoiseOptions d = nf_default_options();
    memcpy(opt, &d, sizeof(d));
}

static NoiseOptions noise_options(const ecal_noise_options *opt) {
    NoiseOptions o = nf_default_options();
    if (opt) memcpy(&o, opt, sizeof(o));
    return o;
}

extern "C" int ecal_noise_verdict_host(const uint8_t *events, uint64_t n_events, const ecal_noise_options *opt, uint8_t *verdict,
                                       ecal_filter_totals *totals) {
    if (totals) memset(totals, 0, sizeof(*totals));
    const NoiseOptions o = noise_options(opt);
    if (nf_options_error(o) || (n_events && (!events || !verdict))) return ECAL_ERR_INVALID;
    const FilterTotals t = nf_verdict_sequential(events, n_events, o, verdict);
    if (totals) memcpy(totals, &t, sizeof(t));
    return ECAL_OK;
}

static int noise_check(ecal_ctx *ctx, const char *who, uint64_t n_events, const NoiseOptions &o) {
    if (const char *bad = nf_options_error(o)) {
        ctx->last_error = std::string(who) + ": " + bad;
        return ECAL_ERR_INVALID;
    }
    return ecal_events_range_check(ctx, who, n_events);
}

namespace {
// ctx->noise_scratch for n events on a plane of pixels: keys and indices in and out of the sort, the stamps in sorted order, the
// start table, the verdict tables (ecal_verdict_tables_at: verdict bytes in whole blocks, per-block counts / offsets), the sort's workspace
struct noise_layout {
    size_t o_kin, o_kout, o_vin, o_vout, o_sts, o_start, o_verdict, o_tmp, total;
    noise_layout(size_t n, size_t plane, size_t nb, size_t tmp_bytes) {
        auto up = [](size_t v) { return (v + 255) & ~(size_t) 255; };
        size_t at = 0;
        o_sts = at, at += up(n * 8);
        o_kin = at, at += up(n * 4);
        o_kout = at, at += up(n * 4);
        o_vin = at, at += up(n * 4);
        o_vout = at, at += up(n * 4);
        o_start = at, at += up((plane + 1) * 4);
        o_verdict = at, at += up(ecal_verdict_tables_bytes((uint32_t) nb));
        o_tmp = at, at += tmp_bytes;
        total = at;
    }
};
}  // namespace

// The verdicts of n_events > 0 events into d_verdict (any alignment; null: the scratch's own whole blocks, for the compaction), the
// totals (may be null; zeroed by the caller).  Leaves the layout in *L_out.  Options checked by the caller.
static int noise_verdicts(ecal_ctx *ctx, const uint8_t *d_events, uint32_t n, const NoiseOptions &o, uint8_t *d_verdict, ecal_filter_totals *d_totals,
                          ecal_load_timer &tm, noise_layout *L_out, hipStream_t st) {
    const uint32_t plane = o.width * o.height, bits = nf_key_bits(plane);
    const uint32_t nb = ecal_stream_blocks(n);
    size_t tmp_bytes = 0;
    uint32_t *k_in = nullptr, *k_out = nullptr, *v_in = nullptr, *v_out = nullptr;
    ECAL_HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, (size_t) n, 0, bits, st));
    const noise_layout L(n, plane, nb, tmp_bytes);
    const int rc = ecal_ensure(ctx, ctx->noise_scratch, L.total);
    if (rc) return rc;
    uint8_t *base = ctx->noise_scratch.as<uint8_t>();
    k_in = reinterpret_cast<uint32_t *>(base + L.o_kin);
    k_out = reinterpret_cast<uint32_t *>(base + L.o_kout);
    v_in = reinterpret_cast<uint32_t *>(base + L.o_vin);
    v_out = reinterpret_cast<uint32_t *>(base + L.o_vout);
    double *sts = reinterpret_cast<double *>(base + L.o_sts);
    uint32_t *start = reinterpret_cast<uint32_t *>(base + L.o_start);
    const uint32_t g_events = (uint32_t) (((uint64_t) n + NF_T - 1) / NF_T);
    const uint64_t n_index = (uint64_t) n > (uint64_t) plane + 1 ? (uint64_t) n : (uint64_t) plane + 1;
    tm.mark("start");
    hipLaunchKernelGGL(noise_key_kernel, dim3(g_events), dim3(NF_T), 0, st, d_events, n, o.width, o.height, k_in, v_in);
    tm.mark("keys");
    ECAL_HIP_TRY(ctx, rocprim::radix_sort_pairs(base + L.o_tmp, tmp_bytes, k_in, k_out, v_in, v_out, (size_t) n, 0, bits, st));   // (stable)
    tm.mark("sort");
    hipLaunchKernelGGL(noise_index_kernel, dim3((uint32_t) ((n_index + NF_T - 1) / NF_T)), dim3(NF_T), 0, st, d_events, n, (const uint32_t *) k_out,
                       (const uint32_t *) v_out, plane, start, sts);
    tm.mark("index");
    hipLaunchKernelGGL(noise_support_kernel, dim3(g_events), dim3(NF_T), 0, st, n, (const uint32_t *) k_out, (const uint32_t *) v_out,
                       (const double *) sts, (const uint32_t *) start, o.width, o.height, o.radius, o.min_support, o.include_self, o.dt,
                       d_verdict ? d_verdict : base + L.o_verdict, (unsigned long long *) d_totals);
    tm.mark("support");
    ECAL_HIP_TRY(ctx, hipGetLastError());
    if (L_out) *L_out = L;
    return ECAL_OK;
}

extern "C" int ecal_noise_verdict_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_noise_options *opt, uint8_t *d_verdict,
                                      ecal_filter_totals *d_totals, void *stream) {
    const ecal_range range__(ctx, "ecal_noise_verdict");
    if (!ctx) return ECAL_ERR_INVALID;
    if (n_events && (!d_events || !d_verdict)) {
        ctx->last_error = "ecal_noise_verdict: null pointer (events or verdict)";
        return ECAL_ERR_INVALID;
    }
    const NoiseOptions o = noise_options(opt);
    const int rc = noise_check(ctx, "ecal_noise_verdict", n_events, o);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    if (d_totals) ECAL_HIP_TRY(ctx, hipMemsetAsync(d_totals, 0, sizeof(ecal_filter_totals), st));
    if (!n_events) return ECAL_OK;
    ecal_load_timer tm("noise filter", ctx->sw.load_trace, st);
    const int vrc = noise_verdicts(ctx, d_events, (uint32_t) n_events, o, d_verdict, d_totals, tm, nullptr, st);
    if (vrc) return vrc;
    if (tm.on) ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));   // (ECAL_TRACE=load alone: the timer reads its events when it goes out of scope)
    return ECAL_OK;
}

extern "C" int ecal_denoise_events_dev(ecal_ctx *ctx, const uint8_t *d_events, uint64_t n_events, const ecal_noise_options *opt, uint8_t *d_out,
                                       uint32_t *d_count, ecal_filter_totals *d_totals, void *stream) {
    const ecal_range range__(ctx, "ecal_denoise_events");
    if (!ctx) return ECAL_ERR_INVALID;
    if (!d_count || (n_events && (!d_events || !d_out))) {
        ctx->last_error = "ecal_denoise_events: null pointer (count, events or output)";
        return ECAL_ERR_INVALID;
    }
    const NoiseOptions o = noise_options(opt);
    int rc = noise_check(ctx, "ecal_denoise_events", n_events, o);
    if (rc) return rc;
    hipStream_t st = (hipStream_t) stream;
    if ((rc = ecal_compact_begin(ctx, "ecal_denoise_events", d_events, n_events, d_out, d_count, d_totals, sizeof(ecal_filter_totals), st))) return rc;
    if (!n_events) return ECAL_OK;
    ecal_load_timer tm("noise filter", ctx->sw.load_trace, st);
    noise_layout L(0, 0, 0, 0);
    rc = noise_verdicts(ctx, d_events, (uint32_t) n_events, o, nullptr, d_totals, tm, &L, st);
    if (rc) return rc;
    const ecal_verdict_tables V = ecal_verdict_tables_at(ctx->noise_scratch.as<uint8_t>() + L.o_verdict, ecal_stream_blocks(n_events));
    hipLaunchKernelGGL(noise_count_kernel, dim3(V.nb), dim3(NF_T), 0, st, (const uint8_t *) V.verdict, (uint32_t) n_events, V.cnt);
    tm.mark("count");
    rc = ecal_compact_copy_by_verdict(ctx, d_events, n_events, V, d_out, d_count, tm, st);
    if (rc) return rc;
    if (tm.on) ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));   // (ECAL_TRACE=load alone: the timer reads its events when it goes out of scope)
    return ECAL_OK;
}

extern "C" int ecal_stream_remove_noise(ecal_ctx *ctx, const ecal_stream *in, const ecal_noise_options *opt, ecal_stream **out,
                                        ecal_filter_totals *totals) {
    if (!ctx || !in || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    if (totals) memset(totals, 0, sizeof(*totals));
    const NoiseOptions o = noise_options(opt);
    const uint64_t n = ecal_stream_size(in);
    int rc = noise_check(ctx, "ecal_stream_remove_noise", n, o);
    if (rc) return rc;
    const uint8_t *d_in = ecal_stream_data(in);
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // filter totals | count
    rc = ecal_ensure(ctx, ctx->noise_results, sizeof(ecal_filter_totals) + 8);
    if (rc) return rc;
    ecal_filter_totals T;
    return ecal_stream_compacted(
        ctx, "ecal_stream_remove_noise", in, ctx->noise_results.ptr, &T, sizeof(T),
        [&](uint8_t *d_out, uint32_t *d_count, void *d_totals, hipStream_t st) {
            return ecal_denoise_events_dev(ctx, d_in, n, opt, d_out, d_count, (ecal_filter_totals *) d_totals, st);
        },
        [&](uint32_t kept, uint64_t n_in) -> const char * {
            if (totals) *totals = T;
            return T.n_kept != kept || T.n_removed + T.n_kept != n_in ? "the filter's counters disagree" : nullptr;
        },
        out);
}
