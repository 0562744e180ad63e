// Continuous-time calibration solve: per-event residual / Jacobian and the stacked normal equations
// on the GPU, Levenberg-Marquardt and the block-banded arrow Cholesky on the host.
//
// Replaces, for the quaternion-spline variant (useSO3 = 0, the shipped default):
//   EventCalibSpline::optimize's Ceres problem (event_camera_calib/src/EventCalibSpline.cpp:196-247):
//     one residual block [9,4,4,4,4,3,3,3,3] per associated event, HuberLoss(0.2 R),
//     EigenQuaternionParameterization, SPARSE_NORMAL_CHOLESKY, tolerances 1e-10, 50 iterations;
//   CalibReprojectionError::operator() (EventCalibSpline.hpp:158-229) — see spline_residual.hpp.
// Residuals are sorted by (segment, time); a "chunk" is a run of residuals inside one knot span, so all
// its rows share the same 33 columns and J^T J of the chunk is one dense 34x34 (33 + residual) Gram
// matrix: a genuine dense contraction, accumulated on the matrix cores with v_mfma_f64_4x4x4_4b_f64 (nine 4-column tiles of
// the padded 36 columns, 45 tile pairs, 16 rows per round — see normal_eq_kernel).  History of the alternatives, each with its
// measurement: v_mfma_f64_16x16x4_f64 (34 -> 48 columns, 2x the multiply-adds: 4.63 ms per evaluation against 3.59,
// profiles/experiments/r02_normal_eq_mfma_f64.patch); register-tiled v_fma_f64 (6x6 tiles, rounds 2 - 5: 2.28 ms) and
// producer / consumer waves on those tiles (2.70 ms) against this kernel's 1.71 ms at 45 M residuals
// (profiles/experiments/r06_normal_eq_fma_tiles_and_two_roles.patch, profiles/r06_ne_mfma_vs_fma.txt).
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <limits>
#include <sched.h>
#include "ecal_solver_state.hpp"
#include "spline_residual.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

namespace ecal {

// (ResRecord, Chunk, NE_T, NE_CHUNK, NeProgress, struct ecal_solver: ecal_solver_state.hpp)

constexpr int NE_LD = 36;   // padded row: 33 Jacobian entries, the residual, 2 zeros
// Gram accumulation: 4-column tiles of the padded row (v_mfma_f64_4x4x4_4b_f64 multiplies four 4x4 blocks per instruction)
constexpr int NE_TW = 4, NE_TG = NE_LD / NE_TW, NE_TILES = NE_TG * (NE_TG + 1) / 2, NE_WAVES = NE_T / 64;
constexpr uint32_t NE_REPL = 64;      // replicas of the shared head (cost, intrinsics block) that the chunks add into

// (accumulation buffer layout: ACC_HEAD, ACC_PER_CP — arrow_layout.hpp)

__device__ __forceinline__ void local_to_unknown(int li, uint32_t c0, bool &is_intr, uint32_t &cp, uint32_t &comp) {
    if (li < 9) {
        is_intr = true;
        cp = 0;
        comp = (uint32_t) li;
    } else if (li < 21) {
        is_intr = false;
        cp = c0 + (uint32_t) (li - 9) / 3u;
        comp = (uint32_t) (li - 9) % 3u;
    } else {
        is_intr = false;
        cp = c0 + (uint32_t) (li - 21) / 3u;
        comp = 3u + (uint32_t) (li - 21) % 3u;
    }
}

// (profiling builds: -DECAL_NE_SKIP_P1 / -DECAL_NE_SKIP_P2 drop the residual code / the Gram accumulation: the phase split of
// profiles/r06_notes.md.  Results are meaningless in those builds.)
// Row index swizzle of the wave's column-major slab (see normal_eq_kernel)
__host__ __device__ constexpr int ne_swz(int c) { return 16 * (c & 1) ^ 2 * ((c >> 1) & 1); }

// (the streamed evaluation's progress block, NeProgress: ecal_solver_state.hpp)

// records [r_lo, r_hi) of the accumulation buffer to the host's copy; the values were added by other workgroups' atomics on
// any of the eight XCDs: agent-scope loads (a plain load could be served from this XCD's L2)
__device__ __forceinline__ void ne_copy_records(const double *accum, double *host, uint32_t r_lo, uint32_t r_hi, int tid, int nthreads) {
    const size_t lo = ACC_HEAD + ACC_PER_CP * (size_t) r_lo, hi = ACC_HEAD + ACC_PER_CP * (size_t) r_hi;
    for (size_t i = lo + (size_t) tid; i < hi; i += 8 * (size_t) nthreads) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const size_t k = i + (size_t) u * nthreads;
            v[u] = k < hi ? __hip_atomic_load(accum + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const size_t k = i + (size_t) u * nthreads;
            if (k < hi) host[k] = v[u];
        }
    }
}

// the end of a chunk's workgroup in a streamed evaluation (NeProgress): the group's (and its separators') records to the host
// when this chunk is the last one of the group.  Called by every thread of the workgroup (nthreads of them) after its adds.
__device__ __forceinline__ void ne_publish_progress(const NeProgress *__restrict__ prog, uint32_t epoch, const double *accum, uint32_t c0, int tid,
                                                    int nthreads) {
    __shared__ uint32_t fin[3];
    __threadfence();
    __syncthreads();   // every thread's adds are out
    const uint32_t P = prog->n_groups;
    if (tid == 0) {
        const uint32_t sg = c0 + 3;
        uint32_t g = 0;
        while (g + 1 < P && prog->cut[g + 1] <= sg) g++;
        uint32_t *left = prog->left;
        const bool last = atomicSub(&left[g], 1u) == 1u;
        fin[0] = last ? g + 1 : 0;
        fin[1] = fin[2] = 0;
        if (last) {
            left[g] = prog->init[g];
            if (g > 0 && atomicSub(&left[NE_MAX_GROUPS + g - 1], 1u) == 1u) {
                fin[1] = 1;
                left[NE_MAX_GROUPS + g - 1] = prog->init[NE_MAX_GROUPS + g - 1];
            }
            if (g + 1 < P && atomicSub(&left[NE_MAX_GROUPS + g], 1u) == 1u) {
                fin[2] = 1;
                left[NE_MAX_GROUPS + g] = prog->init[NE_MAX_GROUPS + g];
            }
        }
    }
    __syncthreads();
    if (fin[0]) {
        __threadfence();
        const uint32_t g = fin[0] - 1;
        const uint32_t c_lo = prog->cut[g], c_next = prog->cut[g + 1];
        double *host = prog->host_acc;
        ne_copy_records(accum, host, c_lo, g + 1 < P ? c_next - 3 : c_next, tid, nthreads);
        if (fin[1]) ne_copy_records(accum, host, c_lo - 3, c_lo, tid, nthreads);
        if (fin[2]) ne_copy_records(accum, host, c_next - 3, c_next, tid, nthreads);
        __threadfence_system();
        __syncthreads();
        if (tid == 0) {
            uint32_t *flag = prog->host_flag;
            __hip_atomic_store(&flag[g], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            if (fin[1]) __hip_atomic_store(&flag[NE_MAX_GROUPS + g - 1], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            if (fin[2]) __hip_atomic_store(&flag[NE_MAX_GROUPS + g], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// WITH_JAC = false: cost only (no rows, no LDS, no tiles) — its own, small instantiation: 66 / 107 / 142 / 168 registers over
// quaternion radial / quaternion fisheye / SO3 radial / SO3 fisheye against 225 / 255 / 374 / 402 with the Jacobian (the SO3 ones
// with 118 / 146 of them AGPRs; ROCm 7.2.0, no scratch)
template <bool SO3, bool WITH_JAC, bool FISHEYE = false>
__global__ __launch_bounds__(NE_T, SO3 ? 1 : 2) void normal_eq_kernel(const ResRecord *__restrict__ rec,
                                                         const Chunk *__restrict__ chunks,
                                                         const double *__restrict__ knots,
                                                         const uint32_t *__restrict__ knot_off,
                                                         const uint32_t *__restrict__ cp_off,
                                                         const double *__restrict__ params, uint32_t n_cp_total,
                                                         const double *__restrict__ landmarks, double radius,
                                                         double huber_a, double *__restrict__ accum,
                                                         double *__restrict__ heads, const NeProgress *__restrict__ prog,
                                                         uint32_t epoch) {
    constexpr bool with_jac = WITH_JAC;
    extern __shared__ __attribute__((aligned(16))) double rows[];  // with_jac: [NE_WAVES][NE_LD columns][64 rows]
    __shared__ double red[NE_T / 64];
    const Chunk ch = chunks[blockIdx.x];
    const int tid = threadIdx.x;
    // every chunk touches the cost and the 9x9 intrinsics block: spread those adds over NE_REPL copies
    double *const head = heads + (size_t) (blockIdx.x % NE_REPL) * ACC_HEAD;
    const double *kn = knots + knot_off[ch.seg];
    const uint32_t c0 = cp_off[ch.seg] + ch.span - 3;
    const double *intr = params;
    const double *qall = params + 9;
    const double *tall = params + 9 + 4 * (size_t) n_cp_total;
    // (this prologue is written out here, in residual_rows_kernel and in report_kernel: shared with ecal_report_px.hip's ChunkPose,
    // as a struct or as a function, it moves those kernels.  The fill of ResidualInput below is residual_input_fill's, written out
    // in this kernel alone: the call moves six of its eight instantiations — design/08_solver.md, "One copy of the residual's
    // pieces")
    double q[4][4], t[4][3], pin[9], binv[6];
    for (int i = 0; i < 9; i++) pin[i] = intr[i];
    spline_span_inverses(kn, ch.span, binv);           // uniform over the chunk: 6 + 2 divisions per thread, not per residual
    const double ifx = 1.0 / pin[0], ify = 1.0 / pin[1], inv_huber_a = 1.0 / huber_a;
    for (int j = 0; j < 4; j++) {
        for (int k = 0; k < 4; k++) q[j][k] = qall[4 * (size_t) (c0 + j) + k];
        for (int k = 0; k < 3; k++) t[j][k] = tall[3 * (size_t) (c0 + j) + k];
    }
    // Gram accumulation on the matrix cores.  v_mfma_f64_4x4x4_4b_f64 multiplies four independent 4x4x4 blocks: block blk takes
    // rows 4 blk .. 4 blk + 3 of a 16-row step, and all four blocks multiply the same pair of column tiles (ta, tb), so lane
    // (x, blk, k) = (l & 3, (l >> 2) & 3, l >> 4) supplies J[row 4 blk + k][column 4 ta + x] as A[blk][i = x][k] and
    // J[row 4 blk + k][4 tb + x] as B[blk][k][j = x]: ONE register per column tile serves as the left and as the right operand
    // (lane maps: profiles/r05_mfma_f64_probe.txt).  Nine 8-byte LDS reads per lane and 45 instructions per 16 rows; 45
    // accumulators per lane (D[blk][i][j] of pair p in lane j + 4 blk + 16 i), summed over blk at the end of the chunk.
    // The rows go through THIS WAVE's slab of the row buffer, column-major ([column][row of the wave's 64]) with the row index
    // XOR-ed by ne_swz(column): lane l writes its row's entry of column c at c * 64 + (l ^ swz(c)) — a permutation of 64
    // consecutive doubles, conflict-free — and the operand read above puts the 32 lanes of either half-wave on 32 different
    // 8-byte bank pairs.  No other wave touches the slab: the batch loop has no workgroup barrier.
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    double acc[NE_TILES];
#pragma unroll
    for (int i = 0; i < NE_TILES; i++) acc[i] = 0.0;
    double cost = 0.0;
    double *const slab = rows + (size_t) wave * (NE_LD * 64);
    if constexpr (with_jac) {
        slab[34 * 64 + lane] = 0.0;     // the two padding columns of tile 8: written once
        slab[35 * 64 + lane] = 0.0;
    }

    // the record of the NEXT batch is asked for before this batch's residual is evaluated: its trip to HBM (the only one a
    // batch makes) runs behind ~2000 cycles of arithmetic instead of in front of them
    ResRecord e_next = rec[ch.start + min((uint32_t) tid, ch.count - 1u)];
    for (uint32_t b0 = 0; b0 < ch.count; b0 += NE_T) {
        const uint32_t k = b0 + tid;
        double J[RES_NJ];
        double r = 0.0, sc = 0.0;
        const ResRecord e = e_next;
        e_next = rec[ch.start + min(k + (uint32_t) NE_T, ch.count - 1u)];
        // (no branch around the residual code: a lane past the chunk's end — the last batch only — evaluates the chunk's last
        // record again, which it holds anyway (clamped load), and its row is scaled by zero: the row's 34 stores need no selects)
        const bool live = k < ch.count;
#ifdef ECAL_NE_SKIP_P1
        {
            r = e.u;
            sc = live ? e.v : 0.0;
            for (int i = 0; i < RES_NJ; i++) J[i] = e.t + i;
            cost += live ? r : 0.0;
        }
        if (false) {
#else
        {
#endif
            ResidualInput in;
            in.u = e.u;
            in.v = e.v;
            in.lmx = landmarks[3 * (size_t) e.lm];
            in.lmy = landmarks[3 * (size_t) e.lm + 1];
            in.lmz = landmarks[3 * (size_t) e.lm + 2];
            in.radius = radius;
            in.ifx = ifx;
            in.ify = ify;
            spline_basis_inv(kn, ch.span, binv, e.t, in.b);
            double hr = 0.0;
            if constexpr (with_jac) {   // the row comes out scaled by sqrt(rho') (ResidualInput)
                in.huber_a = huber_a;
                in.dead = !live;
                in.inv_huber_a = inv_huber_a;
                in.sc_out = &sc;
                in.half_rho_out = &hr;
            }
            r = SO3 ? spline_residual_so3<FISHEYE>(in, pin, q, t, with_jac ? J : nullptr)
                    : spline_residual<FISHEYE>(in, pin, q, t, with_jac ? J : nullptr);
            if constexpr (!with_jac) sc = huber_scale(r, huber_a, &hr, inv_huber_a);
            cost += live ? hr : 0.0;
        }
        if constexpr (with_jac) {
#pragma unroll
            for (int i = 0; i < RES_NJ; i++) slab[i * 64 + (lane ^ ne_swz(i))] = J[i];
            slab[33 * 64 + (lane ^ ne_swz(33))] = r * sc;
            // the slab is this wave's alone: no workgroup barrier.  A wave's LDS operations complete in order; the fence keeps the
            // compiler from moving the reads above the writes (other lanes' data) or the next batch's writes above these reads.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#ifndef ECAL_NE_SKIP_P2
            const uint32_t nrow = min((uint32_t) NE_T, ch.count - b0);
            const int x = lane & 3, r0 = ((lane >> 2) & 3) * 4 + (lane >> 4);
            const int pb = x * 64 + (r0 ^ (x & 2));                   // (row ^ swz) = 16 (s ^ (x & 1)) + (r0 ^ (x & 2))
            const double *const base_e = slab + pb + 16 * (x & 1);      // even steps (s = 0, 2): + 32 (s >> 1)
            const double *const base_o = slab + pb + 16 * (1 - (x & 1));  // odd steps
#pragma unroll
            for (int s4 = 0; s4 < 4; s4++) {
                if ((uint32_t) (64 * wave + 16 * s4) >= nrow) break;     // wave-uniform: only the chunk's last batch
                const double *const bs = ((s4 & 1) ? base_o : base_e) + 32 * (s4 >> 1);
                double R[NE_TG];
#pragma unroll
                for (int t9 = 0; t9 < NE_TG; t9++) R[t9] = bs[t9 * 256];
                int p = 0;
#pragma unroll
                for (int ta = 0; ta < NE_TG; ta++)
#pragma unroll
                    for (int tb = ta; tb < NE_TG; tb++, p++) acc[p] = __builtin_amdgcn_mfma_f64_4x4x4f64(R[ta], R[tb], acc[p], 0, 0, 0);
            }
#endif
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    // cost: block reduction, one atomic per workgroup
    for (int o = 32; o > 0; o >>= 1) cost += __shfl_down(cost, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = cost;
    __syncthreads();
    if (tid == 0) {
        double c = 0;
        for (int w = 0; w < NE_T / 64; w++) c += red[w];
        atomicAdd(&head[0], c);
    }
    if (!with_jac) return;
    // the waves' partial tiles are summed in LDS (the row buffer is free now) so that ONE set of FP64 atomics per chunk goes out
    // (~600 instead of 4 x ~600)
    {
        constexpr int TSZ = NE_TW * NE_TW, NPART = NE_TILES * TSZ;
        double *part = rows;                         // [NE_WAVES][NE_TILES * TSZ]
        double *total = rows;                        // (in place of wave 0's slice: entry e is read and written by ONE thread)
        static_assert(NE_WAVES * NPART <= NE_T * NE_LD, "the row buffer holds the partial tiles");
        __syncthreads();
        // D[blk][i][j] of tile pair p sits in lane j + 4 blk + 16 i: the four blocks (this wave's rows 4 blk + k of every step)
        // are summed across lane bits 2-3, block 0's lanes store entry (i, j) of the wave's partial tile
#pragma unroll
        for (int p = 0; p < NE_TILES; p++) {
            double v = acc[p];
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            if ((lane & 12) == 0) part[(size_t) wave * NPART + p * TSZ + 4 * (lane >> 4) + (lane & 3)] = v;
        }
        __syncthreads();
        for (int e = tid; e < NPART; e += NE_T) {    // every thread sums a few entries over the groups
            double v = 0.0;
#pragma unroll
            for (int g = 0; g < NE_WAVES; g++) v += part[(size_t) g * NPART + e];
            total[e] = v;
        }
        __syncthreads();
        // flush: one entry of the summed tiles per thread and turn (not a tile per thread: nothing of acc[] stays live)
        for (int e = tid; e < NPART; e += NE_T) {
            const double v = total[e];
            if (v == 0.0) continue;
            const int tile = e / TSZ, x = (e % TSZ) / NE_TW, y = e % NE_TW;
            int fi = 0, rem = tile;   // tile -> (fi, fj), fi <= fj, rows of the upper triangle
            for (fi = 0; fi < NE_TG; fi++) {
                if (rem < NE_TG - fi) break;
                rem -= NE_TG - fi;
            }
            const int fj = fi + rem;
            const int li = NE_TW * fi + x, lj = NE_TW * fj + y;
            if (li > lj || lj >= 34 || li >= 33) continue;
            bool ia, ib;
            uint32_t ca, ka, cb, kb;
            local_to_unknown(li, c0, ia, ca, ka);
            if (lj == 33) {  // gradient J^T r
                if (ia) atomicAdd(&head[1 + ka], v);
                else atomicAdd(&accum[ACC_HEAD + ACC_PER_CP * (size_t) ca + ka], v);
                continue;
            }
            local_to_unknown(lj, c0, ib, cb, kb);
            if (ia && ib) {
                atomicAdd(&head[10 + 9 * ka + kb], v);
            } else if (ia) {  // intrinsics x control point
                atomicAdd(&accum[ACC_HEAD + ACC_PER_CP * (size_t) cb + 6 + 9 * kb + ka], v);
            } else {
                if (ca > cb || (ca == cb && ka > kb)) {  // keep blocks (c, c+d), d >= 0; diagonal upper
                    const uint32_t tc = ca, tk = ka;
                    ca = cb;
                    ka = kb;
                    cb = tc;
                    kb = tk;
                }
                atomicAdd(&accum[ACC_HEAD + ACC_PER_CP * (size_t) ca + 60 + 36 * (cb - ca) + 6 * ka + kb], v);
            }
        }
    }
    if (prog) ne_publish_progress(prog, epoch, accum, c0, tid, NE_T);
}

template <bool SO3, bool FISHEYE = false>
__global__ __launch_bounds__(NE_T) void residual_rows_kernel(const ResRecord *__restrict__ rec, const Chunk *__restrict__ chunks,
                                                            const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                                            const uint32_t *__restrict__ cp_off, const double *__restrict__ params,
                                                            uint32_t n_cp_total, const double *__restrict__ landmarks, double radius,
                                                            double *__restrict__ r_out, double *__restrict__ J_out,
                                                            uint32_t *__restrict__ cp0_out) {
    const Chunk ch = chunks[blockIdx.x];
    const double *kn = knots + knot_off[ch.seg];
    const uint32_t c0 = cp_off[ch.seg] + ch.span - 3;
    const double *qall = params + 9;
    const double *tall = params + 9 + 4 * (size_t) n_cp_total;
    double q[4][4], t[4][3], pin[9], binv[6];
    for (int i = 0; i < 9; i++) pin[i] = params[i];
    spline_span_inverses(kn, ch.span, binv);
    const double ifx = 1.0 / pin[0], ify = 1.0 / pin[1];
    for (int j = 0; j < 4; j++) {
        for (int k = 0; k < 4; k++) q[j][k] = qall[4 * (size_t) (c0 + j) + k];
        for (int k = 0; k < 3; k++) t[j][k] = tall[3 * (size_t) (c0 + j) + k];
    }
    for (uint32_t k = threadIdx.x; k < ch.count; k += NE_T) {
        const size_t at = (size_t) ch.start + k;
        const ResRecord e = rec[at];
        ResidualInput in;
        residual_input_fill(in, e, landmarks, radius, ifx, ify, kn, ch.span, binv);
        double J[RES_NJ];
        const double r = SO3 ? spline_residual_so3<FISHEYE>(in, pin, q, t, J_out ? J : nullptr)
                             : spline_residual<FISHEYE>(in, pin, q, t, J_out ? J : nullptr);
        r_out[at] = r;
        if (J_out)
            for (int i = 0; i < RES_NJ; i++) J_out[at * RES_NJ + i] = J[i];
        if (cp0_out) cp0_out[at] = c0;
    }
}

// accum[0..91) = sum over the replicas
__global__ void reduce_heads_kernel(const double *__restrict__ heads, double *__restrict__ accum, uint32_t n_out) {
    const uint32_t i = threadIdx.x;
    if (i >= n_out) return;
    double v = 0.0;
    for (uint32_t r = 0; r < NE_REPL; r++) v += heads[(size_t) r * ACC_HEAD + i];
    accum[i] = v;
}

}  // namespace ecal

using namespace ecal;

extern "C" void ecal_solver_destroy(ecal_solver *s) {
    if (!s) return;
    (void) hipSetDevice(s->ctx->device);
    void *ptrs[] = {s->d_rec, s->d_chunks, s->d_knots, s->d_landmarks, s->d_params, s->d_accum, s->d_heads, s->d_knot_off, s->d_cp_off,
                    s->d_left, s->d_prog, s->d_seg_range};
    for (void *p : ptrs)
        if (p) (void) hipFree(p);
    void *pinned[] = {s->h_acc, s->h_x, s->h_flag};
    for (void *p : pinned)
        if (p) (void) hipHostFree(p);
    delete s;
}

extern "C" size_t ecal_solver_normal_size(const ecal_solver *s) { return s ? s->n_accum() : 0; }
extern "C" size_t ecal_solver_param_size(const ecal_solver *s) { return s ? s->n_params() : 0; }
extern "C" uint32_t ecal_solver_num_chunks(const ecal_solver *s) { return s ? s->n_chunks : 0; }

extern "C" int ecal_solver_create(ecal_ctx *ctx, const ecal_spline_problem *p, ecal_solver **out) {
    if (!ctx || !p || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    if (p->n_segments < 1 || !p->seg_cp_off || !p->knots || !p->landmarks || (p->n_res && (!p->obs || !p->time || !p->lm_id))) {
        ctx->last_error = "null pointer / no segment";
        return ECAL_ERR_INVALID;
    }
    if (p->n_res > 0xFFFFFFFFull) return ECAL_ERR_RANGE;
    ecal_solver *s = new (std::nothrow) ecal_solver;
    if (!s) return ECAL_ERR_NOMEM;
    s->ctx = ctx;
    s->n_res = p->n_res;
    s->n_seg = p->n_segments;
    s->n_lm = p->n_landmarks;
    s->radius = p->circle_radius;
    s->huber_a = p->huber_a;
    s->use_so3 = p->use_so3 != 0;
    s->fisheye = p->camera_model == ECAL_CAMERA_FISHEYE;
    s->cp_off.assign(p->seg_cp_off, p->seg_cp_off + p->n_segments + 1);
    s->n_cp = s->cp_off[p->n_segments];
    s->knot_off.resize(p->n_segments + 1);
    for (uint32_t g = 0; g <= p->n_segments; g++) s->knot_off[g] = s->cp_off[g] + 4 * g;
    s->knots.assign(p->knots, p->knots + s->knot_off[p->n_segments]);
    for (uint32_t g = 0; g < p->n_segments; g++) {
        if (s->cp_off[g + 1] - s->cp_off[g] < 4) {
            ctx->last_error = "a spline segment needs at least degree + 1 = 4 control points";
            delete s;
            return ECAL_ERR_INVALID;
        }
    }
    // chunk table: residuals are sorted by (segment, time); cut at knot-span boundaries
    std::vector<ResRecord> recs(p->n_res);
    std::vector<Chunk> chunks;
    uint64_t i = 0;
    for (uint32_t g = 0; g < p->n_segments; g++) {
        const double *kn = s->knots.data() + s->knot_off[g];
        const uint32_t ncp = s->cp_off[g + 1] - s->cp_off[g];
        uint64_t e = i;
        while (e < p->n_res && (p->seg_id ? p->seg_id[e] : 0u) == g) e++;
        for (uint64_t k = i; k < e; k++) {
            if ((k > i && p->time[k] < p->time[k - 1]) || p->time[k] < kn[3] || p->time[k] > kn[ncp]) {
                ctx->last_error = "residual times must be sorted inside a segment and lie inside its knot range";
                delete s;
                return ECAL_ERR_INVALID;
            }
            if (p->lm_id[k] >= p->n_landmarks) {
                ctx->last_error = "landmark id out of range";
                delete s;
                return ECAL_ERR_INVALID;
            }
        }
        uint64_t a = i;
        for (uint32_t span = 3; span < ncp && a < e; span++) {
            uint64_t b;
            if (span == ncp - 1) {
                b = e;
            } else {
                b = std::lower_bound(p->time + a, p->time + e, kn[span + 1]) - p->time;  // [u_span, u_span+1)
            }
            // a span's residuals in EQUAL chunks of at most NE_CHUNK (whole batches of NE_T rows): with fixed-size chunks and a
            // remainder the workgroups alternate long / short (64 and 25 batches on the benchmark problem) and the launch ran a
            // third longer than with either 32 + 32 + 25 or one chunk of 88 batches (3.52 against 2.66 / 2.65 ms)
            if (b > a) {
                const uint64_t m = b - a, parts = (m + NE_CHUNK - 1) / NE_CHUNK;
                const uint64_t per = ((m + parts - 1) / parts + NE_T - 1) / NE_T * NE_T;
                for (uint64_t c = a; c < b; c += per) chunks.push_back(Chunk{(uint32_t) c, (uint32_t) std::min<uint64_t>(per, b - c), g, span});
            }
            a = b;
        }
        i = e;
    }
    if (i != p->n_res) {
        ctx->last_error = "seg_id must be non-decreasing and < n_segments";
        delete s;
        return ECAL_ERR_INVALID;
    }
    for (uint64_t k = 0; k < p->n_res; k++) {
        recs[k].u = p->obs[2 * k];
        recs[k].v = p->obs[2 * k + 1];
        recs[k].t = p->time[k];
        recs[k].lm = p->lm_id[k];
        recs[k].seg = p->seg_id ? p->seg_id[k] : 0u;
    }
    s->n_chunks = (uint32_t) chunks.size();
    hipError_t e = hipSetDevice(ctx->device);
    auto up = [&](void **dst, const void *src, size_t bytes) {
        if (e != hipSuccess) return;
        e = hipMalloc(dst, bytes ? bytes : 16);
        if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    };
    up((void **) &s->d_rec, recs.data(), recs.size() * sizeof(ResRecord));
    up((void **) &s->d_chunks, chunks.data(), chunks.size() * sizeof(Chunk));
    up((void **) &s->d_knots, s->knots.data(), s->knots.size() * sizeof(double));
    up((void **) &s->d_landmarks, p->landmarks, 3 * (size_t) p->n_landmarks * sizeof(double));
    up((void **) &s->d_knot_off, s->knot_off.data(), s->knot_off.size() * sizeof(uint32_t));
    up((void **) &s->d_cp_off, s->cp_off.data(), s->cp_off.size() * sizeof(uint32_t));
    s->landmarks.assign(p->landmarks, p->landmarks + 3 * (size_t) p->n_landmarks);
    const std::vector<double> seg_range = segment_time_ranges(s->knots, s->knot_off, s->cp_off);
    up((void **) &s->d_seg_range, seg_range.data(), seg_range.size() * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **) &s->d_params, s->n_params() * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **) &s->d_accum, s->n_accum() * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **) &s->d_heads, NE_REPL * ACC_HEAD * sizeof(double));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&normal_eq_kernel<false, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) (NE_T * NE_LD * sizeof(double)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&normal_eq_kernel<true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) (NE_T * NE_LD * sizeof(double)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&normal_eq_kernel<false, true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) (NE_T * NE_LD * sizeof(double)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&normal_eq_kernel<true, true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) (NE_T * NE_LD * sizeof(double)));
    if (e != hipSuccess) {
        ctx->last_error = std::string("ecal_solver_create: ") + hipGetErrorString(e);
        ecal_solver_destroy(s);
        return e == hipErrorOutOfMemory ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;
    }
    *out = s;
    return ECAL_OK;
}

// ---- the problem built in place from DEVICE arrays (the association's outputs) ---------------------------------------------
// EventCalibSpline::optimize adds a residual block per associated event where it finds it (EventCalibSpline.cpp:181-235);
// here the association (ecal_associate_ranges_dev) leaves obs / time / lm_id / seg_id in HBM and the solver's records and
// chunk table are made from them by three small kernels — the 28 bytes per residual never cross PCIe.
namespace {

// flags: 1 residual out of time order / outside its segment's knot range, 2 landmark id out of range, 4 segment ids not
// non-decreasing or >= n_segments
__global__ void solver_pack_kernel(const double *__restrict__ obs, const double *__restrict__ time, const uint32_t *__restrict__ lm,
                                   const uint32_t *__restrict__ seg, const uint32_t *__restrict__ d_n, uint64_t n_cap, uint32_t n_seg,
                                   uint32_t n_lm, const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                   const uint32_t *__restrict__ cp_off, ResRecord *__restrict__ rec, uint32_t *__restrict__ flags) {
    const uint64_t n = d_n ? (uint64_t) *d_n : n_cap;
    const uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0 && n > n_cap) atomicOr(flags, 8u);
    if (k >= n || k >= n_cap) return;
    ResRecord r;
    r.u = obs[2 * k];
    r.v = obs[2 * k + 1];
    r.t = time[k];
    r.lm = lm[k];
    r.seg = seg ? seg[k] : 0u;
    uint32_t f = 0;
    if (r.seg >= n_seg) {
        f |= 4u;
    } else {
        const double *kn = knots + knot_off[r.seg];
        const uint32_t ncp = cp_off[r.seg + 1] - cp_off[r.seg];
        if (r.t < kn[3] || r.t > kn[ncp]) f |= 1u;
        if (k > 0) {
            const uint32_t sp = seg ? seg[k - 1] : 0u;
            if (sp > r.seg) f |= 4u;
            if (sp == r.seg && r.t < time[k - 1]) f |= 1u;
        }
    }
    if (r.lm >= n_lm) f |= 2u;
    if (f) atomicOr(flags, f);
    rec[k] = r;
}

// one thread per (segment, span): the span's residual range [a, b) — [u_span, u_span+1) by lower bounds on the time, the first
// span from the segment's first residual, the last to its last — and how many equal chunks it is cut into (ecal_solver_create)
__global__ void solver_span_kernel(const ResRecord *__restrict__ rec, const uint32_t *__restrict__ d_n, uint64_t n_cap, uint32_t n_seg,
                                   const double *__restrict__ knots, const uint32_t *__restrict__ knot_off,
                                   const uint32_t *__restrict__ cp_off, const uint32_t *__restrict__ span_off /*[n_seg + 1]*/,
                                   uint32_t *__restrict__ span_a, uint32_t *__restrict__ span_m, uint32_t *__restrict__ span_chunks) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= span_off[n_seg]) return;
    const uint32_t n = (uint32_t) (d_n ? (uint64_t) *d_n : n_cap);
    uint32_t g = 0;
    while (j >= span_off[g + 1]) g++;
    const uint32_t ncp = cp_off[g + 1] - cp_off[g], span = 3u + (j - span_off[g]);
    const double *kn = knots + knot_off[g];
    // first index whose (segment, time) is not below (sg, tv)
    auto lower = [&](uint32_t sg, double tv, bool any_time) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const ResRecord &r = rec[mid];
            const bool below = r.seg < sg || (r.seg == sg && !any_time && r.t < tv);
            if (below) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    const uint32_t a = span == 3u ? lower(g, 0.0, true) : lower(g, kn[span], false);
    const uint32_t b = span == ncp - 1u ? lower(g + 1u, 0.0, true) : lower(g, kn[span + 1u], false);
    const uint32_t m = b > a ? b - a : 0u;
    span_a[j] = a;
    span_m[j] = m;
    uint32_t nch = 0;
    if (m) {
        const uint32_t parts = (m + NE_CHUNK - 1u) / NE_CHUNK;
        const uint32_t per = ((m + parts - 1u) / parts + NE_T - 1u) / NE_T * NE_T;
        nch = (m + per - 1u) / per;
    }
    span_chunks[j] = nch;
}

// exclusive scan of the spans' chunk counts (one workgroup), then every span writes its chunks
__global__ __launch_bounds__(1024) void solver_chunks_kernel(uint32_t n_spans, uint32_t n_seg, const uint32_t *__restrict__ span_off,
                                                             const uint32_t *__restrict__ span_a, const uint32_t *__restrict__ span_m,
                                                             const uint32_t *__restrict__ span_chunks, Chunk *__restrict__ chunks,
                                                             uint32_t chunk_cap, uint32_t *__restrict__ n_chunks_out) {
    __shared__ uint32_t red[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t j0 = 0; j0 < n_spans; j0 += 1024) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t v = j < n_spans ? span_chunks[j] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) red[wave] = inc;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wave) pre += red[w];
            tot += red[w];
        }
        if (j < n_spans && v) {
            uint32_t at = carry + pre + inc - v, g = 0;
            while (j >= span_off[g + 1]) g++;
            const uint32_t m = span_m[j], a = span_a[j], parts = (m + NE_CHUNK - 1u) / NE_CHUNK;
            const uint32_t per = ((m + parts - 1u) / parts + NE_T - 1u) / NE_T * NE_T;
            for (uint32_t c = 0; c < m; c += per, at++)
                if (at < chunk_cap) chunks[at] = Chunk{a + c, per < m - c ? per : m - c, g, 3u + (j - span_off[g])};
        }
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_chunks_out = carry;
}

}  // namespace

extern "C" int ecal_solver_create_dev(ecal_ctx *ctx, const ecal_spline_problem *p, const uint32_t *d_n_res, void *stream,
                                      ecal_solver **out) {
    if (!ctx || !p || !out) return ECAL_ERR_INVALID;
    *out = nullptr;
    if (p->n_segments < 1 || !p->seg_cp_off || !p->knots || !p->landmarks || (p->n_res && (!p->obs || !p->time || !p->lm_id))) {
        ctx->last_error = "null pointer / no segment";
        return ECAL_ERR_INVALID;
    }
    if (p->n_res > 0xFFFFFFFFull) return ECAL_ERR_RANGE;
    ecal_solver *s = new (std::nothrow) ecal_solver;
    if (!s) return ECAL_ERR_NOMEM;
    s->ctx = ctx;
    s->n_seg = p->n_segments;
    s->n_lm = p->n_landmarks;
    s->radius = p->circle_radius;
    s->huber_a = p->huber_a;
    s->use_so3 = p->use_so3 != 0;
    s->fisheye = p->camera_model == ECAL_CAMERA_FISHEYE;
    s->cp_off.assign(p->seg_cp_off, p->seg_cp_off + p->n_segments + 1);
    s->n_cp = s->cp_off[p->n_segments];
    s->knot_off.resize(p->n_segments + 1);
    for (uint32_t g = 0; g <= p->n_segments; g++) s->knot_off[g] = s->cp_off[g] + 4 * g;
    s->knots.assign(p->knots, p->knots + s->knot_off[p->n_segments]);
    std::vector<uint32_t> span_off(p->n_segments + 1, 0u);
    for (uint32_t g = 0; g < p->n_segments; g++) {
        if (s->cp_off[g + 1] - s->cp_off[g] < 4) {
            ctx->last_error = "a spline segment needs at least degree + 1 = 4 control points";
            delete s;
            return ECAL_ERR_INVALID;
        }
        span_off[g + 1] = span_off[g] + (s->cp_off[g + 1] - s->cp_off[g] - 3u);
    }
    const uint32_t n_spans = span_off[p->n_segments];
    const size_t n_cap = p->n_res;
    const size_t chunk_cap = n_cap / NE_CHUNK + n_spans + 1;   // a span of m residuals is cut into <= m / NE_CHUNK + 1 chunks
    hipStream_t st = (hipStream_t) stream;
    hipError_t e = hipSetDevice(ctx->device);
    uint32_t *d_tmp = nullptr;   // span_off [n_seg + 1] | span_a, span_m, span_chunks [n_spans] each | flags, n_chunks
    const size_t tmp_words = (p->n_segments + 1) + 3 * (size_t) n_spans + 4;
    auto up = [&](void **dst, const void *src, size_t bytes) {
        if (e != hipSuccess) return;
        e = hipMalloc(dst, bytes ? bytes : 16);
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st);
    };
    if (e == hipSuccess) e = hipMalloc((void **) &s->d_rec, (n_cap ? n_cap : 1) * sizeof(ResRecord));
    if (e == hipSuccess) e = hipMalloc((void **) &s->d_chunks, chunk_cap * sizeof(Chunk));
    if (e == hipSuccess) e = hipMalloc((void **) &d_tmp, tmp_words * sizeof(uint32_t));
    up((void **) &s->d_knots, s->knots.data(), s->knots.size() * sizeof(double));
    up((void **) &s->d_landmarks, p->landmarks, 3 * (size_t) p->n_landmarks * sizeof(double));
    up((void **) &s->d_knot_off, s->knot_off.data(), s->knot_off.size() * sizeof(uint32_t));
    up((void **) &s->d_cp_off, s->cp_off.data(), s->cp_off.size() * sizeof(uint32_t));
    s->landmarks.assign(p->landmarks, p->landmarks + 3 * (size_t) p->n_landmarks);
    const std::vector<double> seg_range = segment_time_ranges(s->knots, s->knot_off, s->cp_off);
    up((void **) &s->d_seg_range, seg_range.data(), seg_range.size() * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **) &s->d_params, s->n_params() * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **) &s->d_accum, s->n_accum() * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **) &s->d_heads, NE_REPL * ACC_HEAD * sizeof(double));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&normal_eq_kernel<false, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) (NE_T * NE_LD * sizeof(double)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&normal_eq_kernel<true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) (NE_T * NE_LD * sizeof(double)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&normal_eq_kernel<false, true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) (NE_T * NE_LD * sizeof(double)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&normal_eq_kernel<true, true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int) (NE_T * NE_LD * sizeof(double)));
    uint32_t h[2] = {0, 0}, h_n = (uint32_t) n_cap;
    if (e == hipSuccess) {
        uint32_t *d_span_off = d_tmp, *d_a = d_span_off + p->n_segments + 1, *d_m = d_a + n_spans, *d_c = d_m + n_spans,
                 *d_flags = d_c + n_spans;
        e = hipMemcpyAsync(d_span_off, span_off.data(), span_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_flags, 0, 4 * sizeof(uint32_t), st);
        if (e == hipSuccess && n_cap) {
            hipLaunchKernelGGL(solver_pack_kernel, dim3((unsigned) ((n_cap + 255) / 256)), dim3(256), 0, st, p->obs, p->time, p->lm_id, p->seg_id,
                               d_n_res, (uint64_t) n_cap, p->n_segments, p->n_landmarks, (const double *) s->d_knots,
                               (const uint32_t *) s->d_knot_off, (const uint32_t *) s->d_cp_off, s->d_rec, d_flags);
            hipLaunchKernelGGL(solver_span_kernel, dim3((n_spans + 255) / 256), dim3(256), 0, st, (const ResRecord *) s->d_rec, d_n_res,
                               (uint64_t) n_cap, p->n_segments, (const double *) s->d_knots, (const uint32_t *) s->d_knot_off,
                               (const uint32_t *) s->d_cp_off, (const uint32_t *) d_span_off, d_a, d_m, d_c);
            hipLaunchKernelGGL(solver_chunks_kernel, dim3(1), dim3(1024), 0, st, n_spans, p->n_segments, (const uint32_t *) d_span_off,
                               (const uint32_t *) d_a, (const uint32_t *) d_m, (const uint32_t *) d_c, s->d_chunks, (uint32_t) chunk_cap,
                               d_flags + 1);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h, d_flags, sizeof(h), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && d_n_res) e = hipMemcpyAsync(&h_n, d_n_res, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);   // (the one round trip of the call: 12 bytes)
    }
    if (d_tmp) (void) hipFree(d_tmp);
    if (e != hipSuccess) {
        ctx->last_error = std::string("ecal_solver_create_dev: ") + hipGetErrorString(e);
        ecal_solver_destroy(s);
        return e == hipErrorOutOfMemory ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;
    }
    if (h[0] || h[1] > chunk_cap) {
        ctx->last_error = (h[0] & 8u)   ? "more residuals than the arrays hold (*d_n_res > problem.n_res)"
                          : (h[0] & 4u) ? "seg_id must be non-decreasing and < n_segments"
                          : (h[0] & 2u) ? "landmark id out of range"
                                        : "residual times must be sorted inside a segment and lie inside its knot range";
        ecal_solver_destroy(s);
        return (h[0] & 8u) ? ECAL_ERR_RANGE : ECAL_ERR_INVALID;
    }
    s->n_res = h_n;
    s->n_chunks = h[1];
    *out = s;
    return ECAL_OK;
}

extern "C" uint64_t ecal_solver_num_residuals(const ecal_solver *s) { return s ? s->n_res : 0; }

// d_prog (with_jacobian only): the streamed form — the records reach the host's pinned buffer group by group (NeProgress)
static int solver_evaluate_dev(ecal_solver *s, const double *d_params, int with_jacobian, double *d_accum, void *stream,
                               const NeProgress *d_prog, uint32_t epoch) {
    const ecal_range range__(s ? s->ctx : nullptr, with_jacobian ? "ecal_solver_evaluate (normal equations)" : "ecal_solver_evaluate (cost)");
    if (!s || !d_params || !d_accum) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_accum, 0, (with_jacobian ? s->n_accum() : 1) * sizeof(double), st));
    ECAL_HIP_TRY(ctx, hipMemsetAsync(s->d_heads, 0, NE_REPL * ACC_HEAD * sizeof(double), st));
    if (s->n_chunks) {
        const size_t lds = with_jacobian ? NE_T * NE_LD * sizeof(double) : 0;
#define ECAL_NE_LAUNCH(SO3_, JAC_, FISH_)                                                                                          \
    hipLaunchKernelGGL((normal_eq_kernel<SO3_, JAC_, FISH_>), dim3(s->n_chunks), dim3(NE_T), lds, st, s->d_rec, s->d_chunks, s->d_knots, \
                       s->d_knot_off, s->d_cp_off, d_params, s->n_cp, s->d_landmarks, s->radius, s->huber_a, d_accum, s->d_heads,   \
                       with_jacobian ? d_prog : nullptr, epoch)
#define ECAL_NE_LAUNCH2(SO3_, JAC_)                                       \
    do {                                                                  \
        if (s->fisheye) ECAL_NE_LAUNCH(SO3_, JAC_, true);                 \
        else ECAL_NE_LAUNCH(SO3_, JAC_, false);                           \
    } while (0)
        if (s->use_so3) {
            if (with_jacobian) ECAL_NE_LAUNCH2(true, true); else ECAL_NE_LAUNCH2(true, false);
        } else {
            if (with_jacobian) ECAL_NE_LAUNCH2(false, true); else ECAL_NE_LAUNCH2(false, false);
        }
#undef ECAL_NE_LAUNCH2
#undef ECAL_NE_LAUNCH
        hipLaunchKernelGGL(reduce_heads_kernel, dim3(1), dim3(128), 0, st, s->d_heads, d_accum,
                           with_jacobian ? (uint32_t) ACC_HEAD : 1u);
        ECAL_HIP_TRY(ctx, hipGetLastError());
    }
    return ECAL_OK;
}
extern "C" int ecal_solver_evaluate_dev(ecal_solver *s, const double *d_params, int with_jacobian, double *d_accum,
                                        void *stream) {
    return solver_evaluate_dev(s, d_params, with_jacobian, d_accum, stream, nullptr, 0);
}

extern "C" int ecal_residuals_dev(ecal_solver *s, const double *d_params, double *d_r, double *d_J, uint32_t *d_cp0, void *stream) {
    if (!s || !d_params || (s->n_res && !d_r)) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t) stream;
    if (s->n_chunks) {
#define ECAL_RR_LAUNCH(SO3_, FISH_)                                                                                                  \
    hipLaunchKernelGGL((residual_rows_kernel<SO3_, FISH_>), dim3(s->n_chunks), dim3(NE_T), 0, st, s->d_rec, s->d_chunks, s->d_knots, \
                       s->d_knot_off, s->d_cp_off, d_params, s->n_cp, s->d_landmarks, s->radius, d_r, d_J, d_cp0)
        if (s->use_so3) {
            if (s->fisheye) ECAL_RR_LAUNCH(true, true); else ECAL_RR_LAUNCH(true, false);
        } else {
            if (s->fisheye) ECAL_RR_LAUNCH(false, true); else ECAL_RR_LAUNCH(false, false);
        }
#undef ECAL_RR_LAUNCH
        ECAL_HIP_TRY(ctx, hipGetLastError());
    }
    return ECAL_OK;
}

extern "C" int ecal_residuals(ecal_solver *s, const double *params, double *r, double *J, uint32_t *cp0) {
    if (!s || !params || (s->n_res && !r)) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = s->n_res;
    double *d_r = nullptr, *d_J = nullptr;
    uint32_t *d_c = nullptr;
    struct Guard {
        void *a = nullptr, *b = nullptr, *c = nullptr;
        ~Guard() {
            if (a) (void) hipFree(a);
            if (b) (void) hipFree(b);
            if (c) (void) hipFree(c);
        }
    } g;
    ECAL_HIP_TRY(ctx, hipMalloc((void **) &d_r, (n ? n : 1) * sizeof(double)));
    g.a = d_r;
    if (J) {
        ECAL_HIP_TRY(ctx, hipMalloc((void **) &d_J, (n ? n : 1) * RES_NJ * sizeof(double)));
        g.b = d_J;
    }
    if (cp0) {
        ECAL_HIP_TRY(ctx, hipMalloc((void **) &d_c, (n ? n : 1) * sizeof(uint32_t)));
        g.c = d_c;
    }
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_params, params, s->n_params() * sizeof(double), hipMemcpyHostToDevice, st));
    int rc = ecal_residuals_dev(s, s->d_params, d_r, d_J, d_c, st);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(r, d_r, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (J) ECAL_HIP_TRY(ctx, hipMemcpyAsync(J, d_J, n * RES_NJ * sizeof(double), hipMemcpyDeviceToHost, st));
    if (cp0) ECAL_HIP_TRY(ctx, hipMemcpyAsync(cp0, d_c, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}

extern "C" int ecal_solver_evaluate(ecal_solver *s, const double *params, int with_jacobian, double *accum) {
    if (!s || !params || !accum) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ECAL_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_params, params, s->n_params() * sizeof(double), hipMemcpyHostToDevice, st));
    int rc = ecal_solver_evaluate_dev(s, s->d_params, with_jacobian, s->d_accum, st);
    if (rc) return rc;
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(accum, s->d_accum, (with_jacobian ? s->n_accum() : 1) * sizeof(double),
                                     hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}

// ------------------------------------------------------------------------------------------------
// Host side: block-banded arrow system and Levenberg-Marquardt (Ceres 1.x trust-region loop restated)
// ------------------------------------------------------------------------------------------------
namespace {
#include "arrow_host.hpp"
#include "lm_loop.hpp"

// a NULL all-reduce is a rank-local solve, whether or not the context has joined a communicator: collectives are the
// caller's explicit choice (opt.allreduce = ecal_comm_allreduce, opt.allreduce_user = ctx, rank / world_size set)
int solve_validate(const ecal_solver *s, const ecal_lm_options &opt, RankShare &share) {
    ecal_ctx *ctx = s->ctx;
    if (opt.allreduce == ecal_comm_allreduce && (opt.allreduce_user != ctx || opt.rank != ctx->comm_rank || opt.world_size != ctx->comm_size)) {
        ctx->last_error = "ecal_solver_solve: ecal_comm_allreduce needs allreduce_user = the solver's context and its rank / world_size";
        return ECAL_ERR_INVALID;
    }
    share.mode = opt.allreduce && (opt.distributed == 1 || opt.distributed == 2) ? opt.distributed : 0;
    if (!share.mode) return ECAL_OK;
    share.world = std::max(1, opt.world_size), share.rank = opt.rank;
    if (share.rank < 0 || share.rank >= share.world || share.world > 1024) return ECAL_ERR_INVALID;
    if (share.mode == 2 && (s->n_seg != 1 || (uint32_t) (7 * share.world) > s->n_cp)) {
        ctx->last_error = "time-sharded solve: one spline segment with at least 7 control points per rank";
        return ECAL_ERR_INVALID;
    }
    if (share.mode == 2) arrow_partition(s->n_cp, share.world, share.ts_first, share.ts_num);
    return ECAL_OK;
}
// the sharded modes' small exchange buffers (device, pinned host), gone at the end of the solve whichever way it ends
struct ExchangeBuffers {
    double *d = nullptr, *h = nullptr;
    int alloc(ecal_ctx *ctx, size_t n) {
        ECAL_HIP_TRY(ctx, hipMalloc((void **) &d, n * sizeof(double)));
        return hipHostMalloc((void **) &h, n * sizeof(double), hipHostMallocDefault) == hipSuccess ? ECAL_OK : ECAL_ERR_NOMEM;
    }
    ~ExchangeBuffers() { (void) hipFree(d), (void) hipHostFree(h); }   // (a null pointer is fine with both)
};
// The HIP side of the loop's seam (LmDevice) for one ecal_solver_solve
struct SolveDevice {
    ecal_solver *const s;
    const ecal_lm_options &opt;
    const RankShare &share;
    ecal_ctx *const ctx = s->ctx;
    const hipStream_t st = ctx->stream;
    const size_t np = s->n_params(), na = s->n_accum();
    ExchangeBuffers small;
    HostPool *pool = nullptr;   // (the solver keeps the threads: starting fifteen of them costs as much as a tenth of an iteration each)
    int n_parts = 1;
    double t_eval = 0, t_pool = 0, t_tail = 0, tl_run = 0, tl_sync = 0;
    std::vector<double> tl_arrive, tl_done;   // ECAL_TRACE=solver: the last streamed evaluation's timeline (seconds from its start)
    const uint32_t epoch_at_start = s->stream_epoch;
    // pinned staging (the solver keeps it): the 3 MB buffer comes back every evaluation; the sharded modes' exchange buffers
    int alloc() {
        if (!s->h_acc) ECAL_HIP_TRY(ctx, hipHostMalloc((void **) &s->h_acc, na * sizeof(double), hipHostMallocDefault));
        if (!s->h_x) ECAL_HIP_TRY(ctx, hipHostMalloc((void **) &s->h_x, np * sizeof(double), hipHostMallocDefault));
        const size_t W = (size_t) share.world;
        return share.mode ? small.alloc(ctx, std::max<size_t>(128 + W, share.mode == 2 ? std::max<size_t>(TS_G * W, ACC_HEAD + 3 * ACC_PER_CP * (W - 1)) : 0)) : ECAL_OK;
    }
    bool upload(const double *x) {
        memcpy(s->h_x, x, np * sizeof(double));
        return hipMemcpyAsync(s->d_params, s->h_x, np * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    }
    int synchronize(hipError_t e = hipSuccess) {   // (e: of the call before it)
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) ctx->last_error = std::string("solver evaluate: ") + hipGetErrorString(e);
        return e == hipSuccess ? ECAL_OK : ECAL_ERR_HIP;
    }
    // time shards: the head and the separators' records (3 control points per cut) are what two ranks both add to
    bool copy_shared_records(bool to_small) {
        size_t at = 0;
        for (int c = -1; c + 1 < share.world; c++) {
            double *a = c < 0 ? s->d_accum : s->d_accum + ACC_HEAD + ACC_PER_CP * (size_t) (share.ts_first[c] + share.ts_num[c]), *b = small.d + at;
            const size_t n = c < 0 ? ACC_HEAD : 3 * ACC_PER_CP;
            if (hipMemcpyAsync(to_small ? b : a, to_small ? a : b, n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
            at += n;
        }
        return true;
    }
    int evaluate(const double *xp, int with_jac, double *cost) {
        const auto te = lm_now();
        if (!upload(xp)) return ECAL_ERR_HIP;
        if (int rc = ecal_solver_evaluate_dev(s, s->d_params, with_jac, s->d_accum, st)) return rc;
        const size_t n = with_jac ? na : 1;
        if (opt.allreduce && share.mode == 2 && with_jac) {
            if (!copy_shared_records(true)) return ECAL_ERR_HIP;
            if (opt.allreduce(opt.allreduce_user, small.d, ACC_HEAD + 3 * ACC_PER_CP * (size_t) (share.world - 1), st) != 0) return ECAL_ERR_HIP;
            if (!copy_shared_records(false)) return ECAL_ERR_HIP;
        } else if (opt.allreduce) {  // per-GPU partials summed over ranks (RCCL all-reduce supplied by the caller)
            // distributed segments: only the head (cost, intrinsics gradient and block) is shared between ranks
            if (opt.allreduce(opt.allreduce_user, s->d_accum, share.mode ? std::min(n, (size_t) ACC_HEAD) : n, st) != 0) return ECAL_ERR_HIP;
        }
        if (int rc = synchronize(hipMemcpyAsync(s->h_acc, s->d_accum, n * sizeof(double), hipMemcpyDeviceToHost, st))) return rc;
        *cost = s->h_acc[0], t_eval += lm_secs(te, lm_now());
        return ECAL_OK;
    }
    // sum v[0..n) over ranks in place, through the device buffer d and the pinned buffer h
    bool reduce_through(double *v, size_t n, double *d, double *h) {
        memcpy(h, v, n * sizeof(double));
        if (hipMemcpyAsync(d, h, n * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return false;
        if (opt.allreduce(opt.allreduce_user, d, n, st) != 0) return false;
        if (hipMemcpyAsync(h, d, n * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return false;
        if (hipStreamSynchronize(st) != hipSuccess) return false;
        memcpy(v, h, n * sizeof(double));
        return true;
    }
    bool reduce_small(double *v, size_t n) { return reduce_through(v, n, small.d, small.h); }
    // time shards: the ranks' parts of the solution summed into the whole (9 + 7 n_cp doubles, through the parameter buffers)
    bool gather(std::vector<double> &x) {
        x = share.gather_part(x, s->n_cp);
        return reduce_through(x.data(), np, s->d_params, s->h_x);
    }
    // one rank, a long spline: the parts of the host's linear solve and the threads for them
    void acquire_pool() {
        n_parts = arrow_parts_for(s->n_cp);
        if ((uint32_t) (7 * n_parts) > s->n_cp) n_parts = 1;
        if (n_parts <= 1) return;
        const auto tp = lm_now();
        const int workers = std::max(0, std::min(n_parts, host_usable_cpus()) - 1);   // (affinity ∩ cgroup quota ÷ the node's ranks — not hardware_concurrency())
        if (!s->host_pool || s->host_pool_workers != workers) {
            try {
                s->host_pool = std::shared_ptr<void>(new HostPool(workers), [](void *q) { delete static_cast<HostPool *>(q); });
                s->host_pool_workers = workers;
            } catch (...) {   // no threads to be had: the sequential routines
                s->host_pool.reset();
                s->host_pool_workers = -1, n_parts = 1;
            }
        }
        pool = static_cast<HostPool *>(s->host_pool.get());
        t_pool = lm_secs(tp, lm_now());
    }
    // the streamed evaluation's progress block (NeProgress) for the host's partition into n_parts groups; *ok: there is a stream to use
    int setup_stream(bool *ok) {
        *ok = !opt.allreduce && pool && n_parts > 1 && !share.mode && n_parts <= NE_MAX_GROUPS && !ctx->sw.solver_no_stream && s->n_chunks > 0;
        if (!*ok) return ECAL_OK;
        NeProgress &pg = s->prog;
        if (pg.n_groups == (uint32_t) n_parts) {
            // the kernel restores the groups' counters itself as it finishes each group — unless an earlier evaluation on this
            // solver stopped half way (an error, a stream that failed to deliver): a solve starts from the full counts whatever
            // the last one left behind (128 words; nothing of this solver is in flight here)
            ECAL_HIP_TRY(ctx, hipMemcpyAsync(s->d_left, pg.init, 2 * NE_MAX_GROUPS * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            return ECAL_OK;
        }
        // first solve with this partition: the groups' chunk counts, the buffers
        std::vector<uint32_t> part_first, part_num;
        arrow_partition_stream(s->n_cp, n_parts, part_first, part_num);
        std::vector<Chunk> ch(s->n_chunks);
        ECAL_HIP_TRY(ctx, hipMemcpy(ch.data(), s->d_chunks, ch.size() * sizeof(Chunk), hipMemcpyDeviceToHost));
        memset(&pg, 0, sizeof(pg));   // (n_groups = 0 until the last step below has succeeded: a failed set-up is redone at the next solve)
        pg.n_cp = s->n_cp;
        for (int g = 0; g < n_parts; g++) pg.cut[g] = part_first[g];
        pg.cut[n_parts] = s->n_cp;
        for (const Chunk &c : ch) {
            const uint32_t sg = s->cp_off[c.seg] + c.span;
            uint32_t g = 0;
            while (g + 1 < (uint32_t) n_parts && pg.cut[g + 1] <= sg) g++;
            pg.init[g]++;
        }
        for (int b = 0; b + 1 < n_parts; b++) pg.init[NE_MAX_GROUPS + b] = (pg.init[b] ? 1u : 0u) + (pg.init[b + 1] ? 1u : 0u);
        if (!s->h_flag) {
            ECAL_HIP_TRY(ctx, hipHostMalloc((void **) &s->h_flag, 2 * NE_MAX_GROUPS * sizeof(uint32_t), hipHostMallocDefault));
            memset(s->h_flag, 0, 2 * NE_MAX_GROUPS * sizeof(uint32_t));
        }
        if (!s->d_left) ECAL_HIP_TRY(ctx, hipMalloc((void **) &s->d_left, 2 * NE_MAX_GROUPS * sizeof(uint32_t)));
        if (!s->d_prog) ECAL_HIP_TRY(ctx, hipMalloc((void **) &s->d_prog, sizeof(NeProgress)));
        ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
        ECAL_HIP_TRY(ctx, hipMemcpy(s->d_left, pg.init, 2 * NE_MAX_GROUPS * sizeof(uint32_t), hipMemcpyHostToDevice));
        pg.left = s->d_left;
        ECAL_HIP_TRY(ctx, hipHostGetDevicePointer((void **) &pg.host_acc, s->h_acc, 0));
        ECAL_HIP_TRY(ctx, hipHostGetDevicePointer((void **) &pg.host_flag, s->h_flag, 0));
        NeProgress ready = pg;
        ready.n_groups = (uint32_t) n_parts;
        ECAL_HIP_TRY(ctx, hipMemcpy(s->d_prog, &ready, sizeof(ready), hipMemcpyHostToDevice));
        pg = ready;
        return ECAL_OK;
    }
    int evaluate_streamed(LmStreamJob &job) {
        const auto te = lm_now();
        const NeProgress &pg = s->prog;
        const int P = n_parts;
        double *const acc = s->h_acc;
        ArrowSystem &An = *job.An;
        if (!upload(job.x)) return ECAL_ERR_HIP;
        const uint32_t epoch = ++s->stream_epoch;
        // records that no chunk touches never arrive: they are zero
        for (int g = 0; g < P; g++) {
            if (!pg.init[g]) memset(acc + ACC_HEAD + ACC_PER_CP * (size_t) pg.cut[g], 0,
                                    ACC_PER_CP * (size_t) ((g + 1 < P ? pg.cut[g + 1] - 3 : pg.cut[g + 1]) - pg.cut[g]) * sizeof(double));
            if (g + 1 < P && !pg.init[NE_MAX_GROUPS + g]) memset(acc + ACC_HEAD + ACC_PER_CP * (size_t) (pg.cut[g + 1] - 3), 0, 3 * ACC_PER_CP * sizeof(double));
        }
        if (int rc = solver_evaluate_dev(s, s->d_params, 1, s->d_accum, st, s->d_prog, epoch)) return rc;
        if (hipMemcpyAsync(acc, s->d_accum, ACC_HEAD * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return ECAL_ERR_HIP;
        if (job.after_launch) (*job.after_launch)();
        unpack_alloc(s->n_cp, An);
        if (job.factor) arrow_parts_setup(An.nc, P, *job.ws, *job.parts, true);
        job.reduced_ok = false;
        const bool trace_ev = ctx->sw.solver_trace;
        tl_arrive.assign(P + 1, 0.0), tl_done.assign(P + 1, 0.0);
        // the host tasks (arrow_host.hpp: an interior per task as its records arrive, the separators behind them)
        const StreamedSource src{pg.init, pg.cut, s->h_flag, epoch, [&]() -> bool { return hipStreamQuery(st) != hipErrorNotReady; }};
        const bool delivered = arrow_streamed_tasks(pool, P, src, acc, An, job.factor, job.r_fact, job.scale, job.dd_next, opt.min_lm_diagonal,
                                                    opt.max_lm_diagonal, *job.ws, *job.parts, &job.reduced_ok, trace_ev ? tl_arrive.data() : nullptr,
                                                    trace_ev ? tl_done.data() : nullptr, te);
        tl_run = lm_secs(te, lm_now());
        if (int rc = synchronize()) return rc;
        const auto tt = lm_now();
        job.streamed = delivered;
        if (!delivered) {
            if (hipMemcpy(acc, s->d_accum, na * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return ECAL_ERR_HIP;
            unpack(acc, s->n_cp, An);
        } else {
            unpack_head(acc, An);
            for (int p = 0; p + 1 < P && !job.factor; p++) unpack_rows(acc, An, pg.cut[p + 1] - 3, pg.cut[p + 1]);
        }
        job.cost = acc[0];
        tl_sync = lm_secs(te, tt), t_tail += lm_secs(tt, lm_now()), t_eval += lm_secs(te, lm_now());
        return ECAL_OK;
    }
    // ecal_debug_solver_last_solve's words and the ECAL_TRACE=solver lines
    void report(const ecal_lm_summary &S, const LmCounters &K) const {
        const uint32_t words[7] = {(uint32_t) n_parts, s->stream_epoch - epoch_at_start, (uint32_t) K.n_prefactored, pool ? (uint32_t) pool->workers() : 0u,
                                   K.stream_ok ? 1u : 0u, (uint32_t) S.iterations, (uint32_t) (share.mode != 0) | (share.mode == 2 ? 2u : 0u)};
        memcpy(s->last_solve, words, sizeof(words));
        if (!ctx->sw.solver_trace) return;
        fprintf(stderr, "ecal_solver_solve: total %.4f s | evaluate %.4f | linear solve %.4f (%d parts) | unpack %.4f | pool %.4f | streamed evaluations: "
                        "%u, behind the kernel %.4f, %d of %d linear solves found their interiors factorised\n", S.seconds,
                t_eval, S.seconds_linear_solve, n_parts, K.t_unpack, t_pool, s->stream_epoch, t_tail, K.n_prefactored, S.iterations);
        fprintf(stderr, "  host items, ms over the solve: LM diagonal %.3f | factorise / finish %.3f | scaling + quadratic forms %.3f | plus %.3f | "
                        "verdict, norms, swap / unpack, gradient norm %.3f | of the finishes: corner %.3f, back-substitution %.3f\n", 1e3 * K.t_dd, 1e3 * K.t_fin,
                1e3 * K.t_quad, 1e3 * K.t_plus, 1e3 * K.t_book, 1e3 * K.t_fin_end, 1e3 * K.t_fin_back);
        if (tl_arrive.empty()) return;
        fprintf(stderr, "  last streamed evaluation, ms from its start: interiors arrived / factorised");
        for (size_t p = 0; p + 1 < tl_arrive.size(); p++) fprintf(stderr, " %.2f/%.2f", 1e3 * tl_arrive[p], 1e3 * tl_done[p]);
        fprintf(stderr, " | separators done %.2f | tasks joined %.2f | stream synchronised %.2f\n", 1e3 * tl_done.back(), 1e3 * tl_run, 1e3 * tl_sync);
    }
};
}  // namespace

extern "C" void ecal_lm_default_options(ecal_lm_options *o) {
    if (!o) return;
    o->max_num_iterations = 50;             // Ceres default, not overridden at EventCalibSpline.cpp:238-243
    o->function_tolerance = 1e-10;          // Sophus::Constants<double>::epsilon(), EventCalibSpline.cpp:240
    o->gradient_tolerance = 1e-10;          // :239
    o->parameter_tolerance = 1e-8;          // Ceres default
    o->initial_trust_region_radius = 1e4;   // Ceres defaults below
    o->max_trust_region_radius = 1e16;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->jacobi_scaling = 1;
    o->allreduce = nullptr;
    o->allreduce_user = nullptr;
    o->distributed = 0;
    o->rank = 0;
    o->world_size = 1;
}

extern "C" int ecal_solver_solve(ecal_solver *s, double *params, const ecal_lm_options *opt_in,
                                 ecal_lm_summary *sum) {
    const ecal_range range__(s ? s->ctx : nullptr, "ecal_solver_solve");
    if (!s || !params) return ECAL_ERR_INVALID;
    ecal_lm_options opt;
    if (opt_in) opt = *opt_in; else ecal_lm_default_options(&opt);
    RankShare share;
    int rc = solve_validate(s, opt, share);
    if (rc) return rc;
    ECAL_HIP_TRY(s->ctx, hipSetDevice(s->ctx->device));
    const auto t_begin = lm_now();
    SolveDevice backend{s, opt, share};
    if ((rc = backend.alloc())) return rc;
    backend.acquire_pool();
    LmCounters K;
    if ((rc = backend.setup_stream(&K.stream_ok))) return rc;
    const LmDevice dev{[&backend](const double *x, int with_jac, double *cost) { return backend.evaluate(x, with_jac, cost); },
                       [&backend](double *v, size_t n) { return backend.reduce_small(v, n); },
                       [&backend](LmStreamJob &job) { return backend.evaluate_streamed(job); }, s->h_acc};
    std::vector<double> x(params, params + backend.np);
    ecal_lm_summary S;
    if ((rc = lm_loop(dev, opt, share, s->n_cp, s->use_so3, backend.pool, backend.n_parts, x, S, K))) return rc;
    if (share.mode == 2 && !backend.gather(x)) return ECAL_ERR_HIP;
    S.seconds = lm_secs(t_begin, lm_now()), S.seconds_evaluate = backend.t_eval;
    backend.report(S, K);
    memcpy(params, x.data(), backend.np * sizeof(double));
    if (sum) *sum = S;
    return ECAL_OK;
}

// The time shards of one spline (ecal_lm_options.distributed == 2): cut_time[c] for c < world - 1 — rank r owns the residuals
// with cut_time[r - 1] <= t < cut_time[r] (rank 0 from the first knot, the last rank to the last).  The cuts sit on knots: the
// control points are cut into `world` interiors with 3-control-point separators, the partition of the host's own multi-core
// solve (arrow_partition); a residual left of the knot behind a separator touches no control point right of it and vice versa.
extern "C" int ecal_solver_time_shard_cuts(const double *knots, uint32_t n_cp, int world, double *cut_time) {
    if (!knots || !cut_time || world < 1 || (uint32_t) (7 * world) > n_cp) return ECAL_ERR_INVALID;
    std::vector<uint32_t> f, m;
    arrow_partition(n_cp, world, f, m);
    for (int c = 0; c + 1 < world; c++) cut_time[c] = knots[f[c] + m[c] + 3];   // spans up to (first separator CP + 2) stay left
    return ECAL_OK;
}

// closed form of PinholeCamera::inverseRadialDistortion (core/sensor/src/PinholeCamera.cpp:69-95)
extern "C" void ecal_inverse_radial_distortion(const double *k4, double *b5) {
    const double k1 = k4[0], k2 = k4[1], k3 = k4[2], k4v = k4[3];
    const double k1_2 = k1 * k1, k1_3 = k1_2 * k1, k1_4 = k1_3 * k1, k1_5 = k1_4 * k1;
    b5[0] = -k1;
    b5[1] = 3 * k1_2 - k2;
    b5[2] = -12 * k1_3 + 8 * k1 * k2 - k3;
    b5[3] = 55 * k1_4 - 55 * k1_2 * k2 + 5 * k2 * k2 + 10 * k1 * k3 - k4v;
    b5[4] = -273 * k1_5 + 364 * k1_3 * k2 - 78 * k1 * k2 * k2 - 78 * k1_2 * k3 + 12 * k2 * k3 + 12 * k1 * k4v;
}

// Test hook: one linear solve (S A S + D) y = -S g, delta = S y, for the normal equations `accum` (host, ecal_solver_normal_size
// doubles) and the column scaling `scale` (host, 6 n_cp + 9) by the host routines (sequential, partitioned, the streamed
// evaluation's partition); tests/test_gpu_solver.py requires them to agree.
// The host's linear solves alone (no GPU involved): the accumulation buffer of n_cp control points (ecal_solver_normal_size
// layout) -> the LM step.  mode 0: the sequential routine (solve_arrow); 2: the partitioned one (arrow_host_parts.hpp) with `parts`
// interiors on a few threads; 3: the same on the streamed evaluation's partition (interiors shrinking towards the end).
extern "C" int ecal_debug_arrow_solve_host(uint32_t n_cp, const double *accum, const double *scale, double radius, double min_diag,
                                           double max_diag, double *delta_out, int *fail_out, int mode, int parts_wanted) {
    const int rc = arrow_debug_solve_host(n_cp, accum, scale, radius, min_diag, max_diag, delta_out, fail_out, mode, parts_wanted);
    return rc == -1 ? ECAL_ERR_INVALID : (rc == -6 ? ECAL_ERR_RANGE : ECAL_OK);
}

// tests: how the last ecal_solver_solve on this solver ran — [0] interiors of the host's partition, [1] streamed evaluations,
// [2] linear solves that found their interiors factorised, [3] worker threads of the pool, [4] 1 = the streamed path was in force
// at the end, [5] iterations, [6] bit 0 distributed, bit 1 time-sharded
extern "C" int ecal_debug_solver_last_solve(const ecal_solver *s, uint32_t *out8) {
    if (!s || !out8) return ECAL_ERR_INVALID;
    memcpy(out8, s->last_solve, sizeof(s->last_solve));
    return ECAL_OK;
}

// tests / bench: the CPUs the solver's worker pool is sized for (affinity ∩ cgroup quota ÷ LOCAL_WORLD_SIZE; ECAL_HOST_THREADS
// overrides) and, in *node_quota, the figure before the division by the node's ranks.  No GPU involved.
extern "C" int ecal_debug_host_usable_cpus(int *node_quota) { return host_usable_cpus(node_quota); }

// tests (no GPU involved): the solve's worker pool — `rounds` runs of 1 .. 40 tasks on `workers` threads, with pauses long enough for
// the workers to go to sleep now and then, nudges from inside tasks (as the streamed evaluation's last interior does) and from the
// caller; every task of every run must have run exactly once, in a run of its own.  Returns the number of violations.
extern "C" int ecal_debug_host_pool_selftest(int workers, int rounds) { return host_pool_selftest(workers, rounds); }

// tests: the host solve's partitions (arrow_partition / arrow_partition_stream)
extern "C" int ecal_debug_arrow_partition(uint32_t n_cp, int parts, int stream, uint32_t *first_cp, uint32_t *num_cp) {
    if (!first_cp || !num_cp || parts < 1 || (uint32_t) (7 * parts) > n_cp) return ECAL_ERR_INVALID;
    std::vector<uint32_t> f, m;
    if (stream) arrow_partition_stream(n_cp, parts, f, m);
    else arrow_partition(n_cp, parts, f, m);
    memcpy(first_cp, f.data(), parts * sizeof(uint32_t));
    memcpy(num_cp, m.data(), parts * sizeof(uint32_t));
    return ECAL_OK;
}

extern "C" int ecal_debug_arrow_solve(ecal_solver *s, const double *accum, const double *scale, double radius, double min_diag,
                                      double max_diag, double *delta_out, int *fail_out, int mode) {
    if (!s || !accum || !scale || !delta_out || !fail_out || mode == 1) return ECAL_ERR_INVALID;   // (1 was the device form, round 3 - 5)
    return ecal_debug_arrow_solve_host(s->n_cp, accum, scale, radius, min_diag, max_diag, delta_out, fail_out, mode, 0);
}


// ------------------------------------------------------------------------------------------------
// Uncertainty of the intrinsics (include/ecal_uncertainty.h): one evaluation with Jacobian and the per-chunk score sums
// (ecal_uncertainty.hip) on the device, the covariance from the banded-arrow system on the host (arrow_covariance.hpp).
// Only the accumulation buffer, the chunk table and the chunk scores cross to the host.
// ------------------------------------------------------------------------------------------------
#include "../../include/ecal_uncertainty.h"
namespace {
#include "arrow_covariance.hpp"
}

extern "C" int ecal_solver_uncertainty(ecal_solver *s, const double *params, const ecal_uncertainty_options *opt_in,
                                       ecal_uncertainty_result *out) {
    if (!s || !params || !out) return ECAL_ERR_INVALID;
    ecal_ctx *ctx = s->ctx;
    ecal_uncertainty_options opt;
    if (opt_in) opt = *opt_in; else ecal_uncertainty_default_options(&opt);
    if (opt.cluster_spans < 1 || opt.reserved != 0) {
        ctx->last_error = "ecal_solver_uncertainty: cluster_spans at least 1, reserved 0";
        return ECAL_ERR_INVALID;
    }
    std::vector<double> accum(s->n_accum()), score((size_t) s->n_chunks * RES_NJ);
    std::vector<uint32_t> table(4 * (size_t) s->n_chunks);
    int rc = ecal_solver_evaluate(s, params, 1, accum.data());
    if (rc) return rc;
    rc = ecal_solver_chunk_scores(s, params, score.data(), nullptr);
    if (rc) return rc;
    rc = ecal_solver_chunk_table(s, table.data());
    if (rc) return rc;
    static_assert(sizeof(ScoreChunk) == 4 * sizeof(uint32_t), "the chunk table's rows");
    arrow_uncertainty(accum.data(), s->n_cp, s->n_res, reinterpret_cast<const ScoreChunk *>(table.data()), score.data(), s->n_chunks,
                      opt.cluster_spans, out);
    return ECAL_OK;
}
