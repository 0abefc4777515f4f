// Device pieces shared by the kernels that turn head entries into eigen-cut rows (rows.hip: cut_rows_kernel, round_rows_kernel,
// round_csr_kernel, round_csr_points_kernel; multirows.hip: multi_csr_kernel, cut_rows_all_kernel): the gather of a candidate with
// its LP columns, the row of an eigenvector, the dispatch over the candidate size, and the two protocols of the ordered CSR
// assembly -- the look-back over the workgroups in front and the completion word for the polling host.  Each exists once, here.
// Everything is forced inline: the kernels are compiled as if the text stood in them.
#pragma once
#include "common.h"
#include "gather.h"

// LDS traffic private to one wave needs no workgroup barrier (see score_mfma.hip)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// fn<K>(arguments) for the candidate size k = K in 2 .. 5; anything else counts as 5.  A macro, so that the switch stands in the
// kernel as it always did: behind a dispatching function (a wrapper, a generic lambda) the row kernels of rows.hip keep 48 more
// bytes per lane in scratch.
#define CALL_FOR_SET_SIZE(k, fn, ...)      \
    switch (k) {                           \
    case 2: fn<2>(__VA_ARGS__); break;     \
    case 3: fn<3>(__VA_ARGS__); break;     \
    case 4: fn<4>(__VA_ARGS__); break;     \
    default: fn<5>(__VA_ARGS__); break;    \
    }

// x, X of the candidate with index set s5 at the LP point `vars` and the LP columns they come from (cut_select_qp.py:529-531,
// :748): cols[0 .. K) = L + s, cols[K ..) the packed upper-triangle positions, row-major.  (gather.h: gather_candidate is the
// form without the columns.)
template <int K>
__device__ __forceinline__ void gather_lifted(const int32_t *s5, const double *vars, int32_t nv, int64_t L, double (&x)[K],
                                              double (&X)[K * (K + 1) / 2], int64_t *cols)
{
    int32_t s[K];
#pragma unroll
    for (int a = 0; a < K; ++a) {
        s[a] = s5[a];
        x[a] = vars[L + s[a]];
        cols[a] = L + s[a];
    }
    int m = 0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
        const int32_t rowbase = nv * s[a] - (s[a] * (s[a] + 1)) / 2;
#pragma unroll
        for (int b = a; b < K; ++b) {
            X[m] = vars[rowbase + s[b]];
            cols[K + m] = rowbase + s[b];
            ++m;
        }
    }
}

// The cut of an eigenvector ev[0 .. K] of the lifted matrix (cut_select_qp.py:744-750): components of magnitude <= 1e-15 count
// as zero; coefficients v_i v_j on the x columns (i = 0) and the diagonal, 2 v_i v_j off it, in column order; rhs = -v_0^2.
// No contraction: the products round as the reference's do.
template <int K>
__device__ __forceinline__ void eigcut_row(const double *ev_in, double *coef, double *rhs)
{
    constexpr int D = K + 1;
    double ev[D];
#pragma unroll
    for (int i = 0; i < D; ++i) ev[i] = (fabs(ev_in[i]) <= -SDPCUT_NEG_EIGVAL) ? 0.0 : ev_in[i];  // :744
    {
#pragma clang fp contract(off)
        int m = 0;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = (i > 1 ? i : 1); j < D; ++j) {     // :745-746
                coef[m++] = (i != j) ? ev[i] * ev[j] * 2 : ev[i] * ev[j];
            }
        *rhs = -ev[0] * ev[0];
    }
}

// The eigen-cut row of ONE candidate (cut_select_qp.py:737-750), one lane per cut: shared by the row kernels of rows.hip and the
// efficacy measure (efficacy.hip), which scores exactly the row a round emits.
template <int K>
__device__ __forceinline__ void cut_row_one(const int32_t *s5, const double *vars, int32_t nv, int64_t L,
                                            double *lam_out, double *coef, double *rhs, int64_t *cols, const double *lam_known = nullptr)
{
    constexpr int M = K * (K + 1) / 2;
    constexpr int D = K + 1;
    double x[K], X[M];
    gather_lifted<K>(s5, vars, nv, L, x, X, cols);
    double a[D][D];
    fill_lifted<K>(a, x, X);
    double lam = 0.0;
    double ev[D];
    bool have = false;
#ifndef SDPCUT_ROWS_INVERSE_ITERATION
#define SDPCUT_ROWS_INVERSE_ITERATION 1
#endif
    if (SDPCUT_ROWS_INVERSE_ITERATION && (lam_known || SDPCUT_LMIN)) {
        // the scoring pass has computed lambda_min of this candidate (the value the selection ranked by): its eigenvector by
        // inverse iteration (jacobi.h: ~700 instead of ~6700 instructions of a wave that has its SIMD to itself).  (r4) A round
        // that ranked without eigenvalues (optimality; explicit sdpcut_cut_rows on an unscored list) computes lambda_min here
        // with the solver the scoring kernels use (lmin.h) instead of running Jacobi with vectors for the whole spectrum.
        bool ok = true;
        if (lam_known) {
            lam = *lam_known;
        } else {
            double b[D][D];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) b[i][j] = a[i][j];
            lam = lmin_laguerre<D>(b, ok);
        }
        have = ok && min_eigvec_known<D>(a, lam, ev) <= 1e-12;
#ifdef SDPCUT_ABL_NOFALLBACK      // timing experiment (tools/build_ablation.sh, ABL_SRC=rows): wrong on multiple eigenvalues
        have = true;
#endif
    }
    if (!have) {      // no lambda_min at hand (optimality rounds, explicit sdpcut_cut_rows) -- or, never observed, a residual too large
        double v[D][D];
        jacobi_eig<D, true>(a, v);
        // eigenvector of the smallest eigenvalue (first minimum, like LAPACK's ascending order)
        lam = a[0][0];
#pragma unroll
        for (int i = 0; i < D; ++i) ev[i] = v[i][0];
#pragma unroll
        for (int j = 1; j < D; ++j) {
            const bool less = a[j][j] < lam;
            lam = less ? a[j][j] : lam;
#pragma unroll
            for (int i = 0; i < D; ++i) ev[i] = less ? v[i][j] : ev[i];
        }
    }
    eigcut_row<K>(ev, coef, rhs);
    *lam_out = lam;
}

// ------------------------------------------------------------------------------------------
// The ordered CSR assembly.  A workgroup is ONE wave (64 lanes, at most one head entry each).  A row's place in the block is the
// number of rows / non-zeros in front of it in head order: inside the workgroup a wave scan (the kernel's), across workgroups
// this look-back over the aggregates the workgroups in front have published.  Word = round serial (32) | rows (16) | non-zeros
// (16): the serial makes the word of an earlier round invisible, so nothing is ever zeroed between rounds.  A workgroup only
// waits for workgroups with a LOWER index, which the dispatcher started before it: the wait cannot deadlock whatever else runs
// on the device.  It is bounded all the same (a device shared with a kernel that holds the others back for long): after
// CSR_SPIN_LIMIT polls of one word the lane gives up.
#define CSR_SPIN_LIMIT (1 << 22)
// what a workgroup can publish: 64 entries with SDPCUT_MULTI_MAX_PER_SET rows of SDPCUT_ROW_LD non-zeros each at the most
static_assert(64 * SDPCUT_MULTI_MAX_PER_SET <= 0xffff, "rows of a workgroup must fit 16 bits");
static_assert(64 * SDPCUT_MULTI_MAX_PER_SET * SDPCUT_ROW_LD <= 0xffff, "non-zeros of a workgroup must fit 16 bits");

// Publishes (wg_rows, wg_nnz) of workgroup blockIdx.x under `tag` in agg[blockIdx.x] and sums the aggregates of the workgroups
// 0 .. blockIdx.x - 1 into pre_rows / pre_nnz (the same values in every lane).  -> non-zero in every lane if some lane gave
// up: the sums are then wrong, the caller marks the block void (header word 10) and the host launches the assembly once more
// (round.hip: csr_assemble_wait).
// inject (SDPCUT_OPT_INJECT_GIVEUP, uniform over the launch; 0 outside tests): every lane with a word to wait for gives up before its
// first poll, whether or not the word has arrived -- what an expired limit looks like, without the wait.
__device__ __forceinline__ int csr_lookback(uint64_t *agg, uint32_t tag, int wg_rows, int wg_nnz, int64_t &pre_rows, int64_t &pre_nnz,
                                            int inject)
{
    const int lane = threadIdx.x;
    if (lane == 0)
        __hip_atomic_store(&agg[blockIdx.x], ((uint64_t)tag << 32) | ((uint64_t)wg_rows << 16) | (uint64_t)wg_nnz, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    pre_rows = 0;
    pre_nnz = 0;
    int gave_up = (inject && lane < (int)blockIdx.x) ? 1 : 0;
    for (int b = lane; b < (int)blockIdx.x && !gave_up; b += 64) {
        uint64_t w = __hip_atomic_load(&agg[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t it = 0;
        while ((uint32_t)(w >> 32) != tag) {
            __builtin_amdgcn_s_sleep(2);
            if (++it > CSR_SPIN_LIMIT) { gave_up = 1; break; }
            w = __hip_atomic_load(&agg[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!gave_up) {
            pre_rows += (int64_t)((w >> 16) & 0xffffull);
            pre_nnz += (int64_t)(w & 0xffffull);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        pre_rows += __shfl_xor(pre_rows, off);
        pre_nnz += __shfl_xor(pre_nnz, off);
        gave_up |= __shfl_xor(gave_up, off);
    }
    return gave_up;
}

// Completion word for the polling host (round.hip: wait_round_done), called by every workgroup of the launch after its last
// store: each makes its stores to the host block visible system-wide, then takes a ticket; the last one leaves the ticket at
// zero for the next launch and publishes the round's serial number in `word` (header word 7 of the pinned block).
__device__ __forceinline__ void publish_round_done(uint32_t *ticket, int64_t *word, int64_t serial)
{
    __threadfence_system();
    if (threadIdx.x == 0) {
        const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == gridDim.x - 1) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence_system();
            __hip_atomic_store(word, serial, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
