// Exact-SDP optimality measure on the device (strategies 3 and -1 of cut_select_algo; replaces the per-candidate MOSEK call of
// cut_select_qp.py:586-598 and :675-685).  One lane solves one candidate entirely in registers, fp64, no LDS: the solver body is
// exact_sdp.h (formulation, stopping rule, degenerate rules).  A wave -- one workgroup: candidates need between 0 and a few dozen
// iterations, so the unit that waits for its slowest lane is kept small -- loops until all its lanes are done or at the cap.
//   exact_sdp_kernel<K>        the handle's candidates of size K at the current point: the gather is gather.h's, so q, max_elem and
//                              negSM are the bits the score kernels use; writes d_sdp = negSM + p*_lower max_elem and the gap
//   exact_sdp_batch_kernel<K>  the same body on explicit inputs [x | Q_slice]; returns the certificate
#include "common.h"
#include "exact_sdp.h"
#include "gather.h"

template <int K>
__device__ __forceinline__ void esdp_run(Esdp<K> &st, bool valid, const EsdpOut &o, unsigned long long *unconverged)
{
    if (!valid) st.done = true;
    else if (st.done) esdp_emit_trivial<K>(st, o);
    while (__any(!st.done))
        if (!st.done) esdp_iterate<K>(st, ESDP_ITER_CAP, o);
    if (valid && !st.converged) atomicAdd(unconverged, 1ull);      // (rare: a lane at the cap)
}

template <int K>
__global__ __launch_bounds__(64) void exact_sdp_kernel(const int32_t *set, const int32_t *orig, int64_t n, const double *vars, const double *Q,
                                                       int32_t nv, int64_t L, double *sdp_out, double *gap_out, unsigned long long *unconverged)
{
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool valid = c < n;
    const int64_t cc = valid ? c : n - 1;
    Esdp<K> st;
    EsdpOut o = {nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 1.0};
    {
        Cand<K> cd;
        gather_candidate<K>(cd, set, n, cc, vars, Q, nv, L, true);
        esdp_init<K>(st, cd.x, cd.q);
        const int32_t slot = orig[cc];
        o.value = sdp_out + slot;
        o.gap = gap_out + slot;
        o.add = cd.negSM;           // cut_select_qp.py:575
        o.scale = cd.max_elem;      // :595
    }
    esdp_run<K>(st, valid, o, unconverged);
}

template <int K>
__global__ __launch_bounds__(64) void exact_sdp_batch_kernel(int64_t count, const double *inputs, double *value, double *gap, double *lam, double *Y,
                                                             int32_t *iters, unsigned long long *unconverged)
{
    constexpr int M = K * (K + 1) / 2;
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool valid = c < count;
    const int64_t cc = valid ? c : count - 1;
    Esdp<K> st;
    {
        double x[K], q[M];
        const double *in = inputs + cc * (K + M);
#pragma unroll
        for (int i = 0; i < K; ++i) x[i] = in[i];
#pragma unroll
        for (int m = 0; m < M; ++m) q[m] = in[K + m];
        esdp_init<K>(st, x, q);
    }
    const EsdpOut o = {value + cc, gap + cc, lam ? lam + cc * K : nullptr, Y ? Y + cc * M : nullptr, iters ? iters + cc : nullptr, 0.0, 1.0};
    esdp_run<K>(st, valid, o, unconverged);
}

void free_sdp_ws(sdpcut_ctx *h)
{
    h->d_sdp.release();
    h->d_sdp_gap.release();
    h->scored &= ~(uint32_t)SDPCUT_SDP;
}

static int ensure_sdp_counter(sdpcut_ctx *h)
{
    if (!h->d_sdp_unconverged.get()) HIP_TRY(h, h->d_sdp_unconverged.reset(1));
    return 0;
}

// d_sdp / d_sdp_gap of every candidate of the handle's list at the current point: one launch per size class present
int launch_exact_sdp(sdpcut_ctx *h)
{
    int rc = ensure_sdp_counter(h);
    if (rc) return rc;
    if (!h->d_sdp.get()) {      // allocated by the first scoring of a list: lists that never ask for the exact measure pay nothing
        const size_t nn = (size_t)(h->N < 1 ? 1 : h->N);
        HIP_TRY(h, h->d_sdp.reset(nn));
        HIP_TRY(h, h->d_sdp_gap.reset(nn));
    }
    HIP_TRY(h, hipMemsetAsync(h->d_sdp_unconverged.get(), 0, sizeof(unsigned long long), h->stream));
    const double *vars = score_vars(h, SDPCUT_SDP), *Q = score_Q(h, SDPCUT_SDP);      // (the box tables at a node, common.h)
#define ESDP_LAUNCH(KK)                                                                                                            \
    if (h->bucket[KK].n > 0)                                                                                                         \
        hipLaunchKernelGGL((exact_sdp_kernel<KK>), dim3((unsigned)((h->bucket[KK].n + 63) / 64)), dim3(64), 0, h->stream, h->bucket[KK].d_set.get(), \
                           h->bucket[KK].d_orig.get(), h->bucket[KK].n, vars, Q, h->nb_vars, h->L, h->d_sdp.get(), h->d_sdp_gap.get(), h->d_sdp_unconverged.get())
    ESDP_LAUNCH(5);
    ESDP_LAUNCH(4);
    ESDP_LAUNCH(3);
    ESDP_LAUNCH(2);
#undef ESDP_LAUNCH
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int sdp_unconverged(sdpcut_ctx *h, int64_t *value)
{
    unsigned long long v = 0;
    if (h->d_sdp_unconverged.get()) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpyAsync(&v, h->d_sdp_unconverged.get(), sizeof(v), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, sdpcut_sync(h));
    }
    *value = (int64_t)v;
    return SDPCUT_OK;
}

extern "C" {

int sdpcut_get_sdp_scores(sdpcut_handle h, double *obj_exact, double *gap)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!(h->scored & SDPCUT_SDP)) return sdpcut_fail(h, SDPCUT_ESTATE, "exact optimality measure not scored");
    HIP_TRY(h, hipSetDevice(h->device));
    if (obj_exact) HIP_TRY(h, hipMemcpyAsync(obj_exact, h->d_sdp.get(), h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (gap) HIP_TRY(h, hipMemcpyAsync(gap, h->d_sdp_gap.get(), h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

int sdpcut_sdp_batch(sdpcut_handle h, int k, int64_t count, const double *inputs, double *value, double *gap, double *lam, double *Y,
                     int32_t *iters)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (k < 2 || k > SDPCUT_MAX_K) return sdpcut_fail(h, SDPCUT_EINVAL, "k must be 2..5");
    if (count < 0 || (count > 0 && (!inputs || !value || !gap))) return sdpcut_fail(h, SDPCUT_EINVAL, "bad sdp_batch arguments");
    if (count == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_sdp_counter(h);
    if (rc) return rc;
    // staging layout: inputs | value | gap | lam | Y | iters
    const size_t c = (size_t)count, m = (size_t)k * (k + 1) / 2, d = (size_t)k + m;
    rc = ensure_stage(h, c * 8 * (d + 2 + k + m) + c * 4);
    if (rc) return rc;
    double *d_in = (double *)h->d_stage.get(), *d_val = d_in + c * d, *d_gap = d_val + c, *d_lam = d_gap + c, *d_Y = d_lam + c * k;
    int32_t *d_it = (int32_t *)(d_Y + c * m);
    HIP_TRY(h, hipMemcpyAsync(d_in, inputs, c * d * 8, hipMemcpyHostToDevice, h->stream));
    unsigned long long *d_cnt = h->d_sdp_unconverged.get();      // SDPCUT_STAT_SDP_UNCONVERGED: of the last solve, scoring or batch
    HIP_TRY(h, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), h->stream));
    const unsigned grid = (unsigned)((count + 63) / 64);
#define ESDP_BATCH(KK)                                                                                                                   \
    hipLaunchKernelGGL((exact_sdp_batch_kernel<KK>), dim3(grid), dim3(64), 0, h->stream, count, d_in, d_val, d_gap, lam ? d_lam : nullptr, \
                       Y ? d_Y : nullptr, iters ? d_it : nullptr, d_cnt)
    switch (k) {
    case 2: ESDP_BATCH(2); break;
    case 3: ESDP_BATCH(3); break;
    case 4: ESDP_BATCH(4); break;
    default: ESDP_BATCH(5); break;
    }
#undef ESDP_BATCH
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(value, d_val, c * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(gap, d_gap, c * 8, hipMemcpyDeviceToHost, h->stream));
    if (lam) HIP_TRY(h, hipMemcpyAsync(lam, d_lam, c * k * 8, hipMemcpyDeviceToHost, h->stream));
    if (Y) HIP_TRY(h, hipMemcpyAsync(Y, d_Y, c * m * 8, hipMemcpyDeviceToHost, h->stream));
    if (iters) HIP_TRY(h, hipMemcpyAsync(iters, d_it, c * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

} // extern "C"
