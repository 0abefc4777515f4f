// SDPCUT_EFF (include/sdpcut.h): the efficacy of the eigen-cut a round would emit for every candidate of the list -- the Euclidean
// distance by which the row cuts off the LP point, the first criterion of a MIP solver's cut selector -- and its parallelism to the LP
// objective.  One lane per candidate in caller order, all size classes in one launch.  The row is cut_row_one's (rows_dev.h) with the
// lambda_min the handle holds: the score is the score of the row sdpcut_cut_rows returns, not of another vector of the eigenspace.
// efficacy.py is the numpy twin; the operation order below is the definition ("Efficacy ranking").
#include <cstring>
#include <cmath>

#include "common.h"
#include "rows_dev.h"

// ||coef||_2 and <coef, obj> of the row of one candidate; sums in column order m = 0 .. M-1, no contraction, IEEE square root
template <int K>
__device__ __forceinline__ void eff_row_one(const int32_t *s5, const double *vars, int32_t nv, int64_t L, const double *lam_known,
                                            const double *lpobj, double *nrm, double *dot)
{
    constexpr int M = K * (K + 3) / 2;
    double coef[M];
    int64_t cols[M];
    double lam, rhs;
    cut_row_one<K>(s5, vars, nv, L, &lam, coef, &rhs, cols, lam_known);
    {
#pragma clang fp contract(off)
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) s = s + coef[m] * coef[m];
        *nrm = sqrt(s);
        double d = 0.0;
        if (lpobj) {
#pragma unroll
            for (int m = 0; m < M; ++m) d = d + coef[m] * lpobj[cols[m]];
        }
        *dot = d;
    }
}

// Candidate i at one LP point: lanes that are not violated leave before the eigenvector; a wave without a violated lane branches
// over the whole row computation (the `if (viol)` below is a branch on EXEC == 0).  The body of both kernels below.
__device__ __forceinline__ void efficacy_one(int64_t i, const int32_t *set5, const int32_t *ks, const double *vars, int32_t nv, int64_t L,
                                             const double *eig, const double *lpobj, double obj_norm, double w, double *eff, double *objpar,
                                             double *escore)
{
    const double lam = eig[i];
    const double neg = -lam;
    // min(-lam, +0.0) with +0 for lam = 0 (the twin's bits).  Chosen among bit patterns: written as a floating-point select it
    // compiles to v_min_f64, which returns -0.0 for lam = 0.
    double e = __longlong_as_double(lam > 0.0 ? __double_as_longlong(neg) : 0ll);
    double p = 0.0, sc = e;
    if (lam < SDPCUT_NEG_EIGVAL) {
        const int k = ks[i];
        const int32_t *s5 = set5 + i * 5;
        double nrm = 0.0, dot = 0.0;
        CALL_FOR_SET_SIZE(k, eff_row_one, s5, vars, nv, L, eig + i, lpobj, &nrm, &dot);
        if (nrm > 0.0) {
#pragma clang fp contract(off)
            e = neg / nrm;
            if (lpobj) p = fabs(dot) / (nrm * obj_norm);
            sc = e + w * p;
        } else {
            e = 0.0;      // (a row of zeros cuts nothing off; never seen: a unit eigenvector of a negative eigenvalue has v_i != 0 for an i >= 1)
            sc = 0.0;
        }
    }
    eff[i] = e;
    objpar[i] = p;
    escore[i] = sc;
}

// A workgroup is one wave.
__global__ __launch_bounds__(64) void efficacy_kernel(int64_t n, const int32_t *set5, const int32_t *ks, const double *vars, int32_t nv,
                                                      int64_t L, const double *eig, const double *lpobj, double obj_norm, double w,
                                                      double *eff, double *objpar, double *escore)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    efficacy_one(i, set5, ks, vars, nv, L, eig, lpobj, obj_norm, w, eff, objpar, escore);
}

// The same with a point axis (sdpcut_efficacy_points, the batched strategy-6 round; points.hip): row blockIdx.y of the grid is LP
// point blockIdx.y -- its row of the point table (stride vars_ld), of the lambda_min array and of the three outputs (stride score_ld).
__global__ __launch_bounds__(64) void efficacy_points_kernel(int64_t n, const int32_t *set5, const int32_t *ks, const double *vars,
                                                             int64_t vars_ld, int32_t nv, int64_t L, const double *eig, int64_t score_ld,
                                                             const double *lpobj, double obj_norm, double w, double *eff, double *objpar,
                                                             double *escore)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = blockIdx.y;
    efficacy_one(i, set5, ks, vars + p * vars_ld, nv, L, eig + p * score_ld, lpobj, obj_norm, w, eff + p * score_ld, objpar + p * score_ld,
                 escore + p * score_ld);
}

void free_eff_ws(sdpcut_ctx *h)
{
    h->d_eff.release();      // one allocation: eff | objpar | escore
    h->d_objpar = h->d_escore = nullptr;
    h->scored &= ~(uint32_t)SDPCUT_EFF;
}

void free_lpobj(sdpcut_ctx *h)
{
    h->d_lpobj.release();
    h->d_lpobj_dense.release();
    h->lpobj_dense_ok = false;
    h->lpobj_norm = 0.0;
    h->scored &= ~(uint32_t)SDPCUT_EFF;
}

// d_eff / d_objpar / d_escore of every candidate at the current point; SDPCUT_EIG has been scored (sdpcut_score sees to it)
int launch_efficacy(sdpcut_ctx *h)
{
    if (!h->d_eff.get()) {      // allocated by the first scoring of a list, as d_sdp is
        const size_t nn = (size_t)(h->N < 1 ? 1 : h->N);
        HIP_TRY(h, h->d_eff.reset(3 * nn));
        h->d_objpar = h->d_eff.get() + nn;
        h->d_escore = h->d_objpar + nn;
    }
    if (h->N == 0) return 0;
    const unsigned grid = (unsigned)((h->N + 63) / 64);
    // the ORIGINAL point: like lambda_min and the rows this measure knows no node box
    hipLaunchKernelGGL(efficacy_kernel, dim3(grid), dim3(64), 0, h->stream, h->N, h->d_set_orig.get(), h->d_k.get(), score_vars(h, SDPCUT_EFF), h->nb_vars,
                       h->L, h->d_eig.get(), (const double *)h->d_lpobj.get(), h->lpobj_norm, h->eff_w, h->d_eff.get(), h->d_objpar, h->d_escore);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// eff / objpar / escore of every candidate at n_points points: rows of d_pts (stride pts_stride), lambda_min in rows of d_eig, the
// outputs in rows of the three arrays (all with stride score_stride); objective and weight are the handle's
int launch_efficacy_points(sdpcut_ctx *h, int n_points, const double *d_pts, int64_t pts_stride, const double *d_eig, int64_t score_stride,
                           double *d_eff, double *d_objpar, double *d_escore)
{
    if (h->N == 0 || n_points <= 0) return 0;
    const unsigned grid = (unsigned)((h->N + 63) / 64);
    hipLaunchKernelGGL(efficacy_points_kernel, dim3(grid, (unsigned)n_points), dim3(64), 0, h->stream, h->N, h->d_set_orig.get(), h->d_k.get(), d_pts, pts_stride,
                       h->nb_vars, h->L, d_eig, score_stride, (const double *)h->d_lpobj.get(), h->lpobj_norm, h->eff_w, d_eff, d_objpar, d_escore);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

extern "C" {

int sdpcut_set_objective(sdpcut_handle h, int64_t n_cols, const double *obj)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (h->nb_vars == 0) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!obj) {
        HIP_TRY(h, sdpcut_sync(h));
        free_lpobj(h);
        return SDPCUT_OK;
    }
    const int64_t len = h->L + h->nb_vars;
    if (n_cols != len) return sdpcut_fail(h, SDPCUT_EINVAL, "set_objective: n_cols must be n(n+1)/2 + n, the length of vars_values");
    // ||obj||_2 once, here: squares summed in index order, no contraction, IEEE square root (efficacy.py: objective_norm)
    double s = 0.0;
    {
#pragma clang fp contract(off)
        for (int64_t i = 0; i < len; ++i) {
            if (!std::isfinite(obj[i])) return sdpcut_fail(h, SDPCUT_EINVAL, "set_objective: a non-finite entry");
            s = s + obj[i] * obj[i];
        }
    }
    const double nrm = std::sqrt(s);
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return sdpcut_fail(h, SDPCUT_EINVAL, "set_objective: the vector is all zero (or its norm overflows)");
    HIP_TRY(h, sdpcut_sync(h));
    if (!h->d_lpobj.get()) HIP_TRY(h, h->d_lpobj.reset((size_t)len));
    h->lpobj_dense_ok = false;      // (sdpcut_node_eval_points builds its dense table of the new vector when it is first called)
    HIP_TRY(h, hipMemcpy(h->d_lpobj.get(), obj, (size_t)len * sizeof(double), hipMemcpyHostToDevice));
    h->lpobj_norm = nrm;
    h->scored &= ~(uint32_t)SDPCUT_EFF;
    return SDPCUT_OK;
}

int sdpcut_set_efficacy_weight(sdpcut_handle h, double w)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!std::isfinite(w) || w < 0.0) return sdpcut_fail(h, SDPCUT_EINVAL, "set_efficacy_weight: w must be finite and >= 0");
    h->eff_w = w;
    h->scored &= ~(uint32_t)SDPCUT_EFF;
    return SDPCUT_OK;
}

int sdpcut_get_efficacy(sdpcut_handle h, double *eff, double *objpar, double *escore)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!h->have_point || !(h->scored & SDPCUT_EFF)) return sdpcut_fail(h, SDPCUT_ESTATE, "efficacy not scored at the current point");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)h->N * sizeof(double);
    if (eff) HIP_TRY(h, hipMemcpyAsync(eff, h->d_eff.get(), bytes, hipMemcpyDeviceToHost, h->stream));
    if (objpar) HIP_TRY(h, hipMemcpyAsync(objpar, h->d_objpar, bytes, hipMemcpyDeviceToHost, h->stream));
    if (escore) HIP_TRY(h, hipMemcpyAsync(escore, h->d_escore, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

} // extern "C"
