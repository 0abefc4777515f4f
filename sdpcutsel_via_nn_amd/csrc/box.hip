// Node boxes (include/sdpcut.h: sdpcut_set_box): the instance tables re-expressed in the variables x' = (x - l) / d of a node's box
// l <= x <= u, d = u - l, in which the node's small SDP is the unit-box problem the networks were trained on.  The map is
// elementwise on the tables, not per candidate: Q' once per box, the transformed point once per LP point; the scoring kernels
// run on those tables as they are (gather.h recomputes max_elem and Q_slice from whatever table it is handed).
//   box_q_kernel       Q'_ij = Q_ij (d_i d_j)
//   box_point_kernel   X'_ij = (((X_ij - l_i x_j) - l_j x_i) + l_i l_j) / (d_i d_j),  x'_i = (x_i - l_i) / d_i
//   box_points_kernel  both tables at the P points of a boxed batch (points.hip), every point inside a box of its own
// fp64 in exactly this order, no contraction: on the unit box every entry is the original's bits.  Each formula is written once
// (box_q_entry, box_X_entry, box_x_entry) and every kernel calls it.
#include <cmath>

#include "common.h"

// (i, j), i <= j, of packed position p (row-major upper triangle: row i starts at i n - i (i - 1) / 2, cut_select_qp.py:531) without
// a walk over the rows: the root of the quadratic, then one step down and one up (the square root is off by less than one row:
// (2 n + 1)^2 and 8 p are exact in fp64 for n <= 40000)
__device__ __forceinline__ void box_unpack(int64_t p, int32_t n, int32_t &i, int32_t &j)
{
    const double b = 2.0 * (double)n + 1.0;
    int64_t r = (int64_t)floor((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
    r = r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
    if (r * n - r * (r - 1) / 2 > p) --r;
    if (r + 1 < n && (r + 1) * n - (r + 1) * r / 2 <= p) ++r;
    i = (int32_t)r;
    j = (int32_t)(r + (p - (r * n - r * (r - 1) / 2)));
}

// the three formulas (their callers inline them: the pragma travels with the operations)
__device__ __forceinline__ double box_q_entry(double q, double di, double dj)
{
#pragma clang fp contract(off)
    return q * (di * dj);
}

__device__ __forceinline__ double box_X_entry(double X, double xi, double xj, double li, double lj, double di, double dj)
{
#pragma clang fp contract(off)
    return (((X - li * xj) - lj * xi) + li * lj) / (di * dj);
}

__device__ __forceinline__ double box_x_entry(double x, double l, double d)
{
#pragma clang fp contract(off)
    return (x - l) / d;
}

__global__ __launch_bounds__(256) void box_q_kernel(const double *Q, const double *ld, int32_t n, int64_t L, double *Qb)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    int32_t i, j;
    box_unpack(p, n, i, j);
    Qb[p] = box_q_entry(Q[p], ld[n + i], ld[n + j]);
}

__global__ __launch_bounds__(256) void box_point_kernel(const double *vars, const double *ld, int32_t n, int64_t L, double *vb)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= L + n) return;
    if (p >= L) {
        const int64_t i = p - L;
        vb[p] = box_x_entry(vars[p], ld[i], ld[n + i]);
        return;
    }
    int32_t i, j;
    box_unpack(p, n, i, j);
    vb[p] = box_X_entry(vars[p], vars[L + i], vars[L + j], ld[i], ld[j], ld[n + i], ld[n + j]);
}

// The tables of a boxed batch: workgroup row y = point y.  Q'_y [L] (row y of Qb) and vars'_y [L + n] (row y of vb) from the shared
// Q, point y of the device point table (rows of pts_stride doubles) and row y of the [P][2 n] (l | d) table.  One box_unpack per
// thread serves both tables; the entries are the ones box_q_kernel / box_point_kernel write for that box and that point.
__global__ __launch_bounds__(256) void box_points_kernel(const double *Q, const double *pts, int64_t pts_stride, const double *ld, int32_t n,
                                                         int64_t L, double *Qb, double *vb)
{
    const int64_t y = (int64_t)blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= L + n) return;
    const double *vars = pts + y * pts_stride;
    ld += y * 2 * (int64_t)n;
    vb += y * (L + n);
    if (p >= L) {
        const int64_t i = p - L;
        vb[p] = box_x_entry(vars[p], ld[i], ld[n + i]);
        return;
    }
    int32_t i, j;
    box_unpack(p, n, i, j);
    const double di = ld[n + i], dj = ld[n + j];
    if (Qb) Qb[y * L + p] = box_q_entry(Q[p], di, dj);      // (uniform; NULL: a caller that reads the point tables only -- the triangle batch)
    vb[p] = box_X_entry(vars[p], vars[L + i], vars[L + j], ld[i], ld[j], di, dj);
}

int launch_box_points(sdpcut_ctx *h, int n_points, const double *d_pts, int64_t pts_stride, const double *d_ld, double *d_Qb, double *d_vb)
{
    const int64_t m = h->L + h->nb_vars;
    hipLaunchKernelGGL(box_points_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)n_points), dim3(256), 0, h->stream, (const double *)h->d_Q.get(),
                       d_pts, pts_stride, d_ld, h->nb_vars, h->L, d_Qb, d_vb);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int box_after_point(sdpcut_ctx *h)
{
    if (!h->box_set) return 0;
    const int64_t m = h->L + h->nb_vars;
    hipLaunchKernelGGL(box_point_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->d_vars.get(),
                       (const double *)h->d_box_ld.get(), h->nb_vars, h->L, h->d_vars_box.get());
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// the rule of a box (include/sdpcut.h: sdpcut_set_box); point >= 0: the box of that point of a batch
int box_check(sdpcut_ctx *h, const char *what, int point, const double *lb, const double *ub)
{
    for (int32_t i = 0; i < h->nb_vars; ++i)      // (written so that a NaN fails)
        if (!(lb[i] >= 0.0 && ub[i] <= 1.0 && ub[i] - lb[i] >= SDPCUT_BOX_MIN_WIDTH))
            return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": " + (point >= 0 ? "point " + std::to_string(point) + ", " : std::string()) +
                                                 "variable " + std::to_string(i) + ": a box needs 0 <= lb, ub <= 1 and ub - lb >= "
                                                 "SDPCUT_BOX_MIN_WIDTH (2^-10)");
    return 0;
}

void box_clear(sdpcut_ctx *h)
{
    h->d_box_ld.release(); h->d_Q_box.release(); h->d_vars_box.release();
    h->box_set = false;
    h->box_lb.clear(); h->box_ub.clear();
}

extern "C" {

int sdpcut_set_box(sdpcut_handle h, const double *lb, const double *ub)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!h->d_Q.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    if ((lb == nullptr) != (ub == nullptr)) return sdpcut_fail(h, SDPCUT_EINVAL, "set_box: lb and ub must both be given or both be NULL");
    const int32_t n = h->nb_vars;
    if (lb) {
        if (h->exact_head) return sdpcut_fail(h, SDPCUT_ESTATE, "set_box: SDPCUT_OPT_EXACT_HEAD is on (reference-exact heads have no node box)");
        const int rc = box_check(h, "set_box", -1, lb, ub);
        if (rc) return rc;
    } else if (!h->box_set) {
        return SDPCUT_OK;      // nothing to clear: the scores stand
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (lb) {      // the tables first: a failed allocation leaves box, scores and tables as they were
        if (!h->d_box_ld.get()) HIP_TRY(h, h->d_box_ld.reset((size_t)2 * n));
        if (!h->d_Q_box.get()) HIP_TRY(h, h->d_Q_box.reset((size_t)h->L));
        if (!h->d_vars_box.get()) HIP_TRY(h, h->d_vars_box.reset((size_t)(h->L + n)));
    }
    HIP_TRY(h, sdpcut_sync(h));      // (the launches of an earlier scoring read the tables rewritten below)
    h->scored &= ~(uint32_t)(SDPCUT_NN | SDPCUT_SDP);      // the measures of the old box; lambda_min knows no box
    h->obj_partial = false;
    h->last_total = -1;
    h->box_set = false;      // (until every table below is in place)
    h->box_lb.clear(); h->box_ub.clear();
    if (!lb) return SDPCUT_OK;
    std::vector<double> ld((size_t)2 * n);
    for (int32_t i = 0; i < n; ++i) { ld[i] = lb[i]; ld[(size_t)n + i] = ub[i] - lb[i]; }
    HIP_TRY(h, hipMemcpy(h->d_box_ld.get(), ld.data(), ld.size() * sizeof(double), hipMemcpyHostToDevice));
    h->box_lb.assign(lb, lb + n);
    h->box_ub.assign(ub, ub + n);
    hipLaunchKernelGGL(box_q_kernel, dim3((unsigned)((h->L + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->d_Q.get(),
                       (const double *)h->d_box_ld.get(), n, h->L, h->d_Q_box.get());
    HIP_TRY(h, hipGetLastError());
    h->box_set = true;
    return h->have_point ? box_after_point(h) : SDPCUT_OK;
}

int sdpcut_get_box(sdpcut_handle h, double *lb, double *ub, int *is_set)
{
    if (!h) return SDPCUT_EINVAL;
    if (!h->d_Q.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    for (int32_t i = 0; i < h->nb_vars; ++i) {
        if (lb) lb[i] = h->box_set ? h->box_lb[i] : 0.0;
        if (ub) ub[i] = h->box_set ? h->box_ub[i] : 1.0;
    }
    if (is_set) *is_set = h->box_set ? 1 : 0;
    return SDPCUT_OK;
}

int sdpcut_get_box_tables(sdpcut_handle h, double *Q_box, double *vars_box)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!h->box_set) return sdpcut_fail(h, SDPCUT_ESTATE, "get_box_tables: no node box is set");
    if (vars_box && !h->have_point) return sdpcut_fail(h, SDPCUT_ESTATE, "get_box_tables: set_point first");
    HIP_TRY(h, hipSetDevice(h->device));
    if (Q_box) HIP_TRY(h, hipMemcpyAsync(Q_box, h->d_Q_box.get(), (size_t)h->L * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (vars_box)
        HIP_TRY(h, hipMemcpyAsync(vars_box, h->d_vars_box.get(), (size_t)(h->L + h->nb_vars) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

} // extern "C"
