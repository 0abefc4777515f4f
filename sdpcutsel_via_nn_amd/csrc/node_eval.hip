// Node evaluation (include/sdpcut.h: sdpcut_node_eval_points): at P LP points in one launch with one host wait, read-only -- the
// projection of x onto the point's box, the true objective f there, a Gauss-Seidel coordinate descent inside the box and a branching
// variable with its value.  The rule is DESIGN.md section 5 "Node evaluation"; nodeeval.py is the numpy twin, equal bit for bit.
//   node_eval_table_kernel   the dense symmetric table A[n][n] of the handle's LP objective (a_ij in both triangles), built once per
//                            objective in front of the first evaluation that follows a sdpcut_set_objective, kept on the handle
//                            and freed with the objective (efficacy.hip: free_lpobj)
//   node_eval_kernel         one wave (a workgroup of 64 lanes) per point; x lives in LDS, the table is read from global memory
// The orders of the sums -- every one is reproduced by the twin, nothing is contracted:
//   lane sum    a vector v[0 .. n): lane l adds v[l], v[l + 64], ... in ascending order to +0.0, then six exchange steps
//               p = p + p(lane ^ off), off = 32, 16, .. 1 (every lane ends with the same bits: the addition commutes)
//   f(x)        U_i = sum over j = i .. n-1 ascending of A[j][i] x_j (one lane per i: the lanes read a ROW of the table side by side);
//               f = lane sum of (c_i + U_i) x_i
//   s_i         c_i + lane sum of (j == i ? 0 : A[i][j] x_j)
//   rule 1      g_i = sum over j = 0 .. n-1 ascending of |A[j][i]| |X_ij - x_i x_j| (one lane per i)
// The coordinate loop is sequential: a coordinate's move changes the s of the next one.  Every step is one row read, six exchange
// steps and a handful of scalar operations that wait for each other -- latency, not throughput; the point axis is the parallelism.
// There is no grid barrier, no wait on another workgroup and no device-coherent hand-over: the results are plain stores into the
// pinned block, read by the host after the one stream wait.
#include <cmath>
#include <cstring>

#include "common.h"

#define NODE_EVAL_MAX_N 1024
#define NODE_EVAL_HDR_BYTES 64      /* doubles 0 f_point, 1 f_local, 2 branch_score, 3 branch_val; int32 at byte 32: sweeps, moves, branch_var */

struct NodeEvalBufs {
    HostBuf stage{false};                           // pinned staging (default memory: the source of a hipMemcpyAsync): the points [P][L + n], then lb [P][n], ub [P][n]
    DevBuf<double> d_in;                            // the same on the device
    HostBuf pinned{true};                           // the result block: slice p = header | x_local [n], padded to 64 bytes
};

struct NodeEvalArgs {
    int32_t n;
    int64_t L;
    const double *pts;      // [P][pts_stride]
    int64_t pts_stride;
    const double *lb, *ub;  // [P][n] each, or both NULL: the unit box
    const double *obj;      // [L + n] the LP objective
    const double *tab;      // [n][n]
    int32_t max_sweeps, rule;
    double rho;
    char *block;
    int64_t slice;
};

__global__ __launch_bounds__(256) void node_eval_table_kernel(int32_t n, const double *obj, double *tab)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n * n) return;
    const int64_t r = t / n, c = t - r * n;
    const int64_t i = r < c ? r : c, j = r < c ? c : r;
    tab[t] = obj[i * n - i * (i - 1) / 2 + (j - i)];
}

__device__ __forceinline__ double node_eval_lane_sum(double p)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p = p + __shfl_xor(p, off);
    return p;
}

// f at the x in LDS (every lane returns the same bits)
__device__ __forceinline__ double node_eval_f(const NodeEvalArgs &A, const double *x, int lane)
{
#pragma clang fp contract(off)
    const int n = A.n;
    const double *c = A.obj + A.L;
    double part = 0.0;
    for (int i = lane; i < n; i += 64) {
        double U = 0.0;
        for (int j = i; j < n; ++j) U = U + A.tab[(int64_t)j * n + i] * x[j];
        part = part + (c[i] + U) * x[i];
    }
    return node_eval_lane_sum(part);
}

// min(max(x, l), u) by comparisons: no choice between a +0 and a -0 is left to a library
__device__ __forceinline__ double node_eval_clamp(double x, double l, double u)
{
    const double t = x < l ? l : x;
    return t > u ? u : t;
}

__device__ __forceinline__ double node_eval_phi(double a, double s, double t)
{
#pragma clang fp contract(off)
    return (a * t + s) * t;
}

// (g1, i1) stands in front of (g2, i2): the larger g, the lower index on ties; i < 0 is "none"
__device__ __forceinline__ bool node_eval_better(double g1, int i1, double g2, int i2)
{
    if (i1 < 0) return false;
    if (i2 < 0) return true;
    return g1 > g2 || (g1 == g2 && i1 < i2);
}

__global__ __launch_bounds__(64) void node_eval_kernel(NodeEvalArgs A)
{
#pragma clang fp contract(off)
    extern __shared__ double s_x[];      // [n]
    const int lane = threadIdx.x, n = A.n;
    const int64_t p = blockIdx.x;
    const double *pt = A.pts + p * A.pts_stride;
    const double *lb = A.lb ? A.lb + p * n : nullptr, *ub = A.ub ? A.ub + p * n : nullptr;
    const double *c = A.obj + A.L;
    char *block = A.block + p * A.slice;
    double *o_x = (double *)(block + NODE_EVAL_HDR_BYTES);

    // projection
    for (int i = lane; i < n; i += 64) {
        const double l = lb ? lb[i] : 0.0, u = ub ? ub[i] : 1.0;
        s_x[i] = node_eval_clamp(pt[A.L + i], l, u);
    }
    __syncthreads();
    const double f_point = node_eval_f(A, s_x, lane);

    // branching, at the projected x and the point's own X
    double bg = 0.0;
    int bi = -1;
    for (int i = lane; i < n; i += 64) {
        const double l = lb ? lb[i] : 0.0, u = ub ? ub[i] : 1.0;
        if (!(u - l >= 4.0 * SDPCUT_BOX_MIN_WIDTH)) continue;
        const double xi = s_x[i];
        const int64_t row_i = (int64_t)i * n - (int64_t)i * (i - 1) / 2;      // pos(i, i)
        double g;
        if (A.rule == 0) {
            g = pt[row_i] - xi * xi;
        } else {
            g = 0.0;
            for (int j = 0; j < n; ++j) {
                const double X = j < i ? pt[(int64_t)j * n - (int64_t)j * (j - 1) / 2 + (i - j)] : pt[row_i + (j - i)];
                g = g + fabs(A.tab[(int64_t)j * n + i]) * fabs(X - xi * s_x[j]);
            }
        }
        if (!(g == g)) g = -INFINITY;      // (an overflowed score never wins a comparison)
        if (node_eval_better(g, i, bg, bi)) { bg = g; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double og = __shfl_xor(bg, off);
        const int oi = __shfl_xor(bi, off);
        if (node_eval_better(og, oi, bg, bi)) { bg = og; bi = oi; }
    }
    double bval = 0.0;
    if (bi >= 0) {
        const double l = lb ? lb[bi] : 0.0, u = ub ? ub[bi] : 1.0;
        const double w = A.rho * (u - l), m = w < SDPCUT_BOX_MIN_WIDTH ? SDPCUT_BOX_MIN_WIDTH : w;
        bval = node_eval_clamp(s_x[bi], l + m, u - m);
        // l + m and u - m are rounded: where m is the minimum width and the sum crosses a binade, a child can come out an ulp
        // narrower than the minimum.  The value moves by single ulps (it is positive: its bit pattern counts them) until both
        // children pass sdpcut_set_box's own test; a candidate is four minimum widths wide, a few steps always do
        for (int k = 0; k < 4 && bval - l < SDPCUT_BOX_MIN_WIDTH; ++k) bval = __longlong_as_double(__double_as_longlong(bval) + 1);
        for (int k = 0; k < 4 && u - bval < SDPCUT_BOX_MIN_WIDTH; ++k) bval = __longlong_as_double(__double_as_longlong(bval) - 1);
    } else {
        bg = 0.0;
    }

    // local search: every lane takes the same decisions from the same bits
    int sweeps = 0, moves = 0;
    for (int sw = 0; sw < A.max_sweeps; ++sw) {
        int moved = 0;
        for (int i = 0; i < n; ++i) {
            const double *row = A.tab + (int64_t)i * n;
            double part = 0.0;
            for (int j = lane; j < n; j += 64) part = part + (j == i ? 0.0 : row[j] * s_x[j]);
            const double s = c[i] + node_eval_lane_sum(part);
            const double a = row[i], xi = s_x[i];
            const double l = lb ? lb[i] : 0.0, u = ub ? ub[i] : 1.0;
            double t;
            if (a > 0.0) t = node_eval_clamp((-s) / (2.0 * a), l, u);
            else t = node_eval_phi(a, s, u) < node_eval_phi(a, s, l) ? u : l;
            if (node_eval_phi(a, s, t) < node_eval_phi(a, s, xi)) {      // (uniform)
                // The workgroup is one wave: nothing waits for another wave here.  The pair only orders the LDS traffic of the
                // wave itself -- every lane's reads of s_x before lane 0's store, the store before the next reads
                __syncthreads();
                if (lane == 0) s_x[i] = t;
                __syncthreads();
                ++moved;
            }
        }
        ++sweeps;
        moves += moved;
        if (!moved) break;
    }
    __syncthreads();
    const double f_local = node_eval_f(A, s_x, lane);

    for (int i = lane; i < n; i += 64) o_x[i] = s_x[i];
    if (lane == 0) {
        double *hd = (double *)block;
        int32_t *hi = (int32_t *)(block + 32);
        hd[0] = f_point; hd[1] = f_local; hd[2] = bg; hd[3] = bval;
        hi[0] = sweeps; hi[1] = moves; hi[2] = bi; hi[3] = 0;
    }
}

// ------------------------------------------------------------------------------------------
void free_node_eval_ws(sdpcut_ctx *h)
{
    delete (NodeEvalBufs *)h->node_eval;
    h->node_eval = nullptr;
}

// The dense table of the vector in d_lpobj, enqueued in front of the first evaluation after a sdpcut_set_objective (which only marks
// the table stale: callers that never evaluate a node pay nothing).  n <= NODE_EVAL_MAX_N: the caller has checked.
static int node_eval_build_table(sdpcut_ctx *h)
{
    if (h->lpobj_dense_ok) return 0;
    const int64_t n = h->nb_vars;
    if (!h->d_lpobj_dense.get()) HIP_TRY(h, h->d_lpobj_dense.reset((size_t)(n * n)));
    hipLaunchKernelGGL(node_eval_table_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, h->stream, (int32_t)n, (const double *)h->d_lpobj.get(),
                       h->d_lpobj_dense.get());
    HIP_TRY(h, hipGetLastError());
    h->lpobj_dense_ok = true;
    return 0;
}

static size_t node_eval_slice(int64_t n) { return ((size_t)NODE_EVAL_HDR_BYTES + (size_t)n * 8 + 63) & ~(size_t)63; }

extern "C" {

int sdpcut_node_eval_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb, const double *ub,
                            int32_t max_sweeps, int32_t branch_rule, double rho, sdpcut_node_eval_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    const std::string what = "sdpcut_node_eval_points: ";
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, what + "out is NULL");
    if (!h->d_vars.get() || h->nb_vars == 0) return sdpcut_fail(h, SDPCUT_ESTATE, what + "set_instance first");
    if (!h->d_lpobj.get()) return sdpcut_fail(h, SDPCUT_ESTATE, what + "set_objective first");
    const int64_t n = h->nb_vars, L = h->L, m = L + n;
    if (n > NODE_EVAL_MAX_N) return sdpcut_fail(h, SDPCUT_EINVAL, what + "instances of at most " + std::to_string(NODE_EVAL_MAX_N) + " variables are served");
    int rc;
    if ((rc = check_point_batch(h, what.c_str(), n_points, points, point_ld, m))) return rc;
    if ((rc = check_box_pair(h, what.c_str(), lb, ub))) return rc;
    if (max_sweeps < 0) return sdpcut_fail(h, SDPCUT_EINVAL, what + "max_sweeps must be >= 0");
    if (branch_rule != 0 && branch_rule != 1) return sdpcut_fail(h, SDPCUT_EINVAL, what + "branch_rule must be 0 (X_ii - x_i^2) or 1 (weighted by the objective)");
    if (!(rho > 0.0 && rho <= 0.5)) return sdpcut_fail(h, SDPCUT_EINVAL, what + "rho must lie in (0, 0.5]");
    const int P = n_points;
    for (int p = 0; p < P; ++p) {
        const double *v = points + (size_t)p * point_ld;
        for (int64_t i = 0; i < m; ++i)
            if (!std::isfinite(v[i])) return sdpcut_fail(h, SDPCUT_EINVAL, what + "point " + std::to_string(p) + " has a non-finite entry");
        if (!lb) continue;
        for (int64_t i = 0; i < n; ++i) {
            const double l = lb[(size_t)p * n + i], u = ub[(size_t)p * n + i];
            if (!(std::isfinite(l) && std::isfinite(u) && 0.0 <= l && l < u && u <= 1.0))
                return sdpcut_fail(h, SDPCUT_EINVAL, what + "point " + std::to_string(p) + ", variable " + std::to_string(i) + ": a box needs 0 <= lb < ub <= 1");
        }
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t slice = node_eval_slice(n);
    const size_t pts = (size_t)P * (size_t)m, bx = lb ? (size_t)P * (size_t)n : 0;
    if (!h->node_eval) h->node_eval = new NodeEvalBufs();
    NodeEvalBufs &b = *(NodeEvalBufs *)h->node_eval;
    if ((rc = grow(h, b.pinned, slice * (size_t)P))) return rc;
    if ((rc = grow(h, b.stage, (pts + 2 * bx) * 8))) return rc;
    if ((rc = grow(h, b.d_in, pts + 2 * bx))) return rc;
    double *st = (double *)b.stage.get();
    pack_points(st, P, points, point_ld, m);
    if (lb) {
        std::memcpy(st + pts, lb, bx * 8);
        std::memcpy(st + pts + bx, ub, bx * 8);
    }
    HIP_TRY(h, hipMemcpyAsync(b.d_in.get(), st, (pts + 2 * bx) * 8, hipMemcpyHostToDevice, h->stream));
    if ((rc = node_eval_build_table(h))) return rc;      // (the first call after a set_objective: one more launch on the stream)
    NodeEvalArgs A;
    A.n = (int32_t)n;
    A.L = L;
    A.pts = b.d_in.get();
    A.pts_stride = m;
    A.lb = lb ? b.d_in.get() + pts : nullptr;
    A.ub = lb ? b.d_in.get() + pts + bx : nullptr;
    A.obj = h->d_lpobj.get();
    A.tab = h->d_lpobj_dense.get();
    A.max_sweeps = max_sweeps;
    A.rule = branch_rule;
    A.rho = rho;
    A.block = (char *)b.pinned.dev();
    A.slice = (int64_t)slice;
    hipLaunchKernelGGL(node_eval_kernel, dim3((unsigned)P), dim3(64), (size_t)n * 8, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sdpcut_sync(h));      // the one wait of the call
    const char *blk = (const char *)b.pinned.get();
    for (int p = 0; p < P; ++p) {
        const char *s = blk + slice * (size_t)p;
        const double *hd = (const double *)s;
        const int32_t *hi = (const int32_t *)(s + 32);
        sdpcut_node_eval_t &o = out[p];
        o.f_point = hd[0]; o.f_local = hd[1]; o.branch_score = hd[2]; o.branch_val = hd[3];
        o.sweeps = hi[0]; o.moves = hi[1]; o.branch_var = hi[2]; o.reserved = 0;
        o.x_local = (const double *)(s + NODE_EVAL_HDR_BYTES);
    }
    h->stat_node_eval_points += P;
    return SDPCUT_OK;
}

} // extern "C"
