// Dense eigen-cuts (strategy 0 of cut_select_algo, cut_select_qp.py:757-786) on the device (include/sdpcut.h: sdpcut_dense_round,
// sdpcut_dense_eig): the eigen-decomposition of the WHOLE lifted matrix [[1, x^T],[x, X]] of order D = n + 1 <= 128 at the handle's
// LP point, and one cut row of n + n(n+1)/2 coefficients for every negative eigenvalue but the largest.
//
// dn_eig_kernel -- one workgroup, the matrix resident in LDS (D x (D|1) doubles, <= 129 KB of the CU's 160 KB).  Two-sided cyclic
//   Jacobi in the round-robin ordering: a step rotates the floor(D/2) DISJOINT index pairs of one tournament round (an odd order
//   plays with a dummy index; whoever meets it has a bye).  With disjoint pairs the 2x2 blocks (rows of pair k) x (columns of pair l)
//   are disjoint too, and J_k^T B J_l touches nothing else: a step is ONE pass in which every block k <= l is read, rotated from both
//   sides and written back together with its mirror image by one thread -- no order among the threads, two barriers per step (angles
//   -> blocks -> next step's angles).  Rotation parameters from jac_sqrt / jac_rcp / jac_rsqrt (jacobi.h).
//   The vectors do not fit beside the matrix: V lives in a workspace of the handle in device memory, TRANSPOSED (row p = column p of
//   V, so a rotation combines two contiguous rows, coalesced); 128 KB that one CU reads and writes, resident in its caches.
//   A sweep starts only while off(A) = sqrt(2 sum_{i<j} a_ij^2) > 2^-52 * 1e-3 * ||A||_F (one workgroup reduction per sweep, in a
//   fixed order: the same point gives the same bits), at most DN_MAX_SWEEPS times.  Then a rank sort of the diagonal (ascending, ties
//   by index), the vectors copied out in that order, each scaled to unit length, and n_rows = #{r < n : lambda_r < -1e-15} (:773-774; the negatives are a prefix).
// dn_rows_kernel -- grid (row r, tile of 8 matrix rows); a workgroup whose r is not below the n_rows it reads from device memory
//   retires (no host round trip between the two kernels).  Values [2 v0 v1 .. 2 v0 vn | v1^2, 2 v1 v2, .., vn^2], rhs -v0^2 (:776-780,
//   nothing zeroed), stored straight into the handle's pinned host block; the column list [L .. L+n-1 | 0 .. L-1] is the same for
//   every row and written once, by the workgroups of r = 0.
#include <cstring>
#include <vector>

#include "common.h"
#include "jacobi.h"

#define DN_THREADS 1024
#define DN_MAX_D (SDPCUT_DENSE_MAX_VARS + 1)
#define DN_MAX_SWEEPS 30
#define DN_OFF_TOL (2.220446049250313e-16 * 1e-3)
#define DN_ROW_THREADS 128
#define DN_ROW_TILE 8

// device workspace of a handle: V^T during the iteration | the sorted vectors (row r = vector of eigenvalue r) | eigenvalues | meta
struct DenseWs {
    double *vt, *vs, *eig;
    int32_t *meta;      // n_rows, sweeps
};
static DenseWs dense_ws(void *base)
{
    DenseWs w;
    w.vt = (double *)base;
    w.vs = w.vt + DN_MAX_D * DN_MAX_D;
    w.eig = w.vs + DN_MAX_D * DN_MAX_D;
    w.meta = (int32_t *)(w.eig + DN_MAX_D);
    return w;
}
static const size_t DN_WS_BYTES = (size_t)(2 * DN_MAX_D * DN_MAX_D + DN_MAX_D) * sizeof(double) + 64;

// the pinned block of a dense round: 64 bytes (word 7 is the completion word of the fused rounds: left alone) | eigenvalues |
// rhs | cols | values
struct DenseLayout {
    size_t eig, rhs, cols, values, bytes;
};
static DenseLayout dense_layout(int n)
{
    const size_t row_len = (size_t)n + (size_t)n * (n + 1) / 2;
    DenseLayout y;
    y.eig = 64;
    y.rhs = y.eig + DN_MAX_D * sizeof(double);
    y.cols = y.rhs + DN_MAX_D * sizeof(double);
    y.values = y.cols + ((row_len * sizeof(int32_t) + 63) & ~(size_t)63);
    y.bytes = y.values + (size_t)n * row_len * sizeof(double);
    return y;
}

// sum over the workgroup in a fixed order; every thread returns the same bits.  red: one double per wave.
__device__ __forceinline__ double dn_block_sum(double v, double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();      // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < DN_THREADS / 64; ++w) s += red[w];
    return s;
}

extern __shared__ double dn_lds[];

__global__ __launch_bounds__(DN_THREADS) void dn_eig_kernel(const double *__restrict__ vars, int n, int64_t L, double *vt, double *vs,
                                                             double *eig_out, int32_t *meta)
{
    const int D = n + 1, ld = D | 1, m = D + (D & 1), h = m >> 1;
    double *A = dn_lds;                       // [D][ld]
    double *rc = A + D * ld;                  // per pair of the step: c, s, t
    double *rs = rc + DN_MAX_D / 2;
    double *rt = rs + DN_MAX_D / 2;
    double *lam = rt + DN_MAX_D / 2;          // [DN_MAX_D] diagonal for the sort
    double *red = lam + DN_MAX_D;             // [DN_THREADS / 64]
    int *rp = (int *)(red + DN_THREADS / 64); // per pair: p < q; q >= D: the pair holds the dummy index, p has a bye
    int *rq = rp + DN_MAX_D / 2;
    int *ord = rq + DN_MAX_D / 2;             // [DN_MAX_D] ord[r] = index of the r-th smallest eigenvalue
    const int tid = threadIdx.x;
    const int col = tid & (DN_MAX_D - 1), row0 = tid >> 7;      // a 128-wide view of the threads: 8 rows at a time
    const double *x = vars + L;

    double part = 0.0;
    if (col < D)
        for (int i = row0; i < D; i += DN_THREADS / DN_MAX_D) {
            double a;
            if (i == 0) a = col == 0 ? 1.0 : x[col - 1];
            else if (col == 0) a = x[i - 1];
            else {
                const int lo = (i < col ? i : col) - 1, hi = (i < col ? col : i) - 1;
                a = vars[(int64_t)lo * n - (int64_t)lo * (lo - 1) / 2 + (hi - lo)];
            }
            A[i * ld + col] = a;
            vt[i * D + col] = i == col ? 1.0 : 0.0;
            part = fma(a, a, part);
        }
    const double fro = jac_sqrt(dn_block_sum(part, red) + 1e-300);

    int sweeps = 0;
#pragma unroll 1
    for (; sweeps < DN_MAX_SWEEPS; ++sweeps) {
        part = 0.0;
        if (col < D)
            for (int i = row0; i < col; i += DN_THREADS / DN_MAX_D) {
                const double a = A[i * ld + col];
                part = fma(a, a, part);
            }
        const double off = jac_sqrt(2.0 * dn_block_sum(part, red) + 1e-300);
        if (!(off > DN_OFF_TOL * fro)) break;      // (uniform: every thread holds the same sum; a NaN point ends here too)
#pragma unroll 1
        for (int step = 0; step < m - 1; ++step) {
            if (tid < h) {
                int a = m - 1, b = step;
                if (tid > 0) {
                    a = step + tid;
                    a -= a >= m - 1 ? m - 1 : 0;
                    b = step - tid;
                    b += b < 0 ? m - 1 : 0;
                }
                const int p = a < b ? a : b, q = a < b ? b : a;
                double c = 1.0, s = 0.0, t = 0.0;
                if (q < D) {
                    const double apq = A[p * ld + q];
                    const double d = A[q * ld + q] - A[p * ld + p];
                    const double bb = 2.0 * apq;
                    const double den = d + copysign(jac_sqrt(fma(d, d, bb * bb) + 1e-300), d);      // (as jacobi_angle: a_pq = d = 0 gives t = 0)
                    t = bb * jac_rcp(den);
                    c = jac_rsqrt(fma(t, t, 1.0));
                    s = t * c;
                }
                rp[tid] = p; rq[tid] = q;
                rc[tid] = c; rs[tid] = s; rt[tid] = t;
            }
            __syncthreads();
            // A <- J^T A J, block by block: k = pair of the rows, l = k + dist (cyclic) = pair of the columns; every unordered {k, l} once
            const int k = tid & 63;
            if (k < h) {
                const int pk = rp[k], qk = rq[k];
                const bool lk = qk < D;
                const double ck = rc[k], sk = rs[k];
                for (int dist = tid >> 6; dist <= (h >> 1); dist += DN_THREADS / 64) {
                    if (dist == 0) {
                        if (lk) {
                            const double tapq = rt[k] * A[pk * ld + qk];
                            A[pk * ld + pk] -= tapq;
                            A[qk * ld + qk] += tapq;
                            A[pk * ld + qk] = 0.0;
                            A[qk * ld + pk] = 0.0;
                        }
                        continue;
                    }
                    if (!(h & 1) && dist == (h >> 1) && k >= dist) continue;      // (the diameter of an even circle: both ends would claim it)
                    int l = k + dist;
                    l -= l >= h ? h : 0;
                    const int pl = rp[l], ql = rq[l];
                    const bool ll = ql < D;
                    const double cl = rc[l], sl = rs[l];
                    const double b00 = A[pk * ld + pl];
                    const double b01 = ll ? A[pk * ld + ql] : 0.0;
                    const double b10 = lk ? A[qk * ld + pl] : 0.0;
                    const double b11 = (lk && ll) ? A[qk * ld + ql] : 0.0;
                    const double t00 = fma(cl, b00, -sl * b01), t01 = fma(sl, b00, cl * b01);
                    const double t10 = fma(cl, b10, -sl * b11), t11 = fma(sl, b10, cl * b11);
                    const double n00 = fma(ck, t00, -sk * t10), n10 = fma(sk, t00, ck * t10);
                    const double n01 = fma(ck, t01, -sk * t11), n11 = fma(sk, t01, ck * t11);
                    A[pk * ld + pl] = n00; A[pl * ld + pk] = n00;
                    if (ll) { A[pk * ld + ql] = n01; A[ql * ld + pk] = n01; }
                    if (lk) { A[qk * ld + pl] = n10; A[pl * ld + qk] = n10; }
                    if (lk && ll) { A[qk * ld + ql] = n11; A[ql * ld + qk] = n11; }
                }
            }
            // V <- V J on the transposed copy: rows p and q of pair kk, component `col`
            if (col < D)
                for (int kk = row0; kk < h; kk += DN_THREADS / DN_MAX_D) {
                    const int p = rp[kk], q = rq[kk];
                    if (q < D) {
                        const double c = rc[kk], s = rs[kk];
                        const double vp = vt[p * D + col], vq = vt[q * D + col];
                        vt[p * D + col] = fma(c, vp, -s * vq);
                        vt[q * D + col] = fma(s, vp, c * vq);
                    }
                }
            __syncthreads();
        }
    }

    // ascending order by rank (ties by index); ord starts as the identity so that a NaN spectrum still indexes inside the matrix
    if (tid < D) {
        lam[tid] = A[tid * ld + tid];
        ord[tid] = tid;
    }
    __syncthreads();
    int rank = 0;
    double mine = 0.0;
    if (tid < D) {
        mine = lam[tid];
        for (int j = 0; j < D; ++j) {
            const double o = lam[j];
            rank += (o < mine || (o == mine && j < tid)) ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid < D) {
        ord[rank] = tid;
        eig_out[rank] = mine;
    }
    __syncthreads();
    // every vector leaves with unit length: the rotations leave ||v|^2 - 1| of the order of D eps (1.4e-14 seen at D = 41), and a cut
    // row is v v^T written out -- it is the row of a unit vector only as far as v is one.  (rc .. rt are free once the sweeps are over.)
    double *scale = rc;                       // [D] <= 3 * (DN_MAX_D / 2) doubles
    if (tid < D) {
        const double *src = vt + ord[tid] * D;
        double ss = 0.0;
        for (int c = 0; c < D; ++c) ss = fma(src[c], src[c], ss);
        scale[tid] = ss > 0.0 ? 1.0 / sqrt(ss) : 1.0;      // (a NaN spectrum is copied out as it is)
    }
    __syncthreads();
    if (col < D)
        for (int r = row0; r < D; r += DN_THREADS / DN_MAX_D) vs[r * D + col] = vt[ord[r] * D + col] * scale[r];
    if (tid == 0) {
        int cnt = 0;
        for (int r = 0; r < n; ++r) cnt += lam[ord[r]] < SDPCUT_NEG_EIGVAL ? 1 : 0;      // (the largest eigenvalue is never a cut, :773)
        meta[0] = cnt;
        meta[1] = sweeps;
    }
}

__global__ __launch_bounds__(DN_ROW_THREADS) void dn_rows_kernel(const double *__restrict__ vs, const double *__restrict__ eig,
                                                                  const int32_t *__restrict__ meta, int n, int64_t L, int32_t *hdr,
                                                                  double *eig_out, double *rhs, int32_t *cols, double *values)
{
    __shared__ double v[DN_MAX_D];
    const int D = n + 1, r = blockIdx.x, tid = threadIdx.x;
    const int n_rows = meta[0];
    const int64_t row_len = (int64_t)n + (int64_t)n * (n + 1) / 2;
    if (r == 0 && blockIdx.y == 0) {
        if (tid == 0) { hdr[0] = n_rows; hdr[1] = meta[1]; }
        if (tid < D) eig_out[tid] = eig[tid];
    }
    if (r >= n_rows && r != 0) return;
    const bool live = r < n_rows;      // (r = 0 of a round without rows still writes the column list)
    if (tid < D) v[tid] = vs[r * D + tid];
    __syncthreads();
    if (live && blockIdx.y == 0 && tid == 0) rhs[r] = -v[0] * v[0];
    double *out = values + (int64_t)r * row_len;
    const int first = blockIdx.y * DN_ROW_TILE, last = first + DN_ROW_TILE < D ? first + DN_ROW_TILE : D;
    for (int i1 = first; i1 < last; ++i1) {
        // position of (i1, i2), i2 >= max(i1, 1): the x block first, then the packed upper triangle of X (row i1 - 1)
        const int i = i1 - 1;
        const int64_t base = i1 == 0 ? -1 : (int64_t)n + (int64_t)i * n - (int64_t)i * (i - 1) / 2 - i1;
        const double vi = v[i1];
        for (int i2 = (i1 > 1 ? i1 : 1) + tid; i2 <= n; i2 += DN_ROW_THREADS) {
            const int64_t pos = base + i2;
            if (live) out[pos] = vi * v[i2] * (i1 == i2 ? 1.0 : 2.0);
            if (r == 0) cols[pos] = (int32_t)(pos < n ? L + pos : pos - n);
        }
    }
}

static int dense_check(sdpcut_ctx *h)
{
    if (!h->d_vars.get() || !h->have_point) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance and set_point first");
    if (h->nb_vars > SDPCUT_DENSE_MAX_VARS)
        return sdpcut_fail(h, SDPCUT_EINVAL, "dense eigen-cuts: nb_vars must not exceed 127 (SDPCUT_DENSE_MAX_VARS: the lifted matrix of order "
                                             "nb_vars + 1 stays in the LDS of one workgroup)");
    return 0;
}

// enqueue the eigensolver at the handle's point; results in the handle's workspace
static int dense_eig_enqueue(sdpcut_ctx *h, DenseWs *ws)
{
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->d_dense.get()) HIP_TRY(h, h->d_dense.reset(DN_WS_BYTES));
    *ws = dense_ws(h->d_dense.get());
    const int D = h->nb_vars + 1;
    const size_t lds = (size_t)(D * (D | 1) + 3 * (DN_MAX_D / 2) + DN_MAX_D + DN_THREADS / 64) * sizeof(double)
                       + (size_t)(2 * (DN_MAX_D / 2) + DN_MAX_D) * sizeof(int);
    // (more than the default 64 KB of dynamic LDS from order 90 on)
    HIP_TRY(h, hipFuncSetAttribute((const void *)dn_eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024));
    if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(dn_eig_kernel, dim3(1), dim3(DN_THREADS), lds, h->stream, h->d_vars.get(), (int)h->nb_vars, h->L, ws->vt, ws->vs, ws->eig,
                       ws->meta);
    HIP_TRY(h, hipGetLastError());
    if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    h->timed_score = h->timing != 0;
    return 0;
}

extern "C" {

int sdpcut_dense_round(sdpcut_handle h, const double *vars_values, sdpcut_dense_round_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    std::memset(out, 0, sizeof(*out));
    SDPCUT_NO_PENDING(h);
    int rc;
    if (vars_values && (rc = sdpcut_set_point(h, vars_values))) return rc;
    if ((rc = dense_check(h))) return rc;
    const int n = h->nb_vars;
    const DenseLayout y = dense_layout(n);
    if ((rc = ensure_pinned(h, y.bytes))) return rc;
    DenseWs ws;
    if ((rc = dense_eig_enqueue(h, &ws))) return rc;
    char *dev = (char *)h->pinned.dev();
    if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[2], h->stream));
    hipLaunchKernelGGL(dn_rows_kernel, dim3(n, (n + 1 + DN_ROW_TILE - 1) / DN_ROW_TILE), dim3(DN_ROW_THREADS), 0, h->stream, ws.vs, ws.eig,
                       ws.meta, n, h->L, (int32_t *)dev, (double *)(dev + y.eig), (double *)(dev + y.rhs), (int32_t *)(dev + y.cols),
                       (double *)(dev + y.values));
    HIP_TRY(h, hipGetLastError());
    if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(h, sdpcut_sync(h));      // the round's one host wait
    const char *b = (const char *)h->pinned.get();
    const int32_t *hdr = (const int32_t *)b;
    out->dim = n + 1;
    out->n_rows = hdr[0];
    out->sweeps = hdr[1];
    out->row_len = (int64_t)n + (int64_t)n * (n + 1) / 2;
    out->eigvals = (const double *)(b + y.eig);
    out->cols = (const int32_t *)(b + y.cols);
    out->values = (const double *)(b + y.values);
    out->rhs = (const double *)(b + y.rhs);
    return SDPCUT_OK;
}

int sdpcut_dense_eig(sdpcut_handle h, double *eigvals, double *evecs)
{
    if (!h) return SDPCUT_EINVAL;
    if (!eigvals) return sdpcut_fail(h, SDPCUT_EINVAL, "eigvals is NULL");
    SDPCUT_NO_PENDING(h);
    int rc;
    if ((rc = dense_check(h))) return rc;
    DenseWs ws;
    if ((rc = dense_eig_enqueue(h, &ws))) return rc;
    const size_t D = (size_t)h->nb_vars + 1;
    std::vector<double> rows;
    HIP_TRY(h, hipMemcpyAsync(eigvals, ws.eig, D * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (evecs) {
        rows.resize(D * D);
        HIP_TRY(h, hipMemcpyAsync(rows.data(), ws.vs, D * D * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, sdpcut_sync(h));
    if (evecs)      // the device keeps vector r as a row; numpy's convention has it as column r
        for (size_t r = 0; r < D; ++r)
            for (size_t i = 0; i < D; ++i) evecs[i * D + r] = rows[r * D + i];
    return SDPCUT_OK;
}

} // extern "C"
