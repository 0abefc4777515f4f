// Exact-SDP optimality measure of one candidate (strategies 3 and -1 of cut_select_algo): the solver body shared by the two kernels
// of exact_sdp.hip and by host code (plain C++: no HIP construct outside ESDP_HD).  exact_sdp.py is its numpy twin -- same
// formulation, same stopping rule, same degenerate rules, constants under the same names.
//
// The reference hands MOSEK, per candidate rho of size k (cut_select_qp.py:556-567, :586-598),
//     p* = min sum_{i<=j} q_ij X_ij   s.t.  [[X, x],[x^T, 1]] >= 0,  X_ii <= x_i            x = x_rho, q = Q_slice (upper triangle)
// With Y = X - x x^T, C symmetric with C_ii = q_ii, C_ij = q_ij / 2 and d_i = x_i - x_i^2:
//     p* = sum q_ij x_i x_j + min{ <C, Y> : Y >= 0, Y_ii <= d_i } = sum q_ij x_i x_j - min{ d^T lam : lam >= 0, C + Diag(lam) >= 0 }
// The solver works on the problem SCALED by r = sqrt(d): A = Diag(r) C Diag(r), Y = Diag(r) Z Diag(r), l_i = d_i lam_i,
//     min{ <A, Z> : Z >= 0, Z_ii <= 1 } = - min{ sum l_i : l >= 0, A + Diag(l) >= 0 }
// (every bound is 1 whatever the LP point) and takes damped Newton steps on the dual barrier function
//     sum l_i - mu log det(A + Diag l) - mu sum log l_i,      gradient 1 - mu (S^-1)_ii - mu / l_i,  Hessian mu (S^-1 o S^-1 + Diag l^-2),
// S = A + Diag l: step length 1 / (1 + delta) with delta the Newton decrement (a step that stays inside the domain in exact
// arithmetic; halved while rounding says otherwise: S must factor and l stay positive), the full step once delta <= 1/4, and mu
// shrinks geometrically after every full step.  One k x k Cholesky factorisation of S and one of the Hessian per iteration.
//
// Certificate of EVERY iterate: l is dual feasible (S has just been factored), and Z = Diag(s) S^-1 Diag(s) is primal feasible
// for any s with s_i^2 (S^-1)_ii <= 1; s puts Z_ii on its bound where the bound is active (l_i (S^-1)_ii >= ESDP_FORCE_DIAG) and at
// l_i V_ii / (1 + l_i V_ii) -- what mu (S^-1)_ii is at a centre -- elsewhere.  gap = <A, Z> + sum l_i >= 0; the iteration stops when
// gap <= ESDP_GAP_TOL max(1, |p*|) or at the iteration cap, and returns the lower bound, the gap and (if asked) lam and Y.
//
// Degenerate rules:
//   * d_i = max(x_i - x_i^2, 0): LP points sit on their bounds and stray outside by the LP tolerance;
//   * an index with d_i = 0 is eliminated: row and column i of Y are zero, lam_i is reported as 0 and takes no part in the dual
//     feasibility of the others (its row of A vanishes, its l_i stays out of the bound);
//   * A positive semidefinite already (LDL^T without pivoting: pivots >= -tiny, the column under a pivot <= tiny itself <= tiny,
//     tiny = 8 eps max|A|): lam = 0, Y = 0, p* = sum q_ij x_i x_j, no iteration.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ESDP_HD __host__ __device__ __forceinline__
#else
#define ESDP_HD inline
#endif

#define ESDP_GAP_TOL 1e-9
#define ESDP_MU_SHRINK 0.2
#define ESDP_DELTA_CENTRED 0.25
#define ESDP_FORCE_DIAG 1e5
#define ESDP_MAX_HALVINGS 30
// twice the largest iteration count of the twin on the CPU test inputs (exact_sdp.py: ITER_CAP)
#define ESDP_ITER_CAP 138

// packed lower triangle: (i, j), i >= j
constexpr int esdp_lo(int i, int j) { return i * (i + 1) / 2 + j; }
constexpr int esdp_sym(int i, int j) { return i >= j ? esdp_lo(i, j) : esdp_lo(j, i); }

template <int K>
struct Esdp {
    static constexpr int M = K * (K + 1) / 2;
    double A[M];      // scaled weights, packed lower
    double L[M];      // Cholesky factor of S = A + Diag(l), packed lower; Linv its reciprocal diagonal
    double Linv[K];
    double l[K], r[K];
    double mu, xqx;
    int32_t iters;
    bool done, converged;
};

// where a candidate's results go (any pointer may be null): value = add + p*_lower * scale
struct EsdpOut {
    double *value, *gap, *lam, *Y;
    int32_t *iters;
    double add, scale;
};

// lower factor of the packed matrix S (+ diag on its diagonal); false where a pivot is not positive (the factor is then finite garbage)
template <int K>
ESDP_HD bool esdp_cholesky(const double (&S)[K * (K + 1) / 2], const double (&diag)[K], double (&L)[K * (K + 1) / 2], double (&Linv)[K])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double p = S[esdp_lo(j, j)] + diag[j];
#pragma unroll
        for (int t = 0; t < j; ++t) p -= L[esdp_lo(j, t)] * L[esdp_lo(j, t)];
        const bool good = p > 0.0;
        ok = ok && good;
        p = good ? p : 1.0;
        const double rinv = 1.0 / sqrt(p);
        L[esdp_lo(j, j)] = p * rinv;
        Linv[j] = rinv;
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
            double s = S[esdp_lo(i, j)];
#pragma unroll
            for (int t = 0; t < j; ++t) s -= L[esdp_lo(i, t)] * L[esdp_lo(j, t)];
            L[esdp_lo(i, j)] = s * rinv;
        }
    }
    return ok;
}

// V = (L L^T)^-1, packed lower
template <int K>
ESDP_HD void esdp_inverse(const double (&L)[K * (K + 1) / 2], const double (&Linv)[K], double (&V)[K * (K + 1) / 2])
{
    double W[K * (K + 1) / 2];      // L^-1
#pragma unroll
    for (int j = 0; j < K; ++j) {
        W[esdp_lo(j, j)] = Linv[j];
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
            double s = 0.0;
#pragma unroll
            for (int t = j; t < i; ++t) s -= L[esdp_lo(i, t)] * W[esdp_lo(t, j)];
            W[esdp_lo(i, j)] = s * Linv[i];
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
#pragma unroll
            for (int t = i; t < K; ++t) s += W[esdp_lo(t, i)] * W[esdp_lo(t, j)];
            V[esdp_lo(i, j)] = s;
        }
}

// x [K], q [K(K+1)/2] upper triangle row-major (the MLP's input [x | Q_slice]).  On return st.done says that A is positive
// semidefinite already: the caller emits the trivial answer (esdp_emit_trivial) and never iterates.
template <int K>
ESDP_HD void esdp_init(Esdp<K> &st, const double (&x)[K], const double (&q)[K * (K + 1) / 2])
{
    constexpr int M = K * (K + 1) / 2;
    double xqx = 0.0, scale = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double d = x[i] - x[i] * x[i];
        st.r[i] = sqrt(d > 0.0 ? d : 0.0);
    }
    {
        int m = 0;
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = a; b < K; ++b, ++m) {
                xqx = xqx + q[m] * x[a] * x[b];
                const double c = a == b ? q[m] : 0.5 * q[m];
                const double v = c * st.r[a] * st.r[b];
                st.A[esdp_lo(b, a)] = v;
                scale = fmax(scale, fabs(v));
            }
    }
    st.xqx = xqx;
    st.iters = 0;
    st.converged = true;
    // positive semidefinite already?
    bool psd = true;
    {
        const double tiny = 8.0 * 2.220446049250313e-16 * scale;
        double W[M];
#pragma unroll
        for (int m = 0; m < M; ++m) W[m] = st.A[m];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double p = W[esdp_lo(j, j)];
            const bool zero = p <= tiny;
            psd = psd && p >= -tiny;
            double col = 0.0;
#pragma unroll
            for (int i = j + 1; i < K; ++i) col = fmax(col, fabs(W[esdp_lo(i, j)]));
            psd = psd && !(zero && col > tiny);
            const double pinv = zero ? 0.0 : 1.0 / (zero ? 1.0 : p);
#pragma unroll
            for (int i = j + 1; i < K; ++i)
#pragma unroll
                for (int t = j + 1; t <= i; ++t) W[esdp_lo(i, t)] -= W[esdp_lo(i, j)] * W[esdp_lo(t, j)] * pinv;
        }
    }
    st.done = psd;
    // start: S strictly diagonally dominant, mu of the size of the data
    st.mu = scale;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double off = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j != i) off += fabs(st.A[esdp_sym(i, j)]);
        const double g = off - st.A[esdp_lo(i, i)];
        st.l[i] = (g > 0.0 ? g : 0.0) + scale;
    }
    if (!psd) (void)esdp_cholesky<K>(st.A, st.l, st.L, st.Linv);
}

template <int K>
ESDP_HD void esdp_emit_trivial(const Esdp<K> &st, const EsdpOut &o)
{
    constexpr int M = K * (K + 1) / 2;
    if (o.value) *o.value = o.add + st.xqx * o.scale;
    if (o.gap) *o.gap = 0.0;
    if (o.iters) *o.iters = 0;
    if (o.lam)
#pragma unroll
        for (int i = 0; i < K; ++i) o.lam[i] = 0.0;
    if (o.Y)
#pragma unroll
        for (int m = 0; m < M; ++m) o.Y[m] = 0.0;
}

// One iteration of a candidate that is not done: certificate of the current iterate, then either the end (results stored through o,
// st.done set) or a Newton step.  cap = iteration cap (ESDP_ITER_CAP).
template <int K>
ESDP_HD void esdp_iterate(Esdp<K> &st, int cap, const EsdpOut &o)
{
    constexpr int M = K * (K + 1) / 2;
    double V[M];
    esdp_inverse<K>(st.L, st.Linv, V);
    double s[K], linv[K];
    double lower = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double dg = V[esdp_lo(i, i)];
        const double lv = st.l[i] * dg;
        const double tau = lv >= ESDP_FORCE_DIAG ? 1.0 : lv / (1.0 + lv);
        const bool act = st.r[i] > 0.0;
        s[i] = act ? sqrt(tau / dg) : 0.0;
        if (act) lower -= st.l[i];
        linv[i] = 1.0 / st.l[i];
    }
    double upper = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double t = st.A[esdp_lo(i, j)] * (s[i] * s[j] * V[esdp_lo(i, j)]);
            upper += i == j ? t : 2.0 * t;
        }
    const bool useZ = upper < 0.0;      // else Y = 0 is the better primal point
    upper = useZ ? upper : 0.0;
    const double pstar = st.xqx + lower;
    const double gap = upper - lower;
    const bool conv = gap <= ESDP_GAP_TOL * fmax(1.0, fabs(pstar));
    if (conv || st.iters >= cap) {
        if (o.value) *o.value = o.add + pstar * o.scale;
        if (o.gap) *o.gap = gap;
        if (o.iters) *o.iters = st.iters;
        if (o.lam)
#pragma unroll
            for (int i = 0; i < K; ++i) o.lam[i] = st.r[i] > 0.0 ? st.l[i] / (st.r[i] * st.r[i]) : 0.0;
        if (o.Y) {
            int m = 0;
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int b = a; b < K; ++b, ++m)
                    o.Y[m] = useZ ? (s[a] * st.r[a]) * V[esdp_lo(b, a)] * (s[b] * st.r[b]) : 0.0;
        }
        st.done = true;
        st.converged = conv;
        return;
    }
    // Newton step
    double g[K], H[M];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        g[i] = 1.0 - st.mu * V[esdp_lo(i, i)] - st.mu * linv[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) H[esdp_lo(i, j)] = st.mu * (V[esdp_lo(i, j)] * V[esdp_lo(i, j)]);
    }
    double hd[K];
#pragma unroll
    for (int i = 0; i < K; ++i) hd[i] = st.mu * (linv[i] * linv[i]);
    double HL[M], HLinv[K], y[K], step[K];
    (void)esdp_cholesky<K>(H, hd, HL, HLinv);      // (positive definite: mu Diag l^-2 alone is)
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double t = g[i];
#pragma unroll
        for (int j = 0; j < i; ++j) t -= HL[esdp_lo(i, j)] * y[j];
        y[i] = t * HLinv[i];
    }
    double gs = 0.0;
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        double t = y[i];
#pragma unroll
        for (int j = i + 1; j < K; ++j) t -= HL[esdp_lo(j, i)] * step[j];
        step[i] = t * HLinv[i];
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        step[i] = -step[i];
        gs += g[i] * step[i];
    }
    const double d2 = -gs / st.mu;
    const double delta = sqrt(d2 > 0.0 ? d2 : 0.0);
    const bool centred = delta <= ESDP_DELTA_CENTRED;
    double ts = centred ? 1.0 : 1.0 / (1.0 + delta);
    double ln[K];
    bool ok = false;
    for (int h = 0; h <= ESDP_MAX_HALVINGS; ++h) {
        bool pos = true;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            ln[i] = st.l[i] + ts * step[i];
            pos = pos && ln[i] > 0.0;
        }
        ok = esdp_cholesky<K>(st.A, ln, st.L, st.Linv) && pos;
        if (ok) break;
        ts *= 0.5;
    }
    if (ok) {
#pragma unroll
        for (int i = 0; i < K; ++i) st.l[i] = ln[i];
    } else {
        (void)esdp_cholesky<K>(st.A, st.l, st.L, st.Linv);      // stay: the iterate remains a certified one up to the cap
    }
    if (centred) st.mu *= ESDP_MU_SHRINK;
    ++st.iters;
}

// the whole solve of one candidate on the calling thread (host code, tests)
template <int K>
ESDP_HD bool esdp_solve(const double (&x)[K], const double (&q)[K * (K + 1) / 2], int cap, const EsdpOut &o)
{
    Esdp<K> st;
    esdp_init<K>(st, x, q);
    if (st.done) {
        esdp_emit_trivial<K>(st, o);
        return true;
    }
    while (!st.done) esdp_iterate<K>(st, cap, o);
    return st.converged;
}
