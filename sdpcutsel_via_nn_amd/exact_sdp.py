"""Numpy twin of the exact-SDP optimality measure (csrc/exact_sdp.h, csrc/exact_sdp.hip): strategies 3 and -1.

The reference ranks a candidate rho of size k by the optimum of a small SDP it hands to MOSEK, one call per candidate
(cut_select_qp.py:556-567, :586-598):

    p* = min sum_{i<=j} q_ij X_ij   s.t.  [[X, x],[x^T, 1]] >= 0,  X_ii <= x_i          x = x_rho, q = Q_slice (upper triangle)

With Y = X - x x^T, C symmetric with C_ii = q_ii, C_ij = q_ij / 2 and d_i = x_i - x_i^2:

    p* = sum q_ij x_i x_j + min{ <C, Y> : Y >= 0, Y_ii <= d_i }
       = sum q_ij x_i x_j - min{ d^T lam : lam >= 0, C + Diag(lam) >= 0 }

The solver works on the problem SCALED by r = sqrt(d):  A = Diag(r) C Diag(r),  Y = Diag(r) Z Diag(r),  l_i = d_i lam_i:

    min{ <A, Z> : Z >= 0, Z_ii <= 1 }  =  - min{ sum l_i : l >= 0, A + Diag(l) >= 0 }

so that every bound is 1 whatever the LP point, and runs damped Newton steps on the dual barrier function
sum l_i - mu log det(A + Diag l) - mu sum log l_i while mu shrinks geometrically.  Every iterate carries a certificate:
l is dual feasible (the Cholesky factorisation of S = A + Diag l succeeded), Z = Diag(s) S^-1 Diag(s) is primal feasible, with s
putting Z_ii on its bound 1 where l_i (S^-1)_ii >= FORCE_DIAG and at l_i V_ii / (1 + l_i V_ii) -- what mu (S^-1)_ii is at a centre --
elsewhere; `gap` = upper - lower bound.  The iteration stops when gap <= GAP_TOL max(1, |p*|) or at ITER_CAP.

Degenerate rules (the same in the kernel):
  * d_i = max(x_i - x_i^2, 0): LP points sit on their bounds and stray outside by the LP tolerance;
  * an index with d_i = 0 is eliminated -- row and column i of Y are zero, lam_i is reported as 0 and plays no part in the dual
    feasibility of the rest (in the scaled problem its row of A vanishes and its l_i is left out of the bound);
  * if A is positive semidefinite already (a pivoted-free LDL^T with pivots >= 0, columns under a zero pivot zero) the answer is
    lam = 0, Y = 0, p* = sum q_ij x_i x_j, zero iterations.  The decision is taken on A, in the scaled units, with an allowance of
    8 eps max|A|: a d_i of 1e-16 (x_i = 1e-16 or 0.9999999999999999: ordinary LP output) puts a pivot of -3e-17 inside it while
    C + Diag(0) itself has lambda_min = -0.33.  The value is right to 3e-17; certificate_check judges dual feasibility in the same
    scaled units, which is where the bound is proved.

Known limitation -- degenerate optima.  Where a bound Y_ii <= d_i is active with a ZERO multiplier (equal-magnitude weights at
x = 0.5: the round-1 point of every BoxQP run on a unit-weight instance) the upper bound may stall: Z_ii sits on its bound while
l_i -> 0, neither of the two recovery rules of s fits, and the primal point stops improving near a gap of 1e-5 .. 1e-3 while the
lower bound reaches the optimum.  Such a lane ends at ITER_CAP, flagged (converged False; SDPCUT_STAT_SDP_UNCONVERGED on the device)
with a valid but wider bracket; `value` remains a certified lower bound.  More iterations do not help (300 and 1000 both leave
the case below at 6.6e-6); the cure is a different primal recovery.  Measured on x = 0.5, q_ij in {0, +-1/k} (tests/sdp_inputs.py `vertex`, 256
inputs per k): none for k = 2, 3; k = 4: twin 2, host-compiled header 3, MI355X 2 (largest gap at the cap 1.9e-3); k = 5: twin 1,
header 1, MI355X 0 (6.9e-4).  Which tied input stalls depends on last-bit rounding: the three implementations disagree on it.
The smallest case, k = 4, x = 0.5, q = (1, -1, 0, 1, 0, 1, 1, 1, 0, 1) / 4, p* = 15/64: the twin ends at the cap with a gap of
5.1e-4 and the lower bound within 1e-9 of 15/64, the header converges in 83 iterations.  Every other family of tests/sdp_inputs.py
(x on, next to and outside its bounds, one-signed, tied-sign and tiny weights, nearly positive semidefinite C, the golden covers
late in a run) converges everywhere, in at most 91 iterations.
"""
import numpy as np

GAP_TOL = 1e-9       # stop when upper - lower <= GAP_TOL * max(1, |p*|), in the normalised units of p*
MU_SHRINK = 0.2      # geometric factor of the barrier parameter, applied after a step taken from a centred point
DELTA_CENTRED = 0.25 # Newton decrement below which a point counts as centred (full step; mu shrinks)
FORCE_DIAG = 1e5     # Z_ii is set to its bound 1 where l_i (S^-1)_ii >= this (l_i >= 1e5 mu at a centre: the bound is active), else to l_i V_ii / (1 + l_i V_ii)
MAX_HALVINGS = 30    # of a step that leaves the domain (the damped step never does in exact arithmetic)
# twice the largest iteration count the twin shows on the CPU test inputs
ITER_CAP = 2 * 69
# feasibility slack of certificate_check in units of eps * (||C||_F + ||lam||_inf), eps * (||A||_F + ||l||_inf) for dual
# feasibility: 4 x the worst the twin shows on the inputs of tests/test_exact_sdp_cpu.py (0.85 on the twin; the
# device's own certificates showed 1.28 on an MI355X, inside it; on the edge families of tests/sdp_inputs.py twin 1.55, device 2.45)
SLACK_UNITS = 3.4
_EPS = np.finfo(np.float64).eps


def _triu(k):
    return np.triu_indices(k)


def unpack(k, inputs):
    """[n, k(k+3)/2] = [x | Q_slice]  ->  x [n, k], C [n, k, k] symmetric (off-diagonal weights halved), xqx [n]."""
    inputs = np.asarray(inputs, dtype=np.float64)
    x, q = inputs[:, :k], inputs[:, k:]
    ia, ib = _triu(k)
    C = np.zeros((inputs.shape[0], k, k))
    C[:, ia, ib] = np.where(ia == ib, q, 0.5 * q)
    C[:, ib, ia] = C[:, ia, ib]
    xqx = np.zeros(inputs.shape[0])
    for m in range(ia.shape[0]):       # index order, as the kernel sums
        xqx = xqx + q[:, m] * x[:, ia[m]] * x[:, ib[m]]
    return x, C, xqx


def _cholesky(S):
    """lower factor of [n, k, k]; ok[n] False where a pivot is not positive (that factor is garbage but finite)"""
    n, k = S.shape[0], S.shape[1]
    L = np.zeros_like(S)
    ok = np.ones(n, dtype=bool)
    for j in range(k):
        p = S[:, j, j].copy()
        for t in range(j):
            p = p - L[:, j, t] * L[:, j, t]
        good = p > 0
        ok &= good
        p = np.where(good, p, 1.0)
        rinv = 1.0 / np.sqrt(p)
        L[:, j, j] = p * rinv
        for i in range(j + 1, k):
            s = S[:, i, j].copy()
            for t in range(j):
                s = s - L[:, i, t] * L[:, j, t]
            L[:, i, j] = s * rinv
    return L, ok


def _inverse_from_factor(L):
    """(L L^T)^-1 for lower factors [n, k, k]"""
    n, k = L.shape[0], L.shape[1]
    W = np.zeros_like(L)                   # W = L^-1 (lower)
    for j in range(k):
        W[:, j, j] = 1.0 / L[:, j, j]
        for i in range(j + 1, k):
            s = np.zeros(n)
            for t in range(j, i):
                s = s - L[:, i, t] * W[:, t, j]
            W[:, i, j] = s / L[:, i, i]
    V = np.zeros_like(L)
    for i in range(k):
        for j in range(i + 1):
            s = np.zeros(n)
            for t in range(i, k):
                s = s + W[:, t, i] * W[:, t, j]
            V[:, i, j] = V[:, j, i] = s
    return V


def _solve_spd(H, g):
    """H^-1 g through a Cholesky factorisation (H = mu (S^-1 o S^-1 + Diag l^-2) is positive definite)"""
    L, _ = _cholesky(H)
    k = H.shape[1]
    y = np.zeros_like(g)
    for i in range(k):
        s = g[:, i].copy()
        for t in range(i):
            s = s - L[:, i, t] * y[:, t]
        y[:, i] = s / L[:, i, i]
    z = np.zeros_like(g)
    for i in range(k - 1, -1, -1):
        s = y[:, i].copy()
        for t in range(i + 1, k):
            s = s - L[:, t, i] * z[:, t]
        z[:, i] = s / L[:, i, i]
    return z


def _is_psd(A, tiny):
    """LDL^T without pivoting: every pivot >= -tiny, and the column under a pivot <= tiny is itself <= tiny"""
    n, k = A.shape[0], A.shape[1]
    W = A.copy()
    psd = np.ones(n, dtype=bool)
    for j in range(k):
        p = W[:, j, j]
        zero = p <= tiny
        psd &= p >= -tiny
        col = np.zeros(n)
        for i in range(j + 1, k):
            col = np.maximum(col, np.abs(W[:, i, j]))
        psd &= ~(zero & (col > tiny))
        pinv = np.where(zero, 0.0, 1.0 / np.where(zero, 1.0, p))
        for i in range(j + 1, k):
            for t in range(j + 1, i + 1):
                W[:, i, t] = W[:, i, t] - W[:, i, j] * W[:, t, j] * pinv
                W[:, t, i] = W[:, i, t]
    return psd


def solve(k, inputs, iter_cap=None):
    """Batched solver: inputs [n, k(k+3)/2] = [x | Q_slice] (the layout of the MLP's input).
    -> dict(value = certified LOWER bound on p*, upper, gap, lam [n, k], Y [n, k(k+1)/2] upper triangle, iters int32 [n],
            converged bool [n])."""
    cap = ITER_CAP if iter_cap is None else int(iter_cap)
    x, C, xqx = unpack(k, inputs)
    n = x.shape[0]
    d = np.maximum(x - x * x, 0.0)
    r = np.sqrt(d)
    act = d > 0
    A = C * r[:, :, None] * r[:, None, :]
    scale = np.abs(A).reshape(n, -1).max(axis=1) if n else np.zeros(0)
    lo, up = np.zeros(n), np.zeros(n)                      # bounds on min <A, Z>  (lower = -sum l)
    l_out, Z_out = np.zeros((n, k)), np.zeros((n, k, k))
    iters = np.zeros(n, dtype=np.int32)
    done = _is_psd(A, 8 * _EPS * scale) if n else np.zeros(0, dtype=bool)
    live = np.flatnonzero(~done)
    # start: S strictly diagonally dominant, mu of the size of the data
    Al, actl = A[live], act[live]
    mu = scale[live].copy()
    off = np.abs(Al).sum(axis=2) - np.abs(Al[:, np.arange(k), np.arange(k)])
    l = np.maximum(off - Al[:, np.arange(k), np.arange(k)], 0.0) + mu[:, None]
    L, _ = _cholesky(Al + l[:, :, None] * np.eye(k))
    tol_of = lambda lower: GAP_TOL * np.maximum(1.0, np.abs(xqx[live] + lower))      # noqa: E731
    for it in range(cap + 1):
        if live.size == 0:
            break
        V = _inverse_from_factor(L)                        # S^-1
        dg = V[:, np.arange(k), np.arange(k)]
        # certificate of this iterate
        lv = l * dg
        tau = np.where(lv >= FORCE_DIAG, 1.0, lv / (1.0 + lv))
        s = np.where(actl, np.sqrt(tau / dg), 0.0)
        Z = s[:, :, None] * V * s[:, None, :]
        upper = np.minimum((Al * Z).sum(axis=(1, 2)), 0.0)
        Z = np.where((upper < 0.0)[:, None, None], Z, 0.0)
        lower = -np.where(actl, l, 0.0).sum(axis=1)
        fin = (upper - lower <= tol_of(lower)) | (it == cap)
        if fin.any():
            w = live[fin]
            lo[w], up[w], l_out[w], Z_out[w], iters[w] = lower[fin], upper[fin], l[fin], Z[fin], it
            done[w] = (upper - lower <= tol_of(lower))[fin]
            keep = ~fin
            live, Al, actl, mu, l, L, V, dg = live[keep], Al[keep], actl[keep], mu[keep], l[keep], L[keep], V[keep], dg[keep]
            if live.size == 0:
                break
        # damped Newton step on sum l - mu log det S - mu sum log l
        g = 1.0 - mu[:, None] * dg - mu[:, None] / l
        H = mu[:, None, None] * (V * V)
        H[:, np.arange(k), np.arange(k)] += mu[:, None] / (l * l)
        step = -_solve_spd(H, g)
        delta = np.sqrt(np.maximum(-(g * step).sum(axis=1) / mu, 0.0))
        centred = delta <= DELTA_CENTRED
        ts = np.where(centred, 1.0, 1.0 / (1.0 + delta))
        l_new = l + ts[:, None] * step
        L, ok = _cholesky(Al + l_new[:, :, None] * np.eye(k))
        bad = ~(ok & (l_new > 0).all(axis=1))
        for _ in range(MAX_HALVINGS):
            if not bad.any():
                break
            ts = np.where(bad, 0.5 * ts, ts)
            l_new = np.where(bad[:, None], l + ts[:, None] * step, l_new)
            Lb, okb = _cholesky(Al[bad] + l_new[bad][:, :, None] * np.eye(k))
            L[bad] = Lb
            bad[np.flatnonzero(bad)] = ~(okb & (l_new[bad] > 0).all(axis=1))
        if bad.any():      # stay: the iterate remains a certified one up to the cap
            l_new = np.where(bad[:, None], l, l_new)
            L[bad], _ = _cholesky(Al[bad] + l[bad][:, :, None] * np.eye(k))
        l = l_new
        mu =np.where(centred, MU_SHRINK * mu, mu)
    # back to the units of the problem
    lam = np.where(act, l_out / np.where(act, d, 1.0), 0.0)
    Yf = Z_out * r[:, :, None] * r[:, None, :]
    ia, ib = _triu(k)
    return dict(value=xqx + lo, upper=xqx + up, gap=up - lo, lam=lam, Y=Yf[:, ia, ib], iters=iters, converged=done.astype(bool))


def measure(k, inputs, negSM, max_elem, **kw):
    """the strategy's score of cut_select_qp.py:575, :595: (-S) max_elem + p*_lower max_elem"""
    return negSM + solve(k, inputs, **kw)["value"] * max_elem


def certificate_check(C, d, lam, Y, slack_units=SLACK_UNITS):
    """Independent optimality proof of one batch: C [n, k, k] symmetric, d [n, k] (already max(., 0)), lam [n, k],
    Y [n, k(k+1)/2] upper triangle.  Checks with numpy.linalg.eigvalsh, on the indices with d_i > 0 (the others are eliminated: their
    rows of Y must vanish):  lam >= 0,  Y >= -s,  Y_ii <= d_i + s,  weak duality  -d^T lam <= <C, Y> + s
    with s = slack_units * eps * (||C||_F + ||lam||_inf), and dual feasibility WHERE THE SOLVER DECIDED IT, in the units scaled by
    r = sqrt(d) (A = Diag(r) C Diag(r), l_i = d_i lam_i):
        Diag(r) (C + Diag(lam)) Diag(r) = A + Diag(l) >= -s_A,      s_A = slack_units * eps * (||A||_F + ||l||_inf)
    plus, for an answer with lam = 0 (the positive-semidefinite shortcut), the shortcut's own allowance 8 eps max|A|.
    That is a proof of  value - k s_A <= p*:  every feasible Y is Diag(r) Z Diag(r) with Z >= 0, Z_ii <= 1 (so trace Z <= k), and
        <C, Y> = <A + Diag(l), Z> - sum l_i Z_ii >= -s_A trace Z - sum l_i >= -k s_A - d^T lam.
    (Judged on C + Diag(lam) itself, a d_i of 1e-16 turns a pivot of A that is -3e-17, rounding, into lambda_min = -0.33: the
    bound such an answer returns is right to 3e-17, and the unscaled matrix says nothing about it.  `dual_min_unscaled` reports it.)
    -> dict(ok bool [n], dual_min (of A + Diag l), dual_min_unscaled (of C + Diag lam), primal_min, diag_excess, units [n]: the
            largest violation of each candidate in units of eps (||C||_F + ||lam||_inf) -- eps (||A||_F + ||l||_inf) for the dual
            one, net of the shortcut's allowance --, worst_units: the largest of them)."""
    C, d, lam = np.asarray(C, float), np.asarray(d, float), np.asarray(lam, float)
    n, k = d.shape
    ia, ib = _triu(k)
    Ym = np.zeros((n, k, k))
    Ym[:, ia, ib] = Y
    Ym[:, ib, ia] = Y
    act = d > 0
    unit = _EPS * (np.sqrt((C * C).sum(axis=(1, 2))) + np.abs(lam).max(axis=1))
    unit = np.where(unit > 0, unit, _EPS)
    s = slack_units * unit
    mask = act[:, :, None] & act[:, None, :]
    # eliminated indices become decoupled unit diagonals: they do not move the smallest eigenvalue of the rest below zero
    eye = np.eye(k)[None]
    r = np.sqrt(d)
    A, l = C * r[:, :, None] * r[:, None, :], d * lam
    SA = A + l[:, :, None] * eye
    size = np.abs(SA).reshape(n, -1).max(axis=1)      # (the eliminated diagonal at the size of the rest: eigvalsh errs by eps x the largest entry)
    dual_min = np.linalg.eigvalsh(np.where(mask, SA, np.where(size > 0, size, 1.0)[:, None, None] * eye))[:, 0]
    dual_min_unscaled = np.linalg.eigvalsh(np.where(mask, C + lam[:, :, None] * eye, eye))[:, 0]
    unit_A = _EPS * (np.sqrt((A * A).sum(axis=(1, 2))) + np.abs(l).max(axis=1))
    unit_A = np.where(unit_A > 0, unit_A, _EPS)
    shortcut = np.where((lam == 0.0).all(axis=1), 8 * _EPS * np.abs(A).reshape(n, -1).max(axis=1), 0.0)
    dual_viol = np.maximum(-dual_min - shortcut, 0.0)
    primal_min = np.linalg.eigvalsh(Ym)[:, 0]
    dgY = Ym[:, np.arange(k), np.arange(k)]
    diag_excess = (dgY - d).max(axis=1)
    elim_rows = np.where(mask, 0.0, np.abs(Ym)).reshape(n, -1).max(axis=1)
    lower, upper = -(d * lam).sum(axis=1), (C * Ym).sum(axis=(1, 2))
    viol = np.maximum.reduce([-primal_min, diag_excess, -lam.min(axis=1), lower - upper, np.zeros(n)])
    ok = (viol <= s) & (dual_viol <= slack_units * unit_A) & (elim_rows == 0.0)
    units = np.maximum(viol / unit, dual_viol / unit_A)
    return dict(ok=ok, dual_min=dual_min, dual_min_unscaled=dual_min_unscaled, primal_min=primal_min, diag_excess=diag_excess, units=units,
                worst_units=float(units.max()) if n else 0.0)


def figure8(nn_measure, exact_measure, cut_round, sel_size):
    """The comparison of cut_select_qp.py:687-702 from the two measures of every candidate (arrays in candidate order):
    -> (order by the estimated measure (stable, descending), overlap / sel_size, std of the sel_size largest exact measures,
        this_round_cuts rows [cut_round, cut_idx, sel_by_estim, sel_by_exact, estimated, exact] in the estimated order)."""
    nn_measure, exact_measure = np.asarray(nn_measure, float), np.asarray(exact_measure, float)
    n = nn_measure.shape[0]
    by_nn = np.argsort(-nn_measure, kind="stable")
    by_ex = np.argsort(-exact_measure, kind="stable")
    pos_ex = np.empty(n, dtype=np.int64)
    pos_ex[by_ex] = np.arange(n)
    std_dev_exact = np.std(exact_measure[by_ex[:sel_size]])
    sel_estim = (np.arange(n) < sel_size).astype(int)
    sel_exact = (pos_ex[by_nn] < sel_size).astype(int)
    rows = [[cut_round, int(c), int(a), int(b), float(e), float(x)]
            for c, a, b, e, x in zip(by_nn, sel_estim, sel_exact, nn_measure[by_nn], exact_measure[by_nn])]
    return by_nn, int((sel_estim & sel_exact).sum()) / sel_size, std_dev_exact, rows
