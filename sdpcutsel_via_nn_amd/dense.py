"""Host side of the dense eigen-cuts (strategy 0, cut_select_qp.py:757-786): the layout of a dense row and a numpy twin of
the device eigensolver of csrc/dense.hip.

The twin runs the kernel's algorithm -- two-sided Jacobi, round-robin ordering, the same stop rule, the same sort -- with numpy
arithmetic (no fused multiply-add, numpy's sqrt and division), so it agrees with the device to rounding, not bit for bit.  It is
what the CPU tests pin against ``numpy.linalg.eigh`` and where the constant of the GPU tests' eigenvalue bound was first measured.
"""
import numpy as np

MAX_VARS = 127             # SDPCUT_DENSE_MAX_VARS: the lifted matrix (order n + 1 <= 128) stays in the LDS of one workgroup
MAX_SWEEPS = 30            # DN_MAX_SWEEPS
EPS = 2.0 ** -52
OFF_TOL = EPS * 1e-3       # a sweep starts only while off(A) > OFF_TOL * ||A||_F
NEG_EIGVAL = -1e-15        # _THRES_NEG_EIGVAL, cut_select_qp.py:24


def lifted_matrix(vars_values, nb_vars):
    """[[1, x^T], [x, X]] of the LP point [X packed upper triangle | x] (cut_select_qp.py:762-769), both triangles filled."""
    n = int(nb_vars)
    L = n * (n + 1) // 2
    vv = np.asarray(vars_values, dtype=np.float64)
    A = np.zeros((n + 1, n + 1))
    A[0, 0] = 1.0
    A[0, 1:] = vv[L:L + n]
    iu = np.triu_indices(n)
    A[iu[0] + 1, iu[1] + 1] = vv[:L]
    return np.triu(A) + np.triu(A, 1).T


def row_len(nb_vars):
    return nb_vars + nb_vars * (nb_vars + 1) // 2


def row_cols(nb_vars):
    """LP columns of a dense row, shared by all rows: [L .. L+n-1 | 0 .. L-1] (cut_select_qp.py:779)."""
    n = int(nb_vars)
    L = n * (n + 1) // 2
    return np.concatenate([np.arange(L, L + n), np.arange(L)]).astype(np.int32)


def row_values(v):
    """coefficients and right-hand side of the cut of the unit vector v = (v0, v1 .. vn), in the order of row_cols:
    [2 v0 v1 .. 2 v0 vn | v1^2, 2 v1 v2, .., vn^2], -v0^2 (cut_select_qp.py:776-780; no zeroing of small components)."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[0] - 1
    iu = np.triu_indices(n)
    tri = v[iu[0] + 1] * v[iu[1] + 1] * np.where(iu[0] == iu[1], 1.0, 2.0)
    return np.concatenate([v[0] * v[1:] * 2.0, tri]), -v[0] * v[0]


def tournament_pairs(m, step):
    """The m / 2 disjoint pairs of step `step` (0 .. m-2) of the round-robin ordering of m players (m even): player m-1 stays,
    the others turn.  -> (p, q) with p < q.  An odd order plays with m = D + 1; a pair that holds index D is the bye."""
    k = np.arange(1, m // 2)
    a = np.concatenate([[m - 1], (step + k) % (m - 1)])
    b = np.concatenate([[step], (step - k) % (m - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_twin(A):
    """-> (eigenvalues ascending, V with V[:, r] the vector of eigenvalue r, sweeps): the iteration of dn_eig_kernel."""
    A = np.array(A, dtype=np.float64)
    D = A.shape[0]
    m = D + (D & 1)
    V = np.eye(D)
    fro = np.sqrt(np.sum(A * A))
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        off = np.sqrt(2.0 * np.sum(np.triu(A, 1) ** 2))
        if not off > OFF_TOL * fro:
            break
        for step in range(m - 1):
            p, q = tournament_pairs(m, step)
            live = q < D
            p, q = p[live], q[live]
            apq = A[p, q]
            d = A[q, q] - A[p, p]
            b = 2.0 * apq
            t = b / (d + np.copysign(np.sqrt(d * d + b * b + 1e-300), d))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            app, aqq = A[p, p] - t * apq, A[q, q] + t * apq
            Ap, Aq = A[:, p].copy(), A[:, q].copy()           # A <- A J
            A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
            Ap, Aq = A[p, :].copy(), A[q, :].copy()           # A <- J^T A
            A[p, :], A[q, :] = c[:, None] * Ap - s[:, None] * Aq, s[:, None] * Ap + c[:, None] * Aq
            A[p, p], A[q, q], A[p, q], A[q, p] = app, aqq, 0.0, 0.0
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
        sweeps += 1
    lam = np.diag(A).copy()
    order = np.argsort(lam, kind="stable")
    V = V / np.sqrt(np.sum(V * V, axis=0))      # every vector leaves with unit length (the rotations leave |v|^2 - 1 ~ D eps)
    return lam[order], V[:, order], sweeps


def count_rows(eigvals):
    """rows of a round: the negative eigenvalues among all but the largest (cut_select_qp.py:773-774)"""
    return int(np.count_nonzero(np.asarray(eigvals)[:-1] < NEG_EIGVAL))
