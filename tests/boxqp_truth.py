"""The exact optimum of a tiny BoxQP, min f(x) = sum_{i <= j} a_ij x_i x_j + sum_i c_i x_i over 0 <= x <= 1, by enumerating the
KKT systems of the 3^n faces of the box (tests/test_tree_cpu.py, tests/test_gpu_tree.py).

A face fixes every variable to 0, to 1, or leaves it free.  A minimiser lies in the relative interior of exactly one face and is a
stationary point of f restricted to it: H_FF x_F = -(c_F + H_FB x_B) with H = A + A^T the Hessian (diagonal 2 a_ii), F the free
and B the fixed variables.  So the minimum of f over the stationary points of all faces that lie in the box IS the optimum.
Points that are not minimisers only add feasible values, which are upper bounds: nothing is lost by taking more candidates than
needed, as long as every candidate is evaluated at a feasible point.  Hence

    singular faces   the system is solved in the least-squares sense; a solution with a residual is no stationary point and is
                     dropped; where stationary points form a continuum f is constant on it (zero gradient along the null space),
                     and if the minimum-norm one leaves the box the continuum meets the boundary -- a smaller face finds the value
    near a bound     a free value within TOL of a bound is accepted and clipped onto the bound before f is evaluated

The free sets are enumerated one by one (2^n) and the 2^|B| fixings of each are solved together.  n <= 12 is practical.
:func:`boxqp_truth` checks itself: the value is at most f at every vertex and at 1000 random points."""
import itertools

import numpy as np

TOL = 1e-9


def dense(n, Q_arr, c):
    """-> (M upper triangular with a_ij, H = M + M^T, c)"""
    M = np.zeros((n, n))
    M[np.triu_indices(n)] = np.asarray(Q_arr, dtype=np.float64)
    return M, M + M.T, np.asarray(c, dtype=np.float64)


def f_value(M, c, X):
    """f at the rows of X [m, n]"""
    X = np.atleast_2d(X)
    return np.einsum("pi,ij,pj->p", X, M, X) + X @ c


def boxqp_truth(n, Q_arr, c, self_check=True):
    """-> (optimal value, a minimiser)"""
    assert 1 <= n <= 12
    M, H, c = dense(n, Q_arr, c)
    scale = max(1.0, np.abs(H).max(), np.abs(c).max())
    best, best_x = np.inf, None
    for mask in range(1 << n):
        F = [i for i in range(n) if mask >> i & 1]
        B = [i for i in range(n) if not mask >> i & 1]
        XB = np.array(list(itertools.product((0.0, 1.0), repeat=len(B)))).reshape(1 << len(B), len(B))      # [m, |B|]
        m = XB.shape[0]
        X = np.zeros((m, n))
        X[:, B] = XB
        if F:
            rhs = -(c[F][:, None] + H[np.ix_(F, B)] @ XB.T)      # [|F|, m]
            sol = np.linalg.lstsq(H[np.ix_(F, F)], rhs, rcond=None)[0]
            resid = np.abs(H[np.ix_(F, F)] @ sol - rhs).max(axis=0)
            ok = (resid <= 1e-9 * scale * max(1, len(F))) & np.all((sol >= -TOL) & (sol <= 1.0 + TOL), axis=0)
            if not ok.any():
                continue
            X = X[ok]
            X[:, F] = np.clip(sol[:, ok].T, 0.0, 1.0)
        v = f_value(M, c, X)
        k = int(np.argmin(v))
        if v[k] < best:
            best, best_x = float(v[k]), X[k].copy()
    if self_check:
        verts = np.array(list(itertools.product((0.0, 1.0), repeat=n)))
        rnd = np.random.default_rng(n).random((1000, n))
        slack = 1e-12 * scale * n * n
        assert best <= f_value(M, c, verts).min() + slack and best <= f_value(M, c, rnd).min() + slack
        assert np.all((best_x >= 0.0) & (best_x <= 1.0)) and abs(f_value(M, c, best_x)[0] - best) <= slack
    return best, best_x


def prototype_instance(n, seed):
    """The dense random instances of the tree tests: integers in [-50, 50] from default_rng(seed), first an n x n matrix whose upper
    triangle (diagonal included) gives a_ij for i <= j, then c -> the dict harness.parse_boxqp returns, in the minimising form
    (sign +1)."""
    rng = np.random.default_rng(seed)
    L = n * (n + 1) // 2
    Q_arr = rng.integers(-50, 51, size=(n, n)).astype(np.float64)[np.triu_indices(n)]
    c = rng.integers(-50, 51, size=n).astype(np.float64)
    return dict(nb_vars=n, nb_lifted=L, Q_arr=Q_arr, c=c, adj=np.ones((n, n), dtype=bool), sign=1.0)


def write_boxqp(path, inst):
    """The instance as a BoxQP ``.in`` file that harness.parse_boxqp reads back to the same Q_arr and c (the file maximises:
    every sign flips, and its diagonal is twice a_ii); the parsed pattern has no edge where a_ij = 0."""
    n = inst["nb_vars"]
    M = np.zeros((n, n))
    M[np.triu_indices(n)] = inst["Q_arr"]
    Q = -(M + M.T)      # (off-diagonal -a_ij in both triangles, diagonal -2 a_ii)
    with open(path, "w") as f:
        f.write("%d 100\n" % n)
        f.write(" ".join("%d" % int(-v) for v in inst["c"]) + "\n")
        for r in range(n):
            f.write(" ".join("%d" % int(v) for v in Q[r]) + "\n")


# (n, seed) of the six instances: n = 5, 6, 6, 8, 8, 10
PROTOTYPES = ((5, 1), (6, 1), (6, 2), (8, 1), (8, 2), (10, 1))
_TRUTH = {}


def truth_of(n, seed):
    """(instance, optimal value, minimiser), computed once per instance and shared"""
    if (n, seed) not in _TRUTH:
        inst = prototype_instance(n, seed)
        _TRUTH[(n, seed)] = (inst,) + boxqp_truth(n, inst["Q_arr"], inst["c"])
    return _TRUTH[(n, seed)]
