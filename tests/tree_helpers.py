"""Shared by the tree tests (tests/test_tree_cpu.py, tests/test_gpu_tree.py): a dense eigen-cut separator from numpy's eigh and the
invariants of a TreeResult against the exact optimum (tests/boxqp_truth.py)."""
import numpy as np


def eigen_separator(n, max_cuts=None, tol=1e-9):
    """separate(points, boxes) for tree.branch_and_cut: at every point the cuts v^T [[1, x^T], [x, X]] v >= 0 of the eigenvectors
    of the lifted matrix with an eigenvalue below -tol, most negative first (all of them, or the first ``max_cuts``), as a CSR
    block over [X packed | x]: X_ii gets v_i^2, X_ij 2 v_i v_j, x_i 2 v_0 v_i, the right-hand side is -v_0^2."""
    iu = np.triu_indices(n)
    L = iu[0].shape[0]
    off = np.where(iu[0] == iu[1], 1.0, 2.0)

    def separate(points, boxes):
        out = []
        for vv in points:
            Y = np.zeros((n + 1, n + 1))
            Y[0, 0] = 1.0
            Y[0, 1:] = Y[1:, 0] = vv[L:]
            Y[1 + iu[0], 1 + iu[1]] = vv[:L]
            Y[1 + iu[1], 1 + iu[0]] = vv[:L]
            w, V = np.linalg.eigh(Y)
            neg = [k for k in range(n + 1) if w[k] < -tol][:max_cuts]
            if not neg:
                out.append(None)
                continue
            rows = [np.concatenate([off * V[1 + iu[0], k] * V[1 + iu[1], k], 2.0 * V[0, k] * V[1:, k]]) for k in neg]
            vals = np.concatenate(rows)
            m = L + n
            out.append((np.arange(len(neg) + 1, dtype=np.int64) * m, np.tile(np.arange(m, dtype=np.int64), len(neg)), vals,
                        np.array([-V[0, k] ** 2 for k in neg])))
        return out
    return separate


def check_result(res, truth, lp_slack=0.0):
    """The validity invariants of a run, at every iteration: lower <= truth <= upper (the lower bounds are LP values: ``lp_slack``
    is the LP solver's feasibility tolerance times the magnitude, stated by the caller), the global bound never decreases, the
    incumbent never increases."""
    assert res.log, "no iteration was logged"
    lo_prev, up_prev = -np.inf, np.inf
    for nodes, lo, up in res.log:
        assert lo <= truth + lp_slack, (nodes, lo, truth)
        assert up >= truth - 1e-12 * max(1.0, abs(truth)), (nodes, up, truth)
        assert lo >= lo_prev and up <= up_prev, (nodes, lo, lo_prev, up, up_prev)
        lo_prev, up_prev = lo, up
    assert res.lower == res.log[-1][1] and res.upper == res.log[-1][2]
