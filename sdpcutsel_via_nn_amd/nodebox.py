"""Node boxes: the instance tables in the variables of a node's box (numpy twin of csrc/box.hip).

A node of a spatial branch and bound differs from the root in its variable bounds ``l <= x <= u``.  The small SDP whose optimum the
MLPs estimate, ``min <Q~, X> s.t. [[1, x^T], [x, X]] >= 0, X_ii <= x_i``, carries the secant of the UNIT box; at a node the valid
constraint is ``X_ii <= (l_i + u_i) x_i - l_i u_i``.  The problem is affine-invariant: with ``d = u - l`` and ``x = l + D x'`` the
node problem in ``x'`` is the unit-box problem, on the tables

    x'_i  = (x_i - l_i) / d_i
    X'_ij = (((X_ij - l_i x_j) - l_j x_i) + l_i l_j) / (d_i d_j)      i <= j, diagonal included
    Q'_ij = Q_ij (d_i d_j)                                            packed positions of Q_arr

The affine terms in ``x`` cancel between ``<Q, X>`` and the minimum, so the measure computed on the primed tables is the objective
improvement in the original units.  All arithmetic is float64 in exactly this operation order (plain numpy does not contract), so
the device's tables (``Scorer.box_tables``) equal these bit for bit, and on the unit box all three equal the originals.
"""
import numpy as np

BOX_MIN_WIDTH = 2.0 ** -10      # SDPCUT_BOX_MIN_WIDTH (include/sdpcut.h): ten halvings of a variable


def check_box(nb_vars, lb, ub):
    """The refusals of sdpcut_set_box that need no device (the library repeats them) -> (lb, ub) as contiguous float64 [n].
    A box is a sub-box of the unit box with every width at least BOX_MIN_WIDTH; non-finite bounds are refused."""
    lb = np.ascontiguousarray(lb, dtype=np.float64)
    ub = np.ascontiguousarray(ub, dtype=np.float64)
    n = int(nb_vars)
    if lb.shape != (n,) or ub.shape != (n,):
        raise ValueError("lb and ub must be [nb_vars]")
    if not (np.all(np.isfinite(lb)) and np.all(np.isfinite(ub))):
        raise ValueError("a box bound is not finite")
    if np.any(lb < 0.0) or np.any(ub > 1.0):
        raise ValueError("a box is a sub-box of the unit box: 0 <= lb, ub <= 1")
    if np.any(ub - lb < BOX_MIN_WIDTH):
        raise ValueError("every variable of a box needs ub - lb >= 2^-10 (fixed and nearly fixed variables are not served)")
    return lb, ub


def check_boxes(nb_vars, boxes, n_points=None):
    """check_box's rule on every box of a batch: boxes [P, 2, n] = (lb, ub) per point (``n_points``: the P it must have) ->
    contiguous float64 [P, 2, n].  The ValueError names the point."""
    bx = np.ascontiguousarray(boxes, dtype=np.float64)
    n = int(nb_vars)
    if bx.ndim != 3 or bx.shape[1:] != (2, n) or bx.shape[0] < 1 or (n_points is not None and bx.shape[0] != int(n_points)):
        raise ValueError("boxes must be [P, 2, nb_vars]: (lb, ub) per point%s, not %s"
                         % ("" if n_points is None else " of the %d points" % int(n_points), bx.shape))
    for p in range(bx.shape[0]):
        try:
            check_box(n, bx[p, 0], bx[p, 1])
        except ValueError as e:
            raise ValueError("point %d: %s" % (p, e)) from None
    return bx


def _pairs(nb_vars):
    """(i, j) of the packed positions: row-major upper triangle"""
    return np.triu_indices(int(nb_vars))


def transform_tables(Q_arr, vars_values, lb, ub):
    """-> (Q', vars') of the box [lb, ub]: what the scoring kernels read while the box is set.  ``vars_values`` may be None
    (-> vars' None).  Works in the dtype of its inputs' common type (float64 for the twin; the tests run it in longdouble)."""
    lb, ub = np.asarray(lb), np.asarray(ub)
    n = lb.shape[0]
    L = n * (n + 1) // 2
    i, j = _pairs(n)
    d = ub - lb
    dd = d[i] * d[j]
    Qb = np.asarray(Q_arr) * dd
    if vars_values is None:
        return Qb, None
    vv = np.asarray(vars_values)
    X, x = vv[:L], vv[L:]
    Xb = (((X - lb[i] * x[j]) - lb[j] * x[i]) + lb[i] * lb[j]) / dd
    xb = (x - lb) / d
    return Qb, np.concatenate([Xb, xb])


def transform_tables_points(Q_arr, points, boxes):
    """The tables of a boxed batch (numpy twin of box_points_kernel, csrc/box.hip): points [P, L + n], boxes [P, 2, n] ->
    (Q' [P, L], vars' [P, L + n]), row p = transform_tables(Q_arr, points[p], *boxes[p]) bit for bit (the same expressions in
    the same order, with a point axis)."""
    bx, pts, Q = np.asarray(boxes), np.asarray(points), np.asarray(Q_arr)
    lb, ub = bx[:, 0, :], bx[:, 1, :]
    n = lb.shape[1]
    L = n * (n + 1) // 2
    i, j = _pairs(n)
    d = ub - lb
    dd = d[:, i] * d[:, j]
    Qb = Q[None, :] * dd
    X, x = pts[:, :L], pts[:, L:]
    Xb = (((X - lb[:, i] * x[:, j]) - lb[:, j] * x[:, i]) + lb[:, i] * lb[:, j]) / dd
    xb = (x - lb) / d
    return Qb, np.concatenate([Xb, xb], axis=1)


def inverse_tables(Q_box, vars_box, lb, ub):
    """The inverse map: (Q', vars') of the box -> (Q, vars) in the original variables (x = l + D x',
    X_ij = d_i d_j X'_ij + l_i x_j + l_j x_i - l_i l_j).  Either table may be None."""
    lb, ub = np.asarray(lb), np.asarray(ub)
    n = lb.shape[0]
    L = n * (n + 1) // 2
    i, j = _pairs(n)
    d = ub - lb
    dd = d[i] * d[j]
    Q = None if Q_box is None else np.asarray(Q_box) / dd
    if vars_box is None:
        return Q, None
    vb = np.asarray(vars_box)
    x = lb + d * vb[L:]
    X = ((dd * vb[:L] + lb[i] * x[j]) + lb[j] * x[i]) - lb[i] * lb[j]
    return Q, np.concatenate([X, x])
