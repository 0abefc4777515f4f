"""Node evaluation: the numpy twin of csrc/node_eval.hip (``Scorer.node_eval_points``) and a checker of its invariants.

After its LP solves and separation rounds a tree node needs an incumbent from its LP point, the true objective there and a branching
variable with its value.  The objective is the LP's own vector ``obj = [a packed | c]`` over ``[X packed | x]``:

    f(x) = sum_{i <= j} a_ij x_i x_j + sum_i c_i x_i

Per point, with its box ``(l, u)`` or the unit box -- include/sdpcut.h states the rule in full:

* projection   ``x <- min(max(x, l), u)``
* local search Gauss-Seidel coordinate descent inside the box, i ascending: ``s = c_i + sum_{j != i} a_ij x_j``, ``a = a_ii``;
  ``a > 0``: ``t = clamp(-s / (2 a), l_i, u_i)``, else the endpoint with the smaller ``phi(t) = (a t + s) t`` (a tie: ``l_i``); the move
  is taken only if ``phi(t) < phi(x_i)`` strictly; a sweep without a move ends the search
* branching    candidates ``u_i - l_i >= 4 BOX_MIN_WIDTH``; rule 0 ``g_i = X_ii - x_i^2``, rule 1 ``g_i = sum_j |a_ij| |X_ij - x_i x_j|``;
  the largest g, lowest index on ties; ``branch_val = clamp(x_i, l_i + m, u_i - m)``, ``m = max(rho (u_i - l_i), BOX_MIN_WIDTH)``,
  moved by single ulps where rounding would leave a child narrower than BOX_MIN_WIDTH

The twin computes every sum in the device's order (csrc/node_eval.hip names them) with separate multiplications and additions, so
its outputs equal the device's bit for bit.  It is vectorised over the points; the coordinate loop is a Python loop.
"""
import numpy as np

from .nodebox import BOX_MIN_WIDTH

MAX_N = 1024            # NODE_EVAL_MAX_N (csrc/node_eval.hip)
MAX_POINTS = 256        # SDPCUT_BATCH_MAX_POINTS
CAND_WIDTH = 4.0 * BOX_MIN_WIDTH
KEYS = ("x_local", "f_point", "f_local", "sweeps", "moves", "branch_var", "branch_score", "branch_val")


def dense_objective(obj, n):
    """obj [L + n] -> (A [n, n] symmetric with a_ij in both triangles, c [n])"""
    obj = np.asarray(obj)
    L = n * (n + 1) // 2
    A = np.zeros((n, n), dtype=obj.dtype)
    iu = np.triu_indices(n)
    A[iu] = obj[:L]
    A[(iu[1], iu[0])] = obj[:L]
    return A, obj[L:]


def dense_X(points, n):
    """points [P, L + n] -> X [P, n, n] symmetric"""
    pts = np.asarray(points)
    iu = np.triu_indices(n)
    L = iu[0].shape[0]
    X = np.zeros((pts.shape[0], n, n), dtype=pts.dtype)
    X[:, iu[0], iu[1]] = pts[:, :L]
    X[:, iu[1], iu[0]] = pts[:, :L]
    return X


def check_args(obj, points, boxes, max_sweeps, branch_rule, rho):
    """The refusals of sdpcut_node_eval_points that need no device (the library repeats them) -> (obj, points [P, L + n], lb, ub
    [P, n] or None, None, n) as contiguous float64."""
    obj = np.ascontiguousarray(obj, dtype=np.float64)
    if obj.ndim != 1 or obj.shape[0] < 2:
        raise ValueError("obj must be the LP objective [a packed | c], n(n+1)/2 + n entries")
    m = obj.shape[0]
    n = int((np.sqrt(9.0 + 8.0 * m) - 3.0) / 2.0 + 0.5)
    if n * (n + 1) // 2 + n != m:
        raise ValueError("obj must have n(n+1)/2 + n entries")
    if n > MAX_N:
        raise ValueError("node evaluation serves at most %d variables" % MAX_N)
    if not np.all(np.isfinite(obj)):
        raise ValueError("obj has a non-finite entry")
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != m:
        raise ValueError("points must be [P, n(n+1)/2 + n]: one LP point [X packed | x] per row")
    if not 1 <= pts.shape[0] <= MAX_POINTS:
        raise ValueError("1 .. %d points per call" % MAX_POINTS)
    if not np.all(np.isfinite(pts)):
        raise ValueError("a point has a non-finite entry")
    lb = ub = None
    if boxes is not None:
        bx = np.ascontiguousarray(boxes, dtype=np.float64)
        if bx.shape != (pts.shape[0], 2, n):
            raise ValueError("boxes must be [P, 2, n]: (lb, ub) per point")
        lb, ub = np.ascontiguousarray(bx[:, 0, :]), np.ascontiguousarray(bx[:, 1, :])
        if not (np.all(np.isfinite(bx)) and np.all(lb >= 0.0) and np.all(lb < ub) and np.all(ub <= 1.0)):
            raise ValueError("a box needs finite 0 <= lb < ub <= 1 in every variable")
    if int(max_sweeps) != max_sweeps or max_sweeps < 0 or max_sweeps > 2 ** 31 - 1:
        raise ValueError("max_sweeps must be an integer >= 0")
    if branch_rule not in (0, 1):
        raise ValueError("branch_rule must be 0 (X_ii - x_i^2) or 1 (weighted by the objective)")
    if not (0.0 < rho <= 0.5):
        raise ValueError("rho must lie in (0, 0.5]")
    return obj, pts, lb, ub, n


def _clamp(x, l, u):
    t = np.where(x < l, l, x)
    return np.where(t > u, u, t)


def _lane_sum(v):
    """v [P, n] -> [P]: lane l adds v[l], v[l + 64], ... to +0.0 in ascending order, then p = p + p(lane ^ off), off = 32 .. 1"""
    P, n = v.shape
    rows = (n + 63) // 64
    pad = np.zeros((P, rows * 64), dtype=v.dtype)
    pad[:, :n] = v
    pad = pad.reshape(P, rows, 64)
    p = np.zeros((P, 64), dtype=v.dtype)
    for r in range(rows):
        p = p + pad[:, r, :]
    h = 32
    while h:
        p = p[:, :h] + p[:, h:]
        h >>= 1
    return p[:, 0]


def _f(A, c, x):
    """f at x [P, n]: U_i = sum_{j >= i} A[j, i] x_j, j ascending; f = lane sum of (c_i + U_i) x_i"""
    P, n = x.shape
    U = np.zeros_like(x)
    for j in range(n):
        U[:, :j + 1] = U[:, :j + 1] + A[j, :j + 1][None, :] * x[:, j:j + 1]
    return _lane_sum((c[None, :] + U) * x)


def _phi(a, s, t):
    return (a * t + s) * t


def node_eval_points(obj, points, boxes=None, max_sweeps=50, branch_rule=1, rho=0.2):
    """The twin of ``Scorer.node_eval_points``: obj [L + n] the LP objective, points [P, L + n], boxes [P, 2, n] or None -> dict of
    x_local [P, n], f_point, f_local, branch_score, branch_val (float64 [P]), sweeps, moves, branch_var (int32 [P])."""
    obj, pts, lb, ub, n = check_args(obj, points, boxes, max_sweeps, branch_rule, rho)
    P = pts.shape[0]
    L = n * (n + 1) // 2
    A, c = dense_objective(obj, n)
    if lb is None:
        lb, ub = np.zeros((P, n)), np.ones((P, n))
    x = _clamp(pts[:, L:], lb, ub)
    with np.errstate(all="ignore"):
        f_point = _f(A, c, x)
        # branching
        cand = (ub - lb) >= CAND_WIDTH
        if branch_rule == 0:
            diag = np.arange(n) * n - np.arange(n) * (np.arange(n) - 1) // 2
            g = pts[:, diag] - x * x
        else:
            X = dense_X(pts, n)
            absA = np.abs(A)
            g = np.zeros((P, n))
            for j in range(n):
                g = g + absA[j][None, :] * np.abs(X[:, :, j] - x * x[:, j:j + 1])
        g = np.where(np.isnan(g), -np.inf, g)
        key = np.where(cand, g, -np.inf)
        # the largest g among the candidates, lowest index on ties (a candidate at -inf still stands in front of a non-candidate)
        best = np.max(key, axis=1)
        bvar = np.argmax(cand & (key == best[:, None]), axis=1).astype(np.int32)
        has = cand.any(axis=1)
        bvar = np.where(has, bvar, -1).astype(np.int32)
        r = np.arange(P)
        iv = np.where(has, bvar, 0)
        li, ui = lb[r, iv], ub[r, iv]
        w = rho * (ui - li)
        m = np.where(w < BOX_MIN_WIDTH, BOX_MIN_WIDTH, w)
        bval = _clamp(x[r, iv], li + m, ui - m)
        # l + m and u - m are rounded: the value moves by single ulps until both children pass set_box's own width test
        for _ in range(4):
            bval = np.where(bval - li < BOX_MIN_WIDTH, np.nextafter(bval, np.inf), bval)
        for _ in range(4):
            bval = np.where(ui - bval < BOX_MIN_WIDTH, np.nextafter(bval, -np.inf), bval)
        bval = np.where(has, bval, 0.0)
        bscore = np.where(has, key[r, iv], 0.0)
        # local search
        x = x.copy()
        sweeps = np.zeros(P, np.int32)
        moves = np.zeros(P, np.int32)
        live = np.ones(P, bool)
        for _ in range(int(max_sweeps)):
            if not live.any():
                break
            idx = np.nonzero(live)[0]
            xs, ls, us = x[idx], lb[idx], ub[idx]
            moved = np.zeros(idx.shape[0], np.int32)
            for i in range(n):
                t = A[i][None, :] * xs
                t[:, i] = 0.0
                s = c[i] + _lane_sum(t)
                a, xi, l, u = A[i, i], xs[:, i], ls[:, i], us[:, i]
                if a > 0.0:
                    cnd = _clamp((-s) / (2.0 * a), l, u)
                else:
                    cnd = np.where(_phi(a, s, u) < _phi(a, s, l), u, l)
                mv = _phi(a, s, cnd) < _phi(a, s, xi)
                xs[:, i] = np.where(mv, cnd, xi)
                moved += mv
            x[idx] = xs
            sweeps[idx] += 1
            moves[idx] += moved
            live[idx[moved == 0]] = False
        f_local = _f(A, c, x)
    return dict(x_local=x, f_point=f_point, f_local=f_local, sweeps=sweeps, moves=moves, branch_var=bvar, branch_score=bscore,
                branch_val=bval)


def f_longdouble(obj, x):
    """f at x [P, n] in long double, and the rounding bound of a float64 evaluation of it in any order:
    -> (f, bound), bound = (n + 4) 2^-53 (sum |a_ij x_i x_j| + sum |c_i x_i|) (1 + tiny)"""
    x = np.asarray(x, dtype=np.longdouble)
    n = x.shape[1]
    A, c = dense_objective(np.asarray(obj, dtype=np.longdouble), n)
    Au = np.triu(A)
    f = np.einsum("pi,ij,pj->p", x, Au, x) + x @ c
    mag = np.einsum("pi,ij,pj->p", np.abs(x), np.abs(Au), np.abs(x)) + np.abs(x) @ np.abs(c)
    return f, (n + 4) * 2.0 ** -53 * mag * 1.000001


def check_node_eval(result, obj, points, boxes=None, branch_rule=1, rho=0.2, max_sweeps=None):
    """Invariants of a node evaluation (the device's or the twin's), independent of the order of its sums.  -> list of strings, one
    per violation (empty: all hold):
      * x_local lies inside the box;
      * x_local is coordinate-wise stationary under the rule -- for every i the rule's candidate t, recomputed in long double, has
        phi(t) >= phi(x_i) - the rounding bound of s -- at every point whose search ended by itself (sweeps < max_sweeps, or
        max_sweeps None: every point);
      * f_local and f_point agree with long double within the rounding bound of the sum, and f_local <= f_point within it;
      * branch_var is an argmax of the rule's g over the candidates within the rounding bound of g (exactly -1 without a candidate),
        branch_score is its g;
      * both children [l, val], [val, u] of the branching variable are admissible boxes (width >= BOX_MIN_WIDTH, as set_box checks)."""
    obj64, pts, lb, ub, n = check_args(obj, points, boxes, 0, branch_rule, rho)
    P, L = pts.shape[0], n * (n + 1) // 2
    if lb is None:
        lb, ub = np.zeros((P, n)), np.ones((P, n))
    bad = []
    xl = np.asarray(result["x_local"], dtype=np.float64)
    if xl.shape != (P, n):
        return ["x_local has shape %s, not %s" % (xl.shape, (P, n))]
    ld = np.longdouble
    eps = 2.0 ** -53
    for p in np.nonzero(((xl < lb) | (xl > ub) | ~np.isfinite(xl)).any(axis=1))[0]:
        bad.append("point %d: x_local leaves the box" % p)
    A, c = dense_objective(obj64.astype(ld), n)
    absA = np.abs(A)
    # f
    xp = _clamp(pts[:, L:], lb, ub)
    fl, bl = f_longdouble(obj64, xl)
    fp, bp = f_longdouble(obj64, xp)
    for p in range(P):
        if not abs(ld(result["f_local"][p]) - fl[p]) <= bl[p]:
            bad.append("point %d: f_local %r is not f(x_local) = %r within %.3g" % (p, result["f_local"][p], float(fl[p]), float(bl[p])))
        if not abs(ld(result["f_point"][p]) - fp[p]) <= bp[p]:
            bad.append("point %d: f_point %r is not f(projected x) = %r within %.3g" % (p, result["f_point"][p], float(fp[p]), float(bp[p])))
        if not fl[p] <= fp[p] + bl[p] + bp[p]:
            bad.append("point %d: f(x_local) = %r above f(projected x) = %r" % (p, float(fl[p]), float(fp[p])))
    # stationarity
    X = xl.astype(ld)
    for p in range(P):
        if max_sweeps is not None and int(result["sweeps"][p]) >= int(max_sweeps):
            continue      # (the cap may have cut the search off: the counts alone do not tell)
        x = X[p]
        Ax = A @ x
        for i in range(n):
            s = c[i] + Ax[i] - A[i, i] * x[i]
            a, l, u = A[i, i], ld(lb[p, i]), ld(ub[p, i])
            if a > 0:
                t = min(max(-s / (2 * a), l), u)
            else:
                t = u if (a * u + s) * u < (a * l + s) * l else l
            tol = (n + 4) * eps * (abs(c[i]) + absA[i] @ np.abs(x)) * (abs(t) + abs(x[i])) + 4 * eps * abs(a) * (t * t + x[i] * x[i])
            if (a * t + s) * t < (a * x[i] + s) * x[i] - tol:
                bad.append("point %d: x_local is not stationary in coordinate %d (phi %r at the candidate %r, %r at x_i = %r)"
                           % (p, i, float((a * t + s) * t), float(t), float((a * x[i] + s) * x[i]), float(x[i])))
    # branching
    Xd = dense_X(pts, n).astype(ld)
    xq = xp.astype(ld)
    bv = np.asarray(result["branch_var"])
    for p in range(P):
        cand = (ub[p] - lb[p]) >= CAND_WIDTH
        v = int(bv[p])
        if not cand.any():
            if v != -1:
                bad.append("point %d: branch_var %d without a candidate" % (p, v))
            continue
        if v < 0 or v >= n or not cand[v]:
            bad.append("point %d: branch_var %d is not a candidate" % (p, v))
            continue
        if branch_rule == 0:
            g = np.diagonal(Xd[p]) - xq[p] * xq[p]
            gtol = 4 * eps * (np.abs(np.diagonal(Xd[p])) + xq[p] * xq[p])
        else:
            terms = absA * np.abs(Xd[p] - np.outer(xq[p], xq[p]))
            g = terms.sum(axis=1)
            gtol = (n + 4) * eps * (absA * (np.abs(Xd[p]) + np.abs(np.outer(xq[p], xq[p])))).sum(axis=1)
        if not abs(ld(result["branch_score"][p]) - g[v]) <= gtol[v]:
            bad.append("point %d: branch_score %r is not g = %r of variable %d" % (p, result["branch_score"][p], float(g[v]), v))
        if not g[v] + gtol[v] >= np.max((g - gtol)[cand]):
            bad.append("point %d: branch_var %d (g = %r) is not the argmax (%r)" % (p, v, float(g[v]), float(np.max(g[cand]))))
        val, l, u = float(result["branch_val"][p]), lb[p, v], ub[p, v]
        if not (val - l >= BOX_MIN_WIDTH and u - val >= BOX_MIN_WIDTH):
            bad.append("point %d: a child of variable %d at %r in [%r, %r] is narrower than BOX_MIN_WIDTH" % (p, v, val, l, u))
    return bad
