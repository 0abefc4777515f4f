"""Numpy twin of the efficacy measure (SDPCUT_EFF, csrc/efficacy.hip; include/sdpcut.h has the definition).

For candidate i at an LP point, with ``lam`` the lambda_min the handle holds and ``coef[0..M)`` / ``cols[0..M)``,
``M = k + k(k+1)/2``, the row ``Scorer.cut_rows`` returns for it::

    nrm       = sqrt(sum_m coef[m]^2)                       sums in column order, products and sums rounded separately
    violated  : lam < -1e-15 and nrm > 0
    eff[i]    = -lam / nrm            (violated)            the Euclidean distance by which the row cuts off the LP point
              = min(-lam, +0.0)       (otherwise)           => eff > 0 <=> violated
    objpar[i] = |sum_m coef[m] obj[cols[m]]| / (nrm ||obj||)   (violated, an objective given), else 0.0
    escore[i] = eff[i] + w objpar[i]  (violated), else eff[i]

Every operation is an IEEE fp64 one in a fixed order, so the device's arrays are compared with these bit for bit.
``||obj||`` is :func:`objective_norm`: squares summed in index order, one square root -- the library computes it the same
way when the vector is set.
"""
import numpy as np

NEG_EIGVAL = -1e-15      # SDPCUT_NEG_EIGVAL, _THRES_NEG_EIGVAL of the reference (cut_select_qp.py:24)


def row_len(ks):
    ks = np.asarray(ks, dtype=np.int64)
    return ks + ks * (ks + 1) // 2


def objective_norm(obj):
    """||obj||_2 as sdpcut_set_objective computes it: squares added in index order (cumsum accumulates sequentially)"""
    obj = np.ascontiguousarray(obj, dtype=np.float64)
    if obj.size == 0:
        return 0.0
    return float(np.sqrt(np.cumsum(obj * obj)[-1]))


def row_norms(coef, ks):
    """sqrt(sum of squares) of every row over its first k + k(k+1)/2 positions, in position order"""
    coef = np.asarray(coef, dtype=np.float64)
    M = row_len(ks)
    s = np.zeros(coef.shape[0])
    for m in range(coef.shape[1]):
        s = np.where(m < M, s + coef[:, m] * coef[:, m], s)
    return np.sqrt(s)


def row_dots(coef, cols, ks, obj):
    """sum_m coef[m] obj[cols[m]] of every row, in position order"""
    coef = np.asarray(coef, dtype=np.float64)
    cols = np.asarray(cols, dtype=np.int64)
    obj = np.asarray(obj, dtype=np.float64)
    M = row_len(ks)
    d = np.zeros(coef.shape[0])
    for m in range(coef.shape[1]):
        live = m < M
        c = np.where(live, cols[:, m], 0)
        d = np.where(live, d + coef[:, m] * obj[c], d)
    return d


def measure(lam, coef, cols, ks, obj=None, w=0.0):
    """-> (eff, objpar, escore), float64 [N] each, from rows as ``Scorer.cut_rows`` returns them (coef / cols [N, >= M])."""
    lam = np.asarray(lam, dtype=np.float64)
    w = float(w)
    if not (0.0 <= w < float("inf")):
        raise ValueError("w must be finite and >= 0")
    nrm = row_norms(coef, ks)
    viol = (lam < NEG_EIGVAL) & (nrm > 0.0)
    neg = -lam
    with np.errstate(divide="ignore", invalid="ignore"):
        eff = np.where(viol, neg / nrm, np.where(neg < 0.0, neg, 0.0))      # (min(-lam, +0.0): +0 for lam = 0)
        objpar = np.zeros(lam.shape[0])
        if obj is not None:
            onorm = objective_norm(obj)
            if not (onorm > 0.0 and np.isfinite(onorm)):
                raise ValueError("the objective vector must be finite and not all zero")
            objpar = np.where(viol, np.abs(row_dots(coef, cols, ks, obj)) / (nrm * onorm), 0.0)
        escore = np.where(viol, eff + w * objpar, eff)
    return eff, objpar, escore


def ranking(escore):
    """strategy 6: all candidates by escore descending, ties by ascending index -> ids int64 [N]"""
    return np.argsort(-np.asarray(escore, dtype=np.float64), kind="stable").astype(np.int64)


def check_round(point, indptr, indices, values, rhs, eff=None, lam=None, quota=None, abs_tol=1e-12, rel_tol=1e-9):
    """The invariants of the rows one strategy-6 round hands to the LP, at the round's LP point ``point`` ([X packed | x]):
    at most ``quota`` rows; every row violated at the point (``a.v < rhs``: the LP's sense is >=) and not a zero row; where ``lam``
    (lambda_min of the entry each row came from) is given, the violation ``rhs - a.v`` is ``-lam`` -- for a unit eigenvector
    ``a.v - rhs = v' A v`` -- and where ``eff`` is, the distance ``(rhs - a.v) / ||a||`` is that efficacy, both within
    ``abs_tol + rel_tol |lam|`` (the eigenvector's residual is a few ulp of ||A|| <= 6, the sums have <= 20 terms).
    -> list of problems (empty: all hold)."""
    point = np.asarray(point, dtype=np.float64)
    indptr = np.asarray(indptr, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    indices = np.asarray(indices, dtype=np.int64)
    rhs = np.asarray(rhs, dtype=np.float64)
    r = rhs.shape[0]
    bad = []
    if indptr.shape[0] != r + 1:
        return ["indptr has %d entries for %d rows" % (indptr.shape[0], r)]
    if quota is not None and r > quota:
        bad.append("%d rows exceed the quota %d" % (r, quota))
    for t in range(r):
        a, c = values[indptr[t]:indptr[t + 1]], indices[indptr[t]:indptr[t + 1]]
        act = float(np.dot(a, point[c]))
        nrm = float(np.sqrt(np.dot(a, a)))
        viol = float(rhs[t]) - act
        # (a violation of a few 1e-15 -- lam_min just below the threshold -- may round to <= 0 in this dot product: then lam decides)
        tiny = lam is not None and float(lam[t]) < NEG_EIGVAL and abs(viol + float(lam[t])) <= abs_tol
        if not ((viol > 0.0 or tiny) and nrm > 0.0):
            bad.append("row %d is not violated at the round's point (rhs - a.v = %.3e)" % (t, viol))
            continue
        if lam is not None:
            tol = abs_tol + rel_tol * abs(float(lam[t]))
            if abs(viol + float(lam[t])) > tol:
                bad.append("row %d: violation %.17g is not -lam_min %.17g" % (t, viol, -float(lam[t])))
            if eff is not None and abs(viol / nrm - float(eff[t])) > tol / nrm:
                bad.append("row %d: distance %.17g is not its efficacy %.17g" % (t, viol / nrm, float(eff[t])))
    return bad
