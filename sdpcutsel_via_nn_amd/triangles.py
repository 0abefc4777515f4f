"""Triangle inequalities at the root and at tree nodes (numpy twin of csrc/tri.hip, csrc/tri_points.hip, csrc/tri_dev.h).

For a triple ``a < b < c`` the four triangle inequalities are facets of the relaxation of ``X = x x^T`` over the UNIT box
(cut_select_qp.py:824-863).  At a node ``l <= x <= u`` of a spatial branch and bound the same inequalities written in the box's own
variables ``x' = (x - l) / d``, ``X'`` (``d = u - l``; :mod:`nodebox`) are valid and tighter; they map back to rows that are linear
in the original ``(x, X)``.  With ``(s1, s2, s4, ta, tb, tc, r)`` of ``FACETS`` the facet of type ``c`` is

    s1 X'_ab + s2 X'_ac + s4 X'_bc + ta x'_a + tb x'_b + tc x'_c >= r

and its violation at a point is ``r`` minus the left-hand side, in the operation order of ``violations`` (the reference's, :836-839).
An entry ``4 t + type`` is violated iff that violation, in the box's units, is at least ``TRI_VIOL_THRES``; the violated entries are
ranked (density 3 first, violation descending, entry ascending) -- density being the original sparsity pattern's -- and the head
of ``max_out`` entries is emitted as rows, sense >=, in the columns of ``vars_values``:

    X_ab : w1 = s1 / (da db)        x_a : (ta / da - w1 lb) - w2 lc
    X_ac : w2 = s2 / (da dc)        x_b : (tb / db - w1 la) - w4 lc
    X_bc : w4 = s4 / (db dc)        x_c : (tc / dc - w2 la) - w4 lb
    rhs  : (r - ((w1 (la lb) + w2 (la lc)) + w4 (lb lc))) + ((ta (la / da) + tb (lb / db)) + tc (lc / dc))

float64, exactly this order, no contraction; an x coefficient that is exactly zero is dropped.  On the unit box (l = 0, d = 1)
every product with l is a zero, so the rows are the reference's: 4 non-zeros +-1 and rhs 0 for types 0 .. 2, 6 non-zeros and rhs
-1 for type 3 -- and the box tables are the original point's bits, so the whole round equals the one without a box byte for byte.
The device reproduces every array here bit for bit (``Scorer.tri_round_csr``, ``Scorer.tri_round_csr_points``).
"""
import numpy as np

from . import nodebox

TRI_VIOL_THRES = 1e-7      # _THRES_TRI_VIOL, cut_select_qp.py:33
TRI_MAX_OUT = 16384

# (s1, s2, s4, ta, tb, tc, r) of the four facets of a triple
FACETS = np.array([[-1.0, -1.0, 1.0, 1.0, 0.0, 0.0, 0.0],
                   [-1.0, 1.0, -1.0, 0.0, 1.0, 0.0, 0.0],
                   [1.0, -1.0, -1.0, 0.0, 0.0, 1.0, 0.0],
                   [1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0]])


def preprocess(adjacency):
    """-> (triples int32 [T, 3], density uint8 [T]): the triples i1 < i2 < i3 with at least two of their three edges in the
    pattern, lexicographic (cut_select_qp.py:799-822; csrc/tri.hip: tri_preprocess)"""
    adj = np.asarray(adjacency) != 0
    n = adj.shape[0]
    tri, dens = [], []
    for i1 in range(n):
        for i2 in range(i1 + 1, n):
            for i3 in range(i2 + 1, n):
                d = int(adj[i1, i2]) + int(adj[i1, i3]) + int(adj[i2, i3])
                if d >= 2:
                    tri.append((i1, i2, i3))
                    dens.append(d)
    return np.array(tri, dtype=np.int32).reshape(-1, 3), np.array(dens, dtype=np.uint8)


def positions(triples, nb_vars):
    """-> packed positions (X_ab, X_ac, X_bc) of every triple, int64 [T] each"""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    n = int(nb_vars)
    ra, rb = n * a - a * (a + 1) // 2, n * b - b * (b + 1) // 2
    return ra + b, ra + c, rb + c


def point_tables(vars_values, box=None):
    """the table the violations are read from: the LP point itself, or at a node the box table [X' | x'] of
    nodebox.transform_tables (the bits of csrc/box.hip: box_point_kernel)"""
    vv = np.asarray(vars_values)
    if box is None:
        return vv
    lb, ub = np.asarray(box[0]), np.asarray(box[1])
    n = lb.shape[0]
    return nodebox.transform_tables(np.zeros(n * (n + 1) // 2, dtype=vv.dtype), vv, lb, ub)[1]


def violations(triples, nb_vars, tables):
    """-> [T, 4] violations of the four facets of every triple at ``tables`` ([X packed | x]), in the dtype of ``tables`` (float64
    for the twin; the tests run it in longdouble).  Operation order of tri_viol_kernel / tri_viol4."""
    tb = np.asarray(tables)
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    n = int(nb_vars)
    L = n * (n + 1) // 2
    p1, p2, p4 = positions(t, n)
    X1, X2, X4 = tb[p1], tb[p2], tb[p4]
    x0, x1, x2 = tb[L + t[:, 0]], tb[L + t[:, 1]], tb[L + t[:, 2]]
    one, zero = tb.dtype.type(1.0), tb.dtype.type(0.0)
    with np.errstate(invalid="ignore"):
        v0 = X1 + X2 - X4 - x0
        v1 = X1 - X2 + X4 - x1
        v2 = -X1 + X2 + X4 - x2
        v3 = -X1 - X2 - X4 + (((zero + x0) + x1) + x2) - one
    return np.stack([v0, v1, v2, v3], axis=1)


def keys(viol, density):
    """selection keys uint64 [T, 4]: bit 63 = density 3, low bits the violation's IEEE image; 0 = not violated (a NaN is not)"""
    v = np.ascontiguousarray(viol, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        is_viol = v >= TRI_VIOL_THRES
    hi = np.where(np.asarray(density).reshape(-1, 1) == 3, np.uint64(1) << np.uint64(63), np.uint64(0))
    return np.where(is_viol, v.view(np.uint64) | hi, np.uint64(0))


def head(viol, density, max_out):
    """-> (entry int64 [w], viol float64 [w], n_violated): the first ``max_out`` violated entries 4 t + type in rank order"""
    k = keys(viol, density).ravel()
    ids = np.flatnonzero(k)
    order = ids[np.lexsort((ids, ~k[ids]))]      # key descending (its complement ascending), entry ascending
    w = max(0, min(int(max_out), order.shape[0]))
    e = order[:w].astype(np.int64)
    return e, np.ascontiguousarray(viol, dtype=np.float64).ravel()[e], int(ids.shape[0])


def rows(triples, nb_vars, entries, box=None):
    """The rows of ``entries`` (4 t + type), sense >=, in the columns of vars_values -> (indptr int32 [r + 1], indices int32,
    values float64, rhs float64 [r]).  Columns X_ab, X_ac, X_bc, then the x columns in ascending variable order, exact zeros
    dropped; the formulas of the module docstring, float64 in that order."""
    e = np.asarray(entries, dtype=np.int64).reshape(-1)
    n = int(nb_vars)
    L = n * (n + 1) // 2
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)[e >> 2]
    f = FACETS[e & 3]
    s1, s2, s4, ta, tb, tc, r = (f[:, j] for j in range(7))
    if box is None:
        lo, d = np.zeros(n), np.ones(n)
    else:
        lo = np.asarray(box[0], dtype=np.float64)
        d = np.asarray(box[1], dtype=np.float64) - lo
    la, lb, lc = lo[t[:, 0]], lo[t[:, 1]], lo[t[:, 2]]
    da, db, dc = d[t[:, 0]], d[t[:, 1]], d[t[:, 2]]
    w1, w2, w4 = s1 / (da * db), s2 / (da * dc), s4 / (db * dc)
    ca = (ta / da - w1 * lb) - w2 * lc
    cb = (tb / db - w1 * la) - w4 * lc
    cc = (tc / dc - w2 * la) - w4 * lb
    rhs = (r - ((w1 * (la * lb) + w2 * (la * lc)) + w4 * (lb * lc))) + ((ta * (la / da) + tb * (lb / db)) + tc * (lc / dc))
    p1, p2, p4 = positions(t, n)
    cols = np.stack([p1, p2, p4, L + t[:, 0], L + t[:, 1], L + t[:, 2]], axis=1)
    vals = np.stack([w1, w2, w4, ca, cb, cc], axis=1)
    keep = np.ones(vals.shape, dtype=bool)
    keep[:, 3:] = vals[:, 3:] != 0.0
    indptr = np.zeros(e.shape[0] + 1, dtype=np.int32)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return indptr, cols[keep].astype(np.int32), np.ascontiguousarray(vals[keep]), np.ascontiguousarray(rhs)


def round_csr(triples, density, nb_vars, vars_values, max_out, box=None):
    """The whole round at one point: what ``Scorer.tri_round_csr(max_out, point=vars_values)`` returns inside ``set_box(*box)``
    (box None: without a box), array for array and bit for bit."""
    viol = violations(triples, nb_vars, point_tables(np.asarray(vars_values, dtype=np.float64), box))
    e, v, nv = head(viol, density, max_out)
    indptr, ind, val, rhs = rows(triples, nb_vars, e, box)
    return dict(entry=e, viol=v, indptr=indptr, indices=ind, values=val, rhs=rhs, n_rows=int(e.shape[0]), n_violated=nv)


SAME_KEYS = ("entry", "viol", "indptr", "indices", "values", "rhs")


def same(a, b):
    """do two results agree byte for byte (arrays, dtypes, counts)?"""
    if a["n_rows"] != b["n_rows"] or a["n_violated"] != b["n_violated"]:
        return False
    for k in SAME_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def check_round(triples, density, nb_vars, vars_values, max_out, res, box=None):
    """The invariants of a round's result, each checked from the definitions and not through ``round_csr``; AssertionError with
    the first one broken.
      head      every emitted entry is violated, its violation is the table's, n_violated is the count of violated entries and
                n_rows = min(max_out, n_violated)
      order     consecutive entries: (density 3 first, violation descending, entry ascending)
      complete  every violated entry that is not emitted ranks behind the last emitted one
      rows      three X columns of the triple, then x columns ascending, no stored zero; and the row's slack equals the facet's
                slack in the box's variables at the eight vertices of the triple's box with X = x x^T -- an affine function of
                (x_a, x_b, x_c, X_ab, X_ac, X_bc) is fixed by those eight points (the multilinear monomials are independent on
                them), so the row IS the facet: valid on the box, and tight exactly where the facet is
    The tolerance of the vertex test is 64 eps times the magnitude the row is computed at (its terms and 1 / (d_i d_j))."""
    n = int(nb_vars)
    L = n * (n + 1) // 2
    tri = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    viol = violations(tri, n, point_tables(np.asarray(vars_values, dtype=np.float64), box))
    k = keys(viol, density).ravel()
    e = np.asarray(res["entry"], dtype=np.int64)
    r = int(res["n_rows"])
    n_viol = int(np.count_nonzero(k))
    assert res["n_violated"] == n_viol, "n_violated %d, the table has %d" % (res["n_violated"], n_viol)
    assert r == min(int(max_out), n_viol) == e.shape[0] == np.asarray(res["rhs"]).shape[0], "n_rows %d of %d violated, max_out %d" % (r, n_viol, max_out)
    assert np.all((e >= 0) & (e < k.shape[0])) and np.unique(e).shape[0] == r, "entry ids out of range or repeated"
    assert np.all(k[e] != 0), "an emitted entry is not violated"
    assert np.asarray(res["viol"], dtype=np.float64).tobytes() == viol.ravel()[e].tobytes(), "a violation is not the table's"
    ke = k[e]
    for i in range(r - 1):
        assert ke[i] > ke[i + 1] or (ke[i] == ke[i + 1] and e[i] < e[i + 1]), "order: entries %d, %d at head positions %d, %d" % (e[i], e[i + 1], i, i + 1)
    if r:
        out = np.ones(k.shape[0], dtype=bool)
        out[e] = False
        out &= k != 0
        ids = np.flatnonzero(out)
        ahead = (k[ids] > ke[-1]) | ((k[ids] == ke[-1]) & (ids < e[-1]))
        assert not np.any(ahead), "complete: violated entry %d ranks in front of the last emitted one and is missing" % ids[np.argmax(ahead)]
    indptr, ind, val, rhs = (np.asarray(res[x]) for x in ("indptr", "indices", "values", "rhs"))
    assert indptr.shape[0] == r + 1 and indptr[0] == 0 and int(indptr[-1]) == ind.shape[0] == val.shape[0], "indptr does not span the rows"
    if box is None:
        lo, d = np.zeros(n), np.ones(n)
    else:
        lo = np.asarray(box[0], dtype=np.float64)
        d = np.asarray(box[1], dtype=np.float64) - lo
    eps = np.finfo(np.float64).eps
    corners = np.array([[(m >> j) & 1 for j in range(3)] for m in range(8)], dtype=np.float64)      # x' of the triple's variables
    for i in range(r):
        abc = tri[e[i] >> 2]
        f = FACETS[e[i] & 3]
        cols, vals = ind[indptr[i]:indptr[i + 1]].astype(np.int64), val[indptr[i]:indptr[i + 1]]
        assert 4 <= cols.shape[0] <= 6, "row %d has %d non-zeros" % (i, cols.shape[0])
        assert np.all(vals != 0.0), "row %d stores a zero" % i
        assert tuple(cols[:3]) == tuple(int(p[0]) for p in positions(abc[None, :], n)), "row %d: X columns" % i
        xc = cols[3:]
        assert np.all(xc[1:] > xc[:-1]) and set(xc - L) <= set(int(v) for v in abc), "row %d: x columns" % i
        coef = dict(zip(cols.tolist(), vals.tolist()))
        scale = 3.0 * float(np.abs(vals[:3]).max())
        for xp in corners:
            x = lo[abc] + d[abc] * xp
            cval = {int(cols[0]): x[0] * x[1], int(cols[1]): x[0] * x[2], int(cols[2]): x[1] * x[2],
                    L + int(abc[0]): x[0], L + int(abc[1]): x[1], L + int(abc[2]): x[2]}
            lhs = sum(c * cval[j] for j, c in coef.items())
            mag = sum(abs(c * cval[j]) for j, c in coef.items()) + abs(float(rhs[i])) + scale
            want = (f[0] * xp[0] * xp[1] + f[1] * xp[0] * xp[2] + f[2] * xp[1] * xp[2] + f[3] * xp[0] + f[4] * xp[1] + f[5] * xp[2]) - f[6]
            assert abs((lhs - float(rhs[i])) - want) <= 64.0 * eps * mag, \
                "row %d (entry %d): slack %r at box vertex %s, the facet's is %r" % (i, e[i], lhs - float(rhs[i]), xp, want)
    return True
