"""All violated eigen-cuts of a selected set: the numpy twin and checker of csrc/multirows.hip (sdpcut_round_csr_multi,
sdpcut_cut_rows_all).

The rule ("All violated eigen-cuts").  Entry i of a head -- an index set of k variables -- has the lifted
matrix ``M = [[1, x^T],[x, X]]`` at the LP point.  It *offers* its eigenpairs with eigenvalue ``< -1e-15`` in ascending eigenvalue
order, at most ``cuts_per_set`` of them.  The row of an eigenpair is what the one-cut kernel builds from a vector: components with
``|v| <= 1e-15`` zeroed, coefficients ``[2 v0 v1 .. 2 v0 vk | v1^2, 2 v1 v2, .., vk^2]`` on the LP columns ``[L + i for i in
set_inds] + Xarr_inds``, rhs ``-v0^2``, sense "G".  Rows are numbered in (entry, eigenvalue) order and rows numbered ``>=
row_quota`` are dropped, so the walk may end inside an entry.

``expected`` builds the rows with ``numpy.linalg.eigh``; ``walk`` applies the quota; ``check_rows`` checks what holds of ANY correct
answer, tied eigenvalues included, where two solvers may return different bases of an eigenspace.
"""
import numpy as np

NEG_EIGVAL = -1e-15      # _THRES_NEG_EIGVAL, cut_select_qp.py:24
ROW_LD = 20
MAX_PER_SET = 5


def _check_m(cuts_per_set):
    m = int(cuts_per_set)
    if m != cuts_per_set or not 1 <= m <= MAX_PER_SET:
        raise ValueError("cuts_per_set must be an integer in 1 .. %d" % MAX_PER_SET)
    return m


def lifted(s, point, nb_vars):
    """-> (M [k+1, k+1], cols int64 [k + k(k+1)/2]) of the index set s at the LP point [X packed | x]"""
    n = int(nb_vars)
    L = n * (n + 1) // 2
    vv = np.asarray(point, dtype=np.float64)
    s = [int(v) for v in s]
    k = len(s)
    M = np.zeros((k + 1, k + 1))
    M[0, 0] = 1.0
    cols = [L + v for v in s]
    for a in range(k):
        M[0, a + 1] = M[a + 1, 0] = vv[L + s[a]]
        base = n * s[a] - s[a] * (s[a] + 1) // 2
        for b in range(a, k):
            M[a + 1, b + 1] = M[b + 1, a + 1] = vv[base + s[b]]
            cols.append(base + s[b])
    return M, np.asarray(cols, dtype=np.int64)


def row_of(v):
    """-> (coef [k + k(k+1)/2], rhs) of the unit vector v [k+1]"""
    v = np.array(v, dtype=np.float64)
    v[np.abs(v) <= -NEG_EIGVAL] = 0.0
    D = v.shape[0]
    co = []
    for i in range(D):
        for j in range(max(i, 1), D):
            co.append(v[i] * v[j] * 2 if i != j else v[i] * v[j])
    return np.asarray(co), -v[0] * v[0]


def expected(set_inds, ks, point, nb_vars, cuts_per_set):
    """The rows every entry OFFERS (no quota) -> dict(n_neg int32 [P], lam_min [P], n_offered int32 [P], row_entry int32 [R],
    row_rank int32 [R], row_lam [R], coef [R, 20] zero padded, rhs [R], indptr int32 [R + 1], indices int32 [nnz], values [nnz],
    eigvals: list of P ascending arrays)."""
    m = _check_m(cuts_per_set)
    S = np.asarray(set_inds)
    ks = np.asarray(ks, dtype=np.int64)
    P = ks.shape[0]
    n_neg = np.zeros(P, dtype=np.int32)
    lam_min = np.zeros(P)
    n_off = np.zeros(P, dtype=np.int32)
    row_entry, row_rank, row_lam, coef, rhs, indptr, indices, values, eigvals = [], [], [], [], [], [0], [], [], []
    for i in range(P):
        k = int(ks[i])
        M, cols = lifted(S[i, :k], point, nb_vars)
        w, V = np.linalg.eigh(M)
        eigvals.append(w)
        n_neg[i] = int((w < NEG_EIGVAL).sum())
        lam_min[i] = w[0]
        n_off[i] = min(int(n_neg[i]), m)
        for r in range(int(n_off[i])):
            co, rh = row_of(V[:, r])
            row_entry.append(i)
            row_rank.append(r)
            row_lam.append(w[r])
            c20 = np.zeros(ROW_LD)
            c20[:co.shape[0]] = co
            coef.append(c20)
            rhs.append(rh)
            indices.extend(cols.tolist())
            values.extend(co.tolist())
            indptr.append(len(indices))
    return dict(n_neg=n_neg, lam_min=lam_min, n_offered=n_off, row_entry=np.asarray(row_entry, dtype=np.int32),
                row_rank=np.asarray(row_rank, dtype=np.int32), row_lam=np.asarray(row_lam, dtype=np.float64),
                coef=np.asarray(coef, dtype=np.float64).reshape(-1, ROW_LD), rhs=np.asarray(rhs, dtype=np.float64),
                indptr=np.asarray(indptr, dtype=np.int32), indices=np.asarray(indices, dtype=np.int32),
                values=np.asarray(values, dtype=np.float64), eigvals=eigvals)


def walk(n_offered, row_quota):
    """The quota on the rows the entries offer -> (kept int32 [P]: rows entry i keeps, n_rows, n_used, quota_hit)."""
    off = np.asarray(n_offered, dtype=np.int64)
    q = int(row_quota)
    if q < 1:
        raise ValueError("row_quota must be >= 1")
    start = np.concatenate([[0], np.cumsum(off)[:-1]]) if off.shape[0] else np.zeros(0, dtype=np.int64)
    kept = np.clip(q - start, 0, off).astype(np.int32)
    n_rows = int(kept.sum())
    used = np.flatnonzero(kept > 0)
    return kept, n_rows, (int(used[-1]) + 1 if used.size else 0), bool(off.sum() > q)


def apply_walk(exp, row_quota):
    """``expected``'s rows cut by the quota -> the same dict restricted to the kept rows, plus n_rows, n_used, quota_hit"""
    kept, n_rows, n_used, hit = walk(exp["n_offered"], row_quota)
    nnz = int(exp["indptr"][n_rows])
    out = dict(exp)
    for f in ("row_entry", "row_rank", "row_lam", "coef", "rhs"):
        out[f] = exp[f][:n_rows]
    out.update(indptr=exp["indptr"][:n_rows + 1], indices=exp["indices"][:nnz], values=exp["values"][:nnz], kept=kept, n_rows=n_rows,
               n_used=n_used, quota_hit=hit)
    return out


def row_matrix(coef, rhs, k):
    """The symmetric matrix B = v v^T a row encodes: B00 = -rhs, B0i = coef / 2, Bii = coef, Bij = coef / 2"""
    k = int(k)
    B = np.zeros((k + 1, k + 1))
    B[0, 0] = -rhs
    m = 0
    for j in range(1, k + 1):
        B[0, j] = B[j, 0] = coef[m] / 2
        m += 1
    for i in range(1, k + 1):
        for j in range(i, k + 1):
            if i == j:
                B[i, i] = coef[m]
            else:
                B[i, j] = B[j, i] = coef[m] / 2
            m += 1
    return B


def check_rows(set_inds, ks, point, nb_vars, cuts_per_set, row_entry, row_rank, row_lam, coef, rhs, row_quota=None, tol=1e-12, spectrum=None):
    """Invariants of an answer (rows in (entry, eigenvalue) order over the P entries given; coef [R, >= row length]) that hold even
    where eigenvalues tie.  With B the matrix of a row (:func:`row_matrix`) and M the entry's lifted matrix:
      * row_entry ascends, row_rank counts 0, 1, .. inside an entry and stays below cuts_per_set;
      * row_lam < -1e-15 and ascends inside an entry;
      * B is rank one with trace 1 up to the zeroing of components <= 1e-15: |tr B - 1| <= tol, ||B B - B||_F <= tol;
      * ||M B - row_lam B||_F <= tol (the residual bound the one-cut kernel accepts for its inverse iteration);
      * |<B_r, B_s>_F| <= tol for two rows of one entry;
      * completeness: every eigenvalue of M below -tol that is among the first cuts_per_set of its entry has its row, unless the
        quota cut it -- then the rows are exactly the first row_quota of the walk and the first entry without all its rows is the
        last one that has any.
    The eigenvalues of M are numpy.linalg.eigvalsh's unless ``spectrum`` gives them: one ascending sequence per entry (floats or
    Fractions), for callers that know the exact ones.
    Raises AssertionError naming the first violation; returns True."""
    m = _check_m(cuts_per_set)
    S = np.asarray(set_inds)
    ks = np.asarray(ks, dtype=np.int64)
    P = ks.shape[0]
    re = np.asarray(row_entry, dtype=np.int64)
    rr = np.asarray(row_rank, dtype=np.int64)
    rl = np.asarray(row_lam, dtype=np.float64)
    C = np.asarray(coef, dtype=np.float64)
    rh = np.asarray(rhs, dtype=np.float64)
    R = re.shape[0]
    assert rr.shape == (R,) and rl.shape == (R,) and rh.shape == (R,) and C.shape[0] == R, "one rank, eigenvalue, rhs and coef row per row"
    assert R == 0 or (re.min() >= 0 and re.max() < P), "row_entry outside the entries"
    assert np.all(np.diff(re) >= 0), "row_entry must ascend"
    if row_quota is not None:
        assert R <= int(row_quota), "%d rows, the quota is %d" % (R, int(row_quota))
    have = np.zeros(P, dtype=np.int64)
    for r in range(R):
        i = int(re[r])
        assert rr[r] == have[i], "row %d: rank %d where entry %d has %d rows so far" % (r, rr[r], i, have[i])
        have[i] += 1
        assert have[i] <= m, "entry %d has more than %d rows" % (i, m)
        assert rl[r] < NEG_EIGVAL, "row %d belongs to eigenvalue %.3e, which is not violated" % (r, rl[r])
    first = 0
    short = []
    for i in range(P):
        k = int(ks[i])
        M, _ = lifted(S[i, :k], point, nb_vars)
        w = np.linalg.eigvalsh(M) if spectrum is None else np.array([float(t) for t in spectrum[i]], dtype=np.float64)
        assert w.shape == (k + 1,) and np.all(np.diff(w) >= 0), "entry %d: the spectrum must hold k + 1 ascending eigenvalues" % i
        rows = list(range(first, first + int(have[i])))
        first += int(have[i])
        Bs = []
        for r in rows:
            B = row_matrix(C[r], rh[r], k)
            assert abs(np.trace(B) - 1.0) <= tol, "row %d: trace %.17g" % (r, np.trace(B))
            assert np.linalg.norm(B @ B - B) <= tol, "row %d is not a rank-one projector: ||B B - B|| = %.3e" % (r, np.linalg.norm(B @ B - B))
            res = np.linalg.norm(M @ B - rl[r] * B)
            assert res <= tol, "row %d: ||M B - lam B|| = %.3e" % (r, res)
            assert np.abs(w - rl[r]).min() <= tol, "row %d: %.17g is no eigenvalue of its matrix" % (r, rl[r])
            for r2, B2 in Bs:
                ip = abs(float((B * B2).sum()))
                assert ip <= tol, "rows %d and %d of entry %d: <B, B'> = %.3e" % (r2, r, i, ip)
            Bs.append((r, B))
        for a, b in zip(rows[:-1], rows[1:]):
            assert rl[a] <= rl[b] + tol, "rows %d, %d: eigenvalues out of order" % (a, b)
        # the rows of an entry are its SMALLEST eigenvalues: row j sits at w[j] up to tol
        for j, r in enumerate(rows):
            assert abs(rl[r] - w[j]) <= tol, "row %d carries eigenvalue %.17g, the entry's %d-th smallest is %.17g" % (r, rl[r], j, w[j])
        need = min(int((w < -tol).sum()), m)
        if have[i] < need:
            short.append(i)
    if short:
        assert row_quota is not None and R == int(row_quota), \
            "entry %d lacks rows of violated eigenvalues and no quota explains it" % short[0]
        used = np.flatnonzero(have > 0)
        last = int(used[-1]) if used.size else -1
        assert short[0] >= last, "entry %d lacks rows but entry %d behind it has some" % (short[0], last)
    return True
