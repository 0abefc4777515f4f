"""lambda_min, the cut rows and the multi-cut rows at multiple and nearly multiple smallest eigenvalues, on the device, against the
EXACT spectrum and eigenspaces of tests/spectra_cases.py (premises: tests/test_spectra_cases_cpu.py).

Per k one LP point over disjoint index sets and two list orders ("sorted": whole waves clustered; "mixed": a clustered lane among
three generic ones), on one handle.  Every assertion is against the truth; bit equality is asserted only where it is a documented
contract (the scoring kernels among each other and under a permutation of the list; round_csr = cut_rows; cut_rows_all(., 1) =
the violated rows of cut_rows; round_csr_multi = cut_rows_all; twins at other index sets).  The lam that sdpcut_cut_rows reports
is Jacobi's wherever the row came from Jacobi (csrc/rows.hip), so it is held to the truth, not to the scored bits.

Bounds.  s = 1 + 2 sum|x| + 2 sum|X|, mu_j the exact eigenvalue of the row's rank, B = multicut.row_matrix(row), all measures in
integer arithmetic (spectra_cases.row_measures):
  |lambda - mu_0| <= 3e-15 s for every path (the bound of test_lambda_min_on_points_outside_the_lp_box);
  |tr B - 1|, ||B B - B||_F <= 1e-14;   |<B, M> - mu_j| <= 3e-15 s and the same for the reported eigenvalue;
  ||M B - rho B||_max / max(||M||_max, 1) <= 32 x LAPACK's maximum on the family (spectra_cases.lapack_maxima: ~2e-14);
  <B, P_cluster> >= 1 - 1e-9 where the cluster is 1e-3 from the rest -- and, beyond what was asked, where Case.near_ok holds (the
  prescribed gaps between 1e-6 and 1e-3: Davis-Kahan with the documented residual 1e-12 gives 1e-10);
  rows of one entry: |<B_r, B_s>| <= 1e-13;  n_neg bracketed by the exact spectrum at -1e-15 -+ 3e-15 s;
  a cluster entirely below the threshold whose rows are all offered: sum_r <B_r, P> >= m - 1e-9.
Measured on an MI355X (profiles/clustered_spectra.txt, printed by tools/clustered_spectra.py): no family exceeds the 32 x LAPACK
residual bound (1.7e-14 .. 2.3e-14); largest device figures |lambda - mu_0| / s 6.5e-16 (scoring kernels, family C, k = 3), residual
1.25e-15, 1 - <B, P> 1.1e-15, <B_r, B_s> 1.1e-16 -- the level of LAPACK's own 1.1e-16 / 7.1e-16 / 4.4e-16.  A library whose Jacobi
fallback starts its minimum search at column 1 fails the single-cut test for every k; one with a single inverse-iteration solve
passes (one solve with lambda_min known to an ulp already converges).
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectra_cases as sc      # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS = ("sorted", "mixed")
SCORE_PATHS = ("eig kernel 1", "eig kernel 0", "eig+nn mfma", "eig+nn valu", "eig+nn simple")
ROW_TOL, IDEM_TOL, ORTHO_TOL, PROJ_TOL, RESID_FACTOR = 1e-14, 1e-14, 1e-13, 1e-9, 32.0
_RUN = {}
_ROWS = {}
MEASURED = {}       # (path, family, k) -> [lambda error / s, residual, 1 - <B, P>, orthogonality defect]: maxima
STRICT = True       # tools/clustered_spectra.py measures with False: a missed bound is listed in MISSED and the walk goes on
MISSED = []


def check(ok, *what):
    if STRICT:
        assert ok, what
    elif not ok:
        MISSED.append(what)


def note(path, case, lam=0.0, resid=0.0, proj=0.0, ortho=0.0):
    m = MEASURED.setdefault((path, case.family, case.k), [0.0, 0.0, 0.0, 0.0])
    for i, v in enumerate((lam, resid, proj, ortho)):
        m[i] = max(m[i], float(v))


@pytest.fixture(scope="module")
def handle():
    import sdpcutsel_via_nn_amd as pkg
    h = pkg.Scorer(0)
    h.set_builtin_networks(5)
    yield h
    h.close()


def run(h, k, order):
    """every device answer for one list, computed once per module"""
    from sdpcutsel_via_nn_amd import _capi
    if (k, order) in _RUN:
        return _RUN[(k, order)]
    p = sc.packed(k)
    o = p["orders"][order]
    vv = p["point"]
    h.drop_pending()
    h.set_instance(p["n"], p["Q_arr"])
    h.set_candidates(o["S"], o["ks"])
    N = o["S"].shape[0]
    ids = np.arange(N, dtype=np.int64)
    out = dict(p=p, o=o, N=N, lam={})
    try:
        for eigk in (1, 0):
            h.set_option(_capi.OPT_EIG_KERNEL, eigk)
            h.set_point(vv)
            h.score(_capi.EIG)
            out["lam"]["eig kernel %d" % eigk] = h.get_scores(obj=False)[0].copy()
        h.set_option(_capi.OPT_EIG_KERNEL, 1)
        for kern, name in ((_capi.KERNEL_MFMA, "mfma"), (_capi.KERNEL_VALU, "valu"), (_capi.KERNEL_SIMPLE, "simple")):
            h.set_option(_capi.OPT_KERNEL, kern)
            h.set_point(vv)
            h.score(_capi.EIG | _capi.NN)
            e, ob = h.get_scores()
            out["lam"]["eig+nn " + name] = e.copy()
            out["obj"] = ob.copy()
    finally:
        h.set_option(_capi.OPT_EIG_KERNEL, 1)
        h.set_option(_capi.OPT_KERNEL, _capi.KERNEL_MFMA)
    h.set_point(vv)
    h.score(_capi.NN)
    out["rows after nn"] = h.cut_rows(ids)                       # no eigenvalue at hand: lambda_min on the spot
    out["all1 after nn"] = h.cut_rows_all(ids, 1)
    h.set_point(vv)
    h.score(_capi.EIG)
    out["rows after eig"] = h.cut_rows(ids)                      # inverse iteration with the known value
    out["all1 after eig"] = h.cut_rows_all(ids, 1)
    out["all5"] = h.cut_rows_all(ids, 5)
    out["round"] = h.round_csr(1, N, point=vv, copy=True)
    out["round rows"] = h.cut_rows(out["round"]["idx"])
    out["multi"] = h.round_csr_multi(vv, 1, N, 5, row_quota="sets", copy=True)
    out["multi rows"] = h.cut_rows_all(out["multi"]["idx"], 5)
    _RUN[(k, order)] = out
    return out


def special(o):
    """-> [(list position, case index, copy)] of the clustered candidates of a list"""
    return [(int(i), int(o["case"][i]), int(o["copy"][i])) for i in np.flatnonzero(o["case"] >= 0)]


def twins(o):
    """-> int64 [cases, 2]: list positions of the two copies of every matrix"""
    t = np.zeros((int(o["case"].max()) + 1, 2), dtype=np.int64)
    for i, c, r in special(o):
        t[c, r] = i
    return t


def lam_err(case, value, j=0):
    return float(abs(Fraction(float(value)) - case.spectrum[j])) / case.s


def measure_row(case, j, coef, rhs):
    """exact measures of one row against eigenvalue j of its matrix (computed once per distinct row)"""
    from sdpcutsel_via_nn_amd import multicut
    m = case.k * (case.k + 3) // 2
    key = (id(case), j, np.asarray(coef[:m]).tobytes(), float(rhs))
    if key not in _ROWS:
        B = multicut.row_matrix(coef, rhs, case.k)
        r = sc.row_measures(B, case.M, case.spectrum[j], case.proj[j])
        r["B"] = B
        _ROWS[key] = r
    return _ROWS[key]


def assert_row(path, case, j, coef, rhs, lam, resid_bound):
    check(np.isfinite(lam) and np.isfinite(rhs) and np.isfinite(coef).all(), path, case.tag)
    r = measure_row(case, j, coef, rhs)
    check(r["trace"] <= ROW_TOL and r["idem"] <= IDEM_TOL, path, case.tag, j, r["trace"], r["idem"])
    check(r["lam_err"] <= sc.LAM_TOL * case.s, path, case.tag, j, r["lam_err"] / case.s)
    check(lam_err(case, lam, j) <= sc.LAM_TOL, path, case.tag, j, lam_err(case, lam, j))
    check(r["resid"] <= resid_bound[case.family], path, case.tag, j, r["resid"], resid_bound[case.family])
    placed = case.qualifies[j] or case.near_ok(j)
    if placed:
        check(r["proj"] >= 1.0 - PROJ_TOL, path, case.tag, j, 1.0 - r["proj"])
    note(path, case, lam=max(r["lam_err"] / case.s, lam_err(case, lam, j)), resid=r["resid"], proj=(1.0 - r["proj"]) if placed else 0.0)
    return r


def resid_bounds():
    """32 x LAPACK's exactly measured residual maximum on the family"""
    _, fam = sc.lapack_maxima()
    return {f: RESID_FACTOR * fam[f][1] for f in fam}


# ------------------------------------------------------------------------------------------------------------ lambda_min
@pytest.mark.parametrize("k", sc.KS)
def test_lambda_min_against_the_exact_spectrum(handle, k):
    per_order = {}
    for order in ORDERS:
        d = run(handle, k, order)
        o, cs = d["o"], d["p"]["cases"]
        base = d["lam"][SCORE_PATHS[0]]
        assert base.shape == (d["N"],)
        for path in SCORE_PATHS:
            lam = d["lam"][path]
            check(np.isfinite(lam).all(), order, path)
            assert np.array_equal(lam, base), (order, path, int((lam != base).sum()))          # the scoring kernels: same bits
        paths = [(path, d["lam"][path]) for path in SCORE_PATHS[:1]] + [("cut_rows after nn", d["rows after nn"][0]), ("cut_rows after eig", d["rows after eig"][0])]
        for path, lam in paths:
            check(np.isfinite(lam).all(), order, path)
            for i, c, r in special(o):
                case = cs[c]
                e = lam_err(case, lam[i])
                note(path, case, lam=e)
                check(e <= sc.LAM_TOL, order, path, case.tag, float(lam[i]), float(case.spectrum[0]), e)
                mu0 = float(case.spectrum[0])
                if abs(mu0 - sc.NEG) > sc.LAM_TOL * case.s:
                    check((lam[i] < sc.NEG) == (mu0 < sc.NEG), order, path, case.tag)
            t = twins(o)
            assert np.array_equal(lam[t[:, 0]], lam[t[:, 1]]), (order, path)                   # twins at other index sets
        t = twins(o)
        per_order[order] = base[t]
        worst = max(lam_err(cs[c], base[i]) for i, c, _ in special(o))
        print("k = %d, %s: max |lambda - mu_0| / s = %.2e over %d clustered lanes" % (k, order, worst, len(special(o))))
    assert np.array_equal(per_order["sorted"], per_order["mixed"])                              # the two orders, through the permutation


# ------------------------------------------------------------------------------------------------------------ one cut per set
@pytest.mark.parametrize("k", sc.KS)
def test_single_cut_rows_against_the_exact_eigenspaces(handle, oracle, k):
    """cut_rows after score(EIG) and after score(NN), round_csr under strategy 1 over the whole list, cut_rows_all(., 1).  Measured:
    residual <= 9.4e-16 against bounds of 1.7e-14 .. 2.3e-14 (profiles/clustered_spectra.txt)."""
    from sdpcutsel_via_nn_amd.cut_solver import rows_to_csr
    bound = resid_bounds()
    m = k * (k + 3) // 2
    for order in ORDERS:
        d = run(handle, k, order)
        o, cs = d["o"], d["p"]["cases"]
        t = twins(o)
        for state in ("after eig", "after nn"):
            lam, coef, rhs, cols, kk = d["rows " + state]
            assert np.all(kk == k) and not coef[:, m:].any()
            for i, c, r in special(o):
                if r == 0:
                    assert_row("cut_rows " + state, cs[c], 0, coef[i], rhs[i], lam[i], bound)
            # twins: equal rows
            assert np.array_equal(coef[t[:, 0]], coef[t[:, 1]]) and np.array_equal(rhs[t[:, 0]], rhs[t[:, 1]]), (order, state)
            # cut_rows_all(., 1): the violated rows of cut_rows, bit for bit
            rp, rl, co, rh, cl, k1 = d["all1 " + state]
            sel = lam < sc.NEG
            assert np.array_equal(rp, np.concatenate([[0], np.cumsum(sel)]))
            assert np.array_equal(rl, lam[sel]) and np.array_equal(co, coef[sel]) and np.array_equal(rh, rhs[sel]) and np.array_equal(cl, cols)
        # the round: the head is the ranking of the device's own lambda, the rows are cut_rows' rows
        r = d["round"]
        eig = d["lam"][SCORE_PATHS[0]]
        head, score, _, _ = oracle.rank_arrays(1, d["obj"], eig, d["N"])
        assert np.array_equal(r["idx"], head) and np.array_equal(r["score"], score + 0.0) and r["n_total"] == head.shape[0]
        lam, coef, rhs, cols, kk = d["round rows"]
        assert np.array_equal(r["lam"], lam)
        keep = np.flatnonzero(lam < sc.NEG)
        indptr, ind, val = rows_to_csr(coef[keep], cols[keep], kk[keep])
        assert np.array_equal(r["row_entry"], keep) and np.array_equal(r["indptr"], indptr) and np.array_equal(r["indices"], ind)
        assert np.array_equal(r["values"], val) and np.array_equal(r["rhs"], rhs[keep])
        # ... and cut_rows' rows for a head are its rows for the list
        full = d["rows after eig"]
        assert np.array_equal(coef, full[1][head]) and np.array_equal(rhs, full[2][head]) and np.array_equal(lam, full[0][head])
        # twins tie: they stand in entry order with equal rows, next to each other unless another matrix shares their bits
        pos = {int(c): n for n, c in enumerate(head)}
        for c in range(t.shape[0]):
            a, b = int(t[c, 0]), int(t[c, 1])
            assert (a in pos) == (b in pos)
            if a in pos:
                lo, hi = sorted((pos[a], pos[b]))
                assert (pos[a] < pos[b]) == (a < b) and np.all(r["score"][lo:hi + 1] == r["score"][lo])
                assert np.array_equal(coef[pos[a]], coef[pos[b]]) and rhs[pos[a]] == rhs[pos[b]]


# ------------------------------------------------------------------------------------------------------------ all violated cuts
def _count_below(case, shift):
    return sum(1 for mu in case.spectrum if float(mu) < sc.NEG + shift * sc.LAM_TOL * case.s)


def _check_entry_rows(path, case, lams, coefs, rhss, bound):
    """the rows one entry offers: ranks 0, 1, ..; -> their measures"""
    assert len(lams) <= 5
    ms = []
    for j in range(len(lams)):
        check(lams[j] < sc.NEG and (j == 0 or lams[j - 1] <= lams[j]), path, case.tag, list(lams))
        ms.append(assert_row(path, case, j, coefs[j], rhss[j], lams[j], bound))
    for a in range(len(ms)):
        for b in range(a):
            ip = abs(float((ms[a]["B"] * ms[b]["B"]).sum()))
            note(path, case, ortho=ip)
            check(ip <= ORTHO_TOL, path, case.tag, a, b, ip)
    lo, hi = min(_count_below(case, -1), 5), min(_count_below(case, +1), 5)
    check(lo <= len(lams) <= hi, path, case.tag, len(lams), lo, hi)
    # a cluster entirely below the threshold whose rows are all there: together they cover its eigenspace
    done = set()
    for j in range(len(lams)):
        mem = case.members[j]
        if tuple(mem) in done or not (case.qualifies[j] or case.near_ok(j)):
            continue
        done.add(tuple(mem))
        if mem[-1] < len(lams) and all(float(case.spectrum[i]) < sc.NEG - sc.LAM_TOL * case.s for i in mem):
            cover = sum(float((ms[i]["B"] * case.proj[j]).sum()) for i in mem)
            note(path, case, proj=(len(mem) - cover) / len(mem))
            check(cover >= len(mem) - PROJ_TOL, path, case.tag, mem, len(mem) - cover)
    return ms


@pytest.mark.parametrize("k", sc.KS)
def test_multi_cut_rows_against_the_exact_eigenspaces(handle, k):
    """cut_rows_all(., 5) and round_csr_multi under strategy 1 with row_quota = 5 sel.  Measured: residual <= 1.25e-15, <B_r, B_s> <=
    1.1e-16 (profiles/clustered_spectra.txt).  multicut.check_rows sees the same rows with the exact spectrum."""
    from sdpcutsel_via_nn_amd import multicut
    bound = resid_bounds()
    for order in ORDERS:
        d = run(handle, k, order)
        o, cs = d["o"], d["p"]["cases"]
        rp, rl, co, rh, cl, kk = d["all5"]
        assert rp.shape == (d["N"] + 1,) and np.all(np.diff(rp) >= 0) and np.all(np.diff(rp) <= 5) and np.isfinite(rl).all()
        offered = 0
        for i, c, r in special(o):
            a, b = int(rp[i]), int(rp[i + 1])
            if r == 0:
                _check_entry_rows("cut_rows_all 5", cs[c], rl[a:b], co[a:b], rh[a:b], bound)
                offered += (b - a) >= 2
        assert offered >= len(cs) // 5, "too few entries offer two rows"
        # the project's own checker on the same rows, with the exact spectrum in place of numpy's
        first = [i for i, c, r in special(o) if r == 0]
        rows = np.concatenate([np.arange(rp[i], rp[i + 1]) for i in first]).astype(np.int64)
        ent = np.repeat(np.arange(len(first)), [int(rp[i + 1] - rp[i]) for i in first])
        rank = np.concatenate([np.arange(int(rp[i + 1] - rp[i])) for i in first])
        assert multicut.check_rows(o["S"][first], o["ks"][first], d["p"]["point"], d["p"]["n"], 5, ent, rank, rl[rows], co[rows], rh[rows],
                                   spectrum=[cs[int(o["case"][i])].spectrum for i in first])
        t = twins(o)
        for c in range(t.shape[0]):                                                           # twins: equal rows
            a0, b0, a1, b1 = int(rp[t[c, 0]]), int(rp[t[c, 0] + 1]), int(rp[t[c, 1]]), int(rp[t[c, 1] + 1])
            assert b0 - a0 == b1 - a1 and np.array_equal(co[a0:b0], co[a1:b1]) and np.array_equal(rl[a0:b0], rl[a1:b1]) and np.array_equal(rh[a0:b0], rh[a1:b1])
        # the round: the plain round's head, the rows cut_rows_all gives for it
        r, plain = d["multi"], d["round"]
        assert np.array_equal(r["idx"], plain["idx"]) and np.array_equal(r["score"], plain["score"]) and not r["quota_hit"]
        rp2, rl2, co2, rh2, cl2, _ = d["multi rows"]
        assert np.array_equal(np.diff(rp2), np.minimum(r["n_neg"], 5)) and rp2[-1] == r["rhs"].shape[0]
        assert np.array_equal(rl2, r["row_lam"]) and np.array_equal(rh2, r["rhs"])
        assert np.array_equal(r["row_entry"], np.repeat(np.arange(r["idx"].shape[0]), np.diff(rp2)))
        for row in range(int(rp2[-1])):
            lo, hi = r["indptr"][row], r["indptr"][row + 1]
            assert np.array_equal(co2[row, :hi - lo], r["values"][lo:hi]) and not co2[row, hi - lo:].any()
        # ... which are its rows for the list; n_neg inside the bracket of the exact spectrum
        for e, i in enumerate(r["idx"]):
            a, b, a2, b2 = int(rp[i]), int(rp[i + 1]), int(rp2[e]), int(rp2[e + 1])
            assert b - a == b2 - a2 and np.array_equal(co[a:b], co2[a2:b2]) and np.array_equal(rl[a:b], rl2[a2:b2])
            c = int(o["case"][i])
            if c >= 0:
                assert _count_below(cs[c], -1) <= r["n_neg"][e] <= _count_below(cs[c], +1), (cs[c].tag, int(r["n_neg"][e]))


# ------------------------------------------------------------------------------------------------------------ the full solver
@pytest.mark.parametrize("k", sc.KS)
def test_eig_batch_against_the_exact_spectrum(handle, k):
    cs = sc.cases(k)
    D = k + 1
    w, v = handle.eig_batch(k, np.stack([c.x for c in cs]), np.stack([c.X for c in cs]), want_vectors=True)
    assert np.isfinite(w).all() and np.isfinite(v).all() and np.all(np.diff(w, axis=1) >= 0)
    bound = resid_bounds()
    for n, case in enumerate(cs):
        V = v[n]
        G = V.T @ V - np.eye(D)
        check(np.abs(G).max() <= ORTHO_TOL, case.tag, np.abs(G).max())
        note("eig_batch", case, ortho=float((G * G).max()))
        for j in range(D):
            e = lam_err(case, w[n, j], j)
            res = sc.vector_residual(case.M, V[:, j])
            placed = case.qualifies[j] or case.near_ok(j)
            defect = 1.0 - float(V[:, j] @ case.proj[j] @ V[:, j]) if placed else 0.0
            note("eig_batch", case, lam=e, resid=res, proj=defect)
            check(e <= sc.LAM_TOL, case.tag, j, e)
            check(res <= bound[case.family], case.tag, j, res)
            check(defect <= PROJ_TOL, case.tag, j, defect)
        for j in range(D):
            mem = case.members[j]
            if mem[0] == j and (case.qualifies[j] or case.near_ok(j)):
                cover = float(np.trace(V[:, mem].T @ case.proj[j] @ V[:, mem]))
                check(cover >= len(mem) - PROJ_TOL, case.tag, mem, len(mem) - cover)
