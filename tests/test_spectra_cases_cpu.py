"""The premises of tests/test_gpu_clustered_spectra.py, without a GPU: the inputs of tests/spectra_cases.py are what they claim to be.

  * family A is exact: Q^T Q = I, M Q = Q Lambda and M_00 = 1 hold in Fraction arithmetic on the doubles, every prescribed gap and
    lambda_0 is there, and the smallest eigenvalue agrees with tests/exact_eig.py (integer characteristic polynomial);
  * every lambda_min cluster is 1e-3 away from the rest of its spectrum, except where the PRESCRIBED gap lies between 1e-6 and 1e-3
    (2^-10 in A, the nominal 1e-5 .. 1e-3 in B): those are clusters of their own, far enough from the rest for the residual bound to place the vector (Case.near_ok);
  * LAPACK's own error on these inputs, measured exactly -- the yardstick of the device bounds (measured: lambda 1.1e-16 s,
    residual 7.2e-16);
  * the numpy twin of csrc/lmin.h (tools/lmin_proto.py) answers within 3e-15 s wherever it answers, and for every k some input is
    deflated by the relative rule, some input is iterated block by block only by the absolute rule after it gave up, and some input
    is left to Jacobi: the device tests reach all three;
  * the packing round-trips: oracle.triu_positions on the packed point returns the bits of every matrix, twins included.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectra_cases as sc      # noqa: E402
import exact_eig                # noqa: E402


def _gap_of(case):
    return case.spectrum[1] - case.spectrum[0]


@pytest.mark.parametrize("k", sc.KS)
def test_family_a_is_exact(k):
    fam = [c for c in sc.cases(k) if c.family == "A"]
    if k == 2:
        assert not fam            # reflectors with two ones only: signed permutations
        return
    assert 48 <= len(fam) <= sc.PER_FAMILY
    for c in fam:
        D = k + 1
        M, Q, lam = sc.frac_matrix(c.M), sc.frac_matrix(c.vectors), c.spectrum
        assert M[0][0] == 1 and all(M[i][j] == M[j][i] for i in range(D) for j in range(D))
        QtQ = sc.fmatmul([list(r) for r in zip(*Q)], Q)
        assert all(QtQ[i][j] == int(i == j) for i in range(D) for j in range(D)), c.tag
        MQ = sc.fmatmul(M, Q)
        assert all(MQ[i][j] == Q[i][j] * lam[j] for i in range(D) for j in range(D)), c.tag          # the spectrum IS lam
        # the product Q Lambda Q^T in Fractions equals the doubles
        back = [[sum(Q[i][t] * lam[t] * Q[j][t] for t in range(D)) for j in range(D)] for i in range(D)]
        assert back == M, c.tag
        assert all(sc.representable(v) for v in lam) and lam == sorted(lam)
        assert any(abs(q) not in (0, 1) for row in Q for q in row), "a signed permutation"
        # the integer characteristic polynomial's smallest root (Newton from the left in 80 digits: a triple root is located to
        # 10^(-80 / 3), and 200 steps of its linear convergence take the start's 1e-3 down to 1e-38)
        root = exact_eig.exact_lambda_min(c.M, float(lam[0]) - 1e-3)
        assert abs(Fraction(root) - lam[0]) <= Fraction(1, 10 ** 20), c.tag
    gaps = {(_gap_of(c), len([v for v in c.spectrum if v - c.spectrum[0] <= 2 * _gap_of(c)])) for c in fam}
    pairs = {g for g, _ in gaps}
    want = set(sc.GAPS_A) - ({Fraction(1, 1 << 52)} if k == 3 else set())      # (D = 4: the large eigenvalue cannot absorb 2^-52)
    assert want <= pairs, sorted(want - pairs)
    assert {c.spectrum[0] for c in fam} == set(sc.LAM0_A)
    triples = [c for c in fam if c.spectrum[2] - c.spectrum[0] <= Fraction(1, 1 << 29)]
    assert any(c.spectrum[2] == c.spectrum[0] for c in triples) and any(0 < c.spectrum[1] - c.spectrum[0] == c.spectrum[2] - c.spectrum[1] for c in triples)
    # singular and positive semidefinite: lambda_0 = 0 multiple; nothing violated: lambda_0 = 1/8
    assert any(c.spectrum[0] == 0 == c.spectrum[1] for c in fam) and any(c.spectrum[0] == Fraction(1, 8) for c in fam)


@pytest.mark.parametrize("k", sc.KS)
def test_clusters_are_separated_from_the_rest(k):
    cs = sc.cases(k)
    assert {c.family for c in cs} == ({"B", "C"} if k == 2 else {"A", "B", "C"})
    assert all(sum(c.family == f for c in cs) <= sc.PER_FAMILY for f in sc.FAMILIES)
    for c in cs:
        if c.qualifies[0]:
            continue
        # the prescribed gaps between TAU and SEP: lambda_min alone, the next eigenvalue more than TAU away
        assert c.family in "AB" and c.members[0] == [0] and sc.TAU < c.gap < 1.5 * sc.SEP and c.near_ok(0), c.tag
        if c.family == "A":
            assert _gap_of(c) == Fraction(1, 1 << 10)
    assert all(all(c.qualifies) for c in cs if c.family == "C")
    assert sum(not c.qualifies[0] for c in cs) <= 30
    # clusters of two and (D >= 4) three eigenvalues, exact multiples among them, and the band the device tests never entered
    sizes = {len(c.members[0]) for c in cs}
    assert {1, 2} <= sizes and (k == 2 or 3 in sizes)
    g = np.array([c.gap for c in cs])
    for lo, hi in ((0.0, 1e-13), (1e-13, 1e-10), (2.0 ** -34 * 0.99, 2.0 ** -33 * 1.01), (1e-10, 1e-8), (1e-8, 1e-6)):
        assert ((g >= lo) & (g <= hi)).any(), (k, lo, hi)


@pytest.mark.parametrize("k", sc.KS)
def test_mpmath_truth_agrees_with_the_integer_characteristic_polynomial(k):
    """families B and C take their truth from mpmath.eigsy; tests/exact_eig.py (integer characteristic polynomial, Newton from the
    left in 80 digits) gives the same lambda_min"""
    for c in sc.cases(k):
        if c.family != "A":
            root = exact_eig.exact_lambda_min(c.M, float(c.spectrum[0]) - 1e-3)
            assert abs(Fraction(root) - c.spectrum[0]) <= Fraction(1, 10 ** 20), c.tag


def test_lapack_yardsticks():
    per, fam = sc.lapack_maxima()
    assert set(fam) == set(sc.FAMILIES) and set(per) == {(f, k) for f in sc.FAMILIES for k in sc.KS} - {("A", 2)}
    for f, (lam_err, resid, _, _) in fam.items():
        print("family %s: LAPACK |lambda - mu_0| / s <= %.2e, residual <= %.2e" % (f, lam_err, resid))
        # two backward-stable LAPACK drivers at order <= 6: a few ulp
        assert 0 < lam_err <= 1e-15 and 0 < resid <= 5e-15, (f, lam_err, resid)


@pytest.mark.parametrize("k", sc.KS)
def test_the_twin_takes_every_route(k):
    sys.path.insert(0, os.path.join(sc.ROOT, "tools"))
    import lmin_proto
    cs = sc.cases(k)
    st = {}
    lam, ok = lmin_proto.lambda_min(np.stack([c.M for c in cs]), st)
    for c, l, o in zip(cs, lam, ok):
        if o:
            assert abs(Fraction(float(l)) - c.spectrum[0]) <= Fraction(sc.LAM_TOL) * Fraction(c.s), (c.tag, float(l))
    relative = st["relative_split"]
    absolute_only = st["blocks"] & ~st["relative_split"]
    jacobi = ~ok
    print("k = %d: %d inputs, %d deflated by the relative rule, %d iterated in blocks by the absolute rule alone, %d left to Jacobi, %d through the hot loop"
          % (k, len(cs), relative.sum(), absolute_only.sum(), jacobi.sum(), (ok & ~st["blocks"]).sum()))
    assert relative.any() and absolute_only.any() and jacobi.any() and (ok & ~st["blocks"]).any()
    assert np.array_equal(st["done"], ok)


@pytest.mark.parametrize("k", sc.KS)
def test_packing_round_trips(oracle, k):
    from sdpcutsel_via_nn_amd import multicut
    p = sc.packed(k)
    n, L, vv, cs = p["n"], p["L"], p["point"], p["cases"]
    assert vv.shape == (L + n,) and p["Q_arr"].shape == (L,)
    for name, o in p["orders"].items():
        S, case, copy = o["S"][:, :k], o["case"], o["copy"]
        special = np.flatnonzero(case >= 0)
        assert np.array_equal(np.sort(case[special] * 2 + copy[special]), np.arange(2 * len(cs))), name      # every matrix twice
        x, X = vv[L:][S], vv[:L][oracle.triu_positions(S, n)]
        for i in special:
            c = cs[case[i]]
            assert x[i].tobytes() == c.x.tobytes() and X[i].tobytes() == c.X.tobytes(), (name, c.tag)
            M, _ = multicut.lifted(S[i], vv, n)
            assert M.tobytes() == c.M.tobytes()
        # disjoint index sets: no variable of a special candidate belongs to any other candidate
        owner = {}
        for i in special:
            for v in S[i]:
                assert owner.setdefault(int(v), (case[i], copy[i])) == (case[i], copy[i])
        assert not np.isin(S[case < 0], list(owner)).any()
    srt, mix = p["orders"]["sorted"], p["orders"]["mixed"]
    assert (srt["case"] >= 0).all() and (mix["case"] < 0).sum() == 3 * (mix["case"] >= 0).sum()


def test_check_rows_takes_an_exact_spectrum():
    """multicut.check_rows with spectrum=: the exact eigenvalues of family A decide, not numpy's"""
    from sdpcutsel_via_nn_amd import multicut
    k = 4
    p = sc.packed(k)
    o = p["orders"]["sorted"]
    pick = [i for i in range(o["S"].shape[0]) if p["cases"][o["case"][i]].family == "A" and o["copy"][i] == 0]
    S, ks = o["S"][pick], o["ks"][pick]
    cs = [p["cases"][o["case"][i]] for i in pick]
    ent, rank, lam, coef, rhs = [], [], [], [], []
    for e, c in enumerate(cs):
        for j, mu in enumerate(c.spectrum):
            if float(mu) < sc.NEG:
                co, rh = multicut.row_of(c.vectors[:, j])
                ent.append(e), rank.append(j), lam.append(float(mu)), rhs.append(rh)
                coef.append(np.concatenate([co, np.zeros(20 - co.shape[0])]))
    assert len(ent) > len(cs)
    args = (S, ks, p["point"], p["n"], 5, ent, rank, lam, np.array(coef), rhs)
    assert multicut.check_rows(*args, spectrum=[c.spectrum for c in cs])
    assert multicut.check_rows(*args)
    wrong = [[v + Fraction(1, 10 ** 6) for v in c.spectrum] for c in cs]
    with pytest.raises(AssertionError):
        multicut.check_rows(*args, spectrum=wrong)
