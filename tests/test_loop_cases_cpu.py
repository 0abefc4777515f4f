"""loop_cases.py without a GPU: the option model against the real entry point, the coverage of the committed combinations, the
row certificate on numpy-built rows (accepted) and on their mutants (rejected), and the measurement behind its tolerances."""
import numpy as np
import pytest

import loop_cases as lc


# ------------------------------------------------------------------------------------------ 1. the model against the code
def test_the_model_is_the_front_door():
    """Over the full product of axis values (x every strategy with and without the opt-in x dim 3 and 4): a refused combination
    raises AssertionError or ValueError, an accepted one gets as far as the file -- the argument checks precede the parser."""
    from sdpcutsel_via_nn_amd import cut_solver
    solvers = {False: cut_solver.CutSolver(), True: cut_solver.CutSolver(exact_sdp=True)}
    wrong, n_ref, n_acc = [], 0, 0
    for combo in lc.full_product():
        kw = lc.call_kwargs(combo, 20)
        try:
            solvers[combo.exact].cut_select_algo("no-such-file.in", combo.dim, lc.SEL_SIZE, nb_rounds_cuts=lc.ROUNDS, **kw)
            got = "returned"
        except (AssertionError, ValueError):
            got = "refused"
        except FileNotFoundError:
            got = "file"
        want = "file" if lc.accepted(combo) else "refused"
        n_acc += want == "file"
        n_ref += want == "refused"
        if got != want:
            wrong.append((lc.name(combo), combo.exact, combo.dim, want, got))
    assert not wrong, (len(wrong), wrong[:10])
    assert n_acc > 1000 and n_ref > 1000


def test_explicit_neutral_values_are_accepted_wherever_the_combination_is():
    """cuts_per_set=1, objpar_weight=0.0 and box=(0.0, 1.0) spelled out refuse nothing; a pool refuses strategy 0 only"""
    from sdpcutsel_via_nn_amd import cut_solver
    for a in lc.NEUTRAL_A:
        for axis, extra in lc.EXPLICIT_NEUTRAL.items():
            kw = dict(lc.call_kwargs(a, 20), **extra(20))
            cs = cut_solver.CutSolver(exact_sdp=True) if a.exact else cut_solver.CutSolver()
            want = AssertionError if (axis == "pool" and a.strat == 0) else FileNotFoundError
            with pytest.raises(want):
                cs.cut_select_algo("no-such-file.in", a.dim, lc.SEL_SIZE, nb_rounds_cuts=lc.ROUNDS, **kw)


# ------------------------------------------------------------------------------------------ 2. coverage
def test_every_accepted_pair_is_committed():
    assert all(lc.accepted(c) for c in lc.COMMITTED + lc.DIM4 + lc.NEUTRAL_A)
    assert lc.uncovered_pairs() == []
    # every axis alone, every strategy alone
    alone = set(lc.ALONE)
    for s in lc.STRATS:
        assert lc.C(s) in alone
    for a, (_, values) in lc.AXES.items():
        for v in values:
            assert any(lc.active(c) == ((a, v),) for c in alone), (a, v)
    # both routes: a pair the model accepts under a family is there under a strategy of that family
    for fam, strats in lc.FAMILIES.items():
        mine = [c for c in lc.COMMITTED if c.strat in strats and len(lc.active(c)) == 2]
        assert len(mine) >= 40 and set(c.strat for c in mine) == set(strats), fam
    # one run with everything per strategy
    assert sorted(c.strat for c in lc.EVERYTHING) == sorted(lc.STRATS)
    for c in lc.EVERYTHING:      # nothing more can be switched on
        for a, (_, values) in lc.AXES.items():
            if getattr(c, a) == lc.AXES[a][0]:
                assert not any(lc.accepted(c._replace(**{a: v})) for v in values), (lc.name(c), a)


def test_the_coverage_check_notices_a_missing_pair_and_a_wrong_model(monkeypatch):
    short = [c for c in lc.COMMITTED if not (c.strat in lc.FAMILIES["feas"] and dict(lc.active(c)).get("pool") and c.tri)]
    assert (("feas", ("tri", True), ("pool", "act")) in lc.uncovered_pairs(short))
    assert (6, ("objpar", 0.1)) in lc.uncovered_pairs([c for c in lc.COMMITTED if not c.objpar])
    # a model that forgets a refusal asks for combinations the list does not have
    real = lc.accepted
    monkeypatch.setattr(lc, "accepted", lambda c: real(c._replace(maxpar=None)))
    assert (5, ("maxpar", 0.5)) in lc.uncovered_pairs()


# ------------------------------------------------------------------------------------------ 3. rows the certificate accepts
@pytest.fixture(scope="module")
def reference():
    """numpy-built eigen-cuts per (n, k), shared and left unchanged"""
    return {(n, k): lc.reference_rows(lc.SEED, n, k, cnt) for n, k, cnt in [(20, 2, 30), (20, 3, 30), (40, 4, 30), (40, 5, 30), (20, 20, 6), (40, 40, 3)]}


def test_accepts_numpy_built_eigen_cuts(reference):
    for (n, k), rows in reference.items():
        for cols, vals, rhs, s, point in rows:
            c = lc.certify(cols, vals, rhs, n)
            assert c.kind == "eig" and c.s == s and c.order == k + 1
            theta, resid = lc.eigenpair(c, point, n)
            assert theta < -1e-6
            # in any column order
            perm = np.random.default_rng(k).permutation(cols.shape[0])
            assert lc.certify(cols[perm], vals[perm], rhs, n).s == s


def test_accepts_the_four_triangle_forms():
    for n, triple in ((20, (0, 1, 2)), (20, (3, 11, 19)), (40, (0, 20, 39))):
        for form in range(4):
            cols, vals, rhs = lc.tri_row(n, triple, form)
            c = lc.certify(cols, vals, rhs, n)
            assert c.kind == "tri" and c.triple == triple and c.form == (3 if form == 3 else 1)


# ------------------------------------------------------------------------------------------ 4. rows it must reject
def _rejects(cols, vals, rhs, n, what):
    with pytest.raises(lc.CertificateError, match=what):
        lc.certify(cols, vals, rhs, n)


def test_rejects_the_mutants(reference):
    rng = np.random.default_rng(lc.SEED)
    for (n, k), rows in reference.items():
        if k == n:
            continue
        L = n * (n + 1) // 2
        for cols, vals, rhs, s, point in rows[:10]:
            # two column indices swapped (two coefficients change places: an x column and an off-diagonal X column)
            a, b = 0, k + 1
            sw = cols.copy()
            sw[a], sw[b] = cols[b], cols[a]
            _rejects(sw, vals, rhs, n, "rank-one|PSD|unit vector")
            # one X position shifted by one
            j = k + int(rng.integers(0, k * (k + 1) // 2))
            for d in (1, -1):
                sh = cols.copy()
                sh[j] += d
                if 0 <= sh[j] < L:
                    _rejects(sh, vals, rhs, n, "pairs of the set|repeated column|neither shape")
            # the rhs sign flipped
            _rejects(cols, vals, -rhs, n, "PSD|rank-one|unit vector")
            # the row of s on the columns of another set
            t = list(s)
            t[-1] = next(i for i in range(n) if i not in s)
            other = lc.eig_row(n, tuple(sorted(t)), np.ones(k + 1))[0]
            c = lc.certify(other, vals, rhs, n)      # (a complete pattern: the shape passes, and so do C's tests -- the same C)
            with pytest.raises(lc.CertificateError, match="eigenpair|not violated"):
                lc.eigenpair(c, point, n)
            # half the columns of another set: an incomplete pattern
            mixed = cols.copy()
            mixed[:k] = other[:k]
            _rejects(mixed, vals, rhs, n, "pairs of the set")
            # off-diagonal coefficients without the factor 2: still PSD, only the rank-one test sees it
            nf = vals.copy()
            off = np.array([False] * k + [p != q for p in range(k) for q in range(p, k)])
            nf[off] /= 2.0
            nf[:k] /= 2.0
            _rejects(cols, nf, rhs, n, "rank-one")
            # a column outside the LP
            out = cols.copy()
            out[0] = L + n
            _rejects(out, vals, rhs, n, "outside")
            out[0] = cols[1]
            _rejects(out, vals, rhs, n, "repeated")
            with pytest.raises(lc.CertificateError, match="sense"):
                lc.certify(cols, vals, rhs, n, sense="L")


def test_the_row_without_the_factor_two_is_psd():
    """... so that only the rank-one test can catch it: the reason that test exists"""
    n, k = 20, 3
    cols, vals, rhs, s, point = lc.reference_rows(lc.SEED, n, k, 1)[0]
    nf = vals.copy()
    nf[:k] /= 2.0
    nf[k:][[p != q for p in range(k) for q in range(p, k)]] /= 2.0
    free = {k + 1: float("inf")}
    c = lc.certify(cols, nf, rhs, n, tol=free)
    assert c.lam_min > 1e-3 and c.lam_2 > 1e-3      # positive definite: valid, but no eigen-cut
    _rejects(cols, nf, rhs, n, "rank-one")


def test_rejects_triangle_mutants():
    n, triple = 20, (2, 7, 13)
    for form in range(4):
        cols, vals, rhs = lc.tri_row(n, triple, form)
        for j in range(cols.shape[0]):      # one sign flipped: cuts off a vertex, or is valid and weaker (tight at 4 vertices)
            fl = vals.copy()
            fl[j] = -fl[j]
            _rejects(cols, fl, rhs, n, "cut off the vertex|no triangle inequality")
        _rejects(cols, vals, rhs - 1.0 if form < 3 else rhs + 1.0, n, "cut off the vertex|no triangle inequality")
        sh = cols.copy()
        sh[1] += 1                          # X_ad -> X_a(d+1): not the pairs of one triple
        _rejects(sh, vals, rhs, n, "one triple|neither shape|pairs of the set")
        _rejects(cols, vals * 0.5, rhs, n, "other than")
    cols, vals, rhs = lc.tri_row(n, triple, 0)
    out = cols.copy()
    out[3] = n * (n + 1) // 2 + 5           # the x column of a variable outside the triple
    _rejects(out, vals, rhs, n, "outside the triple")


def test_pattern_and_violated_triangles():
    """the pattern read off an LP's initial rows is the adjacency it was built on; the triangle inequalities the loop must
    separate are those of the triples with two or three edges"""
    from sdpcutsel_via_nn_amd import harness
    n, L = 8, 36
    rng = np.random.default_rng(lc.SEED)
    adj = np.triu(rng.uniform(size=(n, n)) < 0.4, 1)
    adj = adj | adj.T
    for rel in (harness.mccormick_csr(n, adj), harness.mccormick_csr_box(n, adj, np.full(n, 0.25), np.full(n, 0.75))):
        ptr, ind, val, rhs = rel
        assert np.array_equal(lc.lp_pattern((val, ind, np.diff(ptr), rhs, None), n), adj)
    point = harness.random_mccormick_point(n, rng)
    must, may = lc.violated_triangles(adj, point, n)
    assert must and must <= may
    for (triple, form) in may:
        a, b, d = triple
        assert int(adj[a, b]) + int(adj[a, d]) + int(adj[b, d]) >= 2
        cols, vals, rhs = lc.tri_row(n, triple, form)
        assert lc.row_violation(cols, vals, rhs, point) >= lc.THRES_TRI_VIOL - 8 * lc.EPS
        assert lc.certify(cols, vals, rhs, n).which == form
    # nothing violated is left out
    for triple in [(0, 1, 2), (1, 4, 7), (2, 3, 5)]:
        a, b, d = triple
        for form in range(4):
            cols, vals, rhs = lc.tri_row(n, triple, form)
            inside = int(adj[a, b]) + int(adj[a, d]) + int(adj[b, d]) >= 2 and lc.row_violation(cols, vals, rhs, point) > 2e-7
            assert not inside or (triple, form) in must


# ------------------------------------------------------------------------------------------ 5. the tolerance
def test_tolerance_measurement(capsys):
    """The eigensolver's part of the tolerance, measured on numpy-built rows and printed; the committed table is 2 eps + 4 times the
    committed measurement, and a measurement here (another LAPACK, maybe) stays within a factor 2 of the committed one."""
    worst = lc.measure_tolerances()
    with capsys.disabled():
        print()
        for order in sorted(worst):
            print("order %2d: worst measured %.4e (committed %.4e), tol %.4e" % (order, worst[order], lc.MEASURED[order], lc.TOL[order]))
    assert sorted(worst) == sorted(lc.MEASURED) == [3, 4, 5, 6, 21, 41]
    for order, w in worst.items():
        assert lc.TOL[order] == 2.0 * lc.EPS + 4.0 * lc.MEASURED[order]
        assert 0.5 * lc.MEASURED[order] <= w <= 2.0 * lc.MEASURED[order], (order, w)
